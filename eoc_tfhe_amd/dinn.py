"""Discretised neural networks on encrypted inputs (FHE-DiNN): dense layers with PUBLIC integer weights on
compact lists, one bootstrap per neuron as the activation.

A layer is Engine.linear_device (the weighted sums of a whole input vector, one key switch per OUTPUT), then
Engine.lut_batch_device with the activation's test polynomial, then Engine.pack_device to hand the outputs to the next layer
as a list.  Everything here is integers: inputs x_k are small integers encrypted at x_k * delta_in (PublicKey.encrypt_torus),
weights are int8 in [-127, 127], biases and activation values are Torus32 words.

A blind rotation computes an ANTI-PERIODIC function of its input phase x (f(x + 1/2) = -f(x)): coefficient k of the test
polynomial is the output on [k / 2N, (k + 1) / 2N).  The activations here are symmetric polynomials (tv[k] = tv[N - 1 - k]),
which makes f odd on (-1/4, 1/4); Network.check therefore holds every pre-activation inside (-1/4, 1/4), as IntCircuit
holds its sums inside the message space."""
import numpy as np

N = 1024
_QUARTER = 1 << 30


def sign_test_polynomial(mu):
    """the constant polynomial mu, [N] int32 (Engine.lut_batch_device's input form): +mu for a phase in [0, 1/2), -mu below"""
    return np.full(N, int(mu), np.int64).astype(np.int32)


def staircase_test_polynomial(levels, mu):
    """an odd staircase with `levels` steps on each side of 0, [N] int32: for |x| < 1/4 the output is
    sign(x) * mu * (2j + 1) / (2 levels - 1) (rounded toward zero), j = floor(|x| * 4 levels) -- mu at the top step,
    levels = 1 is sign_test_polynomial.  The polynomial is symmetric about 1/4 (tv[k] = tv[N - 1 - k]), which is what makes
    the function it computes odd.  N / 2 must be a multiple of levels."""
    levels = int(levels)
    if levels < 1 or (N // 2) % levels:
        raise ValueError(f"staircase_test_polynomial: levels = {levels} does not divide {N // 2}")
    j = np.arange(N // 2) * levels // (N // 2)
    half = (int(mu) * (2 * j + 1)) // (2 * levels - 1) if mu >= 0 else -((-int(mu) * (2 * j + 1)) // (2 * levels - 1))
    return np.concatenate((half, half[::-1])).astype(np.int64).astype(np.int32)


def _wrap32(x):
    return ((np.asarray(x, np.int64) + 2**31) % 2**32) - 2**31


def apply_test_polynomial(tv, phase):
    """what a noise-free bootstrap with test polynomial `tv` returns for Torus32 phases (any shape), in integers: the mod
    switch rounds the phase to the nearest multiple of 1 / 2N, k in [0, 2N); the result is tv[k] for k < N, -tv[k - N] above"""
    k = ((np.asarray(phase, np.int64) + (1 << 20)) >> 21) & (2 * N - 1)
    v = np.asarray(tv, np.int64)[k & (N - 1)]
    return np.where(k & N, -v, v)


def decision_boundaries(tv):
    """the phases (Torus32, int64 in [-2^31, 2^31)) at which apply_test_polynomial(tv, .) changes its value: half a grid step
    below every index k of the 2N-cycle whose value differs from its predecessor's"""
    f = np.concatenate((np.asarray(tv, np.int64), -np.asarray(tv, np.int64)))
    k = np.flatnonzero(f != np.roll(f, 1))
    return _wrap32((k << 21) - (1 << 20))


class DenseLayer:
    """rows x cols public integer weights in [-127, 127], bias [rows] Torus32 (or None), and the activation's test
    polynomial [N] int32 (None: no bootstrap -- the layer's outputs are the key-switched sums themselves)"""

    def __init__(self, weights, bias=None, activation_tv=None):
        w = np.asarray(weights)
        if w.ndim != 2 or w.size == 0 or not np.issubdtype(w.dtype, np.integer) or np.abs(w.astype(np.int64)).max() > 127:
            raise ValueError("DenseLayer: weights must be a non-empty integer matrix [rows][cols] in [-127, 127]")
        self.weights = w.astype(np.int8)
        self.rows, self.cols = w.shape
        self.bias = None if bias is None else np.asarray(bias, np.int64).astype(np.int32).reshape(self.rows)
        self.tv = None if activation_tv is None else np.asarray(activation_tv, np.int32).reshape(N)

    def pre_activation(self, values):
        """bias + W values for Torus32 input values [batch][cols] -> [batch][rows], wrapped to [-2^31, 2^31)"""
        s = np.asarray(values, np.int64) @ self.weights.astype(np.int64).T
        return _wrap32(s + (0 if self.bias is None else self.bias.astype(np.int64)))


class Network:
    """layers[0] reads the inputs x (small integers, |x| <= x_max) at x * delta_in; every later layer reads the activation
    values of the one before it, so layers[i].cols == layers[i - 1].rows, and every layer but the last needs an activation"""

    def __init__(self, layers, delta_in, x_max=1):
        self.layers = list(layers)
        if not self.layers:
            raise ValueError("Network: no layer")
        for a, b in zip(self.layers, self.layers[1:]):
            if a.tv is None or b.cols != a.rows:
                raise ValueError("Network: a layer feeds the next one through its activation, cols = the rows before it")
        self.delta_in = int(delta_in)
        self.x_max = int(x_max)
        self._images = {}

    # ---- plain evaluation: integers only -------------------------------------------------------------------------------
    def evaluate_plain(self, x, return_pre=False):
        """x [batch][cols] integers -> the last layer's outputs [batch][rows] as Torus32 values (int64): activation values,
        or the pre-activations themselves when the last layer has no activation.  return_pre: also every layer's
        pre-activations"""
        v = np.asarray(x, np.int64).reshape(-1, self.layers[0].cols) * self.delta_in
        pres = []
        for ly in self.layers:
            pre = ly.pre_activation(v)
            pres.append(pre)
            v = pre if ly.tv is None else apply_test_polynomial(ly.tv, pre)
        return (v, pres) if return_pre else v

    # ---- pricing: ranges and decision margins before anything runs -----------------------------------------------------
    def layer_sigma(self, params, lwe_key, tlwe_key, pk=None, ksk=None):
        """per layer, the predicted standard deviation [rows] (torus units) of the sample in front of the activation's mod
        switch, rounding included: sqrt(||w||^2 V_slot + V_ks + V_ms), V_slot = noise.compact_var for the fresh lists of layer
        0 (with pk: noise.linear_var_row, exact for the row, in place of ||w||^2 V_slot) and a bootstrap output's total_var +
        noise.pack_var behind a pack; and the predicted |mean| per row"""
        from . import noise
        pr = noise.predict(params, lwe_key, tlwe_key, ksk)
        out = []
        for i, ly in enumerate(self.layers):
            w = ly.weights.astype(np.float64)
            if i == 0:
                slot = noise.compact_var(params, tlwe_key, pk)
                mean = np.array([noise.linear_offset(params, pk, r, tlwe_key) for r in w]) if pk is not None else np.zeros(ly.rows)
            else:
                slot = pr["total_var"] + noise.pack_var(params, lwe_key, self.layers[i - 1].rows)
                mean = w.sum(1) * pr["total_mean"]
            if i == 0 and pk is not None:                   # fixed rows under a known key: the exact form, not its mean over rows
                lin = np.array([noise.linear_var_row(params, r, tlwe_key, pk) for r in w])
            else:
                lin = np.array([noise.linear_var(params, r, slot) for r in w])
            var = lin + pr["ks_var"] + noise.modswitch_var(lwe_key)
            out.append((np.sqrt(var), np.abs(mean + pr["ks_mean"])))
        return out

    def check(self, params, lwe_key, tlwe_key, x=None, pk=None, min_sigma=None, ksk=None):
        """Prices every layer for this key, as IntCircuit.check does, before anything runs.
        RANGE: sum_k |w_k| max|input| + |bias| must stay below 1/4 for every row (max|input| = x_max delta_in for layer 0, the
        largest activation value of the layer before otherwise); a layer that reaches 1/4 is refused (ValueError).
        MARGIN: the distance of a pre-activation to the nearest decision boundary of its activation, less the predicted
        |mean| of the noise, in predicted standard deviations (layer_sigma).  With x [batch][cols] the pre-activations are
        those of evaluate_plain and "vector_sigma" [batch] is each vector's smallest margin over all layers and rows; without
        x every value bias + s g, |s g| inside the range, g the gcd of the possible input values, is taken as reachable
        (conservative).  Layers without an activation have no margin.  min_sigma: refuse (ValueError) when the smallest
        margin is below it.  Returns {"layers": [{"range": largest bound / 2^32, "sigma": [rows], "margin_sigma": smallest
        margin of the layer}], "worst_sigma", "vector_sigma" (with x)}."""
        sig = self.layer_sigma(params, lwe_key, tlwe_key, pk, ksk)
        max_in, g = self.x_max * abs(self.delta_in), abs(self.delta_in)
        pres = None if x is None else self.evaluate_plain(x, return_pre=True)[1]
        res, vec = [], None
        for i, ly in enumerate(self.layers):
            absw = np.abs(ly.weights.astype(np.int64)).sum(1)
            bias = np.zeros(ly.rows, np.int64) if ly.bias is None else ly.bias.astype(np.int64)
            bound = absw * max_in + np.abs(bias)
            if bound.max() >= _QUARTER:
                raise ValueError(f"layer {i}: row {int(bound.argmax())} can reach {bound.max() / 2**32:.4f} >= 1/4 "
                                 f"(sum |w| = {int(absw[bound.argmax()])}, max |input| = {max_in / 2**32:.6f})")
            entry = dict(range=float(bound.max()) / 2**32, sigma=sig[i][0], margin_sigma=float("inf"))
            if ly.tv is not None:
                edges = decision_boundaries(ly.tv)
                if pres is not None:
                    cand = pres[i]                                                         # [batch][rows]
                else:
                    steps = int((absw.max() * max_in) // max(g, 1))
                    if steps > 1 << 16:
                        cand = None                                                        # no lattice to speak of: margin 0
                    else:
                        s = np.arange(-steps, steps + 1, dtype=np.int64)[:, None] * g
                        cand = np.where(np.abs(s) <= (absw * max_in)[None, :], s + bias[None, :], bias[None, :])
                if cand is None:
                    m = np.zeros((1, ly.rows))
                else:
                    d = np.abs(_wrap32(cand[..., None] - edges)).min(-1) / 2.0**32         # distance to the nearest boundary
                    m = (d - sig[i][1]) / sig[i][0]
                entry["margin_sigma"] = float(m.min())
                if pres is not None:
                    vec = m.min(1) if vec is None else np.minimum(vec, m.min(1))
                vals = np.unique(np.abs(ly.tv.astype(np.int64)))
                max_in, g = int(vals.max()), int(np.gcd.reduce(vals))
            res.append(entry)
        worst = min(e["margin_sigma"] for e in res)
        if min_sigma is not None and worst < min_sigma:
            k = int(np.argmin([e["margin_sigma"] for e in res]))
            raise ValueError(f"layer {k}: margin {worst:.2f} sigma is below min_sigma = {min_sigma}")
        out = dict(layers=res, worst_sigma=worst)
        if vec is not None:
            out["vector_sigma"] = vec
        return out

    # ---- running on one engine -----------------------------------------------------------------------------------------
    def _image(self, engine, i):
        import torch
        key = (id(engine), i)
        if key not in self._images:
            ly = self.layers[i]
            img = torch.empty(engine.weights_image_bytes(ly.rows, ly.cols), dtype=torch.uint8, device=f"cuda:{engine.device}")
            engine.weights_to_device(ly.weights, img.data_ptr())
            bias = None if ly.bias is None else torch.from_numpy(ly.bias).to(img.device)
            tv = None if ly.tv is None else torch.from_numpy(ly.tv).to(img.device)
            self._images[key] = (img, bias, tv, engine)                 # the engine is kept: its id cannot be re-used
        return self._images[key][:3]

    def run_device(self, engine, lists, stream=None, return_layers=False):
        """lists [batch][ceil(cols / N)][2][N] int32 (numpy, or a torch tensor on the engine's device) -> the last layer's
        LWE samples [batch][rows][n+1] as a torch tensor on the device, not packed.  Per layer: linear_device, then
        lut_batch_device with the activation, then (between layers) pack_device, one list per vector.  Needs the cloud key,
        and the packing key for more than one layer.  return_layers: also every layer's outputs."""
        import torch
        dev = f"cuda:{engine.device}"
        cur = lists if isinstance(lists, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(lists, np.int32)).to(dev)
        L0 = -(-self.layers[0].cols // N)
        cur = cur.reshape(-1, L0, 2, N).contiguous()
        batch, stride = cur.shape[0], engine.n + 1
        outs = []
        for i, ly in enumerate(self.layers):
            img, bias, tv = self._image(engine, i)
            lin = torch.empty((batch, ly.rows, stride), dtype=torch.int32, device=dev)
            engine.linear_device(img.data_ptr(), ly.rows, ly.cols, cur.data_ptr(), batch, None if bias is None else bias.data_ptr(),
                                 lin.data_ptr(), stream)
            out = lin
            if tv is not None:
                out = torch.empty_like(lin)
                engine.lut_batch_device(tv.data_ptr(), 1, lin.data_ptr(), out.data_ptr(), batch * ly.rows, stream)
            outs.append(out)
            if i + 1 < len(self.layers):
                Ln = -(-ly.rows // N)
                cur = torch.empty((batch, Ln, 2, N), dtype=torch.int32, device=dev)
                for b in range(batch):
                    engine.pack_device(out[b].data_ptr(), ly.rows, cur[b].data_ptr(), stream)
        return (outs[-1], outs) if return_layers else outs[-1]
