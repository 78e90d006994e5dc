"""Discretised neural networks on encrypted inputs (FHE-DiNN): dense layers with PUBLIC integer weights on
compact lists, one bootstrap per neuron as the activation.

A layer is Engine.linear_device (the weighted sums of a whole input vector, one key switch per OUTPUT), then
Engine.lut_batch_device with the activation's test polynomial, then Engine.pack_device to hand the outputs to the next layer
as a list.  Everything here is integers: inputs x_k are small integers encrypted at x_k * delta_in (PublicKey.encrypt_torus),
weights are int8 in [-127, 127], biases and activation values are Torus32 words.

A blind rotation computes an ANTI-PERIODIC function of its input phase x (f(x + 1/2) = -f(x)): coefficient k of the test
polynomial is the output on [k / 2N, (k + 1) / 2N).  The activations here are symmetric polynomials (tv[k] = tv[N - 1 - k]),
which makes f odd on (-1/4, 1/4); Network.check therefore holds every pre-activation inside (-1/4, 1/4), as IntCircuit
holds its sums inside the message space.

Convolution layers: a ConvLayer is Engine.conv_linear_device -- every shift of a public filter over a list is a
coefficient of ONE negacyclic product, so a layer costs one spectral product per (output channel, input channel) and one key
switch per output position that is kept --, the same activation, and one Engine.pack_device per (vector, channel): channel c's
activations land in slots 0 ... of list c, and the next layer is a ConvLayer on the smaller grid or a DenseLayer with
cols = channels * N (pad_dense_weights).

Dense layers on LWE samples (opt-in): with hidden="lwe" a DenseLayer behind a DenseLayer is
Engine.lwe_matmul_device on the LUT outputs before it -- no pack, no packing key, no key switch behind the sum, and an error of
exactly sum_k w_k e_k (noise.lwe_linear_var); Network.run_device_samples runs layer 0 that way too, on LWE inputs."""
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
        # what a Network reads of any layer: outputs per vector, the columns the packed outputs occupy in front of the next
        # layer (output k in slot k mod N of list k / N), and the filled slots of such a list
        self.n_out, self.out_cols, self.pack_filled = self.rows, self.rows, self.rows

    def pre_activation(self, values):
        """bias + W values for Torus32 input values [batch][cols] -> [batch][rows], wrapped to [-2^31, 2^31)"""
        s = np.asarray(values, np.int64) @ self.weights.astype(np.int64).T
        return _wrap32(s + (0 if self.bias is None else self.bias.astype(np.int64)))

    def per_output(self, per_row):
        """a quantity per weight row -> per output: a dense layer has one output per row"""
        return np.asarray(per_row)

    def packed_values(self, act):
        """activation values [batch][n_out] -> the values [batch][out_cols] the next layer reads behind the pack"""
        return act

    def fresh_offset(self, params, pk, tlwe_key):
        """predicted mean error per output on FRESH lists under one public key (noise.linear_offset), [n_out] torus units"""
        from . import noise
        return np.array([noise.linear_offset(params, pk, r, tlwe_key) for r in self.weights.astype(np.float64)])


def conv2d_weights(kernel, width):
    """kernel [cout][cin][kh][kw] integers in [-127, 127] -> ConvLayer weights [cout][cin * N] int8 for images stored row-major,
    `width` pixels per row, one list per channel (height * width <= N): tap (i, j) sits at i * width + j of its channel"""
    k = np.asarray(kernel)
    if k.ndim != 4 or k.size == 0 or not np.issubdtype(k.dtype, np.integer) or np.abs(k.astype(np.int64)).max() > 127:
        raise ValueError("conv2d_weights: kernel must be a non-empty integer array [cout][cin][kh][kw] in [-127, 127]")
    cout, cin, kh, kw = k.shape
    width = int(width)
    if kw > width or (kh - 1) * width + kw > N:
        raise ValueError(f"conv2d_weights: a {kh} x {kw} filter on rows of {width} pixels does not fit one list of {N} slots")
    w = np.zeros((cout, cin, N), np.int8)
    at = (np.arange(kh)[:, None] * width + np.arange(kw)[None, :]).reshape(-1)
    w[:, :, at] = k.reshape(cout, cin, kh * kw)
    return w.reshape(cout, cin * N)


def conv_slots(height, width, kh, kw, stride=1):
    """the valid output positions of a kh x kw filter on a height x width image (row-major, height * width <= N), row-major:
    slot y * width + x for y = 0, stride, ... <= height - kh and x = 0, stride, ... <= width - kw"""
    height, width, kh, kw, stride = (int(v) for v in (height, width, kh, kw, stride))
    if min(height, width, kh, kw, stride) < 1 or kh > height or kw > width or height * width > N:
        raise ValueError(f"conv_slots: a {kh} x {kw} filter on a {height} x {width} image (at most {N} pixels)")
    y, x = np.arange(0, height - kh + 1, stride), np.arange(0, width - kw + 1, stride)
    return (y[:, None] * width + x[None, :]).reshape(-1).astype(np.int64)


def pad_dense_weights(weights, channels, per_channel):
    """dense weights [rows][channels * per_channel] on a ConvLayer's outputs (channel-major) -> [rows][channels * N] for the
    packed layout: column c * per_channel + i moves to c * N + i"""
    w = np.asarray(weights)
    channels, per_channel = int(channels), int(per_channel)
    if w.ndim != 2 or w.shape[1] != channels * per_channel or not 1 <= per_channel <= N:
        raise ValueError(f"pad_dense_weights: weights must be [rows][{channels} * {per_channel}] with at most {N} per channel")
    out = np.zeros((w.shape[0], channels, N), w.dtype)
    out[:, :, :per_channel] = w.reshape(w.shape[0], channels, per_channel)
    return out.reshape(w.shape[0], channels * N)


class ConvLayer:
    """cout x (cin * N) public integer taps in [-127, 127] (weights[r][l * N + k] = tap k of the filter from input channel l
    to output channel r; conv2d_weights), the slots kept of EVERY output channel (conv_slots), bias [cout] Torus32 (or None)
    and the activation's test polynomial (None: no bootstrap).  Output (r, i) = bias[r] + sum_l sum_k w[r][l N + k]
    x_l[slots[i] + k], negacyclically (a term past slot N - 1 enters negated); the cout * len(slots) outputs of a vector
    are ordered channel-major."""

    def __init__(self, weights, slots_per_channel, bias=None, activation_tv=None):
        w = np.asarray(weights)
        if w.ndim != 2 or w.size == 0 or w.shape[1] % N or not np.issubdtype(w.dtype, np.integer) or np.abs(w.astype(np.int64)).max() > 127:
            raise ValueError(f"ConvLayer: weights must be a non-empty integer matrix [cout][cin * {N}] in [-127, 127]")
        t = np.asarray(slots_per_channel)
        if t.ndim != 1 or t.size == 0 or not np.issubdtype(t.dtype, np.integer) or t.min() < 0 or t.max() >= N:
            raise ValueError(f"ConvLayer: slots_per_channel must be a non-empty vector of slots in [0, {N})")
        self.weights = w.astype(np.int8)
        self.rows, self.cols = w.shape
        self.cin = self.cols // N
        self.slots = t.astype(np.int64)
        self.bias = None if bias is None else np.asarray(bias, np.int64).astype(np.int32).reshape(self.rows)
        self.tv = None if activation_tv is None else np.asarray(activation_tv, np.int32).reshape(N)
        self.n_out, self.out_cols, self.pack_filled = self.rows * t.size, self.rows * N, t.size

    def pad_input(self, x):
        """inputs [batch][cin][m] (m <= N values per channel, e.g. height * width pixels) -> [batch][cin * N], zeros behind:
        the layout Network.evaluate_plain and PublicKey.encrypt_torus (one list per channel) take"""
        x = np.asarray(x, np.int64).reshape(-1, self.cin, np.shape(x)[-1])
        out = np.zeros((x.shape[0], self.cin, N), np.int64)
        out[:, :, :x.shape[2]] = x
        return out.reshape(x.shape[0], -1)

    def slot_table(self):
        """the public slot table of Engine.conv_linear_device, channel-major: entry r * len(slots) + i = r * N + slots[i]"""
        return (np.arange(self.rows)[:, None] * N + self.slots[None, :]).reshape(-1).astype(np.uint32)

    def correlate(self, values):
        """sum_l sum_k w[r][l N + k] values_l[slots[i] + k], negacyclically, for values [batch][cin * N] of any number type
        -> [batch][rows][len(slots)] in that type's arithmetic (int64 for integers: not wrapped)"""
        v = np.asarray(values)
        v = v.astype(np.int64 if np.issubdtype(v.dtype, np.integer) else np.float64).reshape(-1, self.cin, N)
        out = np.zeros((v.shape[0], self.rows, self.slots.size), v.dtype)
        for r in range(self.rows):
            nz = np.flatnonzero(self.weights[r])
            l, k = nz // N, nz % N
            at = self.slots[:, None] + k[None, :]                                          # [slots][taps]
            wk = np.where(at >= N, -1, 1) * self.weights[r, nz].astype(v.dtype)[None, :]
            out[:, r] = (v[:, l[None, :], at % N] * wk).sum(-1)
        return out

    def pre_activation(self, values):
        """Torus32 input values [batch][cin * N] -> [batch][rows * len(slots)], channel-major, wrapped to [-2^31, 2^31)"""
        s = self.correlate(np.asarray(values, np.int64))
        if self.bias is not None:
            s = s + self.bias.astype(np.int64)[None, :, None]
        return _wrap32(s).reshape(s.shape[0], -1)

    def per_output(self, per_row):
        """a quantity per output channel -> per output (channel-major)"""
        return np.repeat(np.asarray(per_row), self.slots.size)

    def packed_values(self, act):
        """activation values [batch][n_out] -> [batch][rows * N]: channel r's values in slots 0 ... of list r, zeros behind"""
        a = np.asarray(act, np.int64).reshape(-1, self.rows, self.slots.size)
        out = np.zeros((a.shape[0], self.rows, N), np.int64)
        out[:, :, :self.slots.size] = a
        return out.reshape(a.shape[0], -1)

    def fresh_offset(self, params, pk, tlwe_key):
        """predicted mean error per output on FRESH lists under one public key: the correlation of the taps with
        noise.compact_offset (= noise.linear_offset of noise.conv_row(w[r], slot)), [n_out] torus units"""
        from . import noise
        off = noise.compact_offset(tlwe_key, pk)
        return self.correlate(np.tile(off, self.cin)[None, :])[0].reshape(-1)


class Network:
    """layers[0] reads the inputs x (small integers, |x| <= x_max) at x * delta_in; every later layer reads the activation
    values of the one before it, so layers[i].cols == layers[i - 1].rows, and every layer but the last needs an activation.
    Layers are DenseLayer or ConvLayer in any order: behind a ConvLayer of cout channels the next layer has cols = cout * N
    (channel c's outputs in slots 0 ... of list c)."""

    def __init__(self, layers, delta_in, x_max=1):
        self.layers = list(layers)
        if not self.layers:
            raise ValueError("Network: no layer")
        for a, b in zip(self.layers, self.layers[1:]):
            if a.tv is None or b.cols != a.out_cols:
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
            if ly is not self.layers[-1]:
                v = ly.packed_values(v)
        return (v, pres) if return_pre else v

    # ---- pricing: ranges and decision margins before anything runs -----------------------------------------------------
    def _lwe_link(self, i, hidden, input_var=None):
        """whether layer i reads LWE samples through Engine.lwe_matmul_device: layer 0 when the inputs are
        samples (input_var given), a DenseLayer behind a DenseLayer under hidden="lwe".  A link behind a ConvLayer keeps the
        pack: its next layer reads padded list columns."""
        if hidden not in ("pack", "lwe"):
            raise ValueError(f"hidden must be 'pack' or 'lwe', got {hidden!r}")
        if i == 0:
            return input_var is not None
        return hidden == "lwe" and isinstance(self.layers[i], DenseLayer) and isinstance(self.layers[i - 1], DenseLayer)

    def layer_sigma(self, params, lwe_key, tlwe_key, pk=None, ksk=None, hidden="pack", input_var=None):
        """per layer, the predicted standard deviation [rows] (torus units) of the sample in front of the activation's mod
        switch, rounding included: sqrt(||w||^2 V_slot + V_ks + V_ms), V_slot = noise.compact_var for the fresh lists of layer
        0 (with pk: noise.linear_var_row, exact for the row, in place of ||w||^2 V_slot) and a bootstrap output's total_var +
        noise.pack_var behind a pack; and the predicted |mean| per row.  A ConvLayer is priced per output channel -- every slot
        of a channel has the channel's ||taps||^2 (with pk: linear_var_row of the channel's row, the same for every slot, since
        noise.conv_row only multiplies the weight polynomial by a power of X) -- and its arrays are per output, channel-major;
        on layer 0 with pk the |mean| of a slot is the correlation of the taps with noise.compact_offset.
        hidden="lwe": a DenseLayer behind a DenseLayer reads the LUT outputs themselves (Engine.lwe_matmul_device): slot
        variance total_var with no pack_var, no key switch behind the sum (neither ks_var nor ks_mean), mean
        w.sum(1) total_mean -- noise.lwe_linear_var.  input_var (run_device_samples): layer 0 reads LWE samples of that
        variance and zero mean, priced the same way; None: fresh lists, as above."""
        from . import noise
        pr = noise.predict(params, lwe_key, tlwe_key, ksk)
        out = []
        for i, ly in enumerate(self.layers):
            w = ly.weights.astype(np.float64)
            if self._lwe_link(i, hidden, input_var):
                slot = float(input_var) if i == 0 else pr["total_var"]
                mean = np.zeros(ly.n_out) if i == 0 else w.sum(1) * pr["total_mean"]
                lin = np.array([noise.lwe_linear_var(r, slot) for r in w])
                out.append((np.sqrt(lin + noise.modswitch_var(lwe_key)), np.abs(mean)))
                continue
            if i == 0:
                slot = noise.compact_var(params, tlwe_key, pk)
                mean = ly.fresh_offset(params, pk, tlwe_key) if pk is not None else np.zeros(ly.n_out)
            else:
                slot = pr["total_var"] + noise.pack_var(params, lwe_key, self.layers[i - 1].pack_filled)
                mean = ly.per_output(w.sum(1) * pr["total_mean"])
            if i == 0 and pk is not None:                   # fixed rows under a known key: the exact form, not its mean over rows
                lin = np.array([noise.linear_var_row(params, r, tlwe_key, pk) for r in w])
            else:
                lin = np.array([noise.linear_var(params, r, slot) for r in w])
            var = ly.per_output(lin + pr["ks_var"] + noise.modswitch_var(lwe_key))
            out.append((np.sqrt(var), np.abs(mean + pr["ks_mean"])))
        return out

    def check(self, params, lwe_key, tlwe_key, x=None, pk=None, min_sigma=None, ksk=None, hidden="pack", input_var=None):
        """Prices every layer for this key, as IntCircuit.check does, before anything runs.
        RANGE: sum_k |w_k| max|input| + |bias| must stay below 1/4 for every row (max|input| = x_max delta_in for layer 0, the
        largest activation value of the layer before otherwise); a layer that reaches 1/4 is refused (ValueError).
        MARGIN: the distance of a pre-activation to the nearest decision boundary of its activation, less the predicted
        |mean| of the noise, in predicted standard deviations (layer_sigma).  With x [batch][cols] the pre-activations are
        those of evaluate_plain and "vector_sigma" [batch] is each vector's smallest margin over all layers and rows; without
        x every value bias + s g, |s g| inside the range, g the gcd of the possible input values, is taken as reachable
        (conservative).  Layers without an activation have no margin.  min_sigma: refuse (ValueError) when the smallest
        margin is below it.  Returns {"layers": [{"range": largest bound / 2^32, "sigma": [rows], "margin_sigma": smallest
        margin of the layer}], "worst_sigma", "vector_sigma" (with x)}.  hidden and input_var: the route the network will run
        (run_device(hidden=...), run_device_samples), as layer_sigma takes them."""
        sig = self.layer_sigma(params, lwe_key, tlwe_key, pk, ksk, hidden=hidden, input_var=input_var)
        max_in, g = self.x_max * abs(self.delta_in), abs(self.delta_in)
        pres = None if x is None else self.evaluate_plain(x, return_pre=True)[1]
        res, vec = [], None
        for i, ly in enumerate(self.layers):
            absw = ly.per_output(np.abs(ly.weights.astype(np.int64)).sum(1))
            bias = ly.per_output(np.zeros(ly.rows, np.int64) if ly.bias is None else ly.bias.astype(np.int64))
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
                    m = np.zeros((1, ly.n_out))
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

    def _slots(self, engine, i):
        """the device slot table of ConvLayer i (validated once, at this load)"""
        import torch
        key = (id(engine), i, "slots")
        if key not in self._images:
            table = self.layers[i].slot_table()
            d = torch.empty(table.size, dtype=torch.int32, device=f"cuda:{engine.device}")
            engine.conv_slots_to_device(table, self.layers[i].rows, d.data_ptr())
            self._images[key] = (d, engine)
        return self._images[key][0]

    def _lwe_image(self, engine, i):
        """the matrix-core operand image of DenseLayer i (Engine.lwe_weights_to_device), its bias and its activation"""
        import torch
        key = (id(engine), i, "lwe")
        if key not in self._images:
            ly = self.layers[i]
            img = torch.empty(engine.lwe_weights_image_bytes(ly.rows, ly.cols), dtype=torch.uint8, device=f"cuda:{engine.device}")
            engine.lwe_weights_to_device(ly.weights, img.data_ptr())
            bias = None if ly.bias is None else torch.from_numpy(ly.bias).to(img.device)
            tv = None if ly.tv is None else torch.from_numpy(ly.tv).to(img.device)
            self._images[key] = (img, bias, tv, engine)
        return self._images[key][:3]

    def run_device_samples(self, engine, cts, stream=None, return_layers=False):
        """cts [batch][cols][n+1] int32 (numpy, or a torch tensor on the engine's device): LWE samples of the messages
        x_k * delta_in (eoc_lwe_encrypt, or Engine.seeded_expand_device for the integer encodings) -> the last layer's LWE
        samples [batch][rows][n+1].  Every layer is Engine.lwe_matmul_device on samples -- layer 0 on the inputs, every later
        one on the LUT outputs before it -- then lut_batch_device: no list, no packing key, no key switch behind a sum.
        DenseLayer-only networks (ValueError otherwise).  Price it with check(..., hidden="lwe", input_var=...): a fresh
        sample's variance is params.ks_stdev ** 2.  return_layers: also every layer's outputs and the tensors the layers read."""
        import torch
        if not all(isinstance(ly, DenseLayer) for ly in self.layers):
            raise ValueError("run_device_samples: DenseLayer-only networks (a ConvLayer reads compact lists)")
        dev = f"cuda:{engine.device}"
        cur = cts if isinstance(cts, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(cts, np.int32)).to(dev)
        cur = cur.reshape(-1, self.layers[0].cols, engine.n + 1).contiguous()
        return self._run(engine, cur, True, "lwe", stream, return_layers)

    def run_device(self, engine, lists, stream=None, return_layers=False, hidden="pack"):
        """lists [batch][ceil(cols / N)][2][N] int32 (numpy, or a torch tensor on the engine's device) -> the last layer's
        LWE samples [batch][rows][n+1] as a torch tensor on the device, not packed.  Per layer: linear_device, then
        lut_batch_device with the activation, then (between layers) pack_device, one list per vector.  A ConvLayer runs
        conv_linear_device instead ([batch][n_out][n+1], channel-major) and is packed with one call per (vector, channel).
        Needs the cloud key, and the packing key for more than one layer.  return_layers: also every layer's outputs.
        hidden="lwe": a DenseLayer behind a DenseLayer runs as lwe_matmul_device on the LUT outputs before it -- no pack_device
        call, no key switch behind the sum; a network whose links are all of that kind needs no packing key -- and
        return_layers gives (last, outputs per layer, the tensor every layer read)."""
        import torch
        self._lwe_link(0, hidden)
        dev = f"cuda:{engine.device}"
        cur = lists if isinstance(lists, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(lists, np.int32)).to(dev)
        L0 = -(-self.layers[0].cols // N)
        cur = cur.reshape(-1, L0, 2, N).contiguous()
        return self._run(engine, cur, False, hidden, stream, return_layers)

    def _run(self, engine, cur, samples_in, hidden, stream, return_layers):
        import torch
        dev = f"cuda:{engine.device}"
        batch, stride = cur.shape[0], engine.n + 1
        outs, ins = [], []
        for i, ly in enumerate(self.layers):
            lwe = self._lwe_link(i, hidden, 0.0 if samples_in else None)
            img, bias, tv = self._lwe_image(engine, i) if lwe else self._image(engine, i)
            conv = isinstance(ly, ConvLayer)
            lin = torch.empty((batch, ly.n_out, stride), dtype=torch.int32, device=dev)
            d_bias = None if bias is None else bias.data_ptr()
            ins.append(cur)
            if lwe:
                engine.lwe_matmul_device(img.data_ptr(), ly.rows, ly.cols, cur.data_ptr(), stride, batch, d_bias, lin.data_ptr(), stream)
            elif conv:
                engine.conv_linear_device(img.data_ptr(), ly.rows, ly.cols, cur.data_ptr(), batch, d_bias,
                                          self._slots(engine, i).data_ptr(), ly.n_out, lin.data_ptr(), stream)
            else:
                engine.linear_device(img.data_ptr(), ly.rows, ly.cols, cur.data_ptr(), batch, d_bias, lin.data_ptr(), stream)
            out = lin
            if tv is not None:
                out = torch.empty_like(lin)
                engine.lut_batch_device(tv.data_ptr(), 1, lin.data_ptr(), out.data_ptr(), batch * ly.n_out, stream)
            outs.append(out)
            if i + 1 < len(self.layers) and self._lwe_link(i + 1, hidden):
                cur = out                                                   # [batch][rows][n+1]: the next layer's samples
            elif i + 1 < len(self.layers):
                Ln = -(-ly.out_cols // N)
                cur = torch.empty((batch, Ln, 2, N), dtype=torch.int32, device=dev)
                for b in range(batch):
                    if conv:
                        for c in range(ly.rows):
                            engine.pack_device(out[b, c * ly.pack_filled].data_ptr(), ly.pack_filled, cur[b, c].data_ptr(), stream)
                    else:
                        engine.pack_device(out[b].data_ptr(), ly.rows, cur[b].data_ptr(), stream)
        if not return_layers:
            return outs[-1]
        return (outs[-1], outs) if hidden == "pack" and not samples_in else (outs[-1], outs, ins)
