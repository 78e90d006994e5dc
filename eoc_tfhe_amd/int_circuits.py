"""Integer circuits: netlists of linear stages and table lookups on small encrypted integers.

IntCircuit records nodes of the eoc_inode format (include/eoc_tfhe_gpu.h) on wire handles, tracks for every wire its
message space p and an inclusive range [lo, hi] of the messages it can carry, and checks the two preconditions a lookup has:

  range   the linear stage's value must stay inside [0, p - 1]: a phase in the negacyclic half [p, 2p) comes out of the blind
          rotation as -f(m - p).  Violations are ValueErrors of the call that creates the node (allow_padding=True: the
          caller uses that half on purpose);
  noise   1/(4p) must be many standard deviations of the linear stage's noise plus the mod switch's rounding:
          IntCircuit.check prices every bootstrapped node with the model of eoc_tfhe_amd.noise.

Messages are in the integer encoding of SecretKey.encrypt_ints (m at phase m / (2p)).  Nothing here computes on
ciphertexts: run() sends the netlist to eoc_int_circuit_run (the global context), Engine.int_circuit_run_device takes
nodes() and test_polynomials() directly.
"""
from fractions import Fraction

import numpy as np

MAX_TERMS = 4
BIT = "bit"           # message space of a bit_out wire: a gate-bootstrap sample (+-1/8), not an integer-encoded one


def units(k, p):
    """k message steps at message space p as a Torus32 constant: k 2^32 / (2p), wrapped to int32"""
    v = (int(k) << 32) // (2 * int(p)) & 0xFFFFFFFF
    return v - (1 << 32) if v >= 1 << 31 else v


def _torus(values, p_out):
    return np.array([((int(v) % p_out) << 32) // (2 * p_out) for v in values], np.uint64).astype(np.uint32).view(np.int32)


def _torus_bits(values):
    return np.array([(1 << 29) if v else -(1 << 29) for v in values], np.int64).astype(np.int32)


class IntCircuit:
    """Deferred integer nodes, in the style of Circuit:

        c = IntCircuit()
        a, b = c.input(4, max_value=1), c.input(4, max_value=1)
        s, k = c.lut_many([a, b], [lambda m: m % 2, lambda m: m // 2], 4, 4)     # one blind rotation, two outputs
        c.check(params, sk.lwe_key, sk.tlwe_key)["worst_sigma"]
        wires = c.run({a: cts_a, b: cts_b})

    `terms` is a list of wires or (weight, wire) pairs, at most four; `cst` is a Torus32 constant (units(k, p) for k
    message steps)."""

    def __init__(self):
        self._nodes, self._tables, self._meta, self._wires, self.inputs = [], [], [], [], []

    # ---- wires -----------------------------------------------------------------------------------------------------
    @property
    def n_wires(self):
        return len(self._wires)

    def _new_wire(self, p, lo, hi, kind, node=None):
        self._wires.append(dict(p=p, lo=lo, hi=hi, kind=kind, node=node))
        return len(self._wires) - 1

    def wire_range(self, w):
        """(p, lo, hi) of a wire"""
        i = self._wires[w]
        return i["p"], i["lo"], i["hi"]

    def input(self, p, max_value=None, fresh=False):
        """an input wire at message space p carrying messages in [0, max_value]; fresh: a fresh encryption (noise ks_stdev)
        instead of a bootstrap output"""
        if p not in (2, 4, 8):
            raise ValueError(f"input: message space p = {p} is not one of 2, 4, 8")
        hi = p - 1 if max_value is None else int(max_value)
        if not 0 <= hi <= p - 1:
            raise ValueError(f"input: max_value = {hi} outside [0, {p - 1}]")
        w = self._new_wire(p, 0, hi, "fresh" if fresh else "boot")
        self.inputs.append(w)
        return w

    # ---- nodes -----------------------------------------------------------------------------------------------------
    def _terms(self, what, terms, p=None):
        ts = [(1, t) if np.isscalar(t) else (int(t[0]), int(t[1])) for t in terms]
        if not 1 <= len(ts) <= MAX_TERMS:
            raise ValueError(f"{what}: {len(ts)} terms, a node takes 1 to {MAX_TERMS}")
        for _, w in ts:
            if not 0 <= w < self.n_wires:
                raise ValueError(f"{what}: wire {w} does not exist")
        ps = {self._wires[w]["p"] for _, w in ts}
        if BIT in ps:
            raise ValueError(f"{what}: a bit_out wire is a gate-bootstrap sample, not an operand of an integer node")
        if len(ps) != 1 or (p is not None and ps != {p}):
            raise ValueError(f"{what}: terms at message spaces {sorted(ps)}; the terms of one node share p"
                             + (f" = {p}" if p is not None else ""))
        return ts, ps.pop()

    def _interval(self, ts, cst, p):
        c = Fraction(int(cst) * 2 * p, 1 << 32)
        lo = sum(w * (self._wires[x]["lo"] if w > 0 else self._wires[x]["hi"]) for w, x in ts) + c
        hi = sum(w * (self._wires[x]["hi"] if w > 0 else self._wires[x]["lo"]) for w, x in ts) + c
        return lo, hi

    def _emit(self, T, out, tv, ts, cst, **meta):
        from . import INode
        q = INode()
        q.n_tables, q.out, q.tv, q.n_terms, q.cst = T, out, tv, len(ts), int(cst)
        for k, (w, x) in enumerate(ts):
            q.in_[k], q.w[k] = x, w
        self._nodes.append(q)
        self._meta.append(dict(T=T, out=out, terms=ts, cst=int(cst), **meta))
        return len(self._nodes) - 1

    def lin(self, terms, cst=0):
        """free node (no bootstrap): sum_k w_k x_k + cst.  Its range may leave [0, p - 1]; the lookup that reads it is
        what has to hold."""
        ts, p = self._terms("lin", terms)
        lo, hi = self._interval(ts, cst, p)
        out = self._new_wire(p, lo, hi, "free", len(self._nodes))
        self._emit(0, out, 0, ts, cst, p=p)
        return out

    def _lookup(self, what, terms, fs, p, p_out, cst, allow_padding, bits):
        ts, p = self._terms(what, terms, p)
        T = len(fs)
        if T not in (1, 2, 4, 8) or p * T > 16:
            raise ValueError(f"{what}: (p, T) = ({p}, {T}) is not supported (T in 1, 2, 4, 8 and p T <= 16)")
        if not bits and p_out not in (2, 4, 8):
            raise ValueError(f"{what}: output message space p_out = {p_out} is not one of 2, 4, 8")
        lo, hi = self._interval(ts, cst, p)
        name = f"node {len(self._nodes)} ({what})"
        range_ok = lo >= 0 and hi <= p - 1
        if not range_ok and not allow_padding:
            raise ValueError(f"{name}: the linear stage ranges over [{lo}, {hi}], a lookup at p = {p} needs [0, {p - 1}] "
                             f"(allow_padding=True if the negacyclic half is meant)")
        dom = range(p) if not range_ok else range(int(np.floor(lo)), int(np.ceil(hi)) + 1)
        tab = np.stack([_torus_bits([f(m) for m in range(p)]) if bits else _torus([f(m) for m in range(p)], p_out) for f in fs])
        tv = len(self._tables)
        self._tables.append(tab)
        node = len(self._nodes)
        outs = []
        for f in fs:
            if bits:
                outs.append(self._new_wire(BIT, 0, 1, "boot", node))
            else:   # the padding half returns -f: any residue
                outs.append(self._new_wire(p_out, 0, max(int(f(m)) % p_out for m in dom) if range_ok else p_out - 1, "boot", node))
        self._emit(T, outs[0], tv, ts, cst, p=p, p_out=BIT if bits else p_out, fs=list(fs), range_ok=range_ok, name=name)
        return outs

    def lut(self, terms, f, p, p_out, cst=0, allow_padding=False):
        """one bootstrap: f(sum_k w_k x_k + cst) mod p_out, f: Z_p -> Z"""
        return self._lookup("lut", terms, [f], p, p_out, cst, allow_padding, False)[0]

    def lut_many(self, terms, fs, p, p_out, cst=0, allow_padding=False):
        """one blind rotation, T = len(fs) in 2, 4, 8 outputs (many-LUT bootstrapping, p T <= 16): list of T wires"""
        if len(fs) < 2:
            raise ValueError("lut_many: takes 2, 4 or 8 functions; lut takes one")
        return self._lookup("lut_many", terms, list(fs), p, p_out, cst, allow_padding, False)

    def lut_bit_out(self, terms, f, p, cst=0, allow_padding=False):
        """as lut, the table holding +-2^29: a gate-bootstrap sample of the bit f(.) != 0, for the gate circuits"""
        return self._lookup("lut_bit_out", terms, [f], p, None, cst, allow_padding, True)[0]

    def lut_many_bit_out(self, terms, fs, p, cst=0, allow_padding=False):
        """as lut_many, the tables holding +-2^29"""
        if len(fs) < 2:
            raise ValueError("lut_many_bit_out: takes 2, 4 or 8 functions")
        return self._lookup("lut_many_bit_out", terms, list(fs), p, None, cst, allow_padding, True)

    # ---- what the engine takes -------------------------------------------------------------------------------------
    def nodes(self):
        """the netlist: list of INode (eoc_inode)"""
        return list(self._nodes)

    def tables(self):
        """per test polynomial, [T][p] Torus32 output values (the `tables` of int_circuit_run)"""
        return [t.copy() for t in self._tables]

    def test_polynomials(self):
        """[n_tv][N] int32: the nodes' test polynomials (lut_test_polynomial / lut_many_test_polynomial)"""
        from . import N, lut_many_test_polynomial, lut_test_polynomial
        tv = [lut_test_polynomial(t.shape[1], t[0]) if t.shape[0] == 1 else lut_many_test_polynomial(t.shape[1], t)
              for t in self._tables]
        return np.stack(tv) if tv else np.zeros((0, N), np.int32)

    def levels(self):
        """(level of every node, bootstrap levels, blind rotations per instance): int_netlist_levels of this netlist"""
        from . import int_netlist_levels
        return int_netlist_levels(self._nodes, self.n_wires, len(self._tables))

    # ---- plain evaluation ------------------------------------------------------------------------------------------
    def evaluate_plain(self, inputs):
        """the messages every wire carries for the input messages `inputs` ({wire: int or array}, or a sequence in input
        order): list indexed by wire.  Values are phases in steps of 1/(2p): a linear stage that lands in [p, 2p) gives
        -f(m - p), as the blind rotation does, and that output is the step 2 p_out - f (decrypt_ints reads it mod p_out);
        inputs may be given in [0, 2p) likewise.  Constants must be whole message steps."""
        if not isinstance(inputs, dict):
            inputs = dict(zip(self.inputs, inputs))
        val = [None] * self.n_wires
        for w in self.inputs:
            val[w] = np.asarray(inputs[w], np.int64)
        for q in self._meta:
            p = q["p"]
            c = Fraction(q["cst"] * 2 * p, 1 << 32)
            if c.denominator != 1:
                raise ValueError(f"evaluate_plain: the constant {q['cst']} is not a whole number of steps at p = {p}")
            m = sum(w * val[x] for w, x in q["terms"]) + int(c)
            if q["T"] == 0:
                val[q["out"]] = m
                continue
            m = np.asarray(m) % (2 * p)
            neg, idx = m >= p, m % p
            for j, f in enumerate(q["fs"]):
                fv = np.array([int(f(x)) for x in range(p)], np.int64)[idx]
                if q["p_out"] == BIT:
                    val[q["out"] + j] = np.where(neg, 1 - (fv != 0), fv != 0).astype(np.int64)
                else:
                    fv = fv % q["p_out"]
                    val[q["out"] + j] = np.where(neg, (2 * q["p_out"] - fv) % (2 * q["p_out"]), fv)
        return val

    # ---- the checker -----------------------------------------------------------------------------------------------
    def check(self, params, lwe_key, tlwe_key):
        """Prices every bootstrapped node for this key: {"nodes": {node index: (range_ok, margin_sigma)}, "worst": node
        index, "worst_sigma": its margin, "wire_var": predicted variance per wire}.  margin_sigma = (1/(4p)) /
        sqrt(sum_k w_k^2 V(in_k) + modswitch_var(lwe_key, T)) (noise.lut_margin_sigma_var), with V = ks_stdev^2 for a fresh
        input, noise.predict()['total_var'] for any bootstrap output and sum w^2 V behind a free node.  Refuses nothing."""
        from . import noise
        v_out = noise.predict(params, lwe_key, tlwe_key)["total_var"]
        var = [0.0] * self.n_wires
        for w in self.inputs:
            var[w] = float(params.ks_stdev) ** 2 if self._wires[w]["kind"] == "fresh" else v_out
        res = {}
        for k, q in enumerate(self._meta):
            v_in = sum(w * w * var[x] for w, x in q["terms"])
            if q["T"] == 0:
                var[q["out"]] = v_in
                continue
            for j in range(q["T"]):
                var[q["out"] + j] = v_out
            res[k] = (q["range_ok"], noise.lut_margin_sigma_var(q["p"], q["T"], v_in, lwe_key))
        worst = min(res, key=lambda k: res[k][1]) if res else None
        return dict(nodes=res, worst=worst, worst_sigma=res[worst][1] if res else float("inf"), wire_var=var)

    def node_outputs(self, k):
        """the wires node k writes"""
        q = self._meta[k]
        return list(range(q["out"], q["out"] + max(1, q["T"])))

    # ---- running ---------------------------------------------------------------------------------------------------
    def run(self, inputs, min_sigma=None, params=None, lwe_key=None, tlwe_key=None):
        """Runs the circuit on the global context (int_circuit_run): inputs {wire: samples [instances][n+1]} (or a sequence
        in input order) -> wires [n_wires][instances][n+1].  min_sigma: raise ValueError when check(params, lwe_key,
        tlwe_key) prices a node below it (the three are then required)."""
        from . import int_circuit_run
        if min_sigma is not None:
            if params is None or lwe_key is None or tlwe_key is None:
                raise ValueError("run: min_sigma needs params, lwe_key and tlwe_key for the checker")
            chk = self.check(params, lwe_key, tlwe_key)
            if chk["worst_sigma"] < min_sigma:
                raise ValueError(f"{self._meta[chk['worst']]['name']}: margin {chk['worst_sigma']:.2f} sigma is below "
                                 f"min_sigma = {min_sigma}")
        if not isinstance(inputs, dict):
            inputs = dict(zip(self.inputs, inputs))
        first = np.asarray(inputs[self.inputs[0]])
        wires = np.zeros((self.n_wires,) + first.shape, np.int32)
        for w in self.inputs:
            wires[w] = inputs[w]
        return int_circuit_run(self._nodes, self._tables, wires)


# ---- radix builders ---------------------------------------------------------------------------------------------------
# Margins are IntCircuit.check on key seed 1 of each default set (they move by a few hundredths of a sigma between keys).
def radix_add(c, A, B, carry_in=None):
    """A + B on base-2 digits at p = 4 (least significant first): s_i = a_i + b_i + c_i in [0, 3] and ONE T = 2 node per
    digit gives (s mod 2, s div 2) -- DESIGN.md 10.1's adder: n bootstraps on n levels for n digits.  Returns (sum digits,
    carry out).  check: 7.36 sigma on Set A, 8.02 on Set B per digit (three bootstrapped inputs at
    p = 4, T = 2: noise.lut_margin_sigma(..., 4, 2, inputs=3)); the carry-less first digit 8.46 / 8.95."""
    if len(A) != len(B) or not A:
        raise ValueError("radix_add: A and B are non-empty digit lists of one length")
    carry, out = carry_in, []
    for a, b in zip(A, B):
        s, carry = c.lut_many([a, b] if carry is None else [a, b, carry], [lambda m: m % 2, lambda m: m // 2], 4, 4)
        out.append(s)
    return out, carry


def bit_function2(c, a, b, f):
    """any f: {0, 1}^2 -> {0, 1} of two bits at p = 4 as ONE lookup of 2a + b.  check: 6.50 sigma on
    Set A, 7.70 on Set B (sum of w^2 = 5, T = 1)."""
    return c.lut([(2, a), (1, b)], lambda m: int(f(m >> 1, m & 1)), 4, 4)


def radix_less_than(c, A, B):
    """A < B on base-2 digits at p = 4 (least significant first), one T = 1 lookup per digit, n levels: with lt_0 = 0,
    x_i = b_i - a_i + lt_i + 1 in [0, 3] and lt_(i+1) = [x_i >= 2] (b_i > a_i decides, b_i = a_i keeps the lower digits'
    verdict).  Returns the wire of lt_n.  check: 8.25 sigma on Set A, 9.64 on Set B per digit (sum of w^2 = 3, T = 1);
    the first digit 9.89 / 11.40."""
    if len(A) != len(B) or not A:
        raise ValueError("radix_less_than: A and B are non-empty digit lists of one length")
    lt = None
    for a, b in zip(A, B):
        lt = c.lut([(1, b), (-1, a)] + ([] if lt is None else [(1, lt)]), lambda m: int(m >= 2), 4, 4, cst=units(1, 4))
    return lt
