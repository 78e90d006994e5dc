"""The steps of tests/test_gpu_interleave.py: one class per device call family, all of them on ONE engine with ONE
key set (cloud key, packing key, public key) at LWE dimension 40; the schedules that interleave them; and the Runner that queues
a schedule window on a stream and compares every position's words with the family's reference.

A step states, per input set k in (0, 1) and width in ("narrow", "wide"): its host inputs (make), the read-only device inputs
(device), its outputs (outputs: every schedule position gets buffers of its own, poisoned, with a guard row behind them; an
accumulating or in-place output starts from a private copy of its initial words), the call on a given engine and stream, and the
reference words (ref) -- from the helpers the family's own test module uses.  Nothing here computes a reference of its own.

The schedule part (schedule, mode_plan, header_entries) is pure Python and checked by tests/test_interleave_cpu.py."""
import os
import re

import numpy as np

import automaton_oracle as ao
import capture_cases as cc
import cmux_oracle as cx
import compact_oracle as co
import conv_oracle as cv
import dot_oracle as do
import int_circuit_oracle as ico
import leveled_round_oracle as lro
import lut2_oracle as l2
import lut_many_oracle as lmo
import lut_oracle as lo
import lut_tree_oracle as lt
import oracle_lib as ol
import pack_oracle as po
import table_update_oracle as tu
import tv_pack_exact_oracle as tpe

N = 1024
POISON = cc.POISON
SEED = cc.SEED
WIDTHS = ("narrow", "wide")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCHEDULE_SEEDS = {"A": 101, "B": 202, "A-sliced": 303}          # the engine configurations of tests/test_gpu_interleave.py
GLOBAL_SEED = 404                                               # its host-buffer schedule
FULL_SEED = 505                                                 # its full-size cycles
BOTH_SETS = frozenset({"mixed"})                                # the steps whose two input sets the schedules draw (the rest: set 0)


# ---- the schedules (pure Python) ------------------------------------------------------------------------------------------------
def euler_circuit(F, rng):
    """a closed walk over vertices 0 .. F-1 that uses every ordered pair (a, b), a = b included, exactly once: Hierholzer on the
    complete directed graph with one loop per vertex (in-degree = out-degree = F everywhere), neighbours in a seeded order"""
    nxt = [list(rng.permutation(F)) for _ in range(F)]
    stack, walk = [int(rng.integers(0, F))], []
    while stack:
        v = stack[-1]
        if nxt[v]:
            stack.append(int(nxt[v].pop()))
        else:
            walk.append(stack.pop())
    return walk[::-1]


def schedule(names, seed):
    """[(family, input set, width)] of len(names)^2 + 1 calls: every ordered pair of families is adjacent once, and every
    family's widths begin narrow, wide, narrow (the scratch grows mid-sequence; the next narrow call finds it too large and
    full of the wide call's words); the rest of the widths are drawn.  The calls take input set 0: the steps state a second
    input set, the schedules leave it out, which halves the references -- but for the steps of BOTH_SETS,
    whose second set is another path through the engine"""
    rng = np.random.default_rng(seed)
    walk = euler_circuit(len(names), rng)
    seen, out = {}, []
    for v in walk:
        j = seen.get(v, 0)
        seen[v] = j + 1
        width = ("narrow", "wide", "narrow")[j] if j < 3 else WIDTHS[int(rng.integers(0, 2))]
        out.append((names[v], int(rng.integers(0, 2)) if names[v] in BOTH_SETS else 0, width))
    return out


def mode_plan(sched, leveled, every=5):
    """the leveled-rounding mode in force at every position: it flips ahead of every `every`-th leveled position, so the
    switches lie between leveled calls of different families and widths"""
    mode, seen, out = False, 0, []
    for name, _, _ in sched:
        if name in leveled:
            seen += 1
            if seen % every == 0:
                mode = not mode
        out.append(mode)
    return out


def switches(plan):
    return sum(1 for a, b in zip(plan, plan[1:]) if a != b)


def header_entries(path=None):
    """every eoc_*_device( declaration of the public header with an eoc_engine * and a hip_stream parameter"""
    text = open(path or os.path.join(ROOT, "include", "eoc_tfhe_gpu.h")).read()
    found = []
    for m in re.finditer(r"\bint\s+(eoc_\w+_device)\s*\(([^;{]*)\)\s*;", text):
        if re.search(r"eoc_engine\s*\*", m.group(2)) and "hip_stream" in m.group(2):
            found.append(m.group(1))
    return found


# device entries of the header that are no step, each with its reason
EXCLUDED = {
    "eoc_dbg_fft_fwd_device": "debug transform: reads and writes caller buffers only, no engine state",
    "eoc_dbg_fft_inv_device": "debug transform: reads and writes caller buffers only, no engine state",
    "eoc_dbg_chacha20_blocks_device": "debug stream generator: writes a caller buffer only",
    "eoc_weights_to_device": "model load: writes the caller's image only (the steps build their images with it)",
    "eoc_conv_slots_to_device": "slot-table load: writes the caller's table only (the steps build their tables with it)",
}


# ---- keys -------------------------------------------------------------------------------------------------------------------
class KeySet:
    """one key set at LWE dimension n: the secret key, the oracle with the same keys, the packing key (blob, rows, spectra), the
    public key, and a helper engine WITHOUT keys for what only prepares inputs (selector conversion, weight images, slot tables).
    seeded: the cloud key is the seeded export's expansion -- a fresh encryption of the same secret key, so other words."""

    def __init__(self, eoc, pset, seed, n=40, seeded=False):
        self.eoc, self.pset, self.seed, self.seeded = eoc, pset, seed, seeded
        p = eoc.default_params(pset)
        p.n = n
        self.p, self.n = p, n
        self.sk = eoc.SecretKey(p, seed)
        self.orc = ol.Oracle(pset, seed, n_override=n, with_bk=not seeded)
        if seeded:
            self.cloud_blob = self.sk.seeded_cloud_key_bytes()
            bk, ksk = eoc.seeded_cloud_key_expand(self.cloud_blob)
            self.orc.bk, self.orc.ksk = np.ascontiguousarray(bk, np.int32), np.ascontiguousarray(ksk, np.int32)
            self.orc.bkfft = np.zeros((n, self.orc.kpl, 2, N), np.float64)
            self.orc.L.orc_bk_to_fft(ol.C.byref(self.orc.p), self.orc.bk, self.orc.bkfft)
        co.ksk(self.orc)
        self.blob = self.sk.packing_key_bytes()
        self.pk_rows = po.blob_rows(self.blob, n)
        self.kfft = po.key_fft(self.pk_rows)
        self._finish()

    def _finish(self):
        self.pk = self.eoc.PublicKey(self.sk.public_key_bytes())
        self.op, self.kpl = cx.orc_params(self.p), 2 * self.p.l
        self._aux = None

    @classmethod
    def shared(cls, eoc, pset):
        """the full-size key set the family modules share (lut2_oracle.keys; test_gpu_cmux.keys and test_gpu_pack.keys use
        the same seed): nothing is generated twice"""
        self = cls.__new__(cls)
        self.eoc, self.pset, self.seed, self.seeded = eoc, pset, l2.KEY_SEED, False
        self.p, self.sk, self.blob, self.kfft, self.orc = l2.keys(eoc, pset)
        self.n = self.p.n
        self.pk_rows = po.blob_rows(self.blob, self.n)
        self._finish()
        return self

    @property
    def aux(self):
        if self._aux is None:
            with cc.knobs({}):
                self._aux = self.eoc.Engine(self.p)
        return self._aux

    def close(self):
        """closes the helper engine, where one was made"""
        if self._aux is not None:
            self._aux.close()
            self._aux = None

    def install(self, eng):
        if self.seeded:
            eng.load_seeded_cloud_key(self.cloud_blob)
        else:
            eng.load_cloud_key(self.sk)
        eng.load_packing_key(self.blob)


def _seed(*parts):
    """a reproducible 31-bit seed of a step's name, input set and width"""
    h = 0
    for c in "/".join(str(p) for p in parts):
        h = (h * 131 + ord(c)) % (2**31 - 1)
    return h + 1


# ---- the step protocol ------------------------------------------------------------------------------------------------------
class Step:
    name = None
    covers = ()                 # the header's device entries this step calls
    leveled = False             # governed by the leveled-rounding mode
    keyed = False               # in the key swap: its words depend on a derived key image
    sliced_by = None            # the launch counter that counts this family's slices, where it has one
    shape = {}                  # width -> the family's own shape tuple
    full = None                 # the wide shape on the full-size key set, where the reference's cost grows with n
    in_place = ()               # outputs that start from initial words (accumulating or in place): no all-poison check
    host_form = None            # the family's host-buffer call on the global context, where it has one

    def __init__(self, ks):
        self.ks, self.eoc, self._host, self._want = ks, ks.eoc, {}, {}

    def rng(self, *parts):
        return np.random.default_rng(_seed(self.name, *parts))

    def host(self, k, width):
        if (k, width) not in self._host:
            shape = self.full if width == "wide" and self.full is not None and self.ks.n > 40 else self.shape[width]
            self._host[(k, width)] = self.make(k, width, *shape)
        return self._host[(k, width)]

    def want(self, k, width, rounding=False):
        key = (k, width, bool(rounding) and self.leveled)
        if key not in self._want:
            self._want[key] = self.ref(self.host(k, width), key[2])
        return self._want[key]

    def device(self, h):
        """read-only device inputs: every array of h named in h['dev']"""
        from gpu_util import to_dev
        return {name: to_dev(np.ascontiguousarray(h[name])) for name in h["dev"]}

    # make(k, width, *shape) -> h; outputs(h) -> {name: (shape, 'i32' | 'f64', initial words or None)};
    # call(eng, d, o, h, st); ref(h, rounding) -> {name: words}


def convert(ks, sel):
    import test_gpu_cmux as tc
    return tc.convert(ks.aux, sel)


# ---- gates ------------------------------------------------------------------------------------------------------------------
class Gate(Step):
    """one two-input opcode; wide: 150 rows, a full key-switch tile and a partly filled one"""
    name, covers, keyed, sliced_by = "gate", ("eoc_gate_batch_device",), True, "br"
    op, nin = "NAND", 2
    shape, full = dict(narrow=(5,), wide=(150,)), (17,)

    def make(self, k, width, S):
        rng = self.rng(k, width)
        h = dict(S=S, dev=[f"in{a}" for a in range(self.nin)])
        for a in range(self.nin):
            h[f"in{a}"] = self.ks.sk.encrypt_bits(rng.integers(0, 2, S).astype(np.uint8), _seed(self.name, k, width, a))
        return h

    def outputs(self, h):
        return dict(out=((h["S"], self.ks.n + 1), "i32", None))

    def call(self, eng, d, o, h, st):
        eng.gate_batch_device(self.eoc.OPS[self.op], d["in0"].data_ptr(), d["in1"].data_ptr(),
                              d["in2"].data_ptr() if self.nin == 3 else None, o["out"].data_ptr(), h["S"], stream=st)

    def ref(self, h, rounding):
        return dict(out=self.ks.orc.gate_batch(ol.OPS[self.op], *[h[f"in{a}"] for a in range(self.nin)]))


class Mux(Gate):
    """a MUX level: 2 S jobs; wide: S = 70, two partly filled key-switch tiles of 140 rows"""
    name, op, nin = "mux", "MUX", 3
    shape, full = dict(narrow=(3,), wide=(70,)), (9,)


class Mixed(Gate):
    """an opcode per row (the `ops` argument): more than 15 opcode runs at the wide width, the gather path through d_mixed and
    h_perm.  Input set 1 takes the opcodes of input set 0 in reverse order: another permutation through h_perm, but the same
    opcode counts and runs, so a call's counters depend on the width alone.  The schedules draw both sets for this step"""
    name, keyed = "mixed", False
    OPCODES = ("NAND", "AND", "OR", "NOR", "XOR", "XNOR")

    def make(self, k, width, S):
        h = Gate.make(self, k, width, S)
        ops = self.rng(width).choice(np.array([self.eoc.OPS[o] for o in self.OPCODES], np.uint8), S)
        h["ops"] = np.ascontiguousarray(ops[::-1]) if k else ops
        return h

    def call(self, eng, d, o, h, st):
        eng.gate_batch_device(0, d["in0"].data_ptr(), d["in1"].data_ptr(), None, o["out"].data_ptr(), h["S"], ops=h["ops"], stream=st)

    def ref(self, h, rounding):
        return dict(out=self.ks.orc.gate_batch(0, h["in0"], h["in1"], ops=h["ops"]))


class Circuit(Step):
    """circuit_run on wires of the position's own: NAND, MUX, XOR, AND, then XOR and NAND of their outputs"""
    name, covers, sliced_by, in_place = "circuit", ("eoc_circuit_run_device",), "br", ("wires",)
    shape, full = dict(narrow=(2,), wide=(40,)), (5,)
    N_WIRES = 9

    def gates(self):
        G, O = self.eoc.Gate, ol.OPS
        return [G(O["NAND"], 0, 1, -1, 3), G(O["MUX"], 0, 1, 2, 4), G(O["XOR"], 1, 2, -1, 5), G(O["AND"], 0, 2, -1, 6),
                G(O["XOR"], 4, 6, -1, 7), G(O["NAND"], 3, 5, -1, 8)]

    def make(self, k, width, S):
        rng = self.rng(k, width)
        wires = np.full((self.N_WIRES, S, self.ks.n + 1), POISON, np.uint32).view(np.int32)
        for w in range(3):
            wires[w] = self.ks.sk.encrypt_bits(rng.integers(0, 2, S).astype(np.uint8), _seed(self.name, k, width, w))
        return dict(S=S, wires=wires, gates=self.gates(), dev=[])

    def outputs(self, h):
        return dict(wires=(h["wires"].shape, "i32", h["wires"]))

    def call(self, eng, d, o, h, st):
        eng.circuit_run_device(h["gates"], o["wires"].data_ptr(), self.N_WIRES, h["S"], stream=st)

    def ref(self, h, rounding):
        from test_gpu_circuits import _oracle_run
        return dict(wires=_oracle_run(self.ks.orc, h["gates"], h["wires"]))


class BlindRotateKeyswitch(Step):
    """stand-alone blind_rotate, then keyswitch of OTHER rows than the ones the rotation just left in W.d_u: the copies out of
    and into W.d_u (a key switch that skipped its copy would still find the rotation's rows there)"""
    name, covers, keyed, sliced_by = "br-ks", ("eoc_blind_rotate_device", "eoc_keyswitch_device"), True, "br"
    shape, full = dict(narrow=(4,), wide=(140,)), (9,)

    def make(self, k, width, rows):
        rng = self.rng(k, width)
        return dict(rows=rows, t=cc.rand_i32(rng, (rows, self.ks.n + 1)), v=cc.rand_i32(rng, (rows, N + 1)), dev=["t", "v"])

    def outputs(self, h):
        return dict(u=((h["rows"], N + 1), "i32", None), out=((h["rows"], self.ks.n + 1), "i32", None))

    def call(self, eng, d, o, h, st):
        eng.blind_rotate_device(d["t"].data_ptr(), o["u"].data_ptr(), h["rows"], stream=st)
        eng.keyswitch_device(d["v"].data_ptr(), o["out"].data_ptr(), h["rows"], stream=st)

    def ref(self, h, rounding):
        u = np.stack([self.ks.orc.blind_rotate_extract(t) for t in h["t"]])
        return dict(u=u, out=np.stack([self.ks.orc.keyswitch(x) for x in h["v"]]))


# ---- table lookups ----------------------------------------------------------------------------------------------------------
class Lut(Step):
    """p = 4, 2 tables"""
    name, covers, keyed, sliced_by = "lut", ("eoc_lut_batch_device",), True, "br"
    shape, full = dict(narrow=(3,), wide=(70,)), (9,)

    def make(self, k, width, rows):
        import test_gpu_lut as tl
        tv = np.stack([self.eoc.lut_test_polynomial(4, t) for t in tl.tables_for(4)[1][:2]])
        return dict(rows=rows, tv=tv, x=tl.inputs(self.eoc, self.ks.sk, 4, rows, _seed(self.name, k, width))[1], dev=["tv", "x"])

    def outputs(self, h):
        return dict(out=((2, h["rows"], self.ks.n + 1), "i32", None))

    def call(self, eng, d, o, h, st):
        eng.lut_batch_device(d["tv"].data_ptr(), 2, d["x"].data_ptr(), o["out"].data_ptr(), h["rows"], stream=st)

    def ref(self, h, rounding):
        return dict(out=lo.lut_batch(self.ks.orc, h["tv"], h["x"]))


class LutMany(Lut):
    """T = 2, p = 2, 2 polynomials"""
    name, covers, keyed = "lut-many", ("eoc_lut_many_batch_device",), False
    T = 2

    def make(self, k, width, rows):
        import test_gpu_lut_many as tm
        tv = tm.packed(self.eoc, 2, tm.tables_for(self.T, 2, 2)[1])
        return dict(rows=rows, tv=tv, x=tm.inputs(self.eoc, self.ks.sk, 2, rows, _seed(self.name, k, width))[1], dev=["tv", "x"])

    def outputs(self, h):
        return dict(out=((2 * self.T, h["rows"], self.ks.n + 1), "i32", None))

    def call(self, eng, d, o, h, st):
        eng.lut_many_batch_device(self.T, d["tv"].data_ptr(), 2, d["x"].data_ptr(), o["out"].data_ptr(), h["rows"], stream=st)

    def ref(self, h, rounding):
        return dict(out=lmo.lut_many_batch(self.ks.orc, h["tv"], h["x"], self.T).reshape(2 * self.T, h["rows"], self.ks.n + 1))


class LutEnc(Step):
    """blind rotation from encrypted polynomials, one list per (group, row), 2 groups"""
    name, covers, sliced_by = "lut-enc", ("eoc_lut_enc_batch_device",), "br"
    shape, full = dict(narrow=(2,), wide=(70,)), (9,)

    def make(self, k, width, rows):
        import test_gpu_lut as tl
        return dict(rows=rows, lists=cc.rand_i32(self.rng(k, width), (2, rows, 2, N)),
                    y=tl.inputs(self.eoc, self.ks.sk, 4, rows, _seed(self.name, k, width))[1], dev=["lists", "y"])

    def outputs(self, h):
        return dict(out=((2, h["rows"], self.ks.n + 1), "i32", None))

    def call(self, eng, d, o, h, st):
        eng.lut_enc_batch_device(d["lists"].data_ptr(), 2, True, d["y"].data_ptr(), o["out"].data_ptr(), h["rows"], stream=st)

    def ref(self, h, rounding):
        return dict(out=l2.lut_enc_batch(self.ks.orc, h["lists"], h["y"], True))


class Lut2(Step):
    """p = 2, T = 2, both functions of lut2_oracle.functions: level 1, the pack and level 2 in one call"""
    name, covers, keyed, sliced_by = "lut2", ("eoc_lut2_batch_device",), True, "pack_launches"
    shape, full = dict(narrow=(2,), wide=(9,)), (5,)
    pm, T = 2, 2

    def make(self, k, width, rows):
        rng, pm = self.rng(k, width), self.pm
        tv0 = np.stack([self.eoc.lut2_test_polynomials(pm, l2.lut2_tables(f, pm), self.T) for f in l2.functions(pm)])
        x = self.ks.sk.encrypt_ints(rng.integers(0, pm, rows).astype(np.uint8), pm, _seed(self.name, k, width, "x"))
        y = self.ks.sk.encrypt_ints(rng.integers(0, pm, rows).astype(np.uint8), pm, _seed(self.name, k, width, "y"))
        return dict(rows=rows, tv0=tv0, tv=tv0.reshape(-1, N).copy(), x=x, y=y, dev=["tv", "x", "y"])

    def outputs(self, h):
        return dict(out=((2, h["rows"], self.ks.n + 1), "i32", None))

    def call(self, eng, d, o, h, st):
        eng.lut2_batch_device(self.pm, self.T, d["tv"].data_ptr(), 2, d["x"].data_ptr(), d["y"].data_ptr(), o["out"].data_ptr(),
                              h["rows"], stream=st)

    def ref(self, h, rounding):
        return dict(out=l2.lut2_batch(self.ks.orc, self.ks.kfft, self.pm, self.T, h["tv0"], h["x"], h["y"]))


class LutTree(Step):
    """p = 2, d = 3, T = 1, both functions of test_gpu_lut_tree.functions: three levels and two exact packs in one call"""
    name, covers, keyed, sliced_by = "lut-tree", ("eoc_lut_tree_batch_device",), True, "pack_launches"
    shape, full = dict(narrow=(2,), wide=(20,)), (3,)
    pm, d, T = 2, 3, 1

    def make(self, k, width, rows):
        import test_gpu_lut_tree as tt
        rng = self.rng(k, width)
        xs = rng.integers(0, self.pm, (self.d, rows)).astype(np.uint8)
        digits = np.stack([self.ks.sk.encrypt_ints(xs[j], self.pm, _seed(self.name, k, width, j)) for j in range(self.d)])
        return dict(rows=rows, tv0=tt.polynomials(self.eoc, self.pm, self.d, self.T), digits=digits, dev=["tv0", "digits"])

    def outputs(self, h):
        return dict(out=((2, h["rows"], self.ks.n + 1), "i32", None))

    def call(self, eng, d, o, h, st):
        eng.lut_tree_batch_device(self.pm, self.d, self.T, d["tv0"].data_ptr(), 2, d["digits"].data_ptr(), o["out"].data_ptr(),
                                  h["rows"], stream=st)

    def ref(self, h, rounding):
        return dict(out=lt.lut_tree_batch(self.ks.orc, self.ks.pk_rows, self.pm, self.d, self.T, h["tv0"], h["digits"]))


class IntCircuit(Step):
    """the two-level netlist of capture_cases.IntCircuit on wires of the position's own"""
    name, covers, sliced_by, in_place = "int-circuit", ("eoc_int_circuit_run_device",), "br", ("wires",)
    shape, full = dict(narrow=(2,), wide=(7,)), (5,)

    def netlist(self):
        if not hasattr(self, "c"):
            c, x = cc.int_netlist(self.eoc)
            self.c, self.x, self.nodes, self.tv = c, x, c.nodes(), c.test_polynomials()
        return self.c

    def make(self, k, width, rows):
        import test_gpu_int_circuit as ti
        c = self.netlist()
        wires = ti.circuit_inputs(self.eoc, self.ks.sk, c, self.x, rows, _seed(self.name, k, width) % 2**30)[1]
        return dict(rows=rows, wires=wires, tv=self.tv, dev=["tv"])

    def outputs(self, h):
        return dict(wires=(h["wires"].shape, "i32", h["wires"]))

    def call(self, eng, d, o, h, st):
        eng.int_circuit_run_device(self.nodes, d["tv"].data_ptr(), self.tv.shape[0], o["wires"].data_ptr(), self.c.n_wires, h["rows"],
                                   stream=st)

    def ref(self, h, rounding):
        return dict(wires=ico.run(self.ks.orc, self.nodes, self.tv, h["wires"]))


# ---- compact lists and seeded forms -----------------------------------------------------------------------------------------
class CompactExpand(Step):
    """the first `count` slots of public-key encrypted lists -> ordinary samples"""
    name, covers, keyed, sliced_by = "compact-expand", ("eoc_compact_expand_device",), True, "ks_mfma_launches"
    shape, full = dict(narrow=(5,), wide=(200,)), (20,)

    def make(self, k, width, count):
        bits = self.rng(k, width).integers(0, 2, N).astype(np.uint8)
        return dict(count=count, lists=self.ks.pk.encrypt_bits(bits, enc_seed=_seed(self.name, k, width)), dev=["lists"])

    def outputs(self, h):
        return dict(out=((h["count"], self.ks.n + 1), "i32", None))

    def call(self, eng, d, o, h, st):
        eng.compact_expand_device(d["lists"].data_ptr(), h["count"], o["out"].data_ptr(), stream=st)

    def ref(self, h, rounding):
        return dict(out=co.expand(self.ks.orc, h["lists"], np.arange(h["count"])))


class SeededExpand(Step):
    """bodies under a public seed, stream indices that cross 2^32 inside the call"""
    name, covers, sliced_by = "seeded-expand", ("eoc_seeded_expand_device",), None
    shape = dict(narrow=(5,), wide=(300,))
    first = 2**32 - 5

    def make(self, k, width, count):
        return dict(count=count, bodies=cc.rand_i32(self.rng(k, width), count), dev=["bodies"])

    def outputs(self, h):
        return dict(out=((h["count"], self.ks.n + 1), "i32", None))

    def call(self, eng, d, o, h, st):
        eng.seeded_expand_device(SEED, d["bodies"].data_ptr(), h["count"], o["out"].data_ptr(), self.first, stream=st)

    def ref(self, h, rounding):
        return dict(out=self.eoc.seeded_expand_host(self.ks.p, SEED, h["bodies"], self.first))


class TgswToFft(Step):
    """selectors in torus form -> the converted form; the reference is the oracle's transform (an exact 2^-9 apart)"""
    name, covers = "tgsw-to-fft", ("eoc_tgsw_to_fft_device",)
    shape = dict(narrow=(1,), wide=(5,))

    def torus(self, k, width, count):
        bits = self.rng(k, width).integers(0, 2, count)
        return self.ks.sk.encrypt_selector_bits(bits, enc_seed=_seed(self.name, k, width))

    def make(self, k, width, count):
        sel = self.torus(k, width, count)
        return dict(count=count, sel=sel, torus=sel, dev=["sel"])

    def outputs(self, h):
        return dict(out=((h["count"], self.ks.kpl, 2, N), "f64", None))

    def call(self, eng, d, o, h, st):
        eng.tgsw_to_fft_device(d["sel"].data_ptr(), h["count"], o["out"].data_ptr(), stream=st)

    def ref(self, h, rounding):
        return dict(out=(cx.to_fft(h["torus"]) * 2.0**-9).reshape(h["count"], self.ks.kpl, 2, N))


class TgswSeededToFft(TgswToFft):
    """seeded selectors: the masks regenerated on the device, then the conversion"""
    name, covers = "tgsw-seeded-to-fft", ("eoc_tgsw_seeded_to_fft_device",)
    shape = dict(narrow=(1,), wide=(3,))
    first = 3

    def make(self, k, width, count):
        bits = self.rng(k, width).integers(0, 2, count)
        key = bytes((_seed(self.name, k, width, j) & 0xFF) for j in range(32))
        bodies = self.ks.sk.encrypt_selector_bits_seeded(bits, key, SEED, first_idx=self.first)[1]
        return dict(count=count, bodies=bodies, torus=self.eoc.tgsw_seeded_expand_host(self.ks.p, SEED, bodies, self.first), dev=["bodies"])

    def call(self, eng, d, o, h, st):
        eng.tgsw_seeded_to_fft_device(SEED, d["bodies"].data_ptr(), h["count"], o["out"].data_ptr(), self.first, stream=st)


# ---- leveled calls ----------------------------------------------------------------------------------------------------------
class Leveled(Step):
    leveled = True

    def selectors(self, h, sel):
        """adds the reference form and (at device()) the converted form of selectors in torus form"""
        h["sel"], h["fft"] = sel, cx.to_fft(sel)

    def device(self, h):
        d = Step.device(self, h)
        if h["sel"].size:
            d["fft"] = convert(self.ks, h["sel"])
        return d


class Cmux(Leveled):
    """one selector per item; 3 items: one workgroup of two and a remainder; 9: more workgroups"""
    name, covers = "cmux", ("eoc_cmux_device",)
    shape = dict(narrow=(3,), wide=(9,))

    def make(self, k, width, count):
        rng = self.rng(k, width)
        h = dict(count=count, a=cc.rand_i32(rng, (count, 2, N)), b=cc.rand_i32(rng, (count, 2, N)), dev=["a", "b"])
        self.selectors(h, self.ks.sk.encrypt_selector_bits(rng.integers(0, 2, count), enc_seed=_seed(self.name, k, width)))
        return h

    def outputs(self, h):
        return dict(out=((h["count"], 2, N), "i32", None))

    def call(self, eng, d, o, h, st):
        eng.cmux_device(d["fft"].data_ptr(), d["a"].data_ptr(), d["b"].data_ptr(), o["out"].data_ptr(), h["count"], stream=st)

    def ref(self, h, rounding):
        f = lro.cmux if rounding else cx.cmux
        return dict(out=np.stack([f(self.ks.op, h["fft"][q], h["a"][q], h["b"][q]) for q in range(h["count"])]))


class Demux(Cmux):
    """storing: out0 = in - E, out1 = E"""
    name, covers = "demux", ("eoc_demux_device",)
    accumulate = False

    def outputs(self, h):
        return dict(out0=((h["count"], 2, N), "i32", None), out1=((h["count"], 2, N), "i32", None))

    def call(self, eng, d, o, h, st):
        eng.demux_device(d["fft"].data_ptr(), d["a"].data_ptr(), o["out0"].data_ptr(), o["out1"].data_ptr(), h["count"],
                         accumulate=self.accumulate, stream=st)

    def ref(self, h, rounding):
        f = lro.demux if rounding else tu.demux
        r = [f(self.ks.op, h["fft"][q], h["a"][q]) for q in range(h["count"])]
        return dict(out0=np.stack([x[0] for x in r]), out1=np.stack([x[1] for x in r]))


class DemuxAccumulate(Demux):
    """accumulating into base words of the position's own: the reference adds the storing form's words"""
    name, accumulate, in_place = "demux-accumulate", True, ("out0", "out1")

    def make(self, k, width, count):
        h = Demux.make(self, k, width, count)
        rng = self.rng(k, width, "base")
        h["base"] = [cc.rand_i32(rng, (count, 2, N)) for _ in range(2)]
        return h

    def outputs(self, h):
        return dict(out0=((h["count"], 2, N), "i32", h["base"][0]), out1=((h["count"], 2, N), "i32", h["base"][1]))

    def ref(self, h, rounding):
        r = Demux.ref(self, h, rounding)
        return {name: tu.wrap_i32(h["base"][j].astype(np.int64) + r[name]) for j, name in enumerate(("out0", "out1"))}


class TableRead(Leveled):
    """entries of 256 slots; narrow: 2 lists, 2 queries (one tree stage); wide: 4 lists, 5 queries -- a walk one level deeper,
    which ends on the other ping-pong buffer"""
    name, covers, keyed, sliced_by = "table-read", ("eoc_table_read_device",), True, "cmux_launches"
    shape, full = dict(narrow=(1, 8, 2), wide=(2, 8, 5)), (2, 8, 3)

    def make(self, k, width, d, lw, queries):
        import test_gpu_cmux as tc
        rng = self.rng(k, width)
        depth = d + 10 - lw
        h = dict(d=d, lw=lw, queries=queries, table=tc.make_table(self.eoc, self.ks.pk, "ints", d, rng, _seed(self.name, k, width, "t"))[0],
                 dev=["table"])
        idx = [(1 << depth) - 1, 0] + [int(v) for v in rng.integers(0, 1 << depth, max(queries - 2, 0))]
        self.selectors(h, tc.index_selectors(self.ks.sk, idx[:queries], depth, enc_seed=_seed(self.name, k, width, "s")))
        return h

    def outputs(self, h):
        return dict(out=((h["queries"], 1 << h["lw"], self.ks.n + 1), "i32", None))

    def call(self, eng, d, o, h, st):
        eng.table_read_device(d["table"].data_ptr(), h["d"], h["lw"], d["fft"].data_ptr(), h["queries"], o["out"].data_ptr(), stream=st)

    def ref(self, h, rounding):
        f = lro.table_read if rounding else cx.table_read
        return dict(out=f(self.ks.orc, self.ks.op, h["table"], h["d"], h["lw"], h["fft"])[0])


class TableUpdate(TableRead):
    """table[idx_q] += value_q on a table of the position's own; two queries hit one entry at the wide width"""
    name, covers, keyed, sliced_by, in_place = "table-update", ("eoc_table_update_device",), False, "demux_launches", ("table",)

    def make(self, k, width, d, lw, queries):
        import test_gpu_cmux as tc
        rng = self.rng(k, width)
        depth = d + 10 - lw
        h = dict(d=d, lw=lw, queries=queries, table=cc.rand_i32(rng, (1 << d, 2, N)), vals=cc.rand_i32(rng, (queries, 2, N)), dev=["vals"])
        idx = [(1 << depth) - 1, 0] + [int(v) for v in rng.integers(0, 1 << depth, max(queries - 2, 0))]
        idx[-1] = idx[0]
        self.selectors(h, tc.index_selectors(self.ks.sk, idx[:queries], depth, enc_seed=_seed(self.name, k, width, "s")))
        return h

    def outputs(self, h):
        return dict(table=(h["table"].shape, "i32", h["table"]))

    def call(self, eng, d, o, h, st):
        eng.table_update_device(o["table"].data_ptr(), h["d"], h["lw"], d["fft"].data_ptr(), d["vals"].data_ptr(), h["queries"], stream=st)

    def ref(self, h, rounding):
        f = lro.table_update if rounding else tu.table_update
        return dict(table=f(self.ks.op, h["table"], h["d"], h["lw"], h["fft"], h["vals"]))


AUTO_TRANS = np.array([[1, 1, 2, 0], [1, 0, 0, N + 1], [0, 2, 2, 1]], np.int32)


class AutomatonRun(Leveled):
    """a 3-state automaton over encrypted bit strings, 4 slots per start state"""
    name, covers, sliced_by = "automaton-run", ("eoc_automaton_run_device",), "automaton_launches"
    shape = dict(narrow=(2, (2, 0), 2), wide=(3, (2, 0, 1), 9))
    lw = 2

    def make(self, k, width, steps, starts, queries):
        rng = self.rng(k, width)
        h = dict(steps=steps, starts=list(starts), queries=queries, final=cc.rand_i32(rng, (len(AUTO_TRANS), 2, N)), dev=["final"])
        sel = self.ks.sk.encrypt_selector_bits(rng.integers(0, 2, queries * steps), enc_seed=_seed(self.name, k, width))
        self.selectors(h, sel)
        h["fft"] = h["fft"].reshape(queries, steps, self.ks.kpl, 2, N)
        return h

    def outputs(self, h):
        return dict(out=((h["queries"], len(h["starts"]), 1 << self.lw, self.ks.n + 1), "i32", None))

    def call(self, eng, d, o, h, st):
        eng.automaton_run_device(AUTO_TRANS, d["final"].data_ptr(), d["fft"].data_ptr(), h["steps"], h["starts"], self.lw,
                                 o["out"].data_ptr(), h["queries"], stream=st)

    def ref(self, h, rounding):
        f = lro.run if rounding else ao.run
        return dict(out=f(self.ks.orc, self.ks.op, AUTO_TRANS, h["final"], h["fft"], h["starts"], self.lw)[0])


class AutomatonStep(Leveled):
    """one backward step for every state and query from one shared state vector (prev_query_stride = 0)"""
    name, covers = "automaton-step", ("eoc_automaton_step_device",)
    shape = dict(narrow=(2,), wide=(9,))

    def make(self, k, width, queries):
        rng = self.rng(k, width)
        h = dict(queries=queries, prev=cc.rand_i32(rng, (len(AUTO_TRANS), 2, N)), dev=["prev"])
        self.selectors(h, self.ks.sk.encrypt_selector_bits(rng.integers(0, 2, queries), enc_seed=_seed(self.name, k, width)))
        return h

    def outputs(self, h):
        return dict(next=((h["queries"], len(AUTO_TRANS), 2, N), "i32", None))

    def call(self, eng, d, o, h, st):
        eng.automaton_step_device(AUTO_TRANS, d["prev"].data_ptr(), 0, d["fft"].data_ptr(), 1, o["next"].data_ptr(), h["queries"], stream=st)

    def ref(self, h, rounding):
        f = lro.step if rounding else ao.step
        return dict(next=np.stack([f(self.ks.op, AUTO_TRANS, h["prev"], h["fft"][q]) for q in range(h["queries"])]))


# ---- packing ----------------------------------------------------------------------------------------------------------------
class Pack(Step):
    """samples -> compact lists; wide: N + 3 samples, two lists, the second with 3 slots"""
    name, covers, keyed, sliced_by = "pack", ("eoc_pack_device",), True, "pack_launches"
    shape = dict(narrow=(5,), wide=(N + 3,))

    def make(self, k, width, count):
        bits = self.rng(k, width).integers(0, 2, count).astype(np.uint8)
        return dict(count=count, x=self.ks.sk.encrypt_bits(bits, _seed(self.name, k, width)), dev=["x"])

    def outputs(self, h):
        return dict(out=(((h["count"] + N - 1) // N, 2, N), "i32", None))

    def call(self, eng, d, o, h, st):
        eng.pack_device(d["x"].data_ptr(), h["count"], o["out"].data_ptr(), stream=st)

    def ref(self, h, rounding):
        return dict(out=po.pack(self.ks.n, self.ks.kfft, h["x"]))


class TvPack(Step):
    """p = 4, 2 functions: rows x 4 values -> one encrypted test polynomial per (function, row)"""
    name, covers, keyed, sliced_by = "tv-pack", ("eoc_tv_pack_device",), True, "pack_launches"
    shape, full = dict(narrow=(2,), wide=(9,)), (5,)
    pm, F = 4, 2

    def make(self, k, width, rows):
        vals = self.rng(k, width).integers(0, self.pm, self.F * self.pm * rows).astype(np.uint8)
        x = self.ks.sk.encrypt_ints(vals, self.pm, _seed(self.name, k, width)).reshape(self.F, self.pm, rows, self.ks.n + 1)
        return dict(rows=rows, x=x, dev=["x"])

    def outputs(self, h):
        return dict(out=((self.F, h["rows"], 2, N), "i32", None))

    def call(self, eng, d, o, h, st):
        eng.tv_pack_device(self.pm, d["x"].data_ptr(), self.F, h["rows"], o["out"].data_ptr(), stream=st)

    def ref(self, h, rounding):
        return dict(out=l2.tv_pack(self.ks.n, self.ks.kfft, h["x"], self.pm))


class TvPackExact(TvPack):
    """the same lists evaluated exactly on the matrix cores; wide: 2 x 33 x 4 = 264 sample rows, past the 256-row tile"""
    name, covers = "tv-pack-exact", ("eoc_tv_pack_exact_device",)
    shape, full = dict(narrow=(2,), wide=(33,)), (5,)

    def call(self, eng, d, o, h, st):
        eng.tv_pack_exact_device(self.pm, d["x"].data_ptr(), self.F, h["rows"], o["out"].data_ptr(), stream=st)

    def ref(self, h, rounding):
        return dict(out=tpe.tv_pack_exact(self.ks.n, self.ks.pk_rows, h["x"], self.pm))


# ---- linear stages ----------------------------------------------------------------------------------------------------------
class Dot(Step):
    """inner products with public int8 weights; narrow: 3 rows over N + 3 columns (2 lists); wide: 9 lists"""
    name, covers, sliced_by = "dot", ("eoc_dot_device",), "dot_launches"
    shape = dict(narrow=(3, N + 3, 2), wide=(2, 8 * N + 1, 3))
    helpers = "test_gpu_dot"

    def make(self, k, width, rows, cols, batch):
        import importlib
        t = importlib.import_module(self.helpers)
        rng = self.rng(k, width)
        return dict(rows=rows, cols=cols, batch=batch, w=t.rand_weights(rng, rows, cols), lists=t.rand_lists(rng, batch, cols),
                    bias=rng.integers(-2**31, 2**31 - 1, rows, endpoint=True).astype(np.int32), dev=["lists", "bias"])

    def device(self, h):
        import importlib
        d = Step.device(self, h)
        d["img"] = importlib.import_module(self.helpers).model(self.ks.aux, h["w"])
        return d

    def outputs(self, h):
        return dict(out=((h["batch"], h["rows"], N + 1), "i32", None))

    def call(self, eng, d, o, h, st):
        eng.dot_device(d["img"].data_ptr(), h["rows"], h["cols"], d["lists"].data_ptr(), h["batch"], d["bias"].data_ptr(),
                       o["out"].data_ptr(), stream=st)

    def ref(self, h, rounding):
        return dict(out=do.dot(h["w"], h["lists"], h["bias"]).reshape(h["batch"], h["rows"], N + 1))


class Linear(Dot):
    """dot and the key switch"""
    name, covers, keyed = "linear", ("eoc_linear_device",), True

    def outputs(self, h):
        return dict(out=((h["batch"], h["rows"], self.ks.n + 1), "i32", None))

    def call(self, eng, d, o, h, st):
        eng.linear_device(d["img"].data_ptr(), h["rows"], h["cols"], d["lists"].data_ptr(), h["batch"], d["bias"].data_ptr(),
                          o["out"].data_ptr(), stream=st)

    def ref(self, h, rounding):
        import test_gpu_dot as td
        return dict(out=td.keyswitch_ref(self.ks.orc, do.dot(h["w"], h["lists"], h["bias"])).reshape(h["batch"], h["rows"], self.ks.n + 1))


CONV_SLOTS = [N - 1, 0, 511]


class Conv(Dot):
    """convolutions with public int8 kernels; wide: 3 output channels over 9 input lists"""
    name, covers, sliced_by = "conv", ("eoc_conv_device",), "conv_launches"
    shape = dict(narrow=(2, N + 3, 2), wide=(3, 9 * N, 2))
    helpers = "test_gpu_conv"

    def outputs(self, h):
        return dict(out=((h["batch"], h["rows"], 2, N), "i32", None))

    def call(self, eng, d, o, h, st):
        eng.conv_device(d["img"].data_ptr(), h["rows"], h["cols"], d["lists"].data_ptr(), h["batch"], d["bias"].data_ptr(),
                        o["out"].data_ptr(), stream=st)

    def ref(self, h, rounding):
        return dict(out=cv.conv(h["w"], h["lists"], h["bias"]).reshape(h["batch"], h["rows"], 2, N))


class ConvLinear(Conv):
    """conv into the scratch lists, then three slots of the first output channel extracted and key-switched; wide: 23 vectors,
    69 samples, past a key-switch tile of 64"""
    name, covers, keyed = "conv-linear", ("eoc_conv_linear_device",), True
    shape, full = dict(narrow=(2, N + 3, 2), wide=(2, 9 * N, 23)), (2, 9 * N, 5)

    def device(self, h):
        import test_gpu_conv as tcv
        d = Conv.device(self, h)
        d["slots"] = tcv.table(self.ks.aux, CONV_SLOTS, h["rows"])
        return d

    def outputs(self, h):
        return dict(out=((h["batch"], len(CONV_SLOTS), self.ks.n + 1), "i32", None))

    def call(self, eng, d, o, h, st):
        eng.conv_linear_device(d["img"].data_ptr(), h["rows"], h["cols"], d["lists"].data_ptr(), h["batch"], d["bias"].data_ptr(),
                               d["slots"].data_ptr(), len(CONV_SLOTS), o["out"].data_ptr(), stream=st)

    def ref(self, h, rounding):
        import test_gpu_conv as tcv
        return dict(out=tcv.extract_keyswitch_ref(self.ks.orc, cv.conv(h["w"], h["lists"], h["bias"]), CONV_SLOTS))


class ConvExtract(Step):
    """the extraction and the key switch alone, one list per vector"""
    name, covers, sliced_by = "conv-extract", ("eoc_conv_extract_device",), "ks_mfma_launches"
    shape, full = dict(narrow=(2,), wide=(50,)), (7,)

    def make(self, k, width, batch):
        import test_gpu_conv as tcv
        return dict(batch=batch, lists=tcv.rand_lists(self.rng(k, width), batch, N), dev=["lists"])

    def device(self, h):
        import test_gpu_conv as tcv
        d = Step.device(self, h)
        d["slots"] = tcv.table(self.ks.aux, CONV_SLOTS, 1)
        return d

    def outputs(self, h):
        return dict(out=((h["batch"], len(CONV_SLOTS), self.ks.n + 1), "i32", None))

    def call(self, eng, d, o, h, st):
        eng.conv_extract_device(d["lists"].data_ptr(), 1, h["batch"], d["slots"].data_ptr(), len(CONV_SLOTS), o["out"].data_ptr(), stream=st)

    def ref(self, h, rounding):
        import test_gpu_conv as tcv
        return dict(out=tcv.extract_keyswitch_ref(self.ks.orc, h["lists"], CONV_SLOTS))


# ---- the host-buffer forms (csrc/multi.hip): host_form(h) -> {output: words} on the global context ------------------------------
def host_form(cls):
    def attach(fn):
        cls.host_form = fn
        return fn
    return attach


@host_form(Gate)
def _gate(self, h):
    ins = [h[f"in{a}"] for a in range(self.nin)]
    return dict(out=self.eoc.gate_batch(self.eoc.OPS[self.op], *ins))


@host_form(Mixed)
def _mixed(self, h):
    return dict(out=self.eoc.gate_batch(0, h["in0"], h["in1"], ops=h["ops"]))


class GateAsync(Gate):
    """eoc_gate_batch_submit / _wait on pinned buffers: two submissions in flight (the second is the same batch again)"""
    name, covers, op = "gate-async", (), "XOR"

    def host_form(self, h):
        eoc = self.eoc
        pins = [[eoc.PinnedArray(h["in0"].shape) for _ in range(3)] for _b in range(2)]
        try:
            tickets = []
            for pb in pins:
                pb[0].array[:], pb[1].array[:] = h["in0"], h["in1"]
                pb[2].array[:] = POISON
                tickets.append(eoc.gate_batch_submit(eoc.OPS[self.op], pb[0].array, pb[1].array, out=pb[2].array))
            for t in tickets:
                eoc.gate_batch_wait(t)
            first, second = pins[0][2].array.copy(), pins[1][2].array.copy()
        finally:
            for pb in pins:
                for a in pb:
                    a.free()
        return dict(out=first, again=second)

    def ref(self, h, rounding):
        out = Gate.ref(self, h, rounding)["out"]
        return dict(out=out, again=out)


@host_form(Circuit)
def _circuit(self, h):
    return dict(wires=self.eoc.circuit_run(h["gates"], h["wires"].copy(), h["S"]))


@host_form(Lut)
def _lut(self, h):
    import test_gpu_lut as tl
    return dict(out=self.eoc.lut_batch(4, np.stack(tl.tables_for(4)[1][:2]), h["x"]))


@host_form(LutMany)
def _lut_many(self, h):
    import test_gpu_lut_many as tm
    out = self.eoc.lut_many_batch(2, np.asarray(tm.tables_for(self.T, 2, 2)[1]), h["x"])
    return dict(out=out.reshape(2 * self.T, h["rows"], self.ks.n + 1))


@host_form(Lut2)
def _lut2(self, h):
    tables = np.stack([l2.lut2_tables(f, self.pm) for f in l2.functions(self.pm)])
    return dict(out=self.eoc.lut2_batch(self.pm, tables, h["x"], h["y"], n_tables=self.T))


@host_form(LutTree)
def _lut_tree(self, h):
    import test_gpu_lut_tree as tt
    tables = np.stack([lt.torus_table(f, self.pm, self.d) for f in tt.functions(self.pm)])
    return dict(out=self.eoc.lut_tree_batch(self.pm, self.d, tables, h["digits"], n_tables=self.T))


@host_form(IntCircuit)
def _int_circuit(self, h):
    return dict(wires=self.eoc.int_circuit_run(self.nodes, self.c.tables(), h["wires"].copy(), h["rows"]))


@host_form(CompactExpand)
def _compact_expand(self, h):
    return dict(out=self.eoc.compact_expand(h["lists"], h["count"]))


@host_form(SeededExpand)
def _seeded_expand(self, h):
    return dict(out=self.eoc.seeded_expand(SEED, h["bodies"], self.first))


@host_form(TableRead)
def _table_read(self, h):
    return dict(out=self.eoc.table_read(h["table"], h["d"], h["lw"], h["sel"]))


@host_form(TableUpdate)
def _table_update(self, h):
    return dict(table=self.eoc.table_update(h["table"], h["d"], h["lw"], h["sel"], h["vals"]))


@host_form(AutomatonRun)
def _automaton_run(self, h):
    sel = h["sel"].reshape(h["queries"], h["steps"], self.ks.kpl, 2, N)
    return dict(out=self.eoc.automaton_run(AUTO_TRANS, h["final"], sel, h["starts"], self.lw))


@host_form(Pack)
def _pack(self, h):
    return dict(out=self.eoc.pack(h["x"]))


@host_form(Linear)
def _linear(self, h):
    return dict(out=self.eoc.linear(h["w"], h["lists"], h["bias"]))


@host_form(ConvLinear)
def _conv_linear(self, h):
    return dict(out=self.eoc.conv_linear(h["w"], h["lists"], CONV_SLOTS, h["bias"]))


HOST_STEPS = (Gate, Mux, Mixed, GateAsync, Circuit, Lut, LutMany, Lut2, LutTree, IntCircuit, CompactExpand, SeededExpand, Pack, Linear,
              ConvLinear, TableRead, TableUpdate, AutomatonRun)
HOST_NAMES = tuple(s.name for s in HOST_STEPS)


def host_registry(ks, steps=None):
    """the host-buffer steps of a key set; `steps`: its device registry, whose step objects (and so their references) are
    re-used for the families that have both forms"""
    steps = steps or {}
    return {s.name: steps.get(s.name) or s(ks) for s in HOST_STEPS}


def cycle(names, seed):
    """[(family, input set 0, width)] of 2 len(names) calls: every family twice, its narrow call ahead of its wide one, in a
    seeded order in which no ordered neighbour pair occurs twice (the pair that closes the cycle into its repeat included)"""
    rng = np.random.default_rng(seed)
    while True:
        order = [int(v) for v in rng.permutation(np.repeat(np.arange(len(names)), 2))]
        pairs = list(zip(order, order[1:] + order[:1]))
        if len(set(pairs)) == len(pairs):
            break
    seen, out = set(), []
    for v in order:
        out.append((names[v], 0, "wide" if v in seen else "narrow"))
        seen.add(v)
    return out


STEPS = (Gate, Mux, Mixed, Circuit, BlindRotateKeyswitch, Lut, LutMany, LutEnc, Lut2, LutTree, IntCircuit, CompactExpand, SeededExpand,
         TgswToFft, TgswSeededToFft, Cmux, Demux, DemuxAccumulate, TableRead, TableUpdate, AutomatonRun, AutomatonStep, Pack, TvPack,
         TvPackExact, Dot, Linear, Conv, ConvLinear, ConvExtract)
NAMES = tuple(s.name for s in STEPS)
LEVELED = frozenset(s.name for s in STEPS if s.leveled)
KEYED = tuple(s.name for s in STEPS if s.keyed)


def registry(ks):
    return {s.name: s(ks) for s in STEPS}


def precompute(steps, entries):
    """the references of every distinct (name, input set, width, rounding) of `entries`: the host inputs are made one after
    the other, the references on a small thread pool (the ctypes calls release the GIL).  The oracle's calls are OpenMP teams
    of orc_max_threads() threads already, so the pool is there only to overlap the references that are Python loops: a
    quarter of the oracle's thread count, four at the most (the rule of tests/test_noise_cpu.py, halved).  Each reference is
    computed once and never changed"""
    from concurrent.futures import ThreadPoolExecutor
    todo = sorted({(n, k, w, bool(r) and steps[n].leveled) for n, k, w, r in entries})
    for n, k, w, _ in todo:
        steps[n].host(k, w)
    with ThreadPoolExecutor(max(1, min(4, ol.lib().orc_max_threads() // 4))) as ex:
        list(ex.map(lambda t: steps[t[0]].want(t[1], t[2], t[3]), todo))


# ---- running a schedule -----------------------------------------------------------------------------------------------------
def counters(eng):
    """every cumulative counter of an engine"""
    c = eng.stats()
    c.update(dot_launches=eng.dot_launches(), conv_launches=eng.conv_launches(), seed_launches=int(eng.seed_launches))
    return c


def moved(before, after):
    return {k: after[k] - before[k] for k in after}


def guarded(shape, kind):
    """(the output tensor, the guard row behind it), both full of the poison word"""
    from gpu_util import torch_cuda
    torch = torch_cuda()
    per = 2 if kind == "f64" else 1
    words = int(np.prod(shape)) * per
    row = int(shape[-1]) * per
    base = torch.full((words + row,), POISON, dtype=torch.int32, device="cuda")
    out = base[:words]
    out = (out.view(torch.float64) if kind == "f64" else out).view(tuple(int(s) for s in shape))
    return out, base[words:]


def same_words(got, want):
    """byte for byte; integer references of another width are compared by value (none is rounded or wrapped to fit)"""
    if got.dtype == want.dtype:
        return cc.bytes_equal(got, want)
    return got.dtype.kind == want.dtype.kind == "i" and got.shape == want.shape and bool(np.array_equal(got, want))


class Position:
    def __init__(self, index, step, k, width, rounding, outs, guards):
        self.index, self.step, self.k, self.width, self.rounding, self.outs, self.guards = index, step, k, width, rounding, outs, guards

    def __repr__(self):
        return f"#{self.index} {self.step.name}[{self.k}, {self.width}{', rounding' if self.rounding else ''}]"


class Runner:
    """queues steps on one engine; the read-only device inputs are made once per (step, input set, width), shared by every
    position, and compared with their first words by inputs_intact()"""

    def __init__(self, steps, eng):
        self.steps, self.eng, self.dev, self.snap = steps, eng, {}, {}

    def inputs(self, step, k, width):
        key = (step.name, k, width)
        if key not in self.dev:
            self.dev[key] = step.device(step.host(k, width))
            self.snap[key] = {name: t.cpu().numpy().copy() for name, t in self.dev[key].items()}
        return self.dev[key]

    def prepare(self, index, name, k, width, rounding):
        """the position's own outputs, poisoned or holding their initial words"""
        from gpu_util import to_dev
        step = self.steps[name]
        self.inputs(step, k, width)
        outs, guards = {}, {}
        for out, (shape, kind, init) in step.outputs(step.host(k, width)).items():
            outs[out], guards[out] = guarded(shape, kind)
            if init is not None:
                outs[out].copy_(to_dev(np.ascontiguousarray(init)))
        return Position(index, step, k, width, bool(rounding) and step.leveled, outs, guards)

    def launch(self, pos, stream):
        pos.step.call(self.eng, self.dev[(pos.step.name, pos.k, pos.width)], pos.outs, pos.step.host(pos.k, pos.width), stream)

    def window(self, entries, stream, first_index=0):
        """entries [(name, k, width, rounding)] queued back to back on `stream` (None: the NULL stream) with no host
        synchronisation in between; the mode is switched where an entry's differs from the one in force.  Returns the
        positions, to be checked after a synchronise"""
        from gpu_util import sync
        positions = [self.prepare(first_index + j, *e) for j, e in enumerate(entries)]
        sync()
        for pos, (_, _, _, rounding) in zip(positions, entries):
            if bool(rounding) != self.eng.leveled_rounding:
                self.eng.leveled_rounding = bool(rounding)
            self.launch(pos, stream)
        return positions

    def failures(self, positions, prev=None):
        """[(position, the family queued ahead of it, output, what is wrong)] of a synchronised window"""
        bad = []
        for pos in positions:
            want = pos.step.want(pos.k, pos.width, pos.rounding)
            for out, t in pos.outs.items():
                got = t.cpu().numpy()
                if not bool((pos.guards[out] == POISON).all()):
                    bad.append((repr(pos), prev, out, "the guard row behind the output was written"))
                if out not in pos.step.in_place and (got.view(np.uint32) == POISON).all():
                    bad.append((repr(pos), prev, out, "still all poison"))
                elif not same_words(got, np.asarray(want[out]).reshape(got.shape)):
                    w = np.asarray(want[out]).reshape(got.shape)
                    bad.append((repr(pos), prev, out, f"{int((got != w).sum())} wrong words, first at {np.argwhere(got != w)[:3].tolist()}"))
            prev = pos.step.name
        return bad

    def inputs_intact(self):
        return [key for key, d in self.dev.items() for name, t in d.items() if not cc.bytes_equal(t.cpu().numpy(), self.snap[key][name])]
