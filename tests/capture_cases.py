"""The cases of tests/test_gpu_capture.py: one class per device call family.  A case owns a FRESH engine (made under the
case's environment knobs), a second engine with the same keys for the eager cross-check, five host-side input sets (0, 1, 2
for the captured buffers, 3 and 4 for the disturbance) and the references of sets 0 .. 2, all from the helpers the family's own
test module uses.  Test-side only; nothing here computes a reference of its own."""
import contextlib
import ctypes as C
import os

import numpy as np

import cmux_oracle as cx
import compact_oracle as co
import int_circuit_oracle as ico
import lut2_oracle as l2
import lut_many_oracle as lmo
import lut_oracle as lo
import oracle_lib as ol
import pack_oracle as po
import table_update_oracle as tu
import test_gpu_cmux as tc
import test_gpu_int_circuit as ti
import test_gpu_lut as tl
import test_gpu_lut_many as tm
import test_gpu_pack as tp
from gpu_util import dev_empty, sync, to_dev, torch_cuda

N = 1024
POISON = 0x5A5AA5A5
SEED = bytes(range(7, 39))
# every knob eoc_engine_create reads: none of them may leak from one case's engine into another's
KNOBS = ("EOC_TFHE_PRIO_DUTY", "EOC_TFHE_PRIO_MULTI", "EOC_TFHE_BR_SLICE", "EOC_TFHE_NO_FOLD", "EOC_TFHE_NO_POOL",
         "EOC_TFHE_SCALAR_ABAR", "EOC_TFHE_BR_PARTS", "EOC_TFHE_BR_WIDE", "EOC_TFHE_KS_MFMA", "EOC_TFHE_BR_TABLES_LDS",
         "EOC_TFHE_INT_SLICE_ROWS", "EOC_TFHE_TABLE_WS_BYTES", "EOC_TFHE_PACK_WS_BYTES", "EOC_TFHE_SLICE_SAMPLES")
# The sensitivity run (module docstring of test_gpu_capture.py): disturb() makes this many calls of the captured shape on the
# two live disturbance buffer sets and nothing else, so that every slot of the descriptor ring ends up holding a descriptor
# of the captured type that points to live buffers.  0: the ordinary disturbance.
SAME_SHAPE_CALLS = int(os.environ.get("EOC_CAPTURE_TEST_SAME_SHAPE_CALLS", "0"))


@contextlib.contextmanager
def knobs(env):
    saved = {k: os.environ.pop(k) for k in KNOBS if k in os.environ}
    os.environ.update(env)
    try:
        yield
    finally:
        for k in env:
            os.environ.pop(k, None)
        os.environ.update(saved)


def bytes_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


_SMALL = {}


def small_keys(eoc, pset, n, seed, bk=True):
    """(params, secret key, oracle, second engine with the cloud key) at LWE dimension n: the fast oracle of the gate tests"""
    key = (pset, n, seed, bk)
    if key not in _SMALL:
        p = eoc.default_params(pset)
        p.n = n
        sk = eoc.SecretKey(p, seed)
        with knobs({}):
            eng2 = eoc.Engine(p)
        eng2.load_cloud_key(sk)
        _SMALL[key] = (p, sk, ol.Oracle(pset, seed, n_override=n, with_bk=bk), eng2)
    return _SMALL[key]


def rand_i32(rng, shape):
    return rng.integers(-2**31, 2**31, shape).astype(np.int32)


class Case:
    """run / set_inputs / want / fetch / disturb of the protocol, on top of what a family states: alloc() a buffer set, load(b,
    k) input set k into it, call(eng, b, stream), outs(b) the tensors a call only writes, read(b) its outputs as a dict of
    arrays, ref(k) the reference's words per output and pick(name, a) the part of an output the reference covers"""
    env = {}
    expect = {}                                                 # engine counters one call of the captured shape adds

    def __init__(self, eoc):
        self.eoc, self.torch, self.keep, self._ref = eoc, torch_cuda(), [], {}
        self.setup()
        self.bufs = self.alloc()
        self.dbufs = [self.alloc(), self.alloc()]

    def fresh(self, params):
        with knobs(self.env):
            self.eng = self.eoc.Engine(params)
        return self.eng

    def new(self, shape, dtype=None):
        t = dev_empty(shape, dtype or self.torch.int32)
        t.view(self.torch.int32).fill_(POISON)
        self.keep.append(t)
        return t

    # -- the protocol ---------------------------------------------------------------------------------------------------
    def run(self, stream):
        self.call(self.eng, self.bufs, stream)

    def set_inputs(self, k):
        self.load(self.bufs, k)

    def want(self, k):
        if k not in self._ref:
            self._ref[k] = self.ref(k)
        return self._ref[k]

    def fetch(self):
        return self.read(self.bufs)

    def poison(self):
        for t in self.outs(self.bufs):
            t.view(self.torch.int32).fill_(POISON)

    def disturb(self):
        if SAME_SHAPE_CALLS:
            for j in range(SAME_SHAPE_CALLS):
                if j < 2:
                    self.load(self.dbufs[j], 3 + j)
                self.call(self.eng, self.dbufs[j % 2], None)
            return
        for rnd in range(3):                                    # other live buffers, other inputs, the captured shape
            for j, b in enumerate(self.dbufs):
                self.load(b, 3 + (j + rnd) % 2)
                self.call(self.eng, b, None)
        self.other()                                            # another width / opcode mix inside the sized workspace

    def second(self, k):
        """the same call, eagerly, on the second engine and buffers of its own"""
        b = self.alloc()
        self.load(b, k)
        self.call(self.eng2, b, None)
        sync()
        return self.read(b)

    def pick(self, name, a):
        return a

    def outs(self, b):
        return [b["out"]]

    def read(self, b):
        return dict(out=b["out"].cpu().numpy())

    def other(self):
        raise NotImplementedError

    def close(self):
        self.eng.close()
        self.keep.clear()


# ---- gates ------------------------------------------------------------------------------------------------------------------
class GateCase(Case):
    pset, n, S, op, seed = 0, 40, 5, "NAND", 31
    other_calls = (("XOR", 3), ("AND", 70))                     # narrower, and wider than the captured call's last tile

    def setup(self):
        eoc = self.eoc
        self.p, self.sk, self.orc, self.eng2 = small_keys(eoc, self.pset, self.n, self.seed)
        self.fresh(self.p).load_cloud_key(self.sk)
        rng = np.random.default_rng(self.S)
        self.nin = 3 if self.op == "MUX" else 2
        self.inp = [[self.sk.encrypt_bits(rng.integers(0, 2, self.S).astype(np.uint8), 100 + 10 * k + a) for a in range(self.nin)]
                    for k in range(5)]

    def alloc(self, rows=None):
        rows = rows or self.S
        b = {f"in{a}": self.new((rows, self.n + 1)) for a in range(3)}
        b["out"] = self.new((rows, self.n + 1))
        return b

    def load(self, b, k):
        for a in range(self.nin):
            b[f"in{a}"].copy_(to_dev(np.resize(self.inp[k][a], tuple(b[f"in{a}"].shape))))

    def gate(self, eng, b, op, count, st):
        eng.gate_batch_device(self.eoc.OPS[op], b["in0"].data_ptr(), b["in1"].data_ptr(), b["in2"].data_ptr(), b["out"].data_ptr(),
                              count, stream=st)

    def call(self, eng, b, st):
        self.gate(eng, b, self.op, self.S, st)

    def ref(self, k):
        return dict(out=self.orc.gate_batch(ol.OPS[self.op], *self.inp[k]))

    def other(self):
        if not hasattr(self, "wide"):
            self.wide = self.alloc(max(count for _, count in self.other_calls))
            self.load(self.wide, 4)
        for op, count in self.other_calls:
            self.gate(self.eng, self.wide, op, count, None)


class SetBGate(GateCase):
    """one gate: the descriptor travels as a kernel argument, the rotation is cut in two through acc_state"""
    pset = 1
    expect = dict(br_launches=2)


class MuxLevel(GateCase):
    """S = 70: two partly filled key-switch tiles of 2 S = 140 rows, k_prepare and k_ks_init as launches of their own"""
    S, op = 70, "MUX"
    other_calls = (("NAND", 200), ("MUX", 20))                  # 200 rows: past the 140 workspace rows of the captured level
    expect = dict(br_launches=1)


class BlindRotateKeyswitch(Case):
    """blind_rotate_device, then keyswitch_device on its output: one arena slot each, and the copy out of / into W.d_u"""
    rows, n, seed = 9, 40, 33

    def setup(self):
        self.p, self.sk, self.orc, self.eng2 = small_keys(self.eoc, 0, self.n, self.seed)
        self.fresh(self.p).load_cloud_key(self.sk)
        rng = np.random.default_rng(41)
        self.inp = [rand_i32(rng, (self.rows, self.n + 1)) for _ in range(5)]

    def alloc(self, rows=None):
        rows = rows or self.rows
        return dict(t=self.new((rows, self.n + 1)), u=self.new((rows, N + 1)), out=self.new((rows, self.n + 1)))

    def load(self, b, k):
        b["t"].copy_(to_dev(np.resize(self.inp[k], tuple(b["t"].shape))))

    def both(self, eng, b, count, st):
        eng.blind_rotate_device(b["t"].data_ptr(), b["u"].data_ptr(), count, stream=st)
        eng.keyswitch_device(b["u"].data_ptr(), b["out"].data_ptr(), count, stream=st)

    def call(self, eng, b, st):
        self.both(eng, b, self.rows, st)

    def outs(self, b):
        return [b["u"], b["out"]]

    def read(self, b):
        return dict(u=b["u"].cpu().numpy(), out=b["out"].cpu().numpy())

    def ref(self, k):
        u = np.stack([self.orc.blind_rotate_extract(t) for t in self.inp[k]])
        return dict(u=u, out=np.stack([self.orc.keyswitch(x) for x in u]))

    def other(self):
        if not hasattr(self, "wide"):
            self.wide = self.alloc(20)
            self.load(self.wide, 4)
        self.both(self.eng, self.dbufs[0], 4, None)
        self.both(self.eng, self.wide, 20, None)                # leaves rows 9 .. 19 of W.d_u and the operand rows behind


# ---- table lookups ----------------------------------------------------------------------------------------------------------
class Lut(Case):
    """p = 4, 2 tables x 3 rows: one descriptor per table through the arena"""
    p_msg, n_luts, rows, n, seed = 4, 2, 3, 40, 35
    T = 0

    def tvs(self):
        return np.stack([self.eoc.lut_test_polynomial(self.p_msg, t) for t in tl.tables_for(self.p_msg)[1][:self.n_luts]])

    def setup(self):
        self.p, self.sk, self.orc, self.eng2 = small_keys(self.eoc, 0, self.n, self.seed)
        self.fresh(self.p).load_cloud_key(self.sk)
        self.tv = self.tvs()
        cts = tl.inputs(self.eoc, self.sk, self.p_msg, self.rows + 4, 7300 + self.p_msg)[1]
        self.inp = [cts[k:k + self.rows].copy() for k in range(5)]     # every set with other messages, padding half included
        self.d_tv = to_dev(self.tv)
        self.keep.append(self.d_tv)

    def alloc(self, rows=None):
        rows = rows or self.rows
        return dict(x=self.new((rows, self.n + 1)), out=self.new((self.n_luts * max(self.T, 1), rows, self.n + 1)))

    def load(self, b, k):
        b["x"].copy_(to_dev(np.resize(self.inp[k], tuple(b["x"].shape))))

    def lut(self, eng, b, n_luts, rows, st):
        eng.lut_batch_device(self.d_tv.data_ptr(), n_luts, b["x"].data_ptr(), b["out"].data_ptr(), rows, stream=st)

    def call(self, eng, b, st):
        self.lut(eng, b, self.n_luts, self.rows, st)

    def ref(self, k):
        return dict(out=lo.lut_batch(self.orc, self.tv, self.inp[k]))

    def other(self):
        if not hasattr(self, "wide"):
            self.wide = self.alloc(5)
            self.load(self.wide, 4)
        self.lut(self.eng, self.dbufs[0], 1, 2, None)
        self.lut(self.eng, self.wide, self.n_luts, 5, None)     # more jobs than the captured level, inside the workspace


class LutWide(Lut):
    env = {"EOC_TFHE_BR_WIDE": "1"}
    expect = dict(br_wide_launches=1)


class LutMany(Lut):
    """T = 2, p = 2, 2 polynomials x 3 rows: the coarse mod switch reads the first descriptors, the key switch the others"""
    p_msg, T = 2, 2

    def tvs(self):
        return tm.packed(self.eoc, self.p_msg, tm.tables_for(self.T, self.p_msg, self.n_luts)[1])

    def lut(self, eng, b, n_luts, rows, st):
        eng.lut_many_batch_device(self.T, self.d_tv.data_ptr(), n_luts, b["x"].data_ptr(), b["out"].data_ptr(), rows, stream=st)

    def ref(self, k):
        return dict(out=lmo.lut_many_batch(self.orc, self.tv, self.inp[k], self.T).reshape(-1, self.rows, self.n + 1))


# ---- integer circuits -------------------------------------------------------------------------------------------------------
def int_netlist(eoc):
    """(the circuit, its four inputs): two levels -- a free node in level 1's pre-pass, a 4-term node, a T = 2 node behind the
    free node, a level-2 node and a last free node.  Shared with tests/interleave_cases.py"""
    u = eoc.int_circuits.units
    c = eoc.IntCircuit()
    x = [c.input(4, fresh=True) for _ in range(4)]
    f = c.lin([(1, x[0]), (1, x[1])], cst=u(1, 4))
    n4 = c.lut([x[0], x[1], x[2], (2, x[3])], lambda m: (3 * m + 1) % 4, 4, 4, allow_padding=True)
    m2 = c.lut_many([f], [lambda m: m % 2, lambda m: (m + 1) % 4], 4, 4, allow_padding=True)
    n2 = c.lut([(1, n4), (2, m2[0])], lambda m: 3 - m, 4, 4, allow_padding=True)
    c.lin([(1, n2), (-1, m2[1])], cst=u(2, 4))
    return c, x


class IntCircuit(Case):
    """two levels, 5 rows: a free node in level 1's pre-pass, a 4-term node, a T = 2 node behind the free node, a level-2 node
    and a last free node: LinDescs and k_tv_gather's polynomial indices through the arena"""
    rows, n, seed, groups = 5, 40, 37, 3
    expect = dict(br_launches=3)

    def setup(self):
        eoc = self.eoc
        self.p, self.sk, self.orc, self.eng2 = small_keys(eoc, 0, self.n, self.seed)
        self.fresh(self.p).load_cloud_key(self.sk)
        c, x = int_netlist(eoc)
        assert c.levels()[1:] == (2, 3)
        self.c, self.nodes, self.tv = c, c.nodes(), c.test_polynomials()
        self.written = sorted({w for k in range(len(self.nodes)) for w in c.node_outputs(k)})
        self.inp = [ti.circuit_inputs(eoc, self.sk, c, x, self.rows, 9700 + 20 * k)[1] for k in range(5)]
        self.d_tv = to_dev(self.tv)
        self.keep.append(self.d_tv)
        self.small = self.new((c.n_wires, 2, self.n + 1))         # the other width: the same netlist over 2 rows

    def alloc(self):
        return dict(w=self.new((self.c.n_wires, self.rows, self.n + 1)))

    def load(self, b, k):
        b["w"].copy_(to_dev(self.inp[k]))

    def circuit(self, eng, d_w, rows, st):
        eng.int_circuit_run_device(self.nodes, self.d_tv.data_ptr(), self.tv.shape[0], d_w.data_ptr(), self.c.n_wires, rows, stream=st)

    def call(self, eng, b, st):
        self.circuit(eng, b["w"], self.rows, st)

    def outs(self, b):
        return [b["w"][w] for w in self.written]

    def read(self, b):
        return dict(wires=b["w"].cpu().numpy())

    def ref(self, k):
        return dict(wires=ico.run(self.orc, self.nodes, self.tv, self.inp[k]))

    def other(self):
        self.small.copy_(to_dev(self.inp[4][:, :2]))
        self.circuit(self.eng, self.small, 2, None)


class IntCircuitSliced(IntCircuit):
    """slices of 2 rows: 2 + 2 + 1, every slice pushing its own LinDescs"""
    env = {"EOC_TFHE_INT_SLICE_ROWS": "2"}
    expect = dict(br_launches=9)


# ---- compact lists and seeded forms -----------------------------------------------------------------------------------------
class CompactExpand(Case):
    """70 slots from slot 990 of the first list into the second (the engine entry the global context's shards call); the other
    widths are the public call, 33 and 100 slots from slot 0"""
    first, count, n, seed = 990, 70, 40, 39

    def setup(self):
        eoc = self.eoc
        self.p, self.sk, self.orc, self.eng2 = small_keys(eoc, 0, self.n, self.seed, bk=False)
        self.fresh(self.p).load_cloud_key(self.sk)
        pk = eoc.PublicKey(self.sk.public_key_bytes())
        rng = np.random.default_rng(43)
        self.inp = [pk.encrypt_bits(rng.integers(0, 2, 2 * N).astype(np.uint8), enc_seed=300 + k) for k in range(5)]
        self.fn = getattr(eoc.lib(), "_Z30eoc_compact_expand_device_fromP10eoc_enginePKimmPiPv")     # csrc/common.h
        self.fn.restype, self.fn.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p]

    def alloc(self):
        return dict(lists=self.new((2, 2, N)), out=self.new((self.count, self.n + 1)))

    def load(self, b, k):
        b["lists"].copy_(to_dev(self.inp[k]))

    def call(self, eng, b, st):
        rc = self.fn(eng.h, b["lists"].data_ptr(), self.first, self.count, b["out"].data_ptr(), st)
        if rc:
            raise self.eoc.EocError(f"eoc_compact_expand_device_from failed ({rc}): {self.eoc.lib().eoc_last_error().decode()}")

    def ref(self, k):
        return dict(out=co.expand(self.orc, self.inp[k], np.arange(self.first, self.first + self.count)))

    def other(self):
        if not hasattr(self, "wide"):
            self.wide = self.new((100, self.n + 1))
        b = self.dbufs[0]
        self.eng.compact_expand_device(b["lists"].data_ptr(), 33, b["out"].data_ptr())
        self.eng.compact_expand_device(b["lists"].data_ptr(), 100, self.wide.data_ptr())    # operand rows 70 .. 99 left behind


_SEEDED = {}


def seeded_keys(eoc, n=17):
    """(params at LWE dimension n, secret key without a cloud key, second engine): the conversions need no key"""
    if n not in _SEEDED:
        p = eoc.default_params(0)
        p.n = n
        with knobs({}):
            eng2 = eoc.Engine(p)
        _SEEDED[n] = (p, eoc.SecretKey(p, 1, with_cloud_key=False), eng2)
    return _SEEDED[n]


class SeededExpand(Case):
    """70 bodies at n = 17, stream indices that cross 2^32 inside the call; the seed and first_idx are baked, the bodies vary"""
    count, first = 70, 2**32 - 5

    def setup(self):
        self.p, self.sk, self.eng2 = seeded_keys(self.eoc)
        self.fresh(self.p)
        rng = np.random.default_rng(45)
        self.inp = [rand_i32(rng, self.count) for _ in range(5)]

    def alloc(self):
        return dict(bodies=self.new((self.count,)), out=self.new((self.count, self.p.n + 1)))

    def load(self, b, k):
        b["bodies"].copy_(to_dev(self.inp[k]))

    def expand(self, eng, b, count, st):
        eng.seeded_expand_device(SEED, b["bodies"].data_ptr(), count, b["out"].data_ptr(), self.first, stream=st)

    def call(self, eng, b, st):
        self.expand(eng, b, self.count, st)

    def ref(self, k):
        return dict(out=self.eoc.seeded_expand_host(self.p, SEED, self.inp[k], self.first))

    def other(self):
        self.expand(self.eng, self.dbufs[0], 9, None)


class TgswToFft(Case):
    """3 selectors in torus form -> the converted form; the reference is the oracle's transform (an exact 2^-9 apart)"""
    count = 3

    def setup(self):
        self.p, self.sk, self.eng2 = seeded_keys(self.eoc)
        self.fresh(self.p)
        self.kpl = 2 * self.p.l
        self.inp = [self.sk.encrypt_selector_bits([(k >> a) & 1 for a in range(self.count)], enc_seed=50 + k) for k in range(5)]

    def alloc(self):
        return dict(sel=self.new((self.count, self.kpl, 2, N)), out=self.new((self.count, self.kpl, 2, N), self.torch.float64))

    def load(self, b, k):
        b["sel"].copy_(to_dev(self.inp[k]))

    def convert(self, eng, b, count, st):
        eng.tgsw_to_fft_device(b["sel"].data_ptr(), count, b["out"].data_ptr(), stream=st)

    def call(self, eng, b, st):
        self.convert(eng, b, self.count, st)

    def torus(self, k):
        return self.inp[k]

    def ref(self, k):
        return dict(out=cx.to_fft(self.torus(k)) * 2.0**-9)

    def other(self):
        self.convert(self.eng, self.dbufs[0], 1, None)


class SeededSelector(TgswToFft):
    """one seeded selector: new bodies under the same (baked) seed and first_idx; the staging rows are rewritten by the
    disturbance and by a plain conversion in between"""
    count, first = 1, 3

    def setup(self):
        self.p, self.sk, self.eng2 = seeded_keys(self.eoc)
        self.fresh(self.p)
        self.kpl = 2 * self.p.l
        self.inp = [self.sk.encrypt_selector_bits_seeded([k & 1], bytes(range(k, k + 32)), SEED, first_idx=self.first)[1]
                    for k in range(5)]
        self.plain = dict(sel=to_dev(self.sk.encrypt_selector_bits([1], enc_seed=60)), out=self.new((1, self.kpl, 2, N), self.torch.float64))
        self.keep.append(self.plain["sel"])

    def alloc(self):
        return dict(bodies=self.new((1, self.kpl, N)), out=self.new((1, self.kpl, 2, N), self.torch.float64))

    def load(self, b, k):
        b["bodies"].copy_(to_dev(self.inp[k]))

    def call(self, eng, b, st):
        eng.tgsw_seeded_to_fft_device(SEED, b["bodies"].data_ptr(), 1, b["out"].data_ptr(), self.first, stream=st)

    def torus(self, k):
        return self.eoc.tgsw_seeded_expand_host(self.p, SEED, self.inp[k], self.first)

    def other(self):
        TgswToFft.convert(self, self.eng, self.plain, 1, None)


# ---- CMux, demux, table read and update -------------------------------------------------------------------------------------
class Leveled(Case):
    """Set A, the keys of tests/test_gpu_cmux.py (their engine is the second engine and converts every selector set)"""
    def keys(self):
        self.p, self.sk, self.pk, self.orc, self.eng2 = tc.keys(self.eoc, 0)
        self.op, self.kpl = cx.orc_params(self.p), 2 * self.p.l

    def selectors(self, sel):
        """(reference form, device form) of selectors in torus form"""
        sel = np.ascontiguousarray(sel, np.int32).reshape(-1, self.kpl, 2, N)
        d = tc.convert(self.eng2, sel)
        self.keep.append(d)
        return cx.to_fft(sel), d


class Cmux(Leveled):
    """3 items: one workgroup of two and a remainder"""
    count = 3

    def setup(self):
        self.keys()
        self.fresh(self.p)                                      # no key is needed
        rng = np.random.default_rng(47)
        self.inp = []
        for k in range(5):
            fft, d_fft = self.selectors(self.sk.encrypt_selector_bits([(k >> a) & 1 for a in range(self.count)], enc_seed=70 + k))
            self.inp.append(dict(fft=fft, d_fft=d_fft, a=rand_i32(rng, (self.count, 2, N)), b=rand_i32(rng, (self.count, 2, N))))

    def alloc(self):
        return dict(fft=self.new((self.count, self.kpl, 2, N), self.torch.float64), a=self.new((self.count, 2, N)),
                    b=self.new((self.count, 2, N)), out=self.new((self.count, 2, N)))

    def load(self, b, k):
        b["fft"].copy_(self.inp[k]["d_fft"])
        b["a"].copy_(to_dev(self.inp[k]["a"]))
        b["b"].copy_(to_dev(self.inp[k]["b"]))

    def cmux(self, eng, b, count, st):
        eng.cmux_device(b["fft"].data_ptr(), b["a"].data_ptr(), b["b"].data_ptr(), b["out"].data_ptr(), count, stream=st)

    def call(self, eng, b, st):
        self.cmux(eng, b, self.count, st)

    def ref(self, k):
        i = self.inp[k]
        return dict(out=np.stack([cx.cmux(self.op, i["fft"][q], i["a"][q], i["b"][q]) for q in range(self.count)]))

    def other(self):
        self.cmux(self.eng, self.dbufs[0], 1, None)


class Demux(Cmux):
    """3 items, storing: out0 = in - E, out1 = E"""
    accumulate = False

    def setup(self):
        Cmux.setup(self)
        rng = np.random.default_rng(49)
        self.base = [rand_i32(rng, (self.count, 2, N)) for _ in range(2)]

    def alloc(self):
        b = Cmux.alloc(self)
        b["out1"] = self.new((self.count, 2, N))
        return b

    def cmux(self, eng, b, count, st):
        eng.demux_device(b["fft"].data_ptr(), b["a"].data_ptr(), b["out"].data_ptr(), b["out1"].data_ptr(), count,
                         accumulate=self.accumulate, stream=st)

    def outs(self, b):
        return [b["out"], b["out1"]]

    def read(self, b):
        return dict(out0=b["out"].cpu().numpy(), out1=b["out1"].cpu().numpy())

    def ref(self, k):
        i = self.inp[k]
        o = [tu.demux(self.op, i["fft"][q], i["a"][q]) for q in range(self.count)]
        return dict(out0=np.stack([x[0] for x in o]), out1=np.stack([x[1] for x in o]))


class DemuxAccumulate(Demux):
    """accumulating: set_inputs rewrites both outputs to their base words, the reference adds the storing form's words"""
    accumulate = True

    def load(self, b, k):
        Demux.load(self, b, k)
        b["out"].copy_(to_dev(self.base[0]))
        b["out1"].copy_(to_dev(self.base[1]))

    def outs(self, b):
        return []                                               # in place: a poison word would be added to, not overwritten

    def ref(self, k):
        r = Demux.ref(self, k)
        return {name: tu.wrap_i32(self.base[j].astype(np.int64) + r[name]) for j, name in enumerate(("out0", "out1"))}


class TableRead(Leveled):
    """log2_lists = 2, log2_width = 9, 3 queries: two tree stages through both ping-pong buffers, one rotation, the extraction
    and the key switch of 3 x 512 samples.  The reference covers slots 0 .. 7, 250 .. 257 and 504 .. 511 of every query"""
    d, lw, queries = 2, 9, 3
    WS = np.r_[0:8, 250:258, 504:512]
    expect = dict(cmux_launches=3)

    def setup(self):
        eoc = self.eoc
        self.keys()
        self.depth, self.W = self.d + 10 - self.lw, 1 << self.lw
        self.fresh(self.p).load_cloud_key(self.sk)
        rng = np.random.default_rng(51)
        self.table = tc.make_table(eoc, self.pk, "ints", self.d, rng, 651)[0]
        self.d_tab = to_dev(self.table)
        self.keep.append(self.d_tab)
        last = (1 << self.depth) - 1
        self.inp = []
        for k in range(5):
            idx = [last, 0, int(rng.integers(0, last + 1))][k % 3:] + [last, 0][:k % 3]
            sel = tc.index_selectors(self.sk, idx, self.depth, enc_seed=750 + k)
            fft, d_fft = self.selectors(sel)
            self.inp.append(dict(sel=sel, fft=fft.reshape(self.queries, self.depth, self.kpl, 2, N), d_fft=d_fft))
        # the other shape: one query into the first two lists -- depth 2, so its last CMux lands in the other buffer
        self.small = dict(fft=self.selectors(tc.index_selectors(self.sk, [2], 2, enc_seed=760))[1], out=self.new((1, self.W, self.p.n + 1)))

    def alloc(self):
        return dict(fft=self.new((self.queries * self.depth, self.kpl, 2, N), self.torch.float64),
                    out=self.new((self.queries, self.W, self.p.n + 1)))

    def load(self, b, k):
        b["fft"].copy_(self.inp[k]["d_fft"])

    def call(self, eng, b, st):
        eng.table_read_device(self.d_tab.data_ptr(), self.d, self.lw, b["fft"].data_ptr(), self.queries, b["out"].data_ptr(), stream=st)

    def pick(self, name, a):
        return a[:, self.WS]

    def ref(self, k):
        fft = self.inp[k]["fft"]
        samples = np.stack([cx.table_read_tlwe(self.op, self.table, self.d, self.lw, fft[q]) for q in range(self.queries)])
        idx = (np.arange(self.queries)[:, None] * N + self.WS[None, :]).ravel()
        return dict(out=co.expand(self.orc, samples, idx).reshape(self.queries, len(self.WS), self.p.n + 1))

    def other(self):
        self.eng.table_read_device(self.d_tab.data_ptr(), 1, self.lw, self.small["fft"].data_ptr(), 1, self.small["out"].data_ptr())


def table_walk_bytes_per_query(d):
    """TableWalk of csrc/engine.hip: 2^(d-1) samples per query in buffer 0, 2^(d-2) in buffer 1 (one at least), 8 KiB each"""
    return ((1 << (d - 1) if d >= 1 else 1) + (1 << (d - 2) if d >= 2 else 1)) * 2 * N * 4


class TableReadSliced(TableRead):
    """a budget of two queries' samples: slices of 2 and 1 queries, each walking the buffers from their start"""
    env = {"EOC_TFHE_TABLE_WS_BYTES": str(2 * table_walk_bytes_per_query(2))}
    expect = dict(cmux_launches=6)


class TableUpdate(TableRead):
    """table[idx_q] += value_q in place, 3 queries of which two hit one entry.  set_inputs rewrites the table to its base words"""
    expect = dict(cmux_launches=1, demux_launches=2)

    def setup(self):
        self.keys()
        self.depth, self.W = self.d + 10 - self.lw, 1 << self.lw
        self.fresh(self.p)                                      # no key is needed
        rng = np.random.default_rng(53)
        self.base = rand_i32(rng, (1 << self.d, 2, N))
        last = (1 << self.depth) - 1
        self.inp = []
        for k in range(5):
            idx = [last - k, k, last - k]
            fft, d_fft = self.selectors(tc.index_selectors(self.sk, idx, self.depth, enc_seed=850 + k))
            self.inp.append(dict(fft=fft.reshape(self.queries, self.depth, self.kpl, 2, N), d_fft=d_fft,
                                 vals=rand_i32(rng, (self.queries, 2, N))))
        self.small = dict(fft=self.selectors(tc.index_selectors(self.sk, [1], 2, enc_seed=860))[1], table=self.new((2, 2, N)))

    def alloc(self):
        return dict(fft=self.new((self.queries * self.depth, self.kpl, 2, N), self.torch.float64),
                    vals=self.new((self.queries, 2, N)), out=self.new((1 << self.d, 2, N)))

    def load(self, b, k):
        b["fft"].copy_(self.inp[k]["d_fft"])
        b["vals"].copy_(to_dev(self.inp[k]["vals"]))
        b["out"].copy_(to_dev(self.base))

    def call(self, eng, b, st):
        eng.table_update_device(b["out"].data_ptr(), self.d, self.lw, b["fft"].data_ptr(), b["vals"].data_ptr(), self.queries, stream=st)

    def outs(self, b):
        return []                                               # in place

    def pick(self, name, a):
        return a

    def updated(self, table, k):
        return tu.table_update(self.op, table, self.d, self.lw, self.inp[k]["fft"], self.inp[k]["vals"])

    def ref(self, k):
        return dict(out=self.updated(self.base, k))

    def other(self):
        self.eng.table_update_device(self.small["table"].data_ptr(), 1, self.lw, self.small["fft"].data_ptr(),
                                     self.dbufs[0]["vals"].data_ptr(), 1)


# ---- packing ----------------------------------------------------------------------------------------------------------------
_PACK = {}


def pack_keys(eoc, n=17):
    """(params, secret key, packing-key blob, its reference spectra, second engine with the key) at LWE dimension n = 17: one
    full chunk of 16 key indices and a chunk of one"""
    if n not in _PACK:
        p = eoc.default_params(0)
        p.n = n
        sk = eoc.SecretKey(p, 5, with_cloud_key=False)
        blob = sk.packing_key_bytes()
        with knobs({}):
            eng2 = eoc.Engine(p)
        eng2.load_packing_key(blob)
        _PACK[n] = (p, sk, blob, po.key_fft(po.blob_rows(blob, n)), eng2)
    return _PACK[n]


class Pack(Case):
    """N + 3 samples at n = 17: two lists, the second with 3 slots"""
    count = N + 3
    expect = dict(pack_launches=1)

    def setup(self):
        self.p, self.sk, blob, self.kfft, self.eng2 = pack_keys(self.eoc)
        self.fresh(self.p).load_packing_key(blob)
        rng = np.random.default_rng(55)
        self.inp = [self.sk.encrypt_bits(rng.integers(0, 2, self.count).astype(np.uint8), 900 + k) for k in range(5)]

    def alloc(self):
        return dict(x=self.new((self.count, self.p.n + 1)), out=self.new((2, 2, N)))

    def load(self, b, k):
        b["x"].copy_(to_dev(self.inp[k]))

    def pack(self, eng, b, count, st):
        eng.pack_device(b["x"].data_ptr(), count, b["out"].data_ptr(), stream=st)

    def call(self, eng, b, st):
        self.pack(eng, b, self.count, st)

    def ref(self, k):
        return dict(out=po.pack(self.p.n, self.kfft, self.inp[k]))

    def other(self):
        self.pack(self.eng, self.dbufs[0], 5, None)


class PackSliced(Pack):
    """a column budget of one list: two slices, both through the same columns"""
    env = {"EOC_TFHE_PACK_WS_BYTES": str(17 * N * 4 + 100)}
    expect = dict(pack_launches=2)


class TvPack(Case):
    """p = 4: 2 functions x 2 rows, four samples a list"""
    p_msg, F, rows = 4, 2, 2
    expect = dict(pack_launches=1)

    def setup(self):
        self.p, self.sk, blob, self.kfft, self.eng2 = pack_keys(self.eoc)
        self.fresh(self.p).load_packing_key(blob)
        rng = np.random.default_rng(57)
        self.inp = [self.sk.encrypt_ints(rng.integers(0, 4, self.F * 4 * self.rows).astype(np.uint8), 4, 950 + k)
                    .reshape(self.F, 4, self.rows, self.p.n + 1) for k in range(5)]
        self.one = dict(x=to_dev(self.inp[3][:1, :, :1].copy()), out=self.new((1, 1, 2, N)))
        self.keep.append(self.one["x"])

    def alloc(self):
        return dict(x=self.new((self.F, 4, self.rows, self.p.n + 1)), out=self.new((self.F, self.rows, 2, N)))

    def load(self, b, k):
        b["x"].copy_(to_dev(self.inp[k]))

    def call(self, eng, b, st):
        eng.tv_pack_device(self.p_msg, b["x"].data_ptr(), self.F, self.rows, b["out"].data_ptr(), stream=st)

    def ref(self, k):
        return dict(out=l2.tv_pack(self.p.n, self.kfft, self.inp[k], self.p_msg))

    def other(self):
        self.eng.tv_pack_device(self.p_msg, self.one["x"].data_ptr(), 1, 1, self.one["out"].data_ptr())


# ---- two-input lookups ------------------------------------------------------------------------------------------------------
ROW_SETS = ([0, 1], [2, 3], [1, 3], [0, 2], [3, 0])             # rows of the shared (p, T) = (2, 2) case per input set


class Lut2(Case):
    """p = 2, T = 2, both functions of l2.shared_case on 2 rows: level 1, the pack and level 2 in one call.  A job's words do
    not depend on its place in a call, so every input set is a pair of rows of the shared case"""
    rows = 2

    def setup(self):
        eoc = self.eoc
        self.p, self.sk, blob = l2.keys(eoc, 0)[:3]
        self.case = l2.shared_case(eoc, 0, 2, 2)
        self.eng2 = tp.keys(eoc, 0)[4]                          # the same key seed: cloud key and packing key
        self.fresh(self.p).load_cloud_key(self.sk)
        self.eng.load_packing_key(blob)
        self.d_tv = to_dev(self.case["tv0"].reshape(-1, N).copy())
        self.keep.append(self.d_tv)

    def alloc(self):
        return dict(x=self.new((self.rows, self.p.n + 1)), y=self.new((self.rows, self.p.n + 1)), out=self.new((2, self.rows, self.p.n + 1)))

    def load(self, b, k):
        b["x"].copy_(to_dev(self.case["x"][ROW_SETS[k]]))
        b["y"].copy_(to_dev(self.case["y"][ROW_SETS[k]]))

    def lut2(self, eng, b, n_funcs, rows, st):
        eng.lut2_batch_device(2, 2, self.d_tv.data_ptr(), n_funcs, b["x"].data_ptr(), b["y"].data_ptr(), b["out"].data_ptr(), rows,
                              stream=st)

    def call(self, eng, b, st):
        self.lut2(eng, b, 2, self.rows, st)

    def ref(self, k):
        return dict(out=self.case["out"][:, ROW_SETS[k]])

    def other(self):
        self.lut2(self.eng, self.dbufs[0], 1, 1, None)


class LutEnc(Lut2):
    """level 2 alone, one list per (function, row): the lists are the shared case's"""
    def alloc(self):
        b = Lut2.alloc(self)
        b["lists"] = self.new((2, self.rows, 2, N))
        return b

    def load(self, b, k):
        b["lists"].copy_(to_dev(self.case["lists"][:, ROW_SETS[k]]))
        b["y"].copy_(to_dev(self.case["y"][ROW_SETS[k]]))

    def lut2(self, eng, b, n_funcs, rows, st):
        eng.lut_enc_batch_device(b["lists"].data_ptr(), n_funcs, True, b["y"].data_ptr(), b["out"].data_ptr(), rows, stream=st)


# ---- what a server captures -------------------------------------------------------------------------------------------------
class Composed(TableRead):
    """one graph: compact lists -> 16 samples; NAND of the first 8 with the last 8; a table read (log2_lists = 1, one query)
    whose selectors are converted inside the graph; the 8 gate outputs packed into a list.  Replays see new lists and new
    selectors; every stage is compared with the composition of the references"""
    S, d, lw, queries = 8, 1, 9, 1
    expect = dict(cmux_launches=2, pack_launches=1)

    def setup(self):
        eoc = self.eoc
        self.p, self.sk, blob, self.kfft, self.gate_orc = l2.keys(eoc, 0)
        self.pk, self.orc, self.eng2 = eoc.PublicKey(self.sk.public_key_bytes()), tc.keys(eoc, 0)[3], tp.keys(eoc, 0)[4]
        self.op, self.kpl = cx.orc_params(self.p), 2 * self.p.l
        self.depth, self.W = self.d + 10 - self.lw, 1 << self.lw
        self.fresh(self.p).load_cloud_key(self.sk)
        self.eng.load_packing_key(blob)
        rng = np.random.default_rng(59)
        self.table = tc.make_table(eoc, self.pk, "bits", self.d, rng, 671)[0]
        self.d_tab = to_dev(self.table)
        self.keep.append(self.d_tab)
        self.inp = [dict(lists=self.pk.encrypt_bits(rng.integers(0, 2, 2 * self.S).astype(np.uint8), enc_seed=400 + k),
                         sel=tc.index_selectors(self.sk, [(k + 1) % 4], self.depth, enc_seed=770 + k)) for k in range(5)]

    def alloc(self):
        n1 = self.p.n + 1
        return dict(lists=self.new((1, 2, N)), exp=self.new((2 * self.S, n1)), gate=self.new((self.S, n1)),
                    sel=self.new((self.depth, self.kpl, 2, N)), fft=self.new((self.depth, self.kpl, 2, N), self.torch.float64),
                    read=self.new((1, self.W, n1)), packed=self.new((1, 2, N)))

    def load(self, b, k):
        b["lists"].copy_(to_dev(self.inp[k]["lists"]))
        b["sel"].copy_(to_dev(self.inp[k]["sel"].reshape(self.depth, self.kpl, 2, N)))

    def call(self, eng, b, st):
        S, row = self.S, (self.p.n + 1) * 4
        eng.compact_expand_device(b["lists"].data_ptr(), 2 * S, b["exp"].data_ptr(), stream=st)
        eng.gate_batch_device(self.eoc.OPS["NAND"], b["exp"].data_ptr(), b["exp"].data_ptr() + S * row, None, b["gate"].data_ptr(), S,
                              stream=st)
        eng.tgsw_to_fft_device(b["sel"].data_ptr(), self.depth, b["fft"].data_ptr(), stream=st)
        eng.table_read_device(self.d_tab.data_ptr(), self.d, self.lw, b["fft"].data_ptr(), 1, b["read"].data_ptr(), stream=st)
        eng.pack_device(b["gate"].data_ptr(), S, b["packed"].data_ptr(), stream=st)

    def outs(self, b):
        return [b[name] for name in ("exp", "gate", "fft", "read", "packed")]

    def read(self, b):
        return {name: b[name].cpu().numpy() for name in ("exp", "gate", "fft", "read", "packed")}

    def pick(self, name, a):
        return a[:, self.WS] if name == "read" else a

    def ref(self, k):
        i, S = self.inp[k], self.S
        exp = co.expand(self.orc, i["lists"], np.arange(2 * S))
        gate = self.gate_orc.gate_batch(ol.OPS["NAND"], exp[:S], exp[S:])
        sel = i["sel"].reshape(self.depth, self.kpl, 2, N)
        fft = cx.to_fft(sel)
        sample = cx.table_read_tlwe(self.op, self.table, self.d, self.lw, fft)
        read = co.expand(self.orc, sample[None], self.WS).reshape(1, len(self.WS), self.p.n + 1)
        return dict(exp=exp, gate=gate, fft=fft * 2.0**-9, read=read, packed=po.pack(self.p.n, self.kfft, gate))

    def other(self):
        b = self.dbufs[0]
        self.eng.compact_expand_device(b["lists"].data_ptr(), 5, b["exp"].data_ptr())
        self.eng.gate_batch_device(self.eoc.OPS["XOR"], b["exp"].data_ptr(), b["exp"].data_ptr(), None, b["gate"].data_ptr(), 3)
        self.eng.pack_device(b["exp"].data_ptr(), 2, b["packed"].data_ptr())


CASES = {
    "setB-gate-cut-rotation": SetBGate,
    "mux-level": MuxLevel,
    "blind-rotate-keyswitch": BlindRotateKeyswitch,
    "lut": Lut,
    "lut-wide": LutWide,
    "lut-many": LutMany,
    "int-circuit": IntCircuit,
    "int-circuit-sliced": IntCircuitSliced,
    "compact-expand": CompactExpand,
    "seeded-expand": SeededExpand,
    "seeded-selector": SeededSelector,
    "tgsw-to-fft": TgswToFft,
    "cmux": Cmux,
    "table-read": TableRead,
    "table-read-sliced": TableReadSliced,
    "demux": Demux,
    "demux-accumulate": DemuxAccumulate,
    "table-update": TableUpdate,
    "pack": Pack,
    "pack-sliced": PackSliced,
    "tv-pack": TvPack,
    "lut-enc": LutEnc,
    "lut2": Lut2,
    "composed": Composed,
}
