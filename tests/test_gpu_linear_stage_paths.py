"""Every path through the linear stage and the mod switch in front of a blind rotation, on the MI355X, with every word of
the stage's result on the end of a rounding cell (tests/lin_edge_inputs.py): prepare_row folded into the pair and the wide
blind-rotation kernels (descriptor as a kernel argument, descriptors from the ring, OP_MULTI rows, the two-launch blind
rotation of gadget length 3), k_prepare as a launch of its own (EOC_TFHE_NO_FOLD, MUX alone and in a pool, MAJ / XOR3),
k_free_gates, k_modswitch_coarse at theta = 2, and the eight k_lin_modswitch<terms, boot> instances.  One test id per path.

The operands are solved so that the stage yields a wanted row t* exactly; what the gate computes then depends on t* alone,
so ONE oracle reference per set of target rows -- keyswitch(blind_rotate_extract(t*)), or the table-lookup composition of
tests/test_gpu_br_instances.py::oracle_lut -- serves every opcode and path (tests/test_lin_edge_inputs_cpu.py ties it to the
oracle's own gate).  Shapes: Set A's gadget at n = 260 with 35 rows per opcode -- 261 words are a third pass of
prepare_row's 128-thread stride and a fifth of its 64-lane one, put word n (the only one that takes the constant) into
blockIdx.y = 1 of k_prepare / k_lin_modswitch, and 35 is no multiple of any kernel's jobs per workgroup -- and n = 1 with
the rotation sweep as target rows where a path needs every amount.  Every id asserts, beside the words, that its path ran.
GPU == oracle, word for word; nothing is decrypted."""
import time

import numpy as np
import pytest

import br_edge_inputs as bei
import lin_edge_inputs as lei
import lut_many_oracle as lmo
import test_gpu_br_instances as tbi
from gpu_util import dev_empty, sync, to_dev, torch_cuda

pytestmark = pytest.mark.gpu
N = 1024
MU = 1 << 29
SET_A, SET_B = (2, 10), (3, 7)
NBIG, ROWS = 260, 35
KNOBS = tbi.ENV_KNOBS + ("EOC_TFHE_NO_FOLD", "EOC_TFHE_NO_POOL", "EOC_TFHE_INT_SLICE_ROWS")
PAIR, WIDE = {"EOC_TFHE_BR_WIDE": "0"}, {"EOC_TFHE_BR_WIDE": "1"}
NO_FOLD = {"EOC_TFHE_NO_FOLD": "1"}
READBACKS = ("vabar", "sabar")


@pytest.fixture(scope="module")
def eoc(built_lib):
    torch_cuda()
    import eoc_tfhe_amd
    return eoc_tfhe_amd


# -- target rows and their references, shared by all ids ----------------------------------------------------------------
_TARGETS, _CLOCK = {}, {"ref": 0.0, "gpu": 0.0}


def gate_targets(name):
    """'odd' (the +-1 opcodes), 'even' (the doubling ones) and 'mux2' (MUX's second stage): int32 [35][261]"""
    if name not in _TARGETS:
        _TARGETS[name] = lei.targets(NBIG, ROWS, name == "even", {"odd": 1, "even": 2, "mux2": 3}[name])
        _TARGETS[name].setflags(write=False)
    return _TARGETS[name]


def lut_targets(T):
    """35 edge rows on the grid of T at n = 260"""
    if T not in _TARGETS:
        _TARGETS[T] = lei.targets(NBIG, ROWS, False, 40 + T, n_tables=T)
        _TARGETS[T].setflags(write=False)
    return _TARGETS[T]


def timed_reference(key, compute):
    t0 = time.perf_counter()
    want = tbi.reference(key, compute)
    _CLOCK["ref"] += time.perf_counter() - t0
    return want


def extracted(eoc, gadget, name):
    """blind_rotate_extract of the target rows `name`: [35][N+1], before the key switch (MUX adds two of them)"""
    orc = tbi.keys(eoc, *gadget, NBIG)[2]
    return timed_reference(gadget + (NBIG, "lin-u", name), lambda: tbi.oracle_gate(orc, gate_targets(name)))


def gate_reference(eoc, gadget, name):
    """what EVERY bootstrapped gate gives whose linear stage is the target rows `name`: [35][261]"""
    orc = tbi.keys(eoc, *gadget, NBIG)[2]
    u = extracted(eoc, gadget, name)
    return timed_reference(gadget + (NBIG, "lin-gate", name), lambda: np.stack([orc.keyswitch(r) for r in u]))


def mux_reference(eoc, gadget):
    orc = tbi.keys(eoc, *gadget, NBIG)[2]
    u = extracted(eoc, gadget, "odd").astype(np.int64) + extracted(eoc, gadget, "mux2")
    u[:, N] += MU
    return timed_reference(gadget + (NBIG, "lin-mux"), lambda: np.stack([orc.keyswitch(r) for r in lei.wrap32(u)]))


def lut_tvs(eoc, n, T):
    tvs = tbi.lut_polys(eoc, *SET_A, n, T)
    return tvs if n == 1 else np.ascontiguousarray(tvs[[0, 2]])       # n = 260: the real table and the alternating polynomial


def lut_reference_big(eoc, T):
    """[2][35][261] (T = 1) or [2][T][35][261]: the lookups of lut_tvs(260, T) on lut_targets(T)"""
    orc = tbi.keys(eoc, *SET_A, NBIG)[2]
    return timed_reference(SET_A + (NBIG, "lin-lut", T), lambda: tbi.oracle_lut(orc, T, lut_tvs(eoc, NBIG, T), lut_targets(T)))


def lut_reference_sweep(eoc, T):
    """(target rows [R][2], reference [2][T][R][2]) at n = 1: the rows of the rotation sweep that
    tests/test_gpu_br_instances.py compares (the same cache entries; T = 4 is new)"""
    orc = tbi.keys(eoc, *SET_A, 1)[2]
    rows = bei.sweep(T)[0]
    pick = bei.sweep_subset(T) if T <= 2 else np.arange(rows.shape[0])
    tvs = lut_tvs(eoc, 1, T)
    want = timed_reference(SET_A + (1, "tv" if T == 1 else "many", T), lambda: tbi.oracle_lut(orc, T, tvs, rows[pick]))
    return rows[pick], (want[:, None] if T == 1 else want)


# -- engines and the counters that say which path ran -------------------------------------------------------------------
def make_engine(eoc, monkeypatch, gadget, n, env, readback="vabar"):
    p, sk, orc = tbi.keys(eoc, *gadget, n)
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    eng = tbi.engine(eoc, monkeypatch, p, env, readback)
    eng.load_cloud_key(sk)
    eng.set_profiling(True)
    return eng


class Probe:
    """what moved between its creation and done(): prepare spans (k_prepare / k_lin_modswitch / k_modswitch_coarse ran: 0 when
    the prologue is folded), blind-rotate spans and launches, wide launches, bootstraps, batches"""

    def __init__(self, eng):
        self.eng, self.t0 = eng, time.perf_counter()
        eng.kernel_times()
        self.before = eng.stats()

    def done(self):
        kt, st = self.eng.kernel_times(), self.eng.stats()
        _CLOCK["gpu"] += time.perf_counter() - self.t0
        d = {k: st[k] - self.before[k] for k in ("br_launches", "br_wide_launches", "bootstraps", "batches", "keyswitches")}
        d.update(prep=kt["prepare"]["launches"], br_spans=kt["blind_rotate"]["launches"])
        return d


def assert_shape(moved, env):
    """the blind rotation ran on the kernel shape the environment asks for"""
    if env.get("EOC_TFHE_BR_WIDE") == "1":
        assert moved["br_wide_launches"] == moved["br_launches"] > 0, moved
    elif env.get("EOC_TFHE_BR_WIDE") == "0":
        assert moved["br_wide_launches"] == 0 < moved["br_launches"], moved


def assert_words(what, got, want):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert bad.size == 0, (what, len(bad), "first (row, word): " + str(bad[:6].tolist()))


def report(name, rows, shares):
    """one line per id, the figures DESIGN.md quotes: rows through the path, share of words whose exact sum wrapped, wall
    time of the device calls with their copies, time of the references this id was the first to need"""
    share = f"{100 * float(np.mean(shares)):.1f} %" if len(shares) else "n/a"
    print(f"\nLINPATH {name}: rows {rows}, wrapped {share}, gpu {1e3 * _CLOCK['gpu']:.0f} ms, reference {_CLOCK['ref']:.2f} s")
    _CLOCK["gpu"] = _CLOCK["ref"] = 0.0


def dev_gate(eng, op, operands, count, ops=None, width=NBIG + 1):
    d = [None if x is None else to_dev(x) for x in operands] + [None] * (3 - len(operands))
    out = dev_empty((count, width), torch_cuda().int32)
    eng.gate_batch_device(op, *[None if x is None else x.data_ptr() for x in d], out.data_ptr(), count, ops=ops)
    sync()
    return out.cpu().numpy()


def target_name(op):
    return "even" if op in lei.DOUBLING else "odd"


_SOLVED = {}


def solved(op):
    """(operand rows, share of wrapped words) of opcode op on its 35 target rows"""
    if op not in _SOLVED:
        if op == lei.OP_MUX:
            rows = lei.solve(op, gate_targets("odd"), 500 + op, gate_targets("mux2"))
            wr = lei.wrapped(lei.exact_sum(1, rows[:2])) | lei.wrapped(lei.exact_sum(6, (rows[0], rows[2])))
        else:
            rows = lei.solve(op, gate_targets(target_name(op)), 500 + op)
            wr = lei.wrapped(lei.exact_sum(op, rows))
            assert np.array_equal(lei.linear(op, rows), gate_targets(target_name(op)))
        _SOLVED[op] = (rows, float(wr.mean()))
    return _SOLVED[op]


def level_of_gates(eoc, ops):
    """one circuit level, one gate per opcode on wires of its own: (gates, wires [n_wires][35][261], output wire per gate)"""
    gates, wires, outs = [], [], []
    for op in ops:
        rows = solved(op)[0]
        first = len(wires)
        wires += list(rows) + [np.zeros_like(rows[0])]
        ins = list(range(first, first + len(rows))) + [-1] * (3 - len(rows))
        gates.append(eoc.Gate(op, ins[0], ins[1], ins[2], first + len(rows)))
        outs.append(first + len(rows))
    return gates, np.ascontiguousarray(np.stack(wires)), outs


def run_circuit(eng, gates, wires):
    d_w = to_dev(wires)
    eng.circuit_run_device(gates, d_w.data_ptr(), wires.shape[0], wires.shape[1])
    sync()
    return d_w.cpu().numpy()


def scrambled_ops(per_op, seed):
    """every opcode of per_op {op: rows} that often, in a scrambled order without a period; and for every row the index of
    its target row: its rank among the rows of its opcode"""
    ops = np.repeat(np.array(list(per_op), np.uint8), list(per_op.values()))
    ops = ops[np.random.default_rng(seed).permutation(ops.size)]
    rank = np.zeros(ops.size, np.int64)
    for op in per_op:
        rank[ops == op] = np.arange(per_op[op])
    return ops, rank


def mixed_batch(ops, rank, free_rows):
    """operand rows (in0, in1, in2) and expected-row recipe of a mixed batch: every row's operands are solved for ITS opcode"""
    in0, in1, in2 = (np.zeros((ops.size, NBIG + 1), np.int32) for _ in range(3))
    for op in np.unique(ops):
        m = ops == op
        if op in (lei.OP_NOT, lei.OP_COPY, lei.OP_CONST0, lei.OP_CONST1):
            in0[m] = free_rows[rank[m]]
            continue
        rows = solved(int(op))[0]
        for dst, src in zip((in0, in1, in2), rows):
            dst[m] = src[rank[m]]
    return in0, in1, in2


def mixed_expected(eoc, gadget, ops, rank, in0):
    want = np.zeros((ops.size, NBIG + 1), np.int32)
    for op in np.unique(ops):
        m, op = ops == op, int(op)
        if op == lei.OP_NOT:
            want[m] = lei.wrap32(-in0[m].astype(np.int64))
        elif op == lei.OP_COPY:
            want[m] = in0[m]
        elif op in (lei.OP_CONST0, lei.OP_CONST1):
            want[m, NBIG] = MU if op == lei.OP_CONST1 else -MU
        elif op == lei.OP_MUX:
            want[m] = mux_reference(eoc, gadget)[rank[m]]
        else:
            want[m] = gate_reference(eoc, gadget, target_name(op))[rank[m]]
    return want


# -- prepare_row: the folded prologue ------------------------------------------------------------------------------------
def run_inline(eoc, monkeypatch, env, folded, ops=lei.TWO_INPUT, gadget=SET_A, parts=1):
    shares = []
    for readback in READBACKS:
        eng = make_engine(eoc, monkeypatch, gadget, NBIG, env, readback)
        for op in ops:
            rows, share = solved(op)
            probe = Probe(eng)
            got = dev_gate(eng, op, rows, ROWS)
            moved = probe.done()
            assert moved["prep"] == (0 if folded else 1) and moved["br_spans"] == 1 and moved["bootstraps"] == ROWS, (op, moved)
            assert moved["br_launches"] == parts, (op, moved)
            assert_shape(moved, env)
            assert_words((op, readback), got, gate_reference(eoc, gadget, target_name(op)))
            shares.append(share)
        eng.close()
    return shares


def run_descs(eoc, monkeypatch, env, folded):
    gates, wires, outs = level_of_gates(eoc, lei.TWO_INPUT)
    for readback in READBACKS:
        eng = make_engine(eoc, monkeypatch, SET_A, NBIG, env, readback)
        probe = Probe(eng)
        got = run_circuit(eng, gates, wires)
        moved = probe.done()
        eng.close()
        assert moved["prep"] == (0 if folded else 1) and moved["br_launches"] == 1 and moved["bootstraps"] == 10 * ROWS, moved
        assert_shape(moved, env)
        for op, w in zip(lei.TWO_INPUT, outs):
            assert_words((op, readback), got[w], gate_reference(eoc, SET_A, target_name(op)))
        keep = np.setdiff1d(np.arange(wires.shape[0]), outs)
        assert np.array_equal(got[keep], wires[keep])                  # operand wires untouched
    return [solved(op)[1] for op in lei.TWO_INPUT]


def run_multi(eoc, monkeypatch, env, folded):
    ops, rank = scrambled_ops({op: ROWS for op in lei.TWO_INPUT}, 77)
    assert 1 + np.count_nonzero(np.diff(ops)) > 15                     # more runs than opcodes: gathered into sorted order
    assert all((ops[k:] != ops[:-k]).any() for k in range(1, ops.size))    # no period
    in0, in1, in2 = mixed_batch(ops, rank, None)
    bar = lmo.modswitch_coarse(np.stack([gate_targets(target_name(int(o)))[r] for o, r in zip(ops, rank)]))
    for other in lei.TWO_INPUT:                                        # any other opcode on a row's operands rounds elsewhere
        m = ops != other
        assert (lmo.modswitch_coarse(lei.linear(other, (in0[m], in1[m]))) != bar[m]).any(axis=1).all(), other
    want = mixed_expected(eoc, SET_A, ops, rank, in0)
    for readback in READBACKS:
        eng = make_engine(eoc, monkeypatch, SET_A, NBIG, env, readback)
        probe = Probe(eng)
        got = dev_gate(eng, 0, (in0, in1), ops.size, ops=ops)
        moved = probe.done()
        eng.close()
        assert moved["prep"] == (0 if folded else 1) and moved["br_spans"] == 1 and moved["bootstraps"] == ops.size, moved
        assert_words(("multi", readback), got, want)
    return [solved(op)[1] for op in lei.TWO_INPUT]


def path_folded_inline(eoc, monkeypatch, name, shape):
    """prepare_row with the descriptor as a kernel argument (eoc_gate_batch_device of one opcode), all ten two-input
    opcodes, 128 threads per row (pair) and 64 lanes (wide), both read-back forms of the rotation amounts"""
    shares = run_inline(eoc, monkeypatch, PAIR if shape == "pair" else WIDE, True)
    report(name, 2 * 10 * ROWS, shares)


def path_folded_descs(eoc, monkeypatch, name, shape):
    """ks_descs[gjob / S], instance gjob - g S: one circuit level of ten gates, one per opcode, on wires of their own"""
    shares = run_descs(eoc, monkeypatch, PAIR if shape == "pair" else WIDE, True)
    report(name, 2 * 10 * ROWS, shares)


def path_folded_multi(eoc, monkeypatch, name):
    """OP_MULTI: 350 rows of the ten opcodes in scrambled order, every row's operands solved for its own opcode -- the
    opcode bits of the permutation word, k_gather_rows both ways"""
    shares = run_multi(eoc, monkeypatch, {}, True)
    report(name, 2 * 10 * ROWS, shares)


def path_folded_setB_two_parts(eoc, monkeypatch, name):
    """gadget length 3 (l = 3, Bgbit = 7) at n = 260: the shipped rule cuts every blind rotation into two launches; the
    second (step_begin > 0) must neither redo nor lose the prologue's row.  NAND and XOR."""
    shares = run_inline(eoc, monkeypatch, {}, True, ops=(0, 4), gadget=SET_B, parts=2)
    report(name, 2 * 2 * ROWS, shares)


# -- k_prepare as a launch of its own ------------------------------------------------------------------------------------
def path_unfolded(eoc, monkeypatch, name, form):
    """the three forms above under EOC_TFHE_NO_FOLD=1: k_prepare's two-operand branch"""
    shares = dict(inline=run_inline, descs=run_descs, multi=run_multi)[form](eoc, monkeypatch, NO_FOLD, False)
    report(name, 2 * 10 * ROWS, shares)


def path_mux(eoc, monkeypatch, name):
    """MUX alone: k_prepare's variants 0 (AND(a, b)) and 1 (ANDNY(a, c)) over 2 x 35 jobs, k_ks_init's sum of the two"""
    rows, share = solved(lei.OP_MUX)
    eng = make_engine(eoc, monkeypatch, SET_A, NBIG, {})
    probe = Probe(eng)
    got = dev_gate(eng, lei.OP_MUX, rows, ROWS)
    moved = probe.done()
    eng.close()
    assert moved["prep"] == 1 and moved["br_spans"] == 1 and moved["bootstraps"] == 2 * ROWS and moved["keyswitches"] == ROWS, moved
    assert_words("mux", got, mux_reference(eoc, SET_A))
    report(name, ROWS, [share])


def path_mux_in_pool(eoc, monkeypatch, name):
    """MUX rows among two-input rows and NOT / COPY / CONST0 / CONST1 rows, ONE pooled blind rotation: gathered (scrambled
    order: OP_MULTI block at job 0, the MUX run behind it) and in a few runs (MUX first: job_base = 70 for the next run)"""
    free_rows = lei.free_gate_rows()
    per_op = {1: ROWS, 4: ROWS, 8: ROWS, 3: ROWS, lei.OP_MUX: ROWS, lei.OP_NOT: 9, lei.OP_COPY: 9, lei.OP_CONST0: 5, lei.OP_CONST1: 5}
    ops_g, rank_g = scrambled_ops(per_op, 78)
    runs = [(lei.OP_MUX, 20), (1, ROWS), (lei.OP_NOT, 9), (4, ROWS), (lei.OP_CONST1, 5), (lei.OP_MUX, 15), (lei.OP_COPY, 9), (9, ROWS)]
    ops_f = np.concatenate([np.full(c, o, np.uint8) for o, c in runs])
    rank_f = np.concatenate([np.arange(c) for _, c in runs])
    rank_f[ops_f == lei.OP_MUX] = np.arange(ROWS)                       # the second MUX run goes on where the first ended
    eng = make_engine(eoc, monkeypatch, SET_A, NBIG, {})
    for what, ops, rank in (("gathered", ops_g, rank_g), ("few-runs", ops_f, rank_f)):
        assert (1 + np.count_nonzero(np.diff(ops)) > 15) == (what == "gathered")
        in0, in1, in2 = mixed_batch(ops, rank, free_rows)
        want = mixed_expected(eoc, SET_A, ops, rank, in0)
        jobs = int(np.sum(ops < lei.OP_MUX) + 2 * np.sum(ops == lei.OP_MUX))
        probe = Probe(eng)
        got = dev_gate(eng, 0, (in0, in1, in2), ops.size, ops=ops)
        moved = probe.done()
        assert moved["br_spans"] == 1 and moved["prep"] == 1 and moved["batches"] == 1 and moved["bootstraps"] == jobs, (what, moved)
        assert_words(what, got, want)
    eng.close()
    report(name, ops_g.size + ops_f.size, [solved(o)[1] for o in (1, 4, 8, 3, 9, lei.OP_MUX)])


def path_maj_xor3(eoc, monkeypatch, name):
    """gate_lin3's branch of k_prepare with the key-switch set-up still folded (fold = KS): MAJ and XOR3 as batches, and one
    circuit level holding both and a two-input gate"""
    eng = make_engine(eoc, monkeypatch, SET_A, NBIG, {})
    for op in (lei.OP_MAJ, lei.OP_XOR3):
        probe = Probe(eng)
        got = dev_gate(eng, op, solved(op)[0], ROWS)
        moved = probe.done()
        assert moved["prep"] == 1 and moved["br_spans"] == 1 and moved["bootstraps"] == ROWS, (op, moved)
        assert_words(op, got, gate_reference(eoc, SET_A, target_name(op)))
    level = (lei.OP_XOR3, 6, lei.OP_MAJ)
    gates, wires, outs = level_of_gates(eoc, level)
    probe = Probe(eng)
    got = run_circuit(eng, gates, wires)
    moved = probe.done()
    eng.close()
    assert moved["prep"] == 1 and moved["br_launches"] == 1 and moved["bootstraps"] == 3 * ROWS, moved
    for op, w in zip(level, outs):
        assert_words(("level", op), got[w], gate_reference(eoc, SET_A, target_name(op)))
    report(name, 5 * ROWS, [solved(op)[1] for op in level])


def path_free_gates(eoc, monkeypatch, name):
    """k_free_gates: NOT (the negation of INT32_MIN included), COPY, CONST0 / CONST1 (the b-word test i % rowlen at row
    length 261) as batches and as a circuit's pre-pass in front of a bootstrapped gate; plain numpy is the reference"""
    x = lei.free_gate_rows()
    neg = lei.wrap32(-x.astype(np.int64))
    assert (neg[x == lei.INT32_MIN] == lei.INT32_MIN).all()
    const = np.zeros((2, ROWS, NBIG + 1), np.int32)
    const[0, :, NBIG], const[1, :, NBIG] = -MU, MU
    eng = make_engine(eoc, monkeypatch, SET_A, NBIG, {})
    probe = Probe(eng)
    assert_words("NOT", dev_gate(eng, lei.OP_NOT, (x,), ROWS), neg)
    assert_words("COPY", dev_gate(eng, lei.OP_COPY, (x,), ROWS), x)
    assert_words("CONST0", dev_gate(eng, lei.OP_CONST0, (None,), ROWS), const[0])
    assert_words("CONST1", dev_gate(eng, lei.OP_CONST1, (None,), ROWS), const[1])
    moved = probe.done()
    assert moved["bootstraps"] == 0 and moved["br_launches"] == 0 and moved["prep"] == 0, moved
    a, b = solved(0)[0]
    wires = np.ascontiguousarray(np.stack([x, a, b] + [np.full_like(x, 0x5A5A5A5A)] * 5))
    G, O = eoc.Gate, eoc.OPS
    gates = [G(O["NOT"], 0, -1, -1, 3), G(O["COPY"], 0, -1, -1, 4), G(O["CONST0"], -1, -1, -1, 5), G(O["CONST1"], -1, -1, -1, 6),
             G(O["NAND"], 1, 2, -1, 7)]
    probe = Probe(eng)
    got = run_circuit(eng, gates, wires)
    moved = probe.done()
    eng.close()
    assert moved["bootstraps"] == ROWS and moved["prep"] == 0, moved
    for what, w, want in (("NOT", 3, neg), ("COPY", 4, x), ("CONST0", 5, const[0]), ("CONST1", 6, const[1]),
                          ("NAND", 7, gate_reference(eoc, SET_A, "odd"))):
        assert_words(("circuit", what), got[w], want)
    assert np.array_equal(got[:3], wires[:3])
    report(name, 9 * ROWS, [])


# -- k_modswitch_coarse at theta = 2 -------------------------------------------------------------------------------------
def path_coarse_T4(eoc, monkeypatch, name):
    """many-LUT bootstrapping with T = 4: every amount of the grid of 4 from both ends of its cell at n = 1 (the sweep,
    2 048 rows), and 35 rows of edge words at n = 260"""
    T = 4
    for n in (1, NBIG):
        tvs = lut_tvs(eoc, n, T)
        rows, want = lut_reference_sweep(eoc, T) if n == 1 else (lut_targets(T), lut_reference_big(eoc, T))
        eng = make_engine(eoc, monkeypatch, SET_A, n, {})
        probe = Probe(eng)
        got = tbi.run_lut(eng, T, tvs, np.array(rows))
        moved = probe.done()
        eng.close()
        assert moved["prep"] >= 1 and moved["bootstraps"] == tvs.shape[0] * rows.shape[0], (n, moved)
        assert moved["keyswitches"] == T * tvs.shape[0] * rows.shape[0], (n, moved)
        bad = np.argwhere((got != want).any(axis=-1))
        assert got.shape == want.shape and bad.size == 0, (n, len(bad), bad[:8].tolist())
    report(name, 2 * (2 * 2 * N // T) + ROWS, [])


# -- k_lin_modswitch<terms, boot> ----------------------------------------------------------------------------------------
def inode(eoc, T, out, tv, ins, w, cst, n_terms=None):
    q = eoc.INode()
    q.n_tables, q.out, q.tv, q.cst = T, out, tv, int(cst)
    q.n_terms = len(ins) if n_terms is None else n_terms
    for k in range(len(ins)):
        q.in_[k], q.w[k] = ins[k], int(w[k])
    return q


class Netlist:
    """nodes on wires of their own: operand rows in, expected rows per written wire out"""

    def __init__(self, eoc, instances, n):
        self.eoc, self.shape = eoc, (instances, n + 1)
        self.wires, self.nodes, self.tvs, self.expect, self.shares = [], [], [], {}, []

    def wire(self, rows=None):
        self.wires.append(np.full(self.shape, 0x3C3C3C3C, np.int32) if rows is None else np.asarray(rows, np.int32))
        return len(self.wires) - 1

    def solved_node(self, T, tv, t_star, want, terms, seed, which_cst):
        """a node of `terms` terms whose linear stage is t_star; T = 0: a free node (want = None: its wire must be t_star)"""
        w, cst = lei.node_weights(terms, seed), lei.node_cst(which_cst, seed)
        xs = lei.solve_node(w, cst, t_star, seed)
        assert np.array_equal(lei.node_linear(w, cst, xs), t_star)
        exact = lei.node_exact(w, cst, xs)
        self.shares.append(float(np.mean((exact < lei.INT32_MIN) | (exact > lei.INT32_MAX))))
        ins = [self.wire(x) for x in xs]
        outs = [self.wire() for _ in range(max(T, 1))]
        self.nodes.append(inode(self.eoc, T, outs[0], self.tv_index(tv), ins, w, cst))
        for j, o in enumerate(outs):
            self.expect[o] = t_star if T == 0 else want[j]
        return outs

    def tv_index(self, tv):
        if tv is None:
            return 0
        self.tvs.append(tv)
        return len(self.tvs) - 1

    def run(self, eng):
        wires = np.ascontiguousarray(np.stack(self.wires))
        tvs = np.ascontiguousarray(np.stack(self.tvs))
        assert self.eoc.int_netlist_levels(self.nodes, len(self.wires), len(self.tvs))[1] >= 1      # a valid netlist
        d_tv, d_w = to_dev(tvs), to_dev(wires)
        eng.int_circuit_run_device(self.nodes, d_tv.data_ptr(), tvs.shape[0], d_w.data_ptr(), wires.shape[0], wires.shape[1])
        sync()
        got = d_w.cpu().numpy()
        for w in range(len(self.wires)):
            want = self.expect.get(w, wires[w])                        # operand wires stay as they were
            bad = np.argwhere((got[w] != want).any(axis=-1))
            assert bad.size == 0, ("wire", w, len(bad), bad[:8].ravel().tolist())
        return got


def tile_rows(a, count, axis=0):
    return np.take(a, np.arange(count) % a.shape[axis], axis=axis)


def path_lin_boot(eoc, monkeypatch, name, terms):
    """k_lin_modswitch<terms, true>: one level of four nodes of exactly `terms` terms, T = 1, 2, 4, 8 (theta = 0 .. 3), with
    the extreme weights and constants of lin_edge_inputs -- at n = 1 on the rotation sweep of every T (4 096 instances: the
    shorter sweeps repeat), at n = 260 on 35 edge rows for T = 1 and 4; against the lookup composition of t*"""
    inst = 4096
    net = Netlist(eoc, inst, 1)
    for j, T in enumerate((1, 2, 4, 8)):
        rows, want = lut_reference_sweep(eoc, T)
        net.solved_node(T, lut_tvs(eoc, 1, T)[0], tile_rows(rows, inst), tile_rows(want[0], inst, axis=1), terms, 600 + 10 * terms + j, j)
    eng = make_engine(eoc, monkeypatch, SET_A, 1, {})
    probe = Probe(eng)
    net.run(eng)
    moved = probe.done()
    eng.close()
    assert moved["prep"] == 4 and moved["br_spans"] == 4 and moved["bootstraps"] == 4 * inst and moved["keyswitches"] == 15 * inst, moved
    big = Netlist(eoc, ROWS, NBIG)
    for j, T in enumerate((1, 4)):
        want = lut_reference_big(eoc, T)[0]
        big.solved_node(T, lut_tvs(eoc, NBIG, T)[0], lut_targets(T), want[None] if T == 1 else want, terms, 700 + 10 * terms + j, j + 2)
    eng = make_engine(eoc, monkeypatch, SET_A, NBIG, {})
    probe = Probe(eng)
    big.run(eng)
    moved = probe.done()
    eng.close()
    assert moved["prep"] == 2 and moved["br_spans"] == 2 and moved["bootstraps"] == 2 * ROWS and moved["keyswitches"] == 5 * ROWS, moved
    report(name, 4 * inst + 2 * ROWS, net.shares + big.shares)


def path_lin_boot_mixed_terms(eoc, monkeypatch, name):
    """the k < n_terms guard inside <4, true>: one T = 1 group holding a 1-term node -- its unused w[] entries non-zero, its
    unused in[] entries wire 0, which holds full-range words -- and a 4-term node"""
    want = lut_reference_big(eoc, 1)[0]
    tv = lut_tvs(eoc, NBIG, 1)[0]
    net = Netlist(eoc, ROWS, NBIG)
    net.wire(np.random.default_rng(9).integers(lei.INT32_MIN, lei.INT32_MAX + 1, (ROWS, NBIG + 1)))     # wire 0
    (out1,) = net.solved_node(1, tv, lut_targets(1), want[None], 1, 801, 1)
    q = net.nodes[0]
    assert q.n_terms == 1 and [q.in_[k] for k in (1, 2, 3)] == [0, 0, 0]
    q.w[1], q.w[2], q.w[3] = 0x10001, -3, lei.INT32_MIN
    net.solved_node(1, tv, lut_targets(1), want[None], 4, 802, 3)
    assert [x.n_terms for x in net.nodes] == [1, 4]
    eng = make_engine(eoc, monkeypatch, SET_A, NBIG, {})
    probe = Probe(eng)
    net.run(eng)
    moved = probe.done()
    eng.close()
    assert moved["prep"] == 1 and moved["br_spans"] == 1 and moved["bootstraps"] == 2 * ROWS, moved
    report(name, 2 * ROWS, net.shares)


def path_lin_free(eoc, monkeypatch, name, terms):
    """k_lin_modswitch<terms, false>: a free node of `terms` terms whose wire is t* (compared with the numpy wrapping sum),
    and a T = 1 node of one unit term reading it (compared with the lookup composition of t*)"""
    want = lut_reference_big(eoc, 1)[0]
    net = Netlist(eoc, ROWS, NBIG)
    (free,) = net.solved_node(0, None, lut_targets(1), None, terms, 900 + terms, terms)
    out = net.wire()
    net.nodes.append(inode(eoc, 1, out, net.tv_index(lut_tvs(eoc, NBIG, 1)[0]), [free], [1], 0))
    net.expect[out] = want
    eng = make_engine(eoc, monkeypatch, SET_A, NBIG, {})
    probe = Probe(eng)
    net.run(eng)
    moved = probe.done()
    eng.close()
    assert moved["prep"] == 1 and moved["br_spans"] == 1 and moved["bootstraps"] == ROWS and moved["keyswitches"] == ROWS, moved
    report(name, ROWS, net.shares)


PATHS = {"folded-inline[pair]": (path_folded_inline, "pair"), "folded-inline[wide]": (path_folded_inline, "wide"),
         "folded-descs[pair]": (path_folded_descs, "pair"), "folded-descs[wide]": (path_folded_descs, "wide"),
         "folded-multi": (path_folded_multi,), "folded-setB-two-parts": (path_folded_setB_two_parts,),
         "unfolded[inline]": (path_unfolded, "inline"), "unfolded[descs]": (path_unfolded, "descs"),
         "unfolded[multi]": (path_unfolded, "multi"), "mux": (path_mux,), "mux-in-pool": (path_mux_in_pool,),
         "maj-xor3": (path_maj_xor3,), "free-gates": (path_free_gates,), "coarse-T4": (path_coarse_T4,),
         **{f"lin-boot[{k}]": (path_lin_boot, k) for k in (1, 2, 3, 4)}, "lin-boot-mixed-terms": (path_lin_boot_mixed_terms,),
         **{f"lin-free[{k}]": (path_lin_free, k) for k in (1, 2, 3, 4)}}


@pytest.mark.parametrize("path", list(PATHS), ids=list(PATHS))
def test_path_bit_exact_on_cell_edge_operands(eoc, monkeypatch, path):
    fn, *args = PATHS[path]
    _CLOCK["gpu"] = _CLOCK["ref"] = 0.0
    fn(eoc, monkeypatch, path, *args)
