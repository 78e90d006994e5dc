"""The second slice of every device call: the host loops of csrc/engine.hip that cut a call into launches compute
the r0 / g0 / q0 / b0 offsets into inputs, outputs, descriptors, staged polynomials and job bases in their second iteration.
Two kinds of rule cut: the sample rule (at most 2^20 extracted samples per slice; EOC_TFHE_SLICE_SAMPLES lowers it, read at
engine creation) and the grid rules (32 768 gates, nodes or queries, 65 535 vectors per launch; constants, reached here at
their real size with one row per item).

Every id makes its own engine under monkeypatch, writes into poisoned outputs with one guard row behind them, compares every
output word with the family's existing reference (nothing here computes a reference of its own) and asserts from the engine's
counters that the expected number of slices ran.  The sample-rule ids run as 2 + 2 + 1 on the short-LWE rigs of
capture_cases.small_keys.  The grid ids cycle their items through 7 distinct kinds -- 7 is coprime to 32 768, 4 096 and
65 535, so item g0 + i differs from item i and a dropped offset changes words -- with the reference computed once per kind
and tiled; large operands are tiled on the device.  k_free_gates and the free nodes' k_lin_modswitch launches have no counter:
their ids assert that no bootstrap level ran, and their slice count is the constant's.

Each id prints its slice count and the device time of its call (kernel_times), the figures of DESIGN.md 8.3."""
import ctypes as C
import time

import numpy as np
import pytest

import automaton_oracle as ao
import capture_cases as cc
import cmux_oracle as cx
import compact_oracle as co
import conv_oracle as cv
import dot_oracle as do
import int_circuit_oracle as ico
import lut2_oracle as l2
import lut_many_oracle as lmo
import lut_oracle as lo
import oracle_lib as ol
import pack_oracle as po
import test_gpu_cmux as tc
import test_gpu_conv as tcv
import test_gpu_dot as td
import test_gpu_int_circuit as ti
import test_gpu_lut as tl
import test_gpu_lut_many as tm
from gpu_util import sync, to_dev, torch_cuda
from test_gpu_br_instances import custom_params, reference
from test_gpu_circuits import _oracle_run
from test_gpu_linear_stage_paths import inode

pytestmark = pytest.mark.gpu
N = 1024
POISON = cc.POISON
KNOB = "EOC_TFHE_SLICE_SAMPLES"
KINDS = 7
GRID, GRID_T8, GRID_VECS = 32768, 4096, 65535                  # kMaxGatesPerLaunch / kSlice, the same >> 3, kConvMaxVecs


@pytest.fixture(scope="module")
def eoc(built_lib):
    torch_cuda()
    import eoc_tfhe_amd
    return eoc_tfhe_amd


def test_the_kind_count_is_coprime_to_every_grid_constant():
    assert all(np.gcd(KINDS, c) == 1 for c in (GRID, GRID_T8, GRID_VECS))


def fresh_engine(eoc, monkeypatch, p, knob=None):
    """a new engine with every knob cleared and the sample rule at `knob` (None: the shipped 2^20)"""
    for k in cc.KNOBS + ("EOC_TFHE_DOT_WS_BYTES",):
        monkeypatch.delenv(k, raising=False)
    if knob is not None:
        monkeypatch.setenv(KNOB, str(knob))
    return eoc.Engine(p)


def rig(eoc, n, seed, bk=True):
    """(params, secret key, oracle, nothing) at LWE dimension n; the oracle has the key-switch key either way"""
    p, sk, orc, _ = cc.small_keys(eoc, 0, n, seed, bk=bk)
    co.ksk(orc)
    return p, sk, orc


def guarded(rows, stride):
    """[rows + 1][stride] of the poison word: the outputs and one guard row behind them"""
    torch = torch_cuda()
    return torch.full((rows + 1, stride), POISON, dtype=torch.int32, device="cuda")


def fetch(buf, shape):
    sync()
    o = buf.cpu().numpy()
    assert (o[-1].view(np.uint32) == POISON).all(), "the guard row behind the output was written"
    return o[:-1].reshape(shape)


class Probe:
    """the counters one call moves: stats(), the family counters, and the spans of kernel_times() under profiling"""

    def __init__(self, eng, name):
        self.eng, self.name = eng, name
        eng.set_profiling(True)
        eng.kernel_times()
        self.before = self.counters()
        self.t0 = time.perf_counter()

    def counters(self):
        c = self.eng.stats()
        c.update(dot_launches=self.eng.dot_launches(), conv_launches=self.eng.conv_launches())
        return c

    def done(self, slices):
        sync()
        wall = time.perf_counter() - self.t0
        times = self.eng.kernel_times()
        self.eng.set_profiling(False)
        after = self.counters()
        moved = {k: after[k] - self.before[k] for k in after}
        moved.update(prep=times["prepare"]["launches"], br_spans=times["blind_rotate"]["launches"], ks_spans=times["keyswitch"]["launches"])
        ms = sum(t["ms"] for t in times.values())
        print(f"SEAM {self.name}: {slices} slices, device {ms:.2f} ms, call wall {wall * 1e3:.0f} ms")
        return moved


def assert_words(what, got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
    bad = np.argwhere((got != want).reshape(-1, got.shape[-1]).any(axis=-1))
    assert bad.size == 0, (what, len(bad), bad[:8].ravel().tolist())


# ---- the sample rule: 2 + 2 + 1 ---------------------------------------------------------------------------------------------
def lut_case(eoc, kind):
    """(rig, polynomials, input rows, reference [blocks][5][n+1], call(eng, d_tv, d_x, d_out), knob, bootstraps, key switches)"""
    p, sk, orc = rig(eoc, 40, 35)
    rows = 5
    if kind == "lut":
        tvs = np.stack([eoc.lut_test_polynomial(4, t) for t in tl.tables_for(4)[1]])
        x = tl.inputs(eoc, sk, 4, rows, 7500)[1]
        want = reference(("seam", kind), lambda: lo.lut_batch(orc, tvs, x))
        call = lambda eng, d_tv, d_x, d_out: eng.lut_batch_device(d_tv, 3, d_x, d_out, rows)          # noqa: E731
        return p, sk, tvs, x, want, call, 6, 15, 15
    T, pm, polys, knob = (2, 4, 2, 8) if kind == "lut-many[T=2]" else (8, 2, 1, 16)
    tvs = tm.packed(eoc, pm, tm.tables_for(T, pm, polys)[1])
    x = tm.inputs(eoc, sk, pm, rows, 7510 + T)[1]
    want = reference(("seam", kind), lambda: lmo.lut_many_batch(orc, tvs, x, T).reshape(polys * T, rows, p.n + 1))
    call = lambda eng, d_tv, d_x, d_out: eng.lut_many_batch_device(T, d_tv, polys, d_x, d_out, rows)    # noqa: E731
    return p, sk, tvs, x, want, call, knob, polys * rows, polys * T * rows


@pytest.mark.parametrize("kind", ["lut", "lut-many[T=2]", "lut-many[T=8]"])
def test_lut_rows_in_three_slices(eoc, monkeypatch, kind):
    """lut_levels_locked, r0 += rows: 3 tables x 5 rows at 6 samples a slice; 2 polynomials of T = 2 (4 slots) at 8; one
    polynomial of T = 8 at 16 -- rows = 2 each time"""
    p, sk, tvs, x, want, call, knob, boots, switches = lut_case(eoc, kind)
    eng = fresh_engine(eoc, monkeypatch, p, knob)
    eng.load_cloud_key(sk)
    d_tv, d_x, out = to_dev(tvs), to_dev(x), guarded(want.shape[0] * 5, p.n + 1)
    probe = Probe(eng, kind)
    call(eng, d_tv.data_ptr(), d_x.data_ptr(), out.data_ptr())
    moved = probe.done(3)
    eng.close()
    assert moved["batches"] == 3 and moved["br_launches"] == 3 and moved["br_spans"] == 3, moved
    assert moved["bootstraps"] == boots and moved["keyswitches"] == switches, moved
    assert_words(kind, fetch(out, want.shape), want)


@pytest.mark.parametrize("per_row", [False, True], ids=["lut-enc[mode 1]", "lut-enc[mode 2]"])
def test_lut_enc_rows_in_three_slices(eoc, monkeypatch, per_row):
    """3 groups x 5 rows at 6 samples a slice.  One list per group: three levels of 3 x 2, 3 x 2, 3 x 1 jobs.  One list per job:
    a sliced level cannot span the groups (the kernel's list index is job / tv_rows), so it runs group by group -- 3 groups x 3
    slices, lists from d_tv + (g0 count + r0) 2N -- where the unsliced call is one level"""
    p, sk, orc = rig(eoc, 40, 35)
    G, rows = 3, 5
    rng = np.random.default_rng(7600 + per_row)
    lists = cc.rand_i32(rng, (G, rows, 2, N) if per_row else (G, 2, N))
    y = tl.inputs(eoc, sk, 4, rows, 7520)[1]
    want = reference(("seam", "lut-enc", per_row), lambda: l2.lut_enc_batch(orc, lists, y, per_row))
    d_lists, d_y = to_dev(lists), to_dev(y)
    for knob, levels in ((6, 9 if per_row else 3), (None, 1)):
        eng = fresh_engine(eoc, monkeypatch, p, knob)
        eng.load_cloud_key(sk)
        out = guarded(G * rows, p.n + 1)
        probe = Probe(eng, f"lut-enc[mode {1 + per_row}]{'' if knob else ' unsliced'}")
        eng.lut_enc_batch_device(d_lists.data_ptr(), G, per_row, d_y.data_ptr(), out.data_ptr(), rows)
        moved = probe.done(levels)
        eng.close()
        assert moved["batches"] == levels and moved["br_launches"] == levels, (knob, moved)
        assert moved["bootstraps"] == G * rows and moved["keyswitches"] == G * rows, (knob, moved)
        assert_words(("lut-enc", per_row, knob), fetch(out, want.shape), want)


@pytest.mark.parametrize("T", [1, 2], ids=["lut2[T=1]", "lut2[T=2]"])
def test_lut2_rows_in_three_slices(eoc, monkeypatch, T):
    """eoc_lut2_batch_device, r0 += rows: p = 2, 2 functions (4 level-1 outputs a row), 5 rows at 8 samples a slice -> rows = 2;
    per slice one level-1 level, one pack and one level-2 level over its S rows, written at d_out + r0 with out_rows = count"""
    p, sk, orc = rig(eoc, 17, 41)
    blob = sk.packing_key_bytes()
    kfft = po.key_fft(po.blob_rows(blob, p.n))
    pm, rows = 2, 5
    tv0 = np.stack([eoc.lut2_test_polynomials(pm, l2.lut2_tables(f, pm), T) for f in l2.functions(pm)])
    x = sk.encrypt_ints(np.array([0, 1, 0, 1, 1], np.uint8), pm, 7700)
    y = sk.encrypt_ints(np.array([0, 0, 1, 1, 0], np.uint8), pm, 7701)
    want = reference(("seam", "lut2", T), lambda: l2.lut2_batch(orc, kfft, pm, T, tv0, x, y))
    d_tv, d_x, d_y = to_dev(tv0.reshape(-1, N).copy()), to_dev(x), to_dev(y)
    for knob, slices in ((8, 3), (None, 1)):
        eng = fresh_engine(eoc, monkeypatch, p, knob)
        eng.load_cloud_key(sk)
        eng.load_packing_key(blob)
        out = guarded(2 * rows, p.n + 1)
        probe = Probe(eng, f"lut2[T={T}]{'' if knob else ' unsliced'}")
        eng.lut2_batch_device(pm, T, d_tv.data_ptr(), 2, d_x.data_ptr(), d_y.data_ptr(), out.data_ptr(), rows)
        moved = probe.done(slices)
        eng.close()
        assert moved["batches"] == 2 * slices and moved["pack_launches"] == slices, (knob, moved)
        assert moved["bootstraps"] == (2 * pm // T + 2) * rows and moved["keyswitches"] == (2 * pm + 2) * rows, (knob, moved)
        assert_words(("lut2", T, knob), fetch(out, want.shape), want)


def test_circuit_job_cap_cuts_inside_a_level(eoc, monkeypatch):
    """run_level's job cap from eoc_circuit_run_device: NAND, MUX, XOR, AND over S = 4 at 8 jobs a slice -- the MUX counts
    2 S jobs, so the level runs as (NAND), (MUX), (XOR, AND), job_base restarting in each -- and a second level reads all four
    outputs"""
    p, sk, orc = rig(eoc, 40, 35)
    S, O = 4, ol.OPS
    G = eoc.Gate
    gates = [G(O["NAND"], 0, 1, -1, 3), G(O["MUX"], 0, 1, 2, 4), G(O["XOR"], 1, 2, -1, 5), G(O["AND"], 0, 2, -1, 6),
             G(O["XOR"], 4, 6, -1, 7), G(O["NAND"], 3, 5, -1, 8)]
    n_wires = 9
    wires = np.full((n_wires, S, p.n + 1), POISON, np.uint32).view(np.int32)
    rng = np.random.default_rng(7800)
    for w in range(3):
        wires[w] = sk.encrypt_bits(rng.integers(0, 2, S).astype(np.uint8), 7800 + w)
    want = _oracle_run(orc, gates, wires)
    for knob, levels in ((8, 4), (None, 2)):
        eng = fresh_engine(eoc, monkeypatch, p, knob)
        eng.load_cloud_key(sk)
        buf = guarded(n_wires * S, p.n + 1)
        buf[:3 * S].copy_(to_dev(wires[:3].reshape(3 * S, -1)))
        probe = Probe(eng, f"circuit-job-cap{'' if knob else ' unsliced'}")
        eng.circuit_run_device(gates, buf.data_ptr(), n_wires, S)
        moved = probe.done(levels)
        eng.close()
        assert moved["batches"] == levels and moved["br_launches"] == levels, (knob, moved)
        assert moved["bootstraps"] == 7 * S and moved["keyswitches"] == 6 * S, (knob, moved)
        assert_words(("circuit-job-cap", knob), fetch(buf, want.shape), want)


def test_compact_expansion_in_three_slices(eoc, monkeypatch):
    """eoc_compact_expand_device_from: 5 samples from slot 1022 of the first list at 2 samples a slice: (1022, 1023), (1024,
    1025) in the second list, (1026)"""
    p, sk, orc = rig(eoc, 40, 39, bk=False)
    first, count = N - 2, 5
    pk = eoc.PublicKey(sk.public_key_bytes())
    lists = pk.encrypt_bits(np.random.default_rng(7900).integers(0, 2, 2 * N).astype(np.uint8), enc_seed=7901)
    want = co.expand(orc, lists, np.arange(first, first + count))
    fn = getattr(eoc.lib(), "_Z30eoc_compact_expand_device_fromP10eoc_enginePKimmPiPv")     # csrc/common.h
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p]
    eng = fresh_engine(eoc, monkeypatch, p, 2)
    eng.load_cloud_key(sk)
    d_lists, out = to_dev(lists), guarded(count, p.n + 1)
    probe = Probe(eng, "compact")
    assert fn(eng.h, d_lists.data_ptr(), first, count, out.data_ptr(), None) == 0
    moved = probe.done(3)
    eng.close()
    assert moved["prep"] == 3 and moved["ks_spans"] == 3 and moved["keyswitches"] == count, moved
    assert_words("compact", fetch(out, want.shape), want)


def test_table_read_queries_in_three_slices(eoc, monkeypatch):
    """eoc_table_read_device: 4 lists of 4-slot entries (log2_width = 2: two tree stages, eight rotations), 5 queries at 8
    samples a slice -> 2 queries a slice"""
    p, sk, orc = rig(eoc, 40, 35, bk=False)
    op, d, lw, queries = cx.orc_params(p), 2, 2, 5
    depth, W = d + 10 - lw, 1 << lw
    pk = eoc.PublicKey(sk.public_key_bytes())
    rng = np.random.default_rng(8000)
    table = tc.make_table(eoc, pk, "ints", d, rng, 8001)[0]
    sel = tc.index_selectors(sk, [(1 << depth) - 1, 0, 777, 256, 1023], depth, enc_seed=8002)
    fft = cx.to_fft(sel)
    want = cx.table_read(orc, op, table, d, lw, fft)[0]
    eng = fresh_engine(eoc, monkeypatch, p, 8)
    eng.load_cloud_key(sk)
    d_fft, d_tab, out = tc.convert(eng, sel), to_dev(table), guarded(queries * W, p.n + 1)
    probe = Probe(eng, "table-read")
    eng.table_read_device(d_tab.data_ptr(), d, lw, d_fft.data_ptr(), queries, out.data_ptr())
    moved = probe.done(3)
    eng.close()
    assert moved["cmux_launches"] == 3 * depth and moved["prep"] == 3 and moved["keyswitches"] == queries * W, moved
    assert_words("table-read", fetch(out, want.shape), want)


AUTO_TRANS = np.array([[1, 1, 2, 0], [1, 0, 0, N + 1], [0, 2, 2, 1]], np.int32)


def automaton_run(eoc, monkeypatch, name, knob, steps, starts, queries, seed):
    p, sk, orc = rig(eoc, 40, 35, bk=False)
    op, lw, kpl = cx.orc_params(p), 2, 2 * p.l
    rng = np.random.default_rng(seed)
    F = cc.rand_i32(rng, (len(AUTO_TRANS), 2, N))
    sel = sk.encrypt_selector_bits(rng.integers(0, 2, queries * steps), enc_seed=seed + 1) if steps else np.zeros((0, kpl, 2, N), np.int32)
    fft = cx.to_fft(sel).reshape(queries, steps, kpl, 2, N)
    want = ao.run(orc, op, AUTO_TRANS, F, fft, starts, lw)[0]
    eng = fresh_engine(eoc, monkeypatch, p, knob)
    eng.load_cloud_key(sk)
    d_fft = tc.convert(eng, sel) if steps else None
    d_final, out = to_dev(F), guarded(queries * len(starts) << lw, p.n + 1)
    probe = Probe(eng, name)
    eng.automaton_run_device(AUTO_TRANS, d_final.data_ptr(), d_fft.data_ptr() if steps else None, steps, starts, lw, out.data_ptr(), queries)
    moved = probe.done(3 if knob else 1)
    eng.close()
    assert_words(name, fetch(out, want.shape), want)
    return moved


def test_automaton_run_without_steps_in_three_chunks(eoc, monkeypatch):
    """steps = 0: 3 start states of 4 slots at 4 samples a key switch -> one start state a chunk (starts + i0, d_out + i0 W
    stride); 3 queries: the doubling copy runs with a count that is no power of two (1, then 1 of 2)"""
    moved = automaton_run(eoc, monkeypatch, "automaton-run[steps=0]", 4, 0, [2, 0, 1], 3, 8100)
    assert moved["prep"] == 3 and moved["ks_spans"] == 3 and moved["keyswitches"] == 12 and moved["automaton_launches"] == 0, moved
    moved = automaton_run(eoc, monkeypatch, "automaton-run[steps=0] unsliced", None, 0, [2, 0, 1], 3, 8100)
    assert moved["prep"] == 1 and moved["ks_spans"] == 1 and moved["keyswitches"] == 12, moved


def test_automaton_run_queries_in_three_slices(eoc, monkeypatch):
    """steps = 2: 2 start states of 4 slots, 5 queries at 16 samples a slice -> 2 queries a slice, two steps each"""
    moved = automaton_run(eoc, monkeypatch, "automaton-run[steps=2]", 16, 2, [2, 0], 5, 8200)
    assert moved["automaton_launches"] == 6 and moved["prep"] == 3 and moved["keyswitches"] == 40, moved


CONV_SLOTS = [N - 1, 0, 511]


def test_conv_extract_vectors_in_three_slices(eoc, monkeypatch):
    """eoc_conv_extract_device, b0 += bs: one list a vector, a 3-entry slot table, 5 vectors at 6 samples a slice"""
    p, sk, orc = rig(eoc, 40, 63, bk=False)
    lists = tcv.rand_lists(np.random.default_rng(8300), 5, N)
    want = tcv.extract_keyswitch_ref(orc, lists, CONV_SLOTS)
    eng = fresh_engine(eoc, monkeypatch, p, 6)
    eng.load_cloud_key(sk)
    d_slots, d_lists, out = tcv.table(eng, CONV_SLOTS, 1), to_dev(lists), guarded(15, p.n + 1)
    probe = Probe(eng, "conv-extract")
    eng.conv_extract_device(d_lists.data_ptr(), 1, 5, d_slots.data_ptr(), 3, out.data_ptr())
    moved = probe.done(3)
    eng.close()
    assert moved["ks_spans"] == 2 * 3 and moved["keyswitches"] == 15 and moved["conv_launches"] == 0, moved   # extraction + key switch
    assert_words("conv-extract", fetch(out, want.shape), want)


def test_conv_linear_vectors_in_three_slices(eoc, monkeypatch):
    """the same table and vectors through eoc_conv_linear_device: one output channel over two input lists"""
    p, sk, orc = rig(eoc, 40, 63, bk=False)
    rng = np.random.default_rng(8400)
    cols = N + 3
    w, lists = tcv.rand_weights(rng, 1, cols), tcv.rand_lists(rng, 5, cols)
    bias = rng.integers(tcv.INT32_MIN, tcv.INT32_MAX, 1, endpoint=True).astype(np.int32)
    want = tcv.extract_keyswitch_ref(orc, cv.conv(w, lists, bias), CONV_SLOTS)
    eng = fresh_engine(eoc, monkeypatch, p, 6)
    eng.load_cloud_key(sk)
    img, d_slots, d_lists, d_bias = tcv.model(eng, w), tcv.table(eng, CONV_SLOTS, 1), to_dev(lists), to_dev(bias)
    out = guarded(15, p.n + 1)
    probe = Probe(eng, "conv-linear")
    eng.conv_linear_device(img.data_ptr(), 1, cols, d_lists.data_ptr(), 5, d_bias.data_ptr(), d_slots.data_ptr(), 3, out.data_ptr())
    moved = probe.done(3)
    eng.close()
    assert moved["conv_launches"] == 3 and moved["keyswitches"] == 15, moved
    assert_words("conv-linear", fetch(out, want.shape), want)


def test_dot_linear_vectors_in_three_slices(eoc, monkeypatch):
    """eoc_linear_device: 3 rows, 5 vectors at 6 samples a slice -> 2 vectors a slice"""
    p, sk, orc = rig(eoc, 40, 63, bk=False)
    rng = np.random.default_rng(8500)
    rows, cols = 3, N + 3
    w, lists = td.rand_weights(rng, rows, cols), td.rand_lists(rng, 5, cols)
    bias = rng.integers(td.INT32_MIN, td.INT32_MAX, rows, endpoint=True).astype(np.int32)
    want = td.keyswitch_ref(orc, do.dot(w, lists, bias))
    eng = fresh_engine(eoc, monkeypatch, p, 6)
    eng.load_cloud_key(sk)
    img, d_lists, d_bias, out = td.model(eng, w), to_dev(lists), to_dev(bias), guarded(5 * rows, p.n + 1)
    probe = Probe(eng, "dot-linear")
    eng.linear_device(img.data_ptr(), rows, cols, d_lists.data_ptr(), 5, d_bias.data_ptr(), out.data_ptr())
    moved = probe.done(3)
    eng.close()
    assert moved["dot_launches"] == 3 and moved["keyswitches"] == 5 * rows, moved
    assert_words("dot-linear", fetch(out, want.shape), want)


# ---- the grid rules at their real constants ---------------------------------------------------------------------------------
GRID_N, GRID_SEED = 8, 45


def kind_of(count):
    return np.arange(count) % KINDS


def run_gates(eoc, monkeypatch, name, p, sk, gates, wires, inputs, slices):
    """circuit_run_device over wires [n_wires][1][n+1] whose rows `inputs` are set and whose other rows are poisoned"""
    eng = fresh_engine(eoc, monkeypatch, p)
    eng.load_cloud_key(sk)
    buf = guarded(wires.shape[0], p.n + 1)
    host = np.full((wires.shape[0], p.n + 1), POISON, np.uint32).view(np.int32)
    host[inputs] = wires[inputs, 0]
    buf[:-1].copy_(to_dev(host))
    probe = Probe(eng, name)
    eng.circuit_run_device(gates, buf.data_ptr(), wires.shape[0], 1)
    moved = probe.done(slices)
    eng.close()
    return moved, fetch(buf, wires.shape)


def test_level_of_32769_free_gates(eoc, monkeypatch):
    """run_level, free gates: NOT / COPY / CONSTANT over 7 input wires, freeg.data() + g0 in the second launch"""
    p, sk, orc = rig(eoc, GRID_N, GRID_SEED)
    O, count = ol.OPS, GRID + 1
    ops = [O["NOT"], O["COPY"], O["CONST0"], O["NOT"], O["CONST1"], O["COPY"], O["NOT"]]
    gates = [eoc.Gate(ops[k % KINDS], -1 if ops[k % KINDS] in (O["CONST0"], O["CONST1"]) else k % KINDS, -1, -1, KINDS + k) for k in range(count)]
    wires = np.zeros((KINDS + count, 1, p.n + 1), np.int32)
    wires[:KINDS, 0] = sk.encrypt_bits(np.array([0, 1, 1, 0, 1, 0, 0], np.uint8), 8600)
    per_kind = _oracle_run(orc, gates[:KINDS], wires[:2 * KINDS])[KINDS:]
    wires[KINDS:] = per_kind[kind_of(count)]
    assert len({per_kind[j].tobytes() for j in range(KINDS)}) == KINDS    # the NOTs and COPYs differ by their inputs
    moved, got = run_gates(eoc, monkeypatch, "level-32769-free-gates", p, sk, gates, wires, np.arange(KINDS), 2)
    assert moved["batches"] == 0 and moved["bootstraps"] == 0, moved
    assert_words("free gates", got, wires)


def test_level_of_32769_bootstrapped_gates(eoc, monkeypatch):
    """run_level, bootstrapped gates: seven opcodes (a MUX among them: two jobs) cycling over 32 769 gates of one row -- the
    second slice holds gate 32 768 alone, job_base restarting at 0 -- and a second-level gate that reads its output wire"""
    p, sk, orc = rig(eoc, GRID_N, GRID_SEED)
    O, count = ol.OPS, GRID + 1
    ops = [O[k] for k in ("NAND", "XOR", "MUX", "OR", "ANDNY", "XNOR", "NOR")]
    base = count                                                          # outputs on wires 0 .. 32 768, inputs behind them
    gates = [eoc.Gate(ops[k % KINDS], base + 3 * (k % KINDS), base + 3 * (k % KINDS) + 1,
                      base + 3 * (k % KINDS) + 2 if ops[k % KINDS] == O["MUX"] else -1, k) for k in range(count)]
    last = base + 3 * KINDS
    gates.append(eoc.Gate(O["NAND"], count - 1, base, -1, last))
    wires = np.zeros((last + 1, 1, p.n + 1), np.int32)
    wires[base:last, 0] = sk.encrypt_bits(np.random.default_rng(8700).integers(0, 2, 3 * KINDS).astype(np.uint8), 8701)
    small = np.zeros((3 * KINDS + KINDS, 1, p.n + 1), np.int32)           # the seven kinds on wires of their own
    small[:3 * KINDS] = wires[base:last]
    kinds = [eoc.Gate(g.op, g.in0 - base, g.in1 - base, g.in2 - base if g.in2 >= 0 else -1, 3 * KINDS + j) for j, g in enumerate(gates[:KINDS])]
    per_kind = reference(("seam", "boot gates"), lambda: _oracle_run(orc, kinds, small)[3 * KINDS:])
    assert len({per_kind[j].tobytes() for j in range(KINDS)}) == KINDS
    wires[:count] = per_kind[kind_of(count)]
    wires[last] = orc.gate_batch(O["NAND"], wires[count - 1], wires[base])
    n_mux = int((kind_of(count) == 2).sum())
    moved, got = run_gates(eoc, monkeypatch, "level-32769-boot-gates", p, sk, gates, wires, np.arange(base, last), 3)
    assert moved["batches"] == 3 and moved["bootstraps"] == count + n_mux + 1 and moved["keyswitches"] == count + 1, moved
    assert_words("bootstrapped gates", got, wires)


def int_kinds(eoc, sk, T):
    """the 7 kinds of an integer-circuit node: (input wires [7][1][n+1], polynomials [7][N], node(k, out) of kind k mod 7)"""
    pm = 4 if T <= 1 else 2
    x = np.stack([ti.inputs(eoc, sk, pm, 1, 8800 + j, shift=j)[1] for j in range(KINDS)])
    if T <= 1:
        tvs = np.stack([eoc.lut_test_polynomial(pm, lo.int_table(lambda m, j=j: ((2 * j + 1) * m + j) % pm, pm, pm)) for j in range(KINDS)])
    else:
        tvs = np.stack([eoc.lut_many_test_polynomial(pm, [lo.int_table(lambda m, a=j + i: (m + a) % pm, pm, pm) for i in range(T)])
                        for j in range(KINDS)])

    def node(k, out):
        j = k % KINDS
        ins, w = [[j], [j, (j + 1) % KINDS], [j, (j + 2) % KINDS, (j + 3) % KINDS]][j % 3], [1, 2, -1][:1 + j % 3]
        return inode(eoc, T, out, j if T else 0, ins, w, (j * 0x01234567) & 0x7FFFFFFF)
    return x, tvs, node


@pytest.mark.parametrize("T,count", [(0, GRID + 1), (1, GRID + 1), (8, GRID_T8 + 1)],
                         ids=["int-circuit-32769-free-nodes", "int-circuit-32769-T1-nodes", "int-circuit-4097-T8-nodes"])
def test_int_circuit_group_past_the_grid_limit(eoc, monkeypatch, T, count):
    """eoc_int_circuit_run_device: one pre-pass of 32 769 free nodes (pass[g0 + i]); one group of 32 769 T = 1 nodes and one of
    4 097 T = 8 nodes (the cut is at 32 768 >> 3): nodes G.nodes[g0 + i], polynomials staged + (G.staged + g0) N, job bases i S"""
    p, sk, orc = rig(eoc, GRID_N, GRID_SEED)
    name = f"int-circuit-{count}-{'free' if T == 0 else f'T{T}'}-nodes"
    outs = max(T, 1)
    x, tvs, node = int_kinds(eoc, sk, T)
    nodes = [node(k, KINDS + k * outs) for k in range(count)]
    n_wires = KINDS + count * outs
    small = np.zeros((KINDS + KINDS * outs, 1, p.n + 1), np.int32)
    small[:KINDS] = x
    per_kind = reference(("seam", "int kinds", T), lambda: ico.run(orc, nodes[:KINDS], tvs, small)[KINDS:]).reshape(KINDS, outs, p.n + 1)
    assert len({per_kind[j].tobytes() for j in range(KINDS)}) == KINDS
    want = np.concatenate([x.reshape(KINDS, p.n + 1), per_kind[kind_of(count)].reshape(count * outs, p.n + 1)])
    eng = fresh_engine(eoc, monkeypatch, p)
    eng.load_cloud_key(sk)
    buf = guarded(n_wires, p.n + 1)
    buf[:KINDS].copy_(to_dev(x.reshape(KINDS, p.n + 1)))
    d_tv = to_dev(tvs)
    probe = Probe(eng, name)
    eng.int_circuit_run_device(nodes, d_tv.data_ptr(), KINDS, buf.data_ptr(), n_wires, 1)
    moved = probe.done(2)
    eng.close()
    if T == 0:
        assert moved["batches"] == 0 and moved["bootstraps"] == 0, moved
    else:
        assert moved["batches"] == 2 and moved["bootstraps"] == count and moved["keyswitches"] == count * T, moved
    assert_words(name, fetch(buf, want.shape), want)


def test_automaton_step_of_32769_queries(eoc, monkeypatch):
    """eoc_automaton_step_device, q0 += 32 768: one state, prev_query_stride = 1, 32 769 queries whose selectors and state
    vectors cycle through 7 kinds on the (l = 1, Bgbit = 9) shape (32 KiB a selector, 1 GiB of them, tiled on the device)"""
    torch = torch_cuda()
    p = custom_params(eoc, 1, 9, GRID_N)
    sk = eoc.SecretKey(p, 83, with_cloud_key=False)
    op, queries = cx.orc_params(p), GRID + 1
    trans = np.array([[0, 63, 0, N + 1]], np.int32)
    prev = cc.rand_i32(np.random.default_rng(8900), (KINDS, 1, 2, N))
    sel = sk.encrypt_selector_bits([0, 1, 1, 0, 1, 0, 0], enc_seed=8901)
    fft = cx.to_fft(sel)
    per_kind = reference(("seam", "automaton step"), lambda: np.stack([ao.step(op, trans, prev[j], fft[j]) for j in range(KINDS)]))
    assert len({per_kind[j].tobytes() for j in range(KINDS)}) == KINDS
    eng = fresh_engine(eoc, monkeypatch, p)
    kind = torch.arange(queries, device="cuda") % KINDS
    d_sel = tc.convert(eng, sel)[kind].contiguous()
    assert d_sel.numel() * 8 == queries * eng.tgsw_fft_bytes == queries << 15
    d_prev = to_dev(prev.reshape(KINDS, 2, N))[kind].contiguous()
    nxt = guarded(queries, 2 * N)
    probe = Probe(eng, "automaton-step-32769-queries")
    eng.automaton_step_device(trans, d_prev.data_ptr(), 1, d_sel.data_ptr(), 1, nxt.data_ptr(), queries)
    moved = probe.done(2)
    eng.close()
    assert moved["automaton_launches"] == 2 and moved["cmux_launches"] == 0, moved
    sync()
    assert bool((nxt[-1] == POISON).all()), "the guard row behind the output was written"
    bad = (nxt[:-1] != to_dev(per_kind.reshape(KINDS, 2 * N).copy())[kind]).any(dim=1).nonzero().ravel()
    assert bad.numel() == 0, (int(bad.numel()), bad[:8].tolist())


def test_conv_extract_of_65536_vectors(eoc, monkeypatch):
    """eoc_conv_extract_device at kConvMaxVecs: 65 536 vectors of one list and one slot -> 65 535 + 1, d_lists + b0 2N and
    d_out + b0 stride in the second launch; 512 MiB of lists tiled on the device from 7 kinds"""
    torch = torch_cuda()
    p, sk, orc = rig(eoc, GRID_N, GRID_SEED, bk=False)
    vecs, slot = GRID_VECS + 1, 517
    lists = tcv.rand_lists(np.random.default_rng(9000), KINDS, N)
    per_kind = tcv.extract_keyswitch_ref(orc, lists, [slot]).reshape(KINDS, p.n + 1)
    assert len({per_kind[j].tobytes() for j in range(KINDS)}) == KINDS
    eng = fresh_engine(eoc, monkeypatch, p)
    eng.load_cloud_key(sk)
    kind = torch.arange(vecs, device="cuda") % KINDS
    d_lists = to_dev(lists.reshape(KINDS, 2 * N))[kind].contiguous()
    d_slots, out = tcv.table(eng, [slot], 1), guarded(vecs, p.n + 1)
    probe = Probe(eng, "conv-extract-65536-vectors")
    eng.conv_extract_device(d_lists.data_ptr(), 1, vecs, d_slots.data_ptr(), 1, out.data_ptr())
    moved = probe.done(2)
    eng.close()
    assert moved["ks_spans"] == 2 * 2 and moved["keyswitches"] == vecs, moved
    assert_words("conv-extract-65536-vectors", fetch(out, (vecs, p.n + 1)), per_kind[kind_of(vecs)])
