"""The rounding mode of the leveled calls on the MI355X: every governed device call byte for byte against
tests/leveled_round_oracle.py -- the CMux on edge operands, the table read on a sliced workspace, the demultiplexer and the
table update with colliding queries, the automaton step and run --, the mode's hygiene (off / on / off, the global setter, graph
capture), a run twice as long as the truncating budget, and the noise of a read.  The engines are this module's own: the
engines other test modules share stay in the default mode.  Host side: tests/test_leveled_round_cpu.py."""
import ctypes as C

import numpy as np
import pytest

import automaton_oracle as ao
import capture_cases as cc
import cmux_oracle as cx
import compact_oracle as co
import leveled_round_oracle as lr
import table_update_oracle as tu
import test_gpu_automaton as ta
import test_gpu_cmux as tc
import test_leveled_round_cpu as host
from eoc_tfhe_amd import noise
from gpu_util import dev_empty, sync, to_dev, torch_cuda
from test_gpu_capture import capture, side_stream
from test_gpu_table_update import update_device

pytestmark = pytest.mark.gpu
N = 1024
EOC_ERR_STATE = -6


@pytest.fixture(scope="module")
def eoc(built_lib):
    torch_cuda()
    import eoc_tfhe_amd
    return eoc_tfhe_amd


_ENGINES = {}


def rounding_engine(eoc, pset, env=()):
    """an engine of this module's own with the keys of tests/test_gpu_cmux.py, in rounding mode; env: knobs read at creation"""
    if (pset, env) not in _ENGINES:
        p, sk = tc.keys(eoc, pset)[:2]
        with cc.knobs(dict(env)):
            eng = eoc.Engine(p)
        eng.load_cloud_key(sk)
        assert eng.leveled_rounding is False                    # the default
        eng.leveled_rounding = True
        _ENGINES[(pset, env)] = eng
    eng = _ENGINES[(pset, env)]
    assert eng.leveled_rounding is True
    return eng


def cmux_device(eng, d_fft, in0, in1):
    torch = torch_cuda()
    d0, d1 = to_dev(in0), to_dev(in1)
    d_out = dev_empty(in0.shape, torch.int32)
    eng.cmux_device(d_fft.data_ptr(), d0.data_ptr(), d1.data_ptr(), d_out.data_ptr(), len(in0))
    sync()
    return d_out.cpu().numpy()


# ---- eoc_cmux_device ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", host.SHAPES)
def test_cmux_equals_the_rounding_reference_on_edge_operands(eoc, shape):
    """3 items a launch (the dead pair runs), bits 1, 0, 1; every edge difference of the host test, each with one of the rotations
    (the device call takes in1 already rotated: X^rot B is formed here); no key is loaded"""
    p = host.shape_params(eoc, shape)
    sk = eoc.SecretKey(p, 6, with_cloud_key=False)
    eng = eoc.Engine(p)
    eng.leveled_rounding = True
    op = cx.orc_params(p)
    sel = sk.encrypt_selector_bits([1, 0, 1], enc_seed=10)
    fft, d_fft = cx.to_fft(sel), tc.convert(eng, sel)
    rng = np.random.default_rng(320 + sum(x or 0 for x in shape))
    rows = list(host.edge_differences(p.l, p.Bgbit).items())
    rows += rows[:-len(rows) % 3]                               # whole launches of 3
    differs = 0
    for j0 in range(0, len(rows), 3):
        A, B, rots = [], [], []
        for j in range(j0, j0 + 3):
            rot = host.ROTS[j % len(host.ROTS)]
            a, b = host.inputs_for(rows[j][1], rot, rng)
            A.append(a), B.append(b), rots.append(rot)
        A, B = np.stack(A), np.stack(B)
        turned = np.stack([cx._u32(cx.rotate(B[k], rots[k])).view(np.int32) for k in range(3)])
        before = eng.stats()["cmux_launches"]
        got = cmux_device(eng, d_fft, A, turned)
        assert eng.stats()["cmux_launches"] - before == 1
        for k in range(3):
            want = lr.cmux(op, fft[k], A[k], B[k], rots[k])
            assert np.array_equal(got[k], want), (shape, rows[j0 + k][0], rots[k], np.argwhere(got[k] != want)[:4].tolist())
            differs += not np.array_equal(want, cx.cmux(op, fft[k], A[k], B[k], rots[k]))
    assert differs
    eng.close()


def test_the_mode_changes_no_word_at_l_bgbit_32(eoc):
    p = host.custom(eoc, 4, 8)
    sk = eoc.SecretKey(p, 6, with_cloud_key=False)
    eng = eoc.Engine(p)
    sel = sk.encrypt_selector_bits([1, 0, 1], enc_seed=12)
    d_fft = tc.convert(eng, sel)
    rng = np.random.default_rng(18)
    A, B = (cc.rand_i32(rng, (3, 2, N)) for _ in range(2))
    B[2] = A[2] + np.int32(-1)                                  # the difference 0xFFFFFFFF
    off = cmux_device(eng, d_fft, A, B)
    eng.leveled_rounding = True
    on = cmux_device(eng, d_fft, A, B)
    fft = cx.to_fft(sel)
    assert cc.bytes_equal(on, off) and all(np.array_equal(on[k], cx.cmux(cx.orc_params(p), fft[k], A[k], B[k])) for k in range(3))
    eng.close()


# ---- eoc_table_read_device ----------------------------------------------------------------------------------------------------
READ_SHAPES = [(2, 3), (0, 0), (1, 10)]                         # (d, log2 W): (d, W) = (2, 8), (0, 1), (1, 1 024)


@pytest.mark.parametrize("kind", ["trivial", "ints"])
@pytest.mark.parametrize("shape", READ_SHAPES)
def test_table_read_equals_the_rounding_reference_and_decrypts(eoc, shape, kind):
    """Set A, 5 queries on an engine whose byte budget holds two (EOC_TFHE_TABLE_WS_BYTES): slices of 2, 2 and 1"""
    p, sk, pk, orc, _ = tc.keys(eoc, 0)
    d, lw = shape
    eng = rounding_engine(eoc, 0, (("EOC_TFHE_TABLE_WS_BYTES", str(2 * cc.table_walk_bytes_per_query(d) + 100)),))
    op = cx.orc_params(p)
    W, depth = 1 << lw, d + 10 - lw
    rng = np.random.default_rng(520 + d + lw)
    table, vals, q = tc.make_table(eoc, pk, kind, d, rng, 620 + d)
    last = (1 << depth) - 1
    indices = [0, last, int(rng.integers(0, last + 1)), last // 2 + 1 if depth else 0, int(rng.integers(0, last + 1))]
    sel = tc.index_selectors(sk, indices, depth, enc_seed=720 + d)
    before = eng.stats()
    got = tc.read_device(eng, table, d, lw, sel, p.n)
    after = eng.stats()
    assert after["keyswitches"] - before["keyswitches"] == 5 * W
    assert after["cmux_launches"] - before["cmux_launches"] == 3 * depth
    for k, idx in enumerate(indices):
        assert np.array_equal(sk.decrypt_ints(got[k], q), vals[W * idx:W * idx + W]), (shape, kind, idx)
    fft = [cx.to_fft(s) for s in sel]
    with cx.ThreadPoolExecutor(5) as ex:
        tl = np.stack(list(ex.map(lambda s: lr.table_read_tlwe(op, table, d, lw, s), fft)))
    ws = np.arange(W) if W <= 64 else np.r_[0:8, 500:508, W - 8:W]
    idx = (np.arange(5)[:, None] * N + ws[None, :]).ravel()
    want = co.expand(orc, tl, idx).reshape(5, len(ws), p.n + 1)
    assert np.array_equal(got[:, ws], want), (shape, kind)
    if depth and kind == "ints":                                 # and they are not the default mode's words
        trunc = np.stack([cx.table_read_tlwe(op, table, d, lw, fft[1])])
        assert not np.array_equal(co.expand(orc, trunc, ws[:1]), want[1, :1])


# ---- eoc_demux_device and eoc_table_update_device -----------------------------------------------------------------------------
@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("pset", [0, 1])
def test_demux_equals_the_rounding_reference(eoc, pset, accumulate):
    torch = torch_cuda()
    p, sk = tc.keys(eoc, pset)[:2]
    eng = rounding_engine(eoc, pset)
    op = cx.orc_params(p)
    rng = np.random.default_rng(2700 + pset)
    sel = sk.encrypt_selector_bits([1, 0, 1], enc_seed=2701)
    fft, d_fft = cx.to_fft(sel), tc.convert(eng, sel)
    x, base = cc.rand_i32(rng, (3, 2, N)), cc.rand_i32(rng, (2, 3, 2, N))
    x[2] = np.int32(-1)                                         # every word 0xFFFFFFFF
    d_x, d_o = to_dev(x), [to_dev(base[0]), to_dev(base[1])]
    before = eng.stats()["demux_launches"]
    eng.demux_device(d_fft.data_ptr(), d_x.data_ptr(), d_o[0].data_ptr(), d_o[1].data_ptr(), 3, accumulate=accumulate)
    sync()
    assert eng.stats()["demux_launches"] - before == 1
    got = [t.cpu().numpy() for t in d_o]
    for k in range(3):
        for c, w in enumerate(lr.demux(op, fft[k], x[k])):
            want = tu.wrap_i32(base[c, k].astype(np.int64) + w) if accumulate else w
            assert np.array_equal(got[c][k], want), (pset, accumulate, k, c)
    assert not np.array_equal(lr.demux(op, fft[0], x[0])[1], tu.demux(op, fft[0], x[0])[1])


@pytest.mark.parametrize("shape", [(1, 10), (3, 8)])             # d = 1: stages only; d = 3, W = 256: two rotations, three stages
@pytest.mark.parametrize("pset", [0, 1])
def test_table_update_equals_the_rounding_reference(eoc, pset, shape):
    """three queries, two of them on one entry; the last stage accumulates into the table"""
    p, sk = tc.keys(eoc, pset)[:2]
    eng = rounding_engine(eoc, pset)
    op = cx.orc_params(p)
    d, lw = shape
    depth = d + 10 - lw
    rng = np.random.default_rng(2800 + 10 * pset + d)
    table, values = cc.rand_i32(rng, (1 << d, 2, N)), cc.rand_i32(rng, (3, 2, N))
    last = (1 << depth) - 1
    sel = tc.index_selectors(sk, [last, last // 2, last], depth, enc_seed=2801 + d)
    before = eng.stats()
    got = update_device(eng, table, d, lw, sel, values)
    after = eng.stats()
    assert after["demux_launches"] - before["demux_launches"] == d and after["cmux_launches"] - before["cmux_launches"] == 10 - lw
    fft = np.stack([cx.to_fft(s) for s in sel])
    want = lr.table_update(op, table, d, lw, fft, values, threads=3)
    assert np.array_equal(got, want), (pset, shape, np.argwhere(got != want)[:6].tolist())
    assert not np.array_equal(want, tu.table_update(op, table, d, lw, fft, values, threads=3))


# ---- eoc_automaton_step_device and eoc_automaton_run_device ---------------------------------------------------------------------
# {next0, w0, next1, w1}: a rotation by 0 under bit 0 and under bit 1, by N + 1, 2N - 1 and N (wrapping), a self-loop
STEP_TRANS = np.array([[0, 0, 1, N + 1], [2, 2 * N - 1, 2, 0], [1, 63, 0, N]], np.int32)
@pytest.mark.parametrize("pset", [0, 1])
def test_automaton_step_equals_the_rounding_reference(eoc, pset):
    """3 states (a dead pair), weights 0 on either branch and weights that wrap past N, 3 queries with their own vectors"""
    p, sk = tc.keys(eoc, pset)[:2]
    eng = rounding_engine(eoc, pset)
    op = cx.orc_params(p)
    trans = STEP_TRANS
    rng = np.random.default_rng(1250 + pset)
    prev = cc.rand_i32(rng, (3, 3, 2, N))
    sel = sk.encrypt_selector_bits([1, 0, 1], enc_seed=1251)
    fft, d_fft = cx.to_fft(sel), tc.convert(eng, sel)
    got = ta.step_device(eng, trans, prev, 3, d_fft, 3)
    want = np.stack([lr.step(op, trans, prev[q], fft[q]) for q in range(3)])
    assert np.array_equal(got, want), np.argwhere(got != want)[:6].tolist()
    assert not np.array_equal(want[0], ao.step(op, trans, prev[0], fft[0]))


RUN_STEPS = 5


@pytest.mark.parametrize("pset", [0, 1])
def test_automaton_run_equals_the_rounding_reference(eoc, pset):
    """5 steps, 3 states, a weight of 0 and one that wraps past N, 3 queries, 2 start states, W = 2; and on an engine whose byte
    budget holds two queries: slices of 2 and 1, the same words"""
    p, sk, pk, orc, _ = tc.keys(eoc, pset)
    eng = rounding_engine(eoc, pset)
    op = cx.orc_params(p)
    trans, starts = ta.RUN_TRANS, ta.RUN_STARTS
    assert 0 in trans[:, [1, 3]] and (trans[:, [1, 3]] >= N).any()
    rng = np.random.default_rng(1450 + pset)
    F = ta.run_final(eoc, pk, "encrypted", rng, 1451 + pset)
    bits = np.array(ta.RUN_BITS)[:, :RUN_STEPS]
    sel = sk.encrypt_selector_bits(bits.ravel(), enc_seed=1452 + pset)
    fft = cx.to_fft(sel).reshape(3, RUN_STEPS, 2 * p.l, 2, N)
    d_fft = tc.convert(eng, sel)
    want, _ = lr.run(orc, op, trans, F, fft, starts, 1, threads=3)
    got, launches = ta.run_device(eng, trans, F, d_fft, RUN_STEPS, starts, 1, 3, p.n)
    assert launches == RUN_STEPS and np.array_equal(got, want), np.argwhere((got != want).any(axis=-1)).tolist()
    assert not np.array_equal(want[0], ao.run(orc, op, trans, F, fft[:1], starts, 1)[0][0])
    per_query = 2 * max(len(trans), len(starts)) * 2 * N * 4
    small = rounding_engine(eoc, pset, (("EOC_TFHE_TABLE_WS_BYTES", str(2 * per_query)),))
    cut, launches = ta.run_device(small, trans, F, d_fft, RUN_STEPS, starts, 1, 3, p.n)
    assert launches == 2 * RUN_STEPS and cc.bytes_equal(cut, got)


# ---- mode hygiene ---------------------------------------------------------------------------------------------------------------
def test_off_on_off_gives_the_first_words_again(eoc):
    """a CMux, a demux and an automaton step on one engine: off, the truncating references' words; on, other words (those of the
    rounding reference); off again, the first words"""
    torch = torch_cuda()
    p, sk = tc.keys(eoc, 0)[:2]
    eng = eoc.Engine(p)                                         # no key is needed
    op = cx.orc_params(p)
    rng = np.random.default_rng(3000)
    sel = sk.encrypt_selector_bits([1, 1, 0], enc_seed=3001)
    fft, d_fft = cx.to_fft(sel), tc.convert(eng, sel)
    A, B = cc.rand_i32(rng, (3, 2, N)), cc.rand_i32(rng, (3, 2, N))
    trans = STEP_TRANS

    def words():
        out = dict(cmux=cmux_device(eng, d_fft, A, B))
        d_x, d0, d1 = to_dev(A), dev_empty((3, 2, N), torch.int32), dev_empty((3, 2, N), torch.int32)
        eng.demux_device(d_fft.data_ptr(), d_x.data_ptr(), d0.data_ptr(), d1.data_ptr(), 3)
        sync()
        out.update(out0=d0.cpu().numpy(), out1=d1.cpu().numpy())
        out["step"] = ta.step_device(eng, trans, B[None], 0, d_fft, 1)
        return out

    def refs(m, demux, step):
        o = [demux(op, fft[k], A[k]) for k in range(3)]
        return dict(cmux=np.stack([m.cmux(op, fft[k], A[k], B[k]) for k in range(3)]), out0=np.stack([x[0] for x in o]),
                    out1=np.stack([x[1] for x in o]), step=step(op, trans, B, fft[0])[None])

    assert eng.leveled_rounding is False
    first = words()
    eng.leveled_rounding = True
    assert eng.leveled_rounding is True and eoc.lib().eoc_engine_leveled_rounding(eng.h) == 1
    on = words()
    eng.leveled_rounding = False
    again = words()
    trunc, rnd = refs(cx, tu.demux, ao.step), refs(lr, lr.demux, lr.step)
    for name in first:
        assert cc.bytes_equal(first[name], trunc[name]), name
        assert cc.bytes_equal(on[name], rnd[name]) and not cc.bytes_equal(on[name], first[name]), name
        assert cc.bytes_equal(again[name], first[name]), name
    eng.close()


def test_global_setter_on_one_and_two_engines(eoc):
    """eoc_global_set_leveled_rounding ahead of eoc_gpu_init (one engine, created later) and on a live context (two engines):
    table_read, table_update and automaton_run give the single-engine device words of the rounding mode; switched off, the read
    gives the default mode's"""
    p, sk, pk, _, trunc_eng = tc.keys(eoc, 0)
    eng = rounding_engine(eoc, 0)
    rng = np.random.default_rng(3100)
    d, lw, depth = 1, 9, 2
    table = tc.make_table(eoc, pk, "ints", d, rng, 3101)[0]
    sel = tc.index_selectors(sk, [3, 0, 2], depth, enc_seed=3102)
    values = cc.rand_i32(rng, (3, 2, N))
    F = ta.run_final(eoc, pk, "trivial", rng, 0)
    asel = sk.encrypt_selector_bits(np.ravel(ta.RUN_BITS)[:6], enc_seed=3103)         # 3 queries x 2 steps
    ref = dict(read=tc.read_device(eng, table, d, lw, sel, p.n), update=update_device(eng, table, d, lw, sel, values),
               run=ta.run_device(eng, ta.RUN_TRANS, F, tc.convert(eng, asel), 2, ta.RUN_STARTS, 0, 3, p.n)[0])
    off_read = tc.read_device(trunc_eng, table, d, lw, sel, p.n)
    assert not np.array_equal(ref["read"], off_read)

    def calls():
        return dict(read=eoc.table_read(table, d, lw, sel), update=eoc.table_update(table, d, lw, sel, values),
                    run=eoc.automaton_run(ta.RUN_TRANS, F, asel.reshape(3, 2, 2 * p.l, 2, N), ta.RUN_STARTS, 0))

    try:
        eoc.gpu_shutdown()
        eoc.set_leveled_rounding(True)                          # no engine yet
        eoc.gpu_init(p, devices=[0])
        eoc.upload_cloud_key(sk)
        assert eoc.lib().eoc_engine_leveled_rounding(eoc.lib().eoc_global_engine()) == 1
        one = calls()
        eoc.gpu_shutdown()
        eoc.set_leveled_rounding(False)
        eoc.gpu_init(p, devices=[0, 0])
        eoc.upload_cloud_key(sk)
        off = eoc.table_read(table, d, lw, sel)
        eoc.set_leveled_rounding(True)                          # two live engines
        two = calls()
        eoc.set_leveled_rounding(False)
        off_again = eoc.table_read(table, d, lw, sel)
    finally:
        eoc.gpu_shutdown()
        eoc.set_leveled_rounding(False)
    for name, want in ref.items():
        assert np.array_equal(one[name], want) and np.array_equal(two[name], want), name
    assert np.array_equal(off, off_read) and np.array_equal(off_again, off_read)


def test_capture_freezes_the_mode_and_a_graph_replays_the_mode_it_was_captured_under(eoc):
    """tests/capture_cases.py's Cmux case on its fresh engine, in rounding mode: the setter is refused while the capture is open
    (and changes nothing); after the capture the mode is switched off, and the replay on new inputs still gives the rounding
    words while an eager call gives the default mode's"""
    torch, L = torch_cuda(), eoc.lib()
    c = cc.CASES["cmux"](eoc)
    eng = c.eng
    eng.leveled_rounding = True

    def rounding_words(k):
        i = c.inp[k]
        return np.stack([lr.cmux(c.op, i["fft"][q], i["a"][q], i["b"][q]) for q in range(c.count)])

    st = side_stream(torch)
    c.set_inputs(0)
    c.poison()
    sync()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        c.run(st.cuda_stream)
    st.synchronize()
    assert cc.bytes_equal(c.fetch()["out"], rounding_words(0))
    seen = {}

    def run_and_try_the_setter(stream):
        c.run(stream)
        seen["rc"] = L.eoc_engine_set_leveled_rounding(eng.h, 0)
        seen["err"] = L.eoc_last_error().decode()
        seen["mode"] = L.eoc_engine_leveled_rounding(eng.h)

    g = capture(torch, st, run_and_try_the_setter)
    assert seen["rc"] == EOC_ERR_STATE and seen["mode"] == 1 and "capture" in seen["err"], seen
    eng.leveled_rounding = False                                # the capture has ended
    assert eng.leveled_rounding is False
    c.set_inputs(1)
    c.poison()
    sync()
    g.replay()
    sync()
    assert cc.bytes_equal(c.fetch()["out"], rounding_words(1))
    c.poison()
    c.run(None)
    sync()
    assert cc.bytes_equal(c.fetch()["out"], c.want(1)["out"])    # eager, mode off: the truncating reference
    c.poison()
    g.replay()
    sync()
    assert cc.bytes_equal(c.fetch()["out"], rounding_words(1))
    del g
    c.close()


# ---- the long run and the noise of a read -------------------------------------------------------------------------------------
def test_a_run_twice_the_truncating_budget_decrypts_and_equals_the_reference(eoc):
    """S = min(2 automaton_budget(), 1 024) all-ones steps of popcount() on Set A in rounding mode, one query: S launches; the
    key-switched output equals the reference's words (computed once, tests/test_leveled_round_cpu.py) and decrypts"""
    ref = host.long_run_reference(eoc)
    p, sk = tc.keys(eoc, 0)[:2]
    assert host.LONG_SEED == 1 and np.array_equal(sk.lwe_key, ref["sk"].lwe_key)
    eng = rounding_engine(eoc, 0)
    S, aut = len(ref["bits"]), ref["aut"]
    d_fft = tc.convert(eng, ref["sel"])
    out, launches = ta.run_device(eng, aut, ref["final"], d_fft, S, [aut.start], host.LONG_LW, 1, p.n)
    assert launches == S
    assert np.array_equal(out, ref["out"]), np.argwhere((out != ref["out"]).any(axis=-1)).tolist()
    W = 1 << host.LONG_LW
    want = [aut.evaluate_plain(ref["bits"], final=[np.roll(ref["table"], -w)]) for w in range(W)]
    assert sk.decrypt_ints(out.reshape(-1, p.n + 1), 2).tolist() == want


def test_noise_of_a_rounding_read_matches_the_model(eoc):
    """the plan of tests/test_gpu_cmux.py's read measurement on Set A: d = 3, W = 16 (depth 9), 1 024 queries, 16 384 samples.  The
    RAW mean -- no index term is removed: the rounding mode's is 2^-33-sized (noise.table_read_mean(rounding=True), added for
    completeness) -- is within 4 standard errors of the key switch's ks_mean, and the variance within that test's 8 % of
    table_read_var."""
    torch = torch_cuda()
    p, sk = tc.keys(eoc, 0)[:2]
    eng = rounding_engine(eoc, 0)
    d, lw, depth, queries, W = 3, 4, 9, 1024, 16
    rng = np.random.default_rng(1000)
    vals = rng.integers(0, 2, 8 * N).astype(np.uint8)
    table = eoc.trivial_table(co.bit_msgs(vals))
    indices = rng.integers(0, 1 << depth, queries)
    bits = ((indices[:, None] >> np.arange(depth)[None, :]) & 1).astype(np.uint8)
    sel_ints = eoc.lib().eoc_tgsw_len(C.byref(p))
    d_fft = dev_empty((queries * depth, sel_ints), torch.float64)
    step = 64 * depth
    for s0 in range(0, queries * depth, step):
        blk = sk.encrypt_selector_bits(bits.ravel()[s0:s0 + step], enc_seed=1100, first_idx=s0)
        d_blk = to_dev(blk)
        eng.tgsw_to_fft_device(d_blk.data_ptr(), len(blk), d_fft[s0:].data_ptr())
        sync()
    d_tab = to_dev(table)
    d_out = dev_empty((queries, W, p.n + 1), torch.int32)
    eng.table_read_device(d_tab.data_ptr(), d, lw, d_fft.data_ptr(), queries, d_out.data_ptr())
    sync()
    out = d_out.cpu().numpy().astype(np.int64).reshape(queries * W, p.n + 1)
    ph = tc.wrap32(out[:, -1] - out[:, :-1] @ sk.lwe_key.astype(np.int64))
    slots = (indices[:, None] * W + np.arange(W)[None, :]).ravel()
    assert np.array_equal((ph > 0).astype(np.uint8), vals[slots])
    err = (ph - co.bit_msgs(vals[slots])) / 2.0**32
    cond = np.array([[noise.table_read_mean(p, sk.tlwe_key, i, d, lw, w, rounding=True) for w in range(W)] for i in indices]).ravel()
    trunc = np.array([noise.table_read_mean(p, sk.tlwe_key, i, d, lw, 0) for i in indices])
    pred = noise.predict(p, sk.lwe_key, sk.tlwe_key, sk.ksk)
    var = noise.table_read_var(p, sk.lwe_key, sk.tlwe_key, depth, 0.0, sk.ksk)
    z = (err.mean() - (pred["ks_mean"] + cond.mean())) / (err.std() / np.sqrt(len(err)))
    print(f"rounding read: var {err.var():.4e} model {var:.4e} ratio {err.var() / var:.4f}; raw mean {err.mean():.3e}, ks_mean "
          f"{pred['ks_mean']:.3e}, rounding index term {cond.mean():.3e} (the default mode's at slot 0: {trunc.mean():.3e}): z {z:.2f}")
    assert abs(err.var() / var - 1) < 0.08
    assert abs(z) < 4
