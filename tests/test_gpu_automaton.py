"""Finite automata on encrypted bit strings on the MI355X: k_automaton_step and the run driver against the
composed reference (tests/automaton_oracle.py) word for word, the decrypted results against Automaton.evaluate_plain, a run
captured into a hipGraph (the helpers of tests/capture_cases.py), and the calls next to it on the same engine left alone.
Host side: tests/test_automaton_cpu.py.  Every k_automaton_step instance on edge differences, at every weight, with strides of its
own and inside a run of one step: tests/test_gpu_automaton_instances.py."""
import itertools

import numpy as np
import pytest

import automaton_oracle as ao
import capture_cases as cc
import cmux_oracle as cx
import compact_oracle as co
import test_gpu_cmux as tc
from gpu_util import dev_empty, sync, to_dev, torch_cuda
from test_automaton_cpu import CHAIN_STEPS, acceptor_final, table_final
from test_gpu_br_instances import custom_params, reference
from test_gpu_capture import capture, side_stream

pytestmark = pytest.mark.gpu
N = 1024
FILL = 0x5A5A5A5A
EOC_ERR_STATE = -6
W_ALL = (0, 1, 63, 64, N - 1, N, N + 1, 2 * N - 1)
# (next0, w0, next1, w1) per state.  5 states: both successors the state itself (and equal), a self-loop, next0 == next1, and
# every weight of W_ALL on a branch; 3 states: the same structures, the weights spread over both branches
TRANS = {5: [[0, 0, 0, 1], [1, 63, 3, 64], [4, N - 1, 4, N], [2, N + 1, 0, 2 * N - 1], [3, 64, 1, 0]],
         3: [[0, 2 * N - 1, 0, N], [1, N + 1, 2, N - 1], [0, 63, 0, 1]]}
STEP_SHAPES = [(3, 1), (5, 3)]                                  # (states, queries): 3 items and 15 -- a dead pair either way


@pytest.fixture(scope="module")
def eoc(built_lib):
    torch_cuda()
    import eoc_tfhe_amd
    return eoc_tfhe_amd


def test_the_transition_tables_cover_the_named_cases():
    for Q, t in TRANS.items():
        t = np.array(t)
        assert any(t[q, 0] == q and t[q, 2] == q for q in range(Q))                       # both successors the state itself
        assert any((t[q, 0] == q) != (t[q, 2] == q) for q in range(Q))                    # a self-loop on one branch
        assert any(t[q, 0] == t[q, 2] != q for q in range(Q))                             # next0 == next1
    t = np.array(TRANS[5])
    assert set(W_ALL) <= set(t[:, 1]) | set(t[:, 3]) and set(t[:, 1]) & set(W_ALL) and set(t[:, 3]) & set(W_ALL)
    t3 = np.array(TRANS[3])
    assert set(t3[:, [1, 3]].ravel()) <= set(W_ALL)


def step_device(eng, trans, prev, stride, d_fft, queries):
    """next [queries][states][2][N]; the buffer holds one sample more, which must keep its fill"""
    torch = torch_cuda()
    Q = len(trans)
    d_prev = to_dev(prev)
    d_next = torch.full((queries * Q + 1, 2, N), FILL, dtype=torch.int32, device="cuda")
    before = eng.stats()
    eng.automaton_step_device(trans, d_prev.data_ptr(), stride, d_fft.data_ptr(), 1, d_next.data_ptr(), queries)
    sync()
    after = eng.stats()
    assert after["automaton_launches"] - before["automaton_launches"] == 1 == eng.automaton_launches() - before["automaton_launches"]
    assert after["cmux_launches"] == before["cmux_launches"]
    out = d_next.cpu().numpy()
    assert (out[-1] == FILL).all()
    return out[:-1].reshape(queries, Q, 2, N)


def check_step(eng, sk, op, key, Q, queries, shared, seed):
    """both bit assignments of one shape against the reference, computed once under the conversion contract (< 2^51)"""
    trans = np.array(TRANS[Q], np.int32)
    rng = np.random.default_rng(seed)
    prev = cc.rand_i32(rng, (1 if shared else queries, Q, 2, N))
    for flip in (0, 1):
        bits = [(q + flip) & 1 for q in range(queries)]
        sel = sk.encrypt_selector_bits(bits, enc_seed=seed + flip)
        fft = cx.to_fft(sel)
        d_fft = tc.convert(eng, sel)
        want = reference(key + (Q, queries, flip),
                         lambda: np.stack([ao.step(op, trans, prev[0 if shared else q], fft[q]) for q in range(queries)]))
        got = step_device(eng, trans, prev, 0 if shared else Q, d_fft, queries)
        bad = np.argwhere(got != want)
        assert len(bad) == 0, (key, Q, queries, bits, len(bad), bad[:6].tolist())


@pytest.mark.parametrize("shape", STEP_SHAPES)
@pytest.mark.parametrize("pset", [0, 1])
def test_step_equals_the_reference(eoc, pset, shape):
    """Set A and Set B (k_automaton_step<2,10> / <3,7>), pseudo-random full-range state vectors, selectors of 0 and of 1; one
    query reads a shared vector (stride 0), three read their own"""
    p, sk, _, _, eng = tc.keys(eoc, pset)
    Q, queries = shape
    check_step(eng, sk, cx.orc_params(p), ("automaton step", pset), Q, queries, queries == 1, 1200 + 10 * pset + Q)


@pytest.mark.parametrize("gadget", [(1, 9), (2, 8), (3, 6), (4, 6)])
def test_run_time_base_instance_equals_the_reference(eoc, gadget):
    """k_automaton_step<1,0> .. <4,0>: a gadget base read at run time, on a real key at n = 16 built as
    tests/test_gpu_cmux_instances.py builds its keys; no key is loaded"""
    l, Bgbit = gadget
    p = custom_params(eoc, l, Bgbit, 16)
    sk = eoc.SecretKey(p, 83)
    eng = eoc.Engine(p)
    check_step(eng, sk, cx.orc_params(p), ("automaton step", l, Bgbit), 3, 1, True, 1300 + 10 * l + Bgbit)
    eng.close()


# ---- the run ----------------------------------------------------------------------------------------------------------------
RUN_TRANS = np.array([[1, 1, 2, 0], [1, 0, 0, N + 1], [0, 2, 2, 1]], np.int32)
RUN_STEPS, RUN_QUERIES, RUN_STARTS = 6, 3, [2, 0]
RUN_BITS = [[1, 0, 1, 1, 0, 1], [0, 0, 0, 0, 0, 0], [1, 1, 0, 1, 1, 1]]


def run_device(eng, trans, final, d_fft, steps, starts, lw, queries, n):
    torch = torch_cuda()
    d_final = to_dev(np.ascontiguousarray(final, np.int32))
    rows = queries * len(starts) * (1 << lw)
    d_out = torch.full((rows + 1, n + 1), FILL, dtype=torch.int32, device="cuda")
    before = eng.stats()
    eng.automaton_run_device(trans, d_final.data_ptr(), d_fft.data_ptr() if steps else None, steps, starts, lw, d_out.data_ptr(),
                             queries)
    sync()
    after = eng.stats()
    assert after["keyswitches"] - before["keyswitches"] == (rows if steps else len(starts) << lw)
    assert after["cmux_launches"] == before["cmux_launches"]
    out = d_out.cpu().numpy()
    assert (out[-1] == FILL).all()
    return out[:-1].reshape(queries, len(starts), 1 << lw, n + 1), after["automaton_launches"] - before["automaton_launches"]


def run_final(eoc, pk, kind, rng, seed):
    vals = rng.integers(0, 4, 3 * N).astype(np.uint8)
    return eoc.trivial_table(co.int_msgs(vals, 4)) if kind == "trivial" else pk.encrypt_ints(vals, 4, enc_seed=seed)


@pytest.mark.parametrize("kind", ["trivial", "encrypted"])
@pytest.mark.parametrize("pset", [0, 1])
def test_run_equals_the_composed_reference(eoc, pset, kind):
    """6 steps, 3 states with weights (a wrap past N among them), 3 queries, 2 start states, log2_width 2 and 0 (the slot-0 rows
    of the same reference); steps = 0; with the trivial final vector also an engine whose byte budget holds two queries: slices
    of 2 and 1, the same words, steps launches per slice"""
    p, sk, pk, orc, eng = tc.keys(eoc, pset)
    op = cx.orc_params(p)
    rng = np.random.default_rng(1400 + pset)
    F = run_final(eoc, pk, kind, rng, 1410 + pset)
    assert F.shape == (3, 2, N)
    sel = sk.encrypt_selector_bits(np.ravel(RUN_BITS), enc_seed=1420 + pset)
    fft = cx.to_fft(sel).reshape(RUN_QUERIES, RUN_STEPS, 2 * p.l, 2, N)
    d_fft = tc.convert(eng, sel)
    want = reference(("automaton run", pset, kind), lambda: ao.run(orc, op, RUN_TRANS, F, fft, RUN_STARTS, 2)[0])
    got = {}
    for lw in (2, 0):
        got[lw], launches = run_device(eng, RUN_TRANS, F, d_fft, RUN_STEPS, RUN_STARTS, lw, RUN_QUERIES, p.n)
        assert launches == RUN_STEPS
        w = want[:, :, :1 << lw]
        assert got[lw].shape == w.shape
        assert np.array_equal(got[lw], w), (pset, kind, lw, np.argwhere((got[lw] != w).any(axis=-1)).tolist())
    # steps = 0: the start states' samples of the final vector, for every query
    want0 = reference(("automaton run", pset, kind, 0),
                      lambda: ao.run(orc, op, RUN_TRANS, F, np.zeros((RUN_QUERIES, 0, 2 * p.l, 2, N)), RUN_STARTS, 2)[0])
    got0, launches = run_device(eng, RUN_TRANS, F, d_fft, 0, RUN_STARTS, 2, RUN_QUERIES, p.n)
    assert launches == 0 and np.array_equal(got0, want0)
    if kind != "trivial":
        return
    per_query = 2 * max(len(RUN_TRANS), len(RUN_STARTS)) * 2 * N * 4
    with cc.knobs({"EOC_TFHE_TABLE_WS_BYTES": str(2 * per_query)}):
        small = eoc.Engine(p)
    small.load_cloud_key(sk)
    for lw in (2, 0):
        cut, launches = run_device(small, RUN_TRANS, F, d_fft, RUN_STEPS, RUN_STARTS, lw, RUN_QUERIES, p.n)
        assert launches == RUN_STEPS * 2 and np.array_equal(cut, got[lw]), (pset, lw, launches)
    small.close()


# ---- decrypted results ------------------------------------------------------------------------------------------------------
def selectors_of(eng, sk, inputs, steps, seed):
    """device selectors [len(inputs)][steps]: one encrypted selector per (position, bit value), gathered per input on the device"""
    torch = torch_cuda()
    both = tc.convert(eng, sk.encrypt_selector_bits([0, 1] * steps, enc_seed=seed))      # [steps * 2][2l][2][N]
    pick = torch.tensor([[2 * t + int(b) for t, b in enumerate(bits)] for bits in inputs], device="cuda")
    return both[pick.reshape(-1)].contiguous()


@pytest.mark.parametrize("pset", [0, 1])
def test_every_6_bit_input_decrypts_to_the_plain_evaluation(eoc, pset):
    p, sk, _, _, eng = tc.keys(eoc, pset)
    steps = 6
    inputs = list(itertools.product((0, 1), repeat=steps))
    d_fft = selectors_of(eng, sk, inputs, steps, 1500 + pset)
    div3, pop = eoc.Automaton.divisible_by(3), eoc.Automaton.popcount()
    table = np.arange(steps + 1) % 4
    for name, aut, final, q, tab in (("divisible_by(3)", div3, acceptor_final(eoc, div3), 2, None),
                                     ("popcount()", pop, table_final(eoc, table, 4), 4, [table])):
        out, _ = run_device(eng, aut, final, d_fft, steps, [aut.start], 0, len(inputs), p.n)
        got = sk.decrypt_ints(out.reshape(-1, p.n + 1), q).tolist()
        want = [aut.evaluate_plain(bits, final=tab) for bits in inputs]
        assert got == want, (pset, name, [i for i in range(len(inputs)) if got[i] != want[i]])


@pytest.mark.parametrize("pset", [0, 1])
def test_a_chain_inside_the_budget_decrypts(eoc, pset):
    """CHAIN_STEPS = 24 steps of all-ones input (noise.automaton_budget gives 449 / 894 at p = 2 and 199 / 386 at p = 4 on Set A /
    Set B: tests/test_automaton_cpu.py): 2^24 - 1 is divisible by 3, and the count's table entry comes out"""
    p, sk, _, _, eng = tc.keys(eoc, pset)
    bits = [1] * CHAIN_STEPS
    d_fft = tc.convert(eng, sk.encrypt_selector_bits(bits, enc_seed=1600 + pset))
    div3, pop = eoc.Automaton.divisible_by(3), eoc.Automaton.popcount()
    table = (np.arange(CHAIN_STEPS + 1) + 1) % 4
    for aut, final, q, tab in ((div3, acceptor_final(eoc, div3), 2, None), (pop, table_final(eoc, table, 4), 4, [table])):
        out, launches = run_device(eng, aut, final, d_fft, CHAIN_STEPS, [aut.start], 0, 1, p.n)
        assert launches == CHAIN_STEPS
        assert sk.decrypt_ints(out.reshape(-1, p.n + 1), q).tolist() == [aut.evaluate_plain(bits, final=tab)] != [0]


# ---- capture ----------------------------------------------------------------------------------------------------------------
def test_a_captured_run_replays_the_eager_words_and_growth_is_refused(eoc):
    torch = torch_cuda()
    p, sk, pk, orc, eng2 = tc.keys(eoc, 0)
    with cc.knobs({}):
        eng = eoc.Engine(p)
    eng.load_cloud_key(sk)
    lw, rows = 2, RUN_QUERIES * len(RUN_STARTS) * 4
    F = run_final(eoc, pk, "encrypted", np.random.default_rng(1700), 1701)
    d_final = to_dev(F)
    sets = [tc.convert(eng2, sk.encrypt_selector_bits(np.roll(np.ravel(RUN_BITS), 5 * k), enc_seed=1710 + k)) for k in range(3)]
    d_fft = torch.empty_like(sets[0])
    d_out = torch.full((rows, p.n + 1), cc.POISON, dtype=torch.int32, device="cuda")

    def run(stream, e=eng, fft=d_fft, out=d_out, queries=RUN_QUERIES):
        e.automaton_run_device(RUN_TRANS, d_final.data_ptr(), fft.data_ptr(), RUN_STEPS, RUN_STARTS, lw, out.data_ptr(), queries,
                               stream=stream)

    def eager(k):
        out = torch.full_like(d_out, cc.POISON)
        run(None, e=eng2, fft=sets[k], out=out)
        sync()
        return out.cpu().numpy()

    st = side_stream(torch)
    d_fft.copy_(sets[0])
    sync()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        run(st.cuda_stream)                                     # sizes the workspace, loads the code object
    st.synchronize()
    assert cc.bytes_equal(d_out.cpu().numpy(), eager(0))
    grows = eoc.lib().eoc_engine_workspace_grows(eng.h)
    g = capture(torch, st, run)
    assert eoc.lib().eoc_engine_workspace_grows(eng.h) == grows
    for k in (1, 2):
        d_fft.copy_(sets[k])
        run(None, fft=sets[(k + 1) % 3], out=torch.empty_like(d_out))      # the ring advances, the state vectors are rewritten
        d_out.fill_(cc.POISON)
        sync()
        assert eoc.lib().eoc_engine_workspace_grows(eng.h) == grows
        g.replay()
        sync()
        assert cc.bytes_equal(d_out.cpu().numpy(), eager(k)), k
    # a call under capture that would need larger state vectors is refused, and nothing grew
    wide_fft = torch.zeros((8 * RUN_STEPS,) + tuple(sets[0].shape[1:]), dtype=torch.float64, device="cuda")
    wide_out = torch.empty((8 * len(RUN_STARTS) * 4, p.n + 1), dtype=torch.int32, device="cuda")
    with pytest.raises(eoc.EocError, match=rf"code {EOC_ERR_STATE}\).*graph capture: the automaton state vector"):
        capture(torch, st, lambda s: run(s, fft=wide_fft, out=wide_out, queries=8))
    sync()
    assert eoc.lib().eoc_engine_workspace_grows(eng.h) == grows
    d_fft.copy_(sets[1])
    g.replay()                                                  # the graph is still good
    sync()
    assert cc.bytes_equal(d_out.cpu().numpy(), eager(1))
    del g
    eng.close()


# ---- neighbours -------------------------------------------------------------------------------------------------------------
def test_calls_next_to_a_run_are_unchanged(eoc):
    """the scratch rule: a table read (the same two buffers) and a 64-gate NAND batch give the same words before and after an
    automaton run on the same engine"""
    torch = torch_cuda()
    p, sk, pk, _, _ = tc.keys(eoc, 0)
    eng = eoc.Engine(p)
    eng.load_cloud_key(sk)
    rng = np.random.default_rng(1800)
    d, lw = 2, 1
    table = tc.make_table(eoc, pk, "ints", d, rng, 1801)[0]
    rsel = tc.index_selectors(sk, [5, 2047, 1000], d + 10 - lw, enc_seed=1802)
    a, b = (to_dev(sk.encrypt_bits(rng.integers(0, 2, 64), 1803 + j)) for j in range(2))

    def neighbours():
        read = tc.read_device(eng, table, d, lw, rsel, p.n)
        out = dev_empty((64, p.n + 1), torch.int32)
        eng.gate_batch_device(eoc.OPS["NAND"], a.data_ptr(), b.data_ptr(), None, out.data_ptr(), 64)
        sync()
        return read, out.cpu().numpy()

    before = neighbours()
    F = run_final(eoc, pk, "trivial", rng, 0)
    d_fft = tc.convert(eng, sk.encrypt_selector_bits(np.ravel(RUN_BITS), enc_seed=1805))
    out, launches = run_device(eng, RUN_TRANS, F, d_fft, RUN_STEPS, RUN_STARTS, 1, RUN_QUERIES, p.n)
    assert launches == RUN_STEPS
    after = neighbours()
    assert cc.bytes_equal(before[0], after[0]) and cc.bytes_equal(before[1], after[1])
    again, _ = run_device(eng, RUN_TRANS, F, d_fft, RUN_STEPS, RUN_STARTS, 1, RUN_QUERIES, p.n)
    assert cc.bytes_equal(out, again)
    eng.close()


# ---- the global context and the refusals on a live engine -------------------------------------------------------------------
def test_global_context_one_and_two_engines(eoc):
    """eoc_automaton_run (host buffers, selectors in torus form) on one engine and on two (queries cut 2 + 1) gives the device
    call's words"""
    p, sk, pk, _, eng = tc.keys(eoc, 0)
    F = run_final(eoc, pk, "encrypted", np.random.default_rng(1900), 1901)
    sel = sk.encrypt_selector_bits(np.ravel(RUN_BITS), enc_seed=1902)
    ref, _ = run_device(eng, RUN_TRANS, F, tc.convert(eng, sel), RUN_STEPS, RUN_STARTS, 1, RUN_QUERIES, p.n)
    sel5 = sel.reshape(RUN_QUERIES, RUN_STEPS, 2 * p.l, 2, N)
    try:
        eoc.gpu_shutdown()
        eoc.gpu_init(p, devices=[0])
        eoc.upload_cloud_key(sk)
        one = eoc.automaton_run(RUN_TRANS, F, sel5, RUN_STARTS, 1)
        none = eoc.automaton_run(RUN_TRANS, F, sel5[:, :0], RUN_STARTS, 1)
        eoc.gpu_shutdown()
        eoc.gpu_init(p, devices=[0, 0])
        eoc.upload_cloud_key(sk)
        two = eoc.automaton_run(RUN_TRANS, F, sel5, RUN_STARTS, 1)
        per = [e["keyswitches"] for e in eoc.stats_multi()["engines"]]
    finally:
        eoc.gpu_shutdown()
    assert np.array_equal(one, ref) and np.array_equal(two, ref)
    assert per == [2 * len(RUN_STARTS) * 2, 1 * len(RUN_STARTS) * 2]
    zero, _ = run_device(eng, RUN_TRANS, F, None, 0, RUN_STARTS, 1, RUN_QUERIES, p.n)
    assert np.array_equal(none, zero)


def test_refusals_on_a_live_engine_touch_nothing(eoc):
    """a malformed automaton, a null pointer and a missing key are refused with their codes; the output keeps its fill and no
    launch is counted"""
    torch = torch_cuda()
    L = eoc.lib()
    p = eoc.default_params(0)
    sk = eoc.SecretKey(p, 31, with_cloud_key=False)
    eng = eoc.Engine(p)                                         # no key
    d_fft = tc.convert(eng, sk.encrypt_selector_bits([1, 0], enc_seed=1))
    F = to_dev(cc.rand_i32(np.random.default_rng(2), (2, 2, N)))
    out = torch.full((4, p.n + 1), FILL, dtype=torch.int32, device="cuda")
    nxt = torch.full((2, 2, N), FILL, dtype=torch.int32, device="cuda")
    good = np.array([[1, 0, 0, 5], [1, 2047, 1, 0]], np.int32)
    starts = np.array([0, 1], np.int32)

    def run(trans=good, states=2, final=F.data_ptr(), fft=d_fft.data_ptr(), st=starts, lw=0, o=out.data_ptr()):
        t = np.ascontiguousarray(trans, np.int32)
        return L.eoc_automaton_run_device(eng.h, t.ctypes.data, states, final, fft, 2, st.ctypes.data, len(st), lw, o, 1, None)

    def step(trans=good, states=2, prev=F.data_ptr(), stride=0, fft=d_fft.data_ptr(), o=nxt.data_ptr()):
        t = np.ascontiguousarray(trans, np.int32)
        return L.eoc_automaton_step_device(eng.h, t.ctypes.data, states, prev, stride, fft, 1, o, 1, None)

    assert run() == tc.EOC_ERR_NO_KEY                           # well formed: only the key is missing
    for bad in (dict(trans=[[2, 0, 0, 0], [0, 0, 0, 0]]), dict(trans=[[0, 0, 0, 2 * N], [0, 0, 0, 0]]), dict(states=0),
                dict(st=np.array([0, 2], np.int32)), dict(lw=11), dict(final=None), dict(fft=None), dict(o=None)):
        assert run(**bad) == tc.EOC_ERR_ARG, bad
    for bad in (dict(trans=[[0, 0, -1, 0], [0, 0, 0, 0]]), dict(trans=[[0, -1, 0, 0], [0, 0, 0, 0]]), dict(states=4097),
                dict(prev=None), dict(fft=None), dict(o=None), dict(stride=1)):
        assert step(**bad) == tc.EOC_ERR_ARG, bad
    sync()
    assert eng.automaton_launches() == 0 and bool((out == FILL).all()) and bool((nxt == FILL).all())
    assert step() == 0                                          # the step needs no key
    sync()
    assert eng.automaton_launches() == 1 and not bool((nxt == FILL).all())
    eng.close()
