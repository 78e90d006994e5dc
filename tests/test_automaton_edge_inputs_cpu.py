"""The edge inputs of tests/automaton_edge_inputs.py do what they claim (no GPU): through the two rotations of a step
(automaton_oracle.successor) every pair of states decomposes its named difference of leveled_edge_inputs.cmux_differences and
its negation, the alternating pair gives the wrapping words its weights are listed for, every truncation is a closed
automaton, the sweep meets every weight on both branches, the constant selector of the full-scale rows puts the reference's
conversions in the binade the table names in both directions, and on all of these states the reference (tests/c/cmux_ref.c)
stays within the project's 8 LSB of EXACT integer evaluation.  The device side is tests/test_gpu_automaton_instances.py."""
import ctypes as C

import numpy as np
import pytest

import automaton_edge_inputs as aei
import automaton_oracle as ao
import cmux_oracle as cx
import leveled_edge_inputs as lei
import oracle_lib as ol
from test_leveled_edge_inputs_cpu import BOUND_EXTPROD_LSB, params, wrap32

N = 1024
INSTANCES = list(aei.full_scale)


@pytest.fixture(scope="module")
def eoc(built_lib):
    import eoc_tfhe_amd
    return eoc_tfhe_amd


def gadget(name):
    cfg = aei.full_scale[name]
    return cfg, cfg["l"], cfg["Bgbit"]


def params_of(l, Bgbit):
    op = ol.OrcParams()
    assert ol.lib().orc_default_params(0, C.byref(op)) == 0
    op.l, op.Bgbit = l, Bgbit
    return op


def difference(trans, prev, q):
    """X^(-w1) prev[next1] - X^(-w0) prev[next0] of state q as uint32 words: what the step decomposes"""
    n0, w0, n1, w1 = (int(x) for x in trans[q])
    return cx._u32(ao.successor(prev, n1, w1).astype(np.int64) - ao.successor(prev, n0, w0))


def test_the_instances_are_the_cmux_rows_renamed():
    assert list(aei.full_scale) == ["k_automaton_step<2,10>", "k_automaton_step<3,7>", "k_automaton_step<1,0>",
                                    "k_automaton_step<2,0>", "k_automaton_step<3,0>", "k_automaton_step<4,0>"]
    assert list(aei.full_scale.values()) == list(lei.cmux_full_scale.values())
    assert aei.constant_selector is lei.constant_selector


@pytest.mark.parametrize("name", INSTANCES)
def test_every_pair_decomposes_its_named_difference_and_its_negation(name):
    _, l, Bgbit = gadget(name)
    trans, prev, names = aei.edge_automaton(l, Bgbit)
    rows = aei.derived_rows(l, Bgbit)
    Q = len(names)
    assert trans.shape == (Q, 4) and prev.shape == (Q, 2, N) and trans.dtype == prev.dtype == np.int32
    assert Q == 2 * (len(rows) + len(aei.ALT_WEIGHTS)) and len(rows) >= 16
    assert sum(D.shape[0] for nm, D in lei.cmux_differences(l, Bgbit).items() if nm != "alternating") == len(rows)
    assert (trans[:, [0, 2]] >= 0).all() and (trans[:, [0, 2]] < Q).all()
    assert (trans[:, [1, 3]] >= 0).all() and (trans[:, [1, 3]] < 2 * N).all()
    for k, (nm, D) in enumerate(rows):
        assert names[2 * k] == nm and names[2 * k + 1] == nm + " negated"
        w0, w1 = aei.weight_pair(k)
        assert trans[2 * k].tolist() == [2 * k, w0, 2 * k + 1, w1] and trans[2 * k + 1].tolist() == [2 * k + 1, w1, 2 * k, w0]
        assert np.array_equal(difference(trans, prev, 2 * k), D), nm
        assert np.array_equal(difference(trans, prev, 2 * k + 1), cx._u32(-D.astype(np.int64))), nm
        assert prev[2 * k].min() < -2**30 and prev[2 * k].max() > 2**30                    # P0: full-range words
    # the weights: every value of W_ALL on either branch, an equal pair, and a turned zero row
    pairs = [aei.weight_pair(k) for k in range(len(rows))]
    assert {a for a, _ in pairs} == {b for _, b in pairs} == set(aei.W_ALL) and any(a == b for a, b in pairs)
    assert len({aei.weight_pair(k) for k in range(64)}) == 64
    assert names[0] == "zero[0]" and pairs[0][0] != 0 != pairs[0][1]
    # another seed: other words, the same differences
    t2, p2, n2 = aei.edge_automaton(l, Bgbit, seed=1)
    assert np.array_equal(t2, trans) and n2 == names and not np.array_equal(p2[0], prev[0])
    assert all(np.array_equal(difference(t2, p2, q), difference(trans, prev, q)) for q in range(Q))


@pytest.mark.parametrize("name", INSTANCES)
def test_the_alternating_pairs_give_the_wrapping_words(name):
    _, l, Bgbit = gadget(name)
    trans, prev, names = aei.edge_automaton(l, Bgbit)
    first = len(names) - 2 * len(aei.ALT_WEIGHTS)
    a0, a1 = lei.cmux_inputs(l, Bgbit)["alternating"]
    got = {}
    for i, (w0, w1) in enumerate(aei.ALT_WEIGHTS):
        q = first + 2 * i
        assert names[q] == f"alternating({w0},{w1})" and names[q + 1] == names[q] + " negated"
        assert np.array_equal(prev[q], a0[0]) and np.array_equal(prev[q + 1], a1[0])
        assert trans[q].tolist() == [q, w0, q + 1, w1] and trans[q + 1].tolist() == [q + 1, w1, q, w0]
        d = difference(trans, prev, q).view(np.int32)
        assert np.array_equal(difference(trans, prev, q + 1).view(np.int32), -d)           # no INT32_MIN among them
        got[(w0, w1)] = d
    assert aei.ALT_WEIGHTS == ((0, 0), (1, 0), (0, 1), (N, 0), (N + 1, 0), (2 * N - 1, 0), (63, 64))
    assert np.array_equal(cx._u32(got[(0, 0)]), lei.cmux_differences(l, Bgbit)["alternating"][0])
    assert set(np.unique(got[(0, 0)])) == {-1, 1}
    assert set(np.unique(got[(N, 0)])) == {-1}
    assert set(np.unique(got[(1, 0)])) == {0}                   # -INT32_MIN wraps at the turned coefficient
    for wp in ((0, 1), (2 * N - 1, 0)):
        d = got[wp]
        assert np.count_nonzero(d) == 2 and set(np.unique(d[d != 0])) <= {-2, 2}, wp
        assert [np.flatnonzero(d[c]).tolist() for c in range(2)] in ([[0], [0]], [[N - 1], [N - 1]]), wp
    # an odd turn against an even one lines equal words up: 0 but for the turned coefficients; an even against an even: +-1
    assert set(np.unique(got[(N + 1, 0)])) <= {-2, 0, 2} and set(np.unique(got[(63, 64)])) <= {-2, 0, 2}


@pytest.mark.parametrize("name", INSTANCES)
def test_every_truncation_is_closed(name):
    _, l, Bgbit = gadget(name)
    trans, prev, names = aei.edge_automaton(l, Bgbit)
    assert aei.COUNTS == (1, 2, 3, 33) and len(names) > max(aei.COUNTS) and len(names) % 2 == 0
    for count in aei.COUNTS + (len(names),):
        t, p = aei.truncated(trans, prev, count)
        assert t.shape == (count, 4) and p.shape == (count, 2, N) and p.flags.c_contiguous
        assert (t[:, [0, 2]] >= 0).all() and (t[:, [0, 2]] < count).all()
        assert np.array_equal(p, prev[:count])
        whole = count - (count & 1)
        assert np.array_equal(t[:whole], trans[:whole])
        if count & 1:
            q, w, q1, w1 = t[-1].tolist()
            assert q == q1 == count - 1 and w != w1 and w == trans[count - 1, 1]
    t, _ = aei.truncated(trans, prev, 1)
    assert t[0, 0] == t[0, 2] == 0
    # the rule for an equal pair of weights
    same = next(q for q in range(0, len(names), 2) if trans[q, 1] == trans[q, 3])
    t, _ = aei.truncated(trans, prev, same + 1)
    assert t[-1, 1] != t[-1, 3] and 0 <= t[-1, 3] < 2 * N


def test_the_sweep_meets_every_weight_on_both_branches():
    trans, prev = aei.weight_sweep()
    assert trans.shape == (2 * N, 4) and prev.shape == (2 * N, 2, N) and trans.dtype == prev.dtype == np.int32
    every = list(range(2 * N))
    for col in range(4):                                        # successors and weights: permutations on both sides
        assert sorted(trans[:, col].tolist()) == every, col
    assert (trans[:, 1] != trans[:, 3]).all()
    assert len({(a, b) for a, _, b, _ in trans.tolist()}) == 2 * N
    for w in (trans[:, 1], trans[:, 3]):                        # every lane offset and every 64-word block of the period
        assert set((w & 63).tolist()) == set(range(64)) and set((w >> 6).tolist()) == set(range(32))
    assert prev.min() < -2**30 and prev.max() > 2**30
    assert not np.array_equal(aei.weight_sweep(seed=1)[1], prev) and np.array_equal(aei.weight_sweep(seed=1)[0], trans)


@pytest.mark.parametrize("name", INSTANCES)
def test_full_scale_states_lie_in_their_binade_in_both_directions(oracle_mod, name):
    """The condition on the inputs of tests/test_gpu_automaton_instances.py's full-scale part: under the constant-K selector of
    leveled_edge_inputs.cmux_full_scale the largest value the reference converts on the digits_min and digits_max states, D
    and -D, lies in the row's interval and below 2^51.  The rotation does not move it: D is constant.
    Measured: max converted 2^50.585 on digits_min and 2^50.574 .. 2^50.584 on digits_max, 2^50.576 .. 2^50.585 on
    -digits_min and 2^50.574 .. 2^50.585 on -digits_max (<3,7>: 2^49.585 / 2^49.562 and 2^49.570 / 2^49.570);
    |reference - exact| = 1 LSB on every state."""
    cfg, l, Bgbit = gadget(name)
    op = cx.orc_params(params_of(l, Bgbit))
    trans, prev, names = aei.full_scale_states(l, Bgbit)
    assert names == ["digits_min[0]", "digits_min[0] negated", "digits_max[0]", "digits_max[0] negated"]
    assert (trans[:, [0, 2]] < 4).all() and set(trans[:, 0].tolist()) == {0, 1, 2, 3}
    D = lei.cmux_differences(l, Bgbit)
    for q, want in enumerate((D["digits_min"][0], -D["digits_min"][0].astype(np.int64), D["digits_max"][0],
                              -D["digits_max"][0].astype(np.int64))):
        assert np.array_equal(difference(trans, prev, q), cx._u32(want)), names[q]
    sel = aei.constant_selector(l, cfg["K"])
    fft = cx.to_fft(sel)
    L = ol.lib()
    for q in range(4):
        L.orc_dbg_max_conv(1)
        out = ao.step(op, trans, prev, fft, [q])[0]
        mx = L.orc_dbg_max_conv(0)
        d = difference(trans, prev, q)
        exact = cx.extprod_exact(op, sel, d).astype(np.int64) + ao.successor(prev, trans[q, 0], trans[q, 1])
        worst = int(np.abs(wrap32(out.astype(np.int64) - exact)).max())
        print(f"{name} {names[q]}: (l, Bgbit, K) = ({l}, {Bgbit}, {cfg['K']}): max converted 2^{np.log2(mx):.3f}, "
              f"reference vs exact max |diff| = {worst} LSB")
        assert cfg["lo"] <= mx < cfg["hi"] and mx < 2.0**51, (name, names[q], np.log2(mx))
        assert worst <= BOUND_EXTPROD_LSB, (name, names[q], worst)


@pytest.mark.parametrize("name", INSTANCES)
def test_reference_against_exact_on_every_edge_state(eoc, name):
    """Real selectors of 0 and of 1 on every state of edge_automaton: the step of the reference is A + its external product of
    the state's difference, that product within 8 LSB of the exact schoolbook product, every conversion inside
    the contract; on the zero pair the step returns the turned successor word for word.
    Measured max |reference - exact|: <2,10> 1, <3,7> 1, <1,0> 1, <2,0> 1, <3,0> 1, <4,0> 1 LSB."""
    _, l, Bgbit = gadget(name)
    p = params(eoc, l, Bgbit)
    op = cx.orc_params(p)
    sk = eoc.SecretKey(p, 21, with_cloud_key=False)
    sel = sk.encrypt_selector_bits([0, 1], enc_seed=5)
    fft = cx.to_fft(sel)
    trans, prev, names = aei.edge_automaton(l, Bgbit)
    L = ol.lib()
    L.orc_dbg_max_conv(1)
    worst = 0
    for q, nm in enumerate(names):
        D = difference(trans, prev, q)
        A = ao.successor(prev, trans[q, 0], trans[q, 1])
        for b in range(2):
            ref = cx.extprod(op, fft[b], D)
            d = int(np.abs(wrap32(ref.astype(np.int64) - cx.extprod_exact(op, sel[b], D))).max())
            worst = max(worst, d)
            assert d <= BOUND_EXTPROD_LSB, (name, nm, b, d)
            out = ao.step(op, trans, prev, fft[b], [q])[0]
            assert np.array_equal(out, cx._u32(A.astype(np.int64) + ref).view(np.int32)), (name, nm, b)
            if nm.startswith("zero"):
                assert np.array_equal(out, A)
    assert L.orc_dbg_max_conv(0) < 2.0**51
    print(f"{name}: {len(names)} edge states, real selectors: reference vs exact max |diff| = {worst} LSB")
