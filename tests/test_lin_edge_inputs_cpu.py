"""The inputs of tests/lin_edge_inputs.py do what they claim (no GPU): every target word is an extreme word of its rounding
cell, the solved operands give exactly the target row through the oracle's own linear stage, the wrap and top-bit quotas
hold, and the gate of the solved operands equals the reference composed from the target row alone -- which is what lets
tests/test_gpu_linear_stage_paths.py share one reference between all opcodes and code paths."""
import numpy as np
import pytest

import br_edge_inputs as bei
import lin_edge_inputs as lei
import lut_many_oracle as lmo
import oracle_lib as ol

N = 1024
MU = 1 << 29
ALL_OPS = lei.TWO_INPUT + (lei.OP_MAJ, lei.OP_XOR3)


def is_even_op(op):
    return op in lei.DOUBLING


@pytest.mark.parametrize("T", [1, 2, 4, 8])
@pytest.mark.parametrize("n,rows", [(260, 35), (1, 32)])
def test_every_target_word_is_an_extreme_word_of_its_cell(T, n, rows):
    L = ol.lib()
    for even in (False, True):
        t, amount, end = lei.target_cells(n, rows, even, 11 + T, n_tables=T)
        assert t.dtype == np.int32 and t.shape == (rows, n + 1)
        assert np.array_equal(lmo.modswitch_coarse(t, T), amount)
        step = 2 if even else 1
        out = lei.wrap32(t.astype(np.int64) + np.where(end == 0, -step, step))
        moved = lmo.modswitch_coarse(out, T)
        assert (moved != amount).all()                       # one step outwards rounds elsewhere ...
        assert np.array_equal(moved, (amount + np.where(end == 0, -T, T)) % (2 * N))      # ... into the adjacent cell
        inward = lei.wrap32(t.astype(np.int64) - np.where(end == 0, -step, step))
        assert np.array_equal(lmo.modswitch_coarse(inward, T), amount)
        if even:
            assert (t & 1 == 0).all()
        if T == 1:                                            # the oracle's own rounding, word by word
            flat, o = t.ravel(), out.ravel()
            for k in range(0, flat.size, 7):
                assert L.orc_modswitch_from_torus32(int(flat[k]), 2 * N) == amount.ravel()[k]
                assert L.orc_modswitch_from_torus32(int(o[k]), 2 * N) != amount.ravel()[k]
        # both ends of every edge amount, in the mask words and in word n
        want = {(int(a), e) for a in bei.edge_amounts(T) for e in (0, 1)}
        assert {(int(a), int(e)) for a, e in zip(amount[:, :n].ravel(), end[:, :n].ravel())} == want
        assert {(int(a), int(e)) for a, e in zip(amount[:, n], end[:, n])} == want


def test_solved_operands_give_the_target_row_and_meet_the_quotas():
    orc = ol.Oracle(0, 3, n_override=260, with_bk=False)
    for op in ALL_OPS:
        t = lei.targets(260, 35, is_even_op(op), 21)
        rows = lei.solve(op, t, 100 + op)
        assert all(x.dtype == np.int32 and x.shape == t.shape for x in rows)
        assert np.array_equal(lei.linear(op, rows), t), op
        if op in lei.TWO_INPUT:
            for r in range(t.shape[0]):
                assert np.array_equal(orc.gate_linear(op, rows[0][r], rows[1][r]), t[r]), (op, r)
        share = lei.wrapped(lei.exact_sum(op, rows)).mean()
        print(f"op {op}: {100 * share:.1f} % of the words wrap")
        assert share >= 0.25, (op, share)
        free = rows[0].astype(np.int64)                       # drawn over the whole range: both signs, large magnitudes
        assert (free < -2**30).any() and (free > 2**30).any()
        if op in lei.DOUBLING:                                # the top bit the factor 2 drops: both values, every row
            top = rows[-1] < 0
            assert 0.4 < top.mean() < 0.6 and top.any(axis=1).all() and (~top).any(axis=1).all()
            flipped = lei.wrap32(rows[-1].astype(np.int64) ^ (1 << 31))
            assert np.array_equal(lei.linear(op, rows[:-1] + (flipped,)), t)


def test_mux_operands_share_one_selector():
    orc = ol.Oracle(0, 3, n_override=260, with_bk=False)
    t1, t2 = lei.targets(260, 35, False, 21), lei.targets(260, 35, False, 23)
    assert (t1 != t2).any(axis=1).all()
    a, b, c = lei.solve(lei.OP_MUX, t1, 110, t2)
    for r in range(35):
        assert np.array_equal(orc.gate_linear(1, a[r], b[r]), t1[r])
        assert np.array_equal(orc.gate_linear(6, a[r], c[r]), t2[r])
    either = lei.wrapped(lei.exact_sum(1, (a, b))) | lei.wrapped(lei.exact_sum(6, (a, c)))
    print(f"MUX: {100 * either.mean():.1f} % of the words wrap in one of the two stages")
    assert either.mean() >= 0.25


_ORC = {}


def small_oracle():
    if "o" not in _ORC:
        _ORC["o"] = ol.Oracle(0, 83, n_override=260, with_bk=False)
        _ORC["o"].gen_cloud()
    return _ORC["o"]


def raw_reference(orc, t):
    return np.stack([orc.keyswitch(orc.blind_rotate_extract(r)) for r in t])


def test_gate_of_the_solved_operands_is_the_reference_of_the_target_row():
    """four rows per opcode at n = 260: orc.gate_batch == keyswitch(blind_rotate_extract(t*)), and MUX == the key switch of
    the two extracted samples' sum plus (0, mu)"""
    orc = small_oracle()
    tt = {even: lei.targets(260, 35, even, 31 + even)[:4] for even in (False, True)}
    ref = {even: raw_reference(orc, t) for even, t in tt.items()}
    for op in ALL_OPS:
        even = is_even_op(op)
        rows = lei.solve(op, tt[even], 200 + op)
        got = orc.gate_batch(op, *rows)
        assert np.array_equal(got, ref[even]), op
    t2 = lei.targets(260, 35, False, 37)[:4]
    a, b, c = lei.solve(lei.OP_MUX, tt[False], 210, t2)
    want = []
    for r in range(4):
        u = orc.blind_rotate_extract(tt[False][r]).astype(np.int64) + orc.blind_rotate_extract(t2[r])
        u[N] += MU
        want.append(orc.keyswitch(lei.wrap32(u)))
    assert np.array_equal(orc.gate_batch(lei.OP_MUX, a, b, c), np.stack(want))


def test_the_other_opcodes_round_the_same_operands_elsewhere():
    """what tells an OP_MULTI row's opcode from any other: the same operands through another opcode's table change at least
    one rotation amount, in every row"""
    for op in lei.TWO_INPUT:
        t = lei.targets(260, 35, is_even_op(op), 41)
        rows = lei.solve(op, t, 300 + op)
        bar = lmo.modswitch_coarse(t)
        for other in lei.TWO_INPUT:
            if other != op:
                assert (lmo.modswitch_coarse(lei.linear(other, rows)) != bar).any(axis=1).all(), (op, other)


@pytest.mark.parametrize("theta", [0, 1, 2, 3])
@pytest.mark.parametrize("terms", [1, 2, 3, 4])
def test_node_solver_agrees_with_the_numpy_restatement(theta, terms):
    """as tests/test_int_circuit_cpu.py::test_linear_stage_and_coarse_modswitch_in_numpy: uint32 arithmetic of the solved
    operands gives t*, its rounding is the target amount, and the exact sum wraps"""
    T = 1 << theta
    seen_w, seen_c = set(), set()
    for k in range(5):
        t, amount, _ = lei.target_cells(260, 35, False, 50 + k, n_tables=T)
        w = lei.node_weights(terms, 7 * theta + k)
        cst = lei.node_cst(k, 60 + k)
        xs = lei.solve_node(w, cst, t, 70 + k)
        assert len(xs) == terms and abs(w[-1]) == 1 and all(v in lei.NODE_WEIGHTS for v in w[:-1])
        seen_w.update(w[:-1])
        seen_c.add(k % 4)
        acc = np.zeros(t.shape, np.uint32)
        for j in range(terms):
            acc = acc + np.uint32(w[j] & 0xFFFFFFFF) * xs[j].view(np.uint32)
        acc[:, -1] += np.uint32(cst & 0xFFFFFFFF)
        assert np.array_equal(acc.view(np.int32), t) and np.array_equal(lei.node_linear(w, cst, xs), t)
        bara = (((acc + np.uint32(1 << (20 + theta))) >> np.uint32(21 + theta)) << np.uint32(theta)) & np.uint32(2047)
        assert np.array_equal(bara.astype(np.int64), amount)
        exact = lei.node_exact(w, cst, xs)
        assert np.array_equal(lmo.modswitch_coarse((exact & 0xFFFFFFFF).astype(np.int64), T), amount)
        if terms > 1:
            assert np.mean((exact < lei.INT32_MIN) | (exact > lei.INT32_MAX)) >= 0.25
    if terms > 1:
        assert seen_w == set(lei.NODE_WEIGHTS)
    assert seen_c == {0, 1, 2, 3}


def test_free_gate_rows_hold_the_special_words():
    rows = lei.free_gate_rows()
    assert rows.shape == (35, 261) and rows.dtype == np.int32
    for col in (0, 259, 260):
        assert {0, -1, 1, lei.INT32_MIN, lei.INT32_MAX} <= set(rows[:, col].tolist())
    special = np.isin(rows, [0, -1, 1, lei.INT32_MIN, lei.INT32_MAX])
    assert 0.5 < special.mean() < 0.75
