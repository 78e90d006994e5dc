"""The edge inputs of tests/br_edge_inputs.py do what they claim (no GPU): the sweeps reach every rotation amount from both
ends of its rounding cell, the two-step rows reach the borrow edges and switch cases, the extreme-digit constants decompose
to the end digits, and the crafted keys of the full-scale case put the oracle's conversions where the table says.  The
device side is tests/test_gpu_br_instances.py."""
import ctypes as C

import numpy as np
import pytest

import br_edge_inputs as bei
import lut_many_oracle as lmo
import lut_oracle as lo
import oracle_lib as ol

N = 1024
# (l, Bgbit) of every shape of the instance matrix (tests/test_gpu_br_instances.py) and of the full-scale case
MATRIX_SHAPES = [(2, 10), (2, 8), (3, 7), (3, 6), (1, 9), (4, 6)]
ALL_SHAPES = sorted(set(MATRIX_SHAPES) | {(c["l"], c["Bgbit"]) for c in bei.FULL_SCALE.values()})


def oracle_modswitch(rows):
    """orc_modswitch_sample on rows [..][n+1] -> int32 [..][n+1] (barb last)"""
    rows = np.ascontiguousarray(rows, np.int32)
    p = ol.OrcParams()
    L = ol.lib()
    assert L.orc_default_params(0, C.byref(p)) == 0
    p.n = rows.shape[1] - 1
    out = np.zeros_like(rows)
    barb = np.zeros(1, np.int32)
    for r, o in zip(rows, out):
        L.orc_modswitch_sample(C.byref(p), r, o[: p.n], barb)
        o[p.n] = barb[0]
    return out


def modswitch(rows, T):
    got = lmo.modswitch_coarse(rows, T)
    if T == 1:
        assert np.array_equal(got, oracle_modswitch(rows))          # the numpy restatement IS the oracle's at T = 1
    return got


@pytest.mark.parametrize("T", [1, 2, 8])
def test_sweep_reaches_every_amount_from_both_ends_of_its_cell(oracle_mod, T):
    rows, abar, barb = bei.sweep(T)
    assert rows.shape == (8 * N // T, 2) and rows.dtype == np.int32
    bar = modswitch(rows, T)
    assert np.array_equal(bar[:, 0], abar) and np.array_equal(bar[:, 1], barb)
    g = bei.grid(T)
    for col in (0, 1):
        amounts, counts = np.unique(bar[:, col], return_counts=True)
        assert np.array_equal(amounts, g) and counts.min() >= 2, (T, col)
    half = rows.shape[0] // 2
    assert np.array_equal(np.unique(bar[:half, 0]), g) and np.array_equal(np.unique(bar[half:, 1]), g)
    assert set(np.unique(bar[:half, 1])) == set(bei.edge_amounts(T)) == set(np.unique(bar[half:, 0]))
    if T == 1:
        assert tuple(sorted(bei.edge_amounts(1))) == tuple(sorted(bei.EDGE_AMOUNTS))
        pairs = {(int(a) >> 6, int(a) & 63) for a in bar[:, 0]}
        assert pairs == {(q, s) for q in range(32) for s in range(64)}
    # every word is the extreme word of its cell: one step outwards rounds elsewhere, and both extremes of every swept
    # amount are present (row 2k its smallest word, row 2k + 1 its largest)
    w = rows.astype(np.int64)
    which = np.arange(half) & 1
    for col, sl in ((0, slice(0, half)), (1, slice(half, None))):
        words, want = w[sl, col], bar[sl, col]
        out = np.where(which == 0, words - 1, words + 1)
        inw = np.where(which == 0, words + 1, words - 1)
        probe = np.zeros((half, 2), np.int64)
        probe[:, 0] = out
        step = (want + np.where(which == 0, -T, T)) % (2 * N)
        assert np.array_equal(modswitch(probe.astype(np.uint32).view(np.int32).reshape(half, 2), T)[:, 0], step)
        probe[:, 0] = inw
        assert np.array_equal(modswitch(probe.astype(np.uint32).view(np.int32).reshape(half, 2), T)[:, 0], want)
    # the cycling column arrives by extreme words too
    lo_w, hi_w = bei.cell_words(bar[:half, 1], T)
    assert ((rows[:half, 1] == lo_w) | (rows[:half, 1] == hi_w)).all()
    for e in bei.edge_amounts(T):
        sel = bar[:half, 1] == e
        assert (rows[:half, 1][sel] == lo_w[sel]).any() and (rows[:half, 1][sel] == hi_w[sel]).any(), e
    # the wrap of 2N to 0: amount 0's smallest word is the largest words of the torus
    assert rows[0, 0] == -(1 << (20 + T.bit_length() - 1)) and bar[0, 0] == 0


@pytest.mark.parametrize("T", [1, 2, 8])
def test_sweep_subset_keeps_every_abar_and_every_barb(oracle_mod, T):
    rows, abar, barb = bei.sweep(T)
    idx = bei.sweep_subset(T)
    assert idx.size == rows.shape[0] // 2 and np.unique(idx).size == idx.size and (T > 1 or idx.size >= 2048)
    g = bei.grid(T)
    assert np.array_equal(np.unique(abar[idx]), g) and np.array_equal(np.unique(barb[idx]), g)
    # both kinds of word stay in
    lo_w, hi_w = bei.cell_words(abar[idx], T)
    assert (rows[idx, 0] == lo_w).sum() >= idx.size // 4 and (rows[idx, 0] == hi_w).sum() >= idx.size // 4


@pytest.mark.parametrize("T", [1, 2, 8])
def test_two_step_rows_cross_borrow_edges_with_switch_cases(oracle_mod, T):
    rows, a0, a1, b = bei.two_step_rows(T)
    assert rows.shape == (256, 3)
    bar = modswitch(rows, T)
    assert np.array_equal(bar, np.stack([a0, a1, b], axis=1))
    lows = {0, T, 64 - 2 * T, 64 - T}
    if T == 1:
        assert lows == {0, 1, 62, 63}
    want = {(q << 6) | s for q in bei.SWITCH_CASES for s in lows}
    assert len(want) == 16
    assert {(int(x), int(y)) for x, y in bar[:, :2]} == {(x, y) for x in want for y in want}
    assert (bar[:, 0] != 0).sum() >= 240 and (bar[:, 1] != 0).sum() >= 240      # two real steps almost everywhere
    assert set(bar[:, 2]) == set(bei.edge_amounts(T))


@pytest.mark.parametrize("l,Bgbit", ALL_SHAPES)
def test_extreme_digit_constants_decompose_to_the_end_digits(l, Bgbit):
    Bg = 1 << Bgbit
    polys = bei.extreme_polys(l, Bgbit)
    img_min = (-2 * polys["digits_min"].astype(np.int64)) & 0xFFFFFFFF         # (X^N - 1) c = -2c
    img_max = (-2 * polys["digits_max"].astype(np.int64)) & 0xFFFFFFFF
    d_min, d_max = bei.decomp_digits(img_min, l, Bgbit), bei.decomp_digits(img_max, l, Bgbit)
    assert d_min.shape == (l, N) and (d_min == -Bg // 2).all()
    if l * Bgbit < 32:
        assert (d_max == Bg // 2 - 1).all()
    else:                                                                      # bit 0 is decomposed: -2c cannot set it
        assert (d_max[:-1] == Bg // 2 - 1).all() and (d_max[-1] == Bg // 2 - 2).all()
    # decomp_digits is the gadget decomposition: the digits recompose to the word with its bits below the lowest
    # decomposed weight dropped (the offset carries no rounding term: tGswTorus32PolynomialDecompH truncates)
    x = np.random.default_rng(l * 100 + Bgbit).integers(0, 2**32, 4096)
    x[:4] = [0, 2**32 - 1, 2**31, 2**31 - 1]
    d = bei.decomp_digits(x, l, Bgbit)
    assert d.min() >= -Bg // 2 and d.max() <= Bg // 2 - 1
    rec = sum(d[p - 1] << (32 - p * Bgbit) for p in range(1, l + 1))
    err = ((rec - x + 2**31) % 2**32) - 2**31
    assert np.array_equal(-err, x & ((1 << (32 - l * Bgbit)) - 1))
    assert polys["alternating"][0] == -2**31 and polys["alternating"][1] == 2**31 - 1 and not polys["zero"].any()


# -- full-scale operands inside the step loop ----------------------------------------------------------------------------
def full_scale_oracle(name, seed=61):
    """the oracle of FULL_SCALE[name] at n = 2: a real key-switch key, every bootstrapping-key word K"""
    cfg = bei.FULL_SCALE[name]
    orc = ol.Oracle(0, seed, n_override=2, with_bk=False)
    orc.p.l, orc.p.Bgbit = cfg["l"], cfg["Bgbit"]
    orc.l, orc.kpl = cfg["l"], 2 * cfg["l"]
    orc.gen_cloud()
    orc.bk[:] = cfg["K"]
    orc.L.orc_bk_to_fft(C.byref(orc.p), orc.bk, orc.bkfft)
    return orc, cfg


@pytest.mark.parametrize("name", list(bei.FULL_SCALE))
def test_full_scale_inputs_lie_in_their_binade_and_fft_matches_exact(oracle_mod, name):
    """The condition on the inputs of test_gpu_br_instances.py::test_full_scale_operands_in_the_step_loop: with the crafted
    key the largest value the oracle's inverse transform converts over the whole case lies in the shape's interval of
    br_edge_inputs.FULL_SCALE -- [2^50, 2^51), the top binade of the conversion contract, for the run-time-base shapes;
    <3,7> and <4,0> cannot reach it (reasons there) and sit at 1.5 x 2^48 and 1.5 x 2^49.

    And the FFT path against the exact one at that scale: every step of every row runs from the same accumulator through
    orc_blind_rotate_step with use_fft = 1 and with use_fft = 0 (schoolbook, mod 2^32).  Measured max |difference| per
    output word, in LSB of the Torus32 word (deterministic; x86-64, gcc -O2 -ffp-contract=off):
        pair<3,7> 1    pair<4,0> 1    pair<1,0> 1    lds<2,0> 1    wide<0> 1
    asserted at twice that; the margin only covers libm / compiler differences between machines."""
    orc, cfg = full_scale_oracle(name)
    polys = bei.extreme_polys(cfg["l"], cfg["Bgbit"])
    rows = bei.full_scale_rows()
    bar = oracle_modswitch(rows)
    assert {tuple(r) for r in bar[:, :2]} == {(x, y) for x in bei.FULL_SCALE_ABARS for y in bei.FULL_SCALE_ABARS}
    L, p = orc.L, orc.p
    step = orc.kpl * 2 * N
    worst = 0
    L.orc_dbg_max_conv(1)
    for tv in (polys["digits_min"], polys["digits_max"]):
        for r in bar:
            acc = np.zeros(2 * N, np.int32)
            acc[N:] = lo.rotate(tv, (2 * N - int(r[2])) & (2 * N - 1))
            for i in range(2):
                exact = acc.copy()
                L.orc_blind_rotate_step(C.byref(p), C.c_void_p(orc.bkfft.ctypes.data + i * step * 8), None, int(r[i]), acc, 1)
                L.orc_blind_rotate_step(C.byref(p), None, C.c_void_p(orc.bk.ctypes.data + i * step * 4), int(r[i]), exact, 0)
                d = (acc.astype(np.int64) - exact.astype(np.int64) + 2**31) % 2**32 - 2**31
                worst = max(worst, int(np.abs(d).max()))
    mx = L.orc_dbg_max_conv(0)
    print(f"{name}: (l, Bgbit, K) = ({cfg['l']}, {cfg['Bgbit']}, {cfg['K']}): max converted 2^{np.log2(mx):.3f}, "
          f"FFT vs exact max |diff| = {worst} LSB")
    assert cfg["lo"] <= mx < cfg["hi"], (name, np.log2(mx))
    assert mx < 2.0**51                                                        # the conversion contract itself
    assert worst <= 2 * MEASURED_FFT_VS_EXACT_LSB[name], (name, worst)


MEASURED_FFT_VS_EXACT_LSB = {"pair<3,7>": 1, "pair<4,0>": 1, "pair<1,0>": 1, "lds<2,0>": 1, "wide<0>": 1}
