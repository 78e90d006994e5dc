"""Edge inputs for the blind-rotation kernels (numpy only; shared by tests/test_br_edge_inputs_cpu.py and
tests/test_gpu_br_instances.py).

What differs most between the kernel instances is the rotation (X^abar - 1) ACC -- a 32-way switch on abar >> 6, an in-wave
shift by abar & 63 with its borrow --, the initial X^(2N - barb) tv with its sign wrap, and the biased digit conversion at
its end values.  Random ciphertexts at small n reach a few dozen of the 2 048 rotation amounts; the rows made here reach all
of them, every one from both ends of its rounding cell.

  sweep(T)          n = 1 rows (a-word, b-word).  For every amount a on the grid of T = 2^theta (the multiples of T in
                    [0, 2N)) the smallest and the largest Torus32 word that the mod switch rounds to a: a 2^21 - 2^(20+theta)
                    and a 2^21 + 2^(20+theta) - 1 in wrapping uint32 (a = 0: the wrap of 2N to 0).  First half: abar sweeps
                    (both words of every amount), barb cycles through EDGE_AMOUNTS; second half: barb sweeps, abar cycles.
                    Both words of the 2N / T amounts make 2 x 2N / T rows per half: 8 192 rows in all for T = 1, 4 096 for
                    T = 2, 1 024 for T = 8; every amount occurs at least twice as abar and at least twice as barb.
  sweep_subset(T)   row indices of a fixed half of sweep(T) that still holds every abar and every barb of the grid (even
                    amounts by their smallest word, odd ones by their largest).
  two_step_rows(T)  n = 2 rows (a0-word, a1-word, b-word), 256 of them: (abar0, abar1) over the borrow edges abar & 63 in
                    {0, T, 64 - 2T, 64 - T} crossed with the switch cases abar >> 6 in {0, 15, 16, 31}, so that the second
                    step decomposes a full accumulator in both polynomials.
  extreme_polys(l, Bgbit)  test polynomials: all zero; alternating INT32_MIN / INT32_MAX; the constants c whose image
                    (X^N - 1) c = -2c decomposes to all digits -Bg/2, and to all digits Bg/2 - 1.
"""
import numpy as np

N = 1024
EDGE_AMOUNTS = (0, 1, 63, 64, 1023, 1024, 1025, 2047)
SWITCH_CASES = (0, 15, 16, 31)


def _theta(n_tables):
    theta = int(n_tables).bit_length() - 1
    assert 1 << theta == n_tables and 0 <= theta <= 3
    return theta


def cell_words(a, n_tables=1):
    """(smallest, largest) Torus32 word (as int32 arrays) of the rounding cell of amount a, a multiple of T in [0, 2N)"""
    theta = _theta(n_tables)
    a = np.asarray(a, np.int64)
    assert ((a >= 0) & (a < 2 * N) & (a % n_tables == 0)).all()
    half = 1 << (20 + theta)
    lo = ((a << 21) - half) & 0xFFFFFFFF
    hi = ((a << 21) + half - 1) & 0xFFFFFFFF
    return lo.astype(np.uint32).view(np.int32), hi.astype(np.uint32).view(np.int32)


def grid(n_tables=1):
    return np.arange(0, 2 * N, n_tables, dtype=np.int64)


def edge_amounts(n_tables=1):
    """EDGE_AMOUNTS moved onto the grid of T (the neighbours 1, 63, 1023, 1025, 2047 become +-T): for T = 1 the set itself"""
    T = int(n_tables)
    return np.array([0, T, 64 - T, 64, 1024 - T, 1024, 1024 + T, 2 * N - T], np.int64)


def sweep(n_tables=1):
    """int32 [2 x 2 x 2N / T][2]: see the module docstring.  Returns (rows, abar, barb), the amounts the rows are built for."""
    g = grid(n_tables)
    swept = np.repeat(g, 2)                                   # amount a at rows 2k (smallest word) and 2k + 1 (largest)
    which = np.arange(swept.size) & 1
    edges = edge_amounts(n_tables)
    cyc = edges[(np.arange(swept.size) // 2 + np.arange(swept.size)) % len(edges)]   # both words of an amount meet different edges
    cyc_which = (np.arange(swept.size) // 16) & 1             # ... and every edge amount arrives by both of its words

    def words(a, w):
        lo, hi = cell_words(a, n_tables)
        return np.where(w == 0, lo, hi)

    first = np.stack([words(swept, which), words(cyc, cyc_which)], axis=1)
    second = np.stack([words(cyc, cyc_which), words(swept, which)], axis=1)
    rows = np.ascontiguousarray(np.concatenate([first, second]).astype(np.int32))
    abar = np.concatenate([swept, cyc])
    barb = np.concatenate([cyc, swept])
    return rows, abar, barb


def sweep_subset(n_tables=1):
    """indices into sweep(T): of every swept amount one word (even multiples of T the smallest, odd ones the largest), in
    both halves: every abar and every barb of the grid, half the rows"""
    m = 2 * N // int(n_tables)
    k = np.arange(m)
    half = 2 * k + (k & 1)
    return np.concatenate([half, 2 * m + half])


def two_step_rows(n_tables=1):
    """int32 [256][3] and the amounts (abar0, abar1, barb) they are built for"""
    T = int(n_tables)
    lows = (0, T, 64 - 2 * T, 64 - T)
    amounts = np.array([(q << 6) | s for q in SWITCH_CASES for s in lows], np.int64)        # 16 amounts
    a0, a1 = [x.ravel() for x in np.meshgrid(amounts, amounts, indexing="ij")]
    k = np.arange(a0.size)
    edges = edge_amounts(n_tables)
    b = edges[(k + k // 16) % len(edges)]

    def words(a, w):
        lo, hi = cell_words(a, n_tables)
        return np.where(w == 0, lo, hi)

    rows = np.stack([words(a0, k & 1), words(a1, (k >> 1) & 1), words(b, (k >> 2) & 1)], axis=1)
    return np.ascontiguousarray(rows.astype(np.int32)), a0, a1, b


# -- the gadget decomposition, restated (oracle/tfhe_oracle.c: decomp_offset, decomp_digit) ---------------------------------
def decomp_offset(l, Bgbit):
    return sum((1 << (Bgbit - 1)) << (32 - p * Bgbit) for p in range(1, l + 1)) & 0xFFFFFFFF


def decomp_digits(x, l, Bgbit):
    """digits [l][...] of the Torus32 words x: ((x + offset) >> (32 - p Bgbit)) mod Bg - Bg/2, p = 1 .. l"""
    u = (np.asarray(x, np.int64) + decomp_offset(l, Bgbit)) & 0xFFFFFFFF
    Bg = 1 << Bgbit
    return np.stack([((u >> (32 - p * Bgbit)) & (Bg - 1)) - (Bg >> 1) for p in range(1, l + 1)])


def extreme_digit_constants(l, Bgbit):
    """(c_min, c_max) as Python ints in int32 range: -2 c_min decomposes to all digits -Bg/2 (x + offset = 0 on the l Bgbit
    decomposed bits), -2 c_max to all digits Bg/2 - 1 (x + offset = all ones there).  With l Bgbit = 32 the lowest
    decomposed bit is bit 0, which the even word -2c cannot set: the last digit of c_max's image is Bg/2 - 2 there."""
    assert l * Bgbit <= 32
    off = decomp_offset(l, Bgbit)
    low = max(2, 1 << (32 - l * Bgbit))                             # weight of the lowest decomposed bit an even word reaches
    x_min = (0 - off) & 0xFFFFFFFF                                  # x + off = 0
    x_max = ((1 << 32) - low - off) & 0xFFFFFFFF                    # x + off = 2^32 - low: every decomposed bit set
    out = []
    for x in (x_min, x_max):
        assert x % 2 == 0
        c = ((0 - x) & 0xFFFFFFFF) // 2                             # -2c = x (mod 2^32)
        assert (-2 * c) & 0xFFFFFFFF == x
        out.append(c - (1 << 32) if c >= 1 << 31 else c)
    top = np.full(l, (1 << (Bgbit - 1)) - 1)
    top[-1] -= l * Bgbit == 32
    assert (decomp_digits((-2 * out[0]) & 0xFFFFFFFF, l, Bgbit) == -(1 << (Bgbit - 1))).all()
    assert np.array_equal(decomp_digits((-2 * out[1]) & 0xFFFFFFFF, l, Bgbit), top)
    return out[0], out[1]


def extreme_polys(l, Bgbit):
    """dict name -> int32 [N]"""
    c_min, c_max = extreme_digit_constants(l, Bgbit)
    alt = np.where(np.arange(N) & 1, 2**31 - 1, -2**31).astype(np.int32)
    return dict(zero=np.zeros(N, np.int32), alternating=alt,
                digits_min=np.full(N, c_min, np.int64).astype(np.int32), digits_max=np.full(N, c_max, np.int64).astype(np.int32))


# -- full-scale operands inside the step loop (crafted bootstrapping key) ---------------------------------------------------
# The conversion contract (include/eoc_tfhe_gpu.h): the kernels' two-operation conversion is Torus32(int64(v)) for
# |v| < 2^51.  An external-product coefficient is bounded by 2 l N (Bg/2) 2^31 = l Bg 2^41, so the contract holds for ANY
# input when l Bg < 1024; above that it is a condition on the inputs, which these rows meet by construction and the tests
# assert on the oracle's recorded maximum.
# With every bootstrapping-key word equal to K, a constant test polynomial c and abar = N, the first step decomposes -2c in
# every coefficient of ACC_1 (ACC_0 = 0) and its product is l N d |K| at coefficient N - 1, d the digit magnitude (all N
# terms of the negacyclic product of two constant polynomials align there): l Bg 2^40 |K| / 2^31 for d = Bg/2.  The second
# step decomposes a full accumulator in both polynomials; with these keys it stays below the first (measured).
# (l, Bgbit, K, [lo, hi)): the run-time-base shapes take a gadget base large enough for [2^50, 2^51), the top binade of the
# contract, with K = -1.5 x 2^e placing the maximum at 1.5 x 2^50.  Two shapes cannot get there with ANY int32 key and a
# constant K, and ask for the top binade they do reach at 1.5 x 2^(hi - 1):
#   <3,7>  is Set B's compile-time base: l Bg 2^40 = 1.5 x 2^48 with K = -2^31;
#   <4,0>  has l Bgbit <= 32, so Bgbit <= 8: l Bg 2^40 = 2^50 exactly at K = -2^31, the closed end of [2^49, 2^50].
FULL_SCALE = {
    "pair<3,7>": dict(l=3, Bgbit=7, K=-2**31, lo=2.0**48, hi=2.0**49),
    "pair<4,0>": dict(l=4, Bgbit=8, K=-3 * 2**29, lo=2.0**49, hi=2.0**50),
    "pair<1,0>": dict(l=1, Bgbit=11, K=-3 * 2**29, lo=2.0**50, hi=2.0**51),
    "lds<2,0>": dict(l=2, Bgbit=11, K=-3 * 2**28, lo=2.0**50, hi=2.0**51),
    "wide<0>": dict(l=2, Bgbit=11, K=-3 * 2**28, lo=2.0**50, hi=2.0**51),
}
FULL_SCALE_ABARS = (1024, 1, 2047)


def full_scale_rows():
    """n = 2 rows (a0-word, a1-word, b-word): (abar0, abar1) over FULL_SCALE_ABARS squared, barb = 0; centre words"""
    a = np.array([(x, y, 0) for x in FULL_SCALE_ABARS for y in FULL_SCALE_ABARS], np.int64)
    return np.ascontiguousarray(((a << 21) & 0xFFFFFFFF).astype(np.uint32).view(np.int32))
