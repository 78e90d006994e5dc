"""Edge inputs for the leveled kernels -- k_cmux, k_pack_gather, k_pack_rows, k_tvpack_cols (numpy only; shared by
tests/test_leveled_edge_inputs_cpu.py, tests/test_gpu_cmux_instances.py and tests/test_gpu_pack_edges.py).

A CMux decomposes BOTH polynomials of an arbitrary difference in1 - in0, and the packing key switch the mask words of
arbitrary samples; random words meet neither a rounding-cell end nor an all-end-digits word, and the top binade of the
conversion contract (|v| < 2^51, include/eoc_tfhe_gpu.h) needs a crafted key.  The rows made here do.

  cmux_differences(l, Bgbit)  named TLWE differences [k][2][N] uint32: zero, digits_min, digits_max, cells, deltas,
                              alternating (the difference the alternating INPUTS of cmux_inputs have).  Also what
                              k_demux decomposes as x itself (tests/test_gpu_demux_instances.py) and what the states of
                              tests/automaton_edge_inputs.py put under k_automaton_step through its two rotations.
  cmux_inputs(l, Bgbit)       name -> (in0, in1) int32 [k][2][N] with in1 - in0 the named difference: in0 random full-range
                              words (so that the final + A wraps too), except `alternating`: INT32_MIN / INT32_MAX words in
                              opposite phase, where the subtraction itself wraps.
  cmux_full_scale             per k_cmux instance (l, Bgbit, K, [lo, hi)): a selector of one constant word K on digits_min /
                              digits_max converts values in [lo, hi).
  constant_selector(l, K)     that selector in torus form, [2l][2][N] int32.
  pack_mask_words()           named mask words for the rounding base-16 decomposition of the packing key switch.
  pack_samples(n, count)      LWE samples [count][n+1]: every mask column cycles through pack_mask_words, b random.
  pack_shapes, pack_counts    the n and the sample counts at which the packing kernels take another path.
  PACK_FULL_SCALE             a packing key of one constant word at n = 16 and the all-digits -8 batch: [2^49, 2^50).
  tv_values(n, p, rows)       values [2][p][rows][n+1] for eoc_tv_pack_device with INT32_MIN / INT32_MAX / 0 / -1 words.
"""
import numpy as np

from br_edge_inputs import decomp_digits, decomp_offset  # noqa: F401  (re-used, not restated: the tests reach both here)

N = 1024
DELTA_POSITIONS = (0, 63, 64, 511, 512, 1023)


def _i32(x):
    return (np.asarray(x, np.int64) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)


# -- k_cmux ------------------------------------------------------------------------------------------------------------------
def cell_end_words(l, Bgbit):
    """uint32 [2 l Bg]: for every digit position p = 1 .. l and every value k of that digit's field the two words x with
    x + offset = k 2^(32 - p Bgbit) and that minus 1 -- the first word of a cell of position p and the last word of the cell
    below it (every lower decomposed and every truncated bit set; k = 0 borrows from the digit above, at p = 1 around the
    torus).  Order: [p][k][first, last-of-the-cell-below]."""
    off = decomp_offset(l, Bgbit)
    out = []
    for p in range(1, l + 1):
        k = np.arange(1 << Bgbit, dtype=np.int64) << (32 - p * Bgbit)
        out.append(np.stack([k - off, k - 1 - off], axis=1).ravel())
    return (np.concatenate(out) & 0xFFFFFFFF).astype(np.uint32)


def cmux_differences(l, Bgbit):
    """dict name -> uint32 [k][2][N]"""
    assert l * Bgbit <= 32
    off = decomp_offset(l, Bgbit)
    w_min = (0 - off) & 0xFFFFFFFF                                  # x + offset = 0: every digit -Bg/2
    w_max = ((1 << 32) - 1 - off) & 0xFFFFFFFF                      # x + offset = 2^32 - 1: every digit Bg/2 - 1, every
    words = cell_end_words(l, Bgbit)                                # truncated bit set (a difference may be odd)
    k = -(-words.size // N)
    chunks = np.resize(words, (k, N))                               # the last sample starts over at the first words
    cells = np.stack([chunks, chunks[:, ::-1]], axis=1)             # every word in both polynomials, at mirrored coefficients
    deltas = np.zeros((2 * len(DELTA_POSITIONS), 2, N), np.uint32)
    for q in range(2):
        for i, j in enumerate(DELTA_POSITIONS):
            deltas[q * len(DELTA_POSITIONS) + i, q, j] = w_min
    odd = (np.arange(N) & 1).astype(bool)
    alt = np.where(odd, 1, 0xFFFFFFFF).astype(np.uint32)            # INT32_MAX - INT32_MIN = -1, INT32_MIN - INT32_MAX = 1
    return dict(zero=np.zeros((1, 2, N), np.uint32), digits_min=np.full((1, 2, N), w_min, np.uint32),
                digits_max=np.full((1, 2, N), w_max, np.uint32), cells=np.ascontiguousarray(cells), deltas=deltas,
                alternating=np.ascontiguousarray(np.broadcast_to(alt, (1, 2, N))))


def cmux_inputs(l, Bgbit, seed=0):
    """dict name -> (in0, in1), int32 [k][2][N] each, in1 - in0 = cmux_differences(l, Bgbit)[name] in wrapping arithmetic"""
    rng = np.random.default_rng(1000 * l + Bgbit + seed)
    out = {}
    for name, D in cmux_differences(l, Bgbit).items():
        if name == "alternating":
            odd = (np.arange(N) & 1).astype(bool)
            in0 = np.broadcast_to(np.where(odd, 2**31 - 1, -2**31), D.shape).astype(np.int64)
            in1 = np.broadcast_to(np.where(odd, -2**31, 2**31 - 1), D.shape).astype(np.int64)
        else:
            in0 = rng.integers(-2**31, 2**31, D.shape)
            in1 = in0 + D.astype(np.int64)
        out[name] = (np.ascontiguousarray(_i32(in0)), np.ascontiguousarray(_i32(in1)))
    return out


# The conversion contract (include/eoc_tfhe_gpu.h): the kernels convert like Torus32(int64(v)) for |v| < 2^51.  A CMux
# decomposes both polynomials of its difference, so a coefficient of its external product is bounded by 2 l N (Bg/2) 2^31 =
# l Bg 2^41 -- twice the blind rotation's full-scale case (ACC_0 = 0 there, br_edge_inputs.FULL_SCALE).  With every selector
# word equal to K and a constant difference of digit magnitude d in both polynomials, all 2 l N terms align at coefficient
# N - 1: 2 l N d |K|.  K = -1.5 x 2^e puts d = Bg/2 at 1.5 x 2^50, the middle of the contract's top binade [2^50, 2^51), for
# every instance but <3,7>, whose compile-time base reaches 2 l N (Bg/2) 2^31 = 1.5 x 2^49 with the largest int32 magnitude
# and asks for that binade.  (1, 11) at K = -3 x 2^29 and (2, 11) at -3 x 2^28 reach 1.5 x 2^51, OUTSIDE the contract: the
# table holds half of each.  tests/test_leveled_edge_inputs_cpu.py confirms every row on the reference's recorded maximum.
cmux_full_scale = {
    "k_cmux<2,10>": dict(l=2, Bgbit=10, K=-3 * 2**28, lo=2.0**50, hi=2.0**51),
    "k_cmux<3,7>": dict(l=3, Bgbit=7, K=-2**31, lo=2.0**49, hi=2.0**50),
    "k_cmux<1,0>": dict(l=1, Bgbit=11, K=-3 * 2**28, lo=2.0**50, hi=2.0**51),
    "k_cmux<2,0>": dict(l=2, Bgbit=11, K=-3 * 2**27, lo=2.0**50, hi=2.0**51),
    "k_cmux<3,0>": dict(l=3, Bgbit=8, K=-2**31, lo=2.0**50, hi=2.0**51),
    "k_cmux<4,0>": dict(l=4, Bgbit=8, K=-3 * 2**29, lo=2.0**50, hi=2.0**51),
}


def constant_selector(l, K):
    """a selector whose 2l x 2 x N words all equal K, torus form"""
    return np.full((2 * l, 2, N), K, np.int64).astype(np.int32)


# -- the packing key switch --------------------------------------------------------------------------------------------------
PACK_T, PACK_BASEBIT, PACK_CHUNK = 4, 4, 16
PACK_OFFSET = (1 << 15) + 0x88880000          # the rounding term 2^(31 - 16) and DecompH's offset sum_p 8 2^(32 - 4p)
pack_shapes = (1, 16, 17, 63, 64)             # n: a short chunk only; exactly one full chunk; a full chunk and a chunk of one
                                              # index; n + 1 = 64 (one column tile) and 65 (b alone in the second tile)


# sample counts: one slot; both sides of the 64-sample tile; both sides of a full list; three lists with one slot in the last
# (at n = 17: 3 lists x 2 chunks = 6 items, no multiple of the 4 waves of a k_pack_rows workgroup)
pack_counts = (1, 63, 64, 65, N - 1, N + 1, 2 * N + 1)


def pack_mask_words():
    """dict name -> mask word (Python int in [0, 2^32)).  The digits are those of a + PACK_OFFSET, four signed base-16
    digits of its upper 16 bits: a rounds to the nearest multiple of 2^16, low half 0x8000 upwards."""
    w = {
        "digits_min": (0 - PACK_OFFSET) & 0xFFFFFFFF,               # a + offset = 0: all four digits -8
        "digits_max": (0xFFFFFFFF - PACK_OFFSET) & 0xFFFFFFFF,      # a + offset = 2^32 - 1: all four digits 7; low half 0x7FFF
        "carry_out": 0xFFFF8000,                                    # the rounding term carries out of bit 31
        "zero": 0, "int32_min": 0x80000000, "int32_max": 0x7FFFFFFF,
    }
    for t in range(16):
        w[f"top{t}_down"] = (t << 28) | 0x7FFF                      # the largest low half that rounds down
        w[f"top{t}_up"] = (t << 28) | 0x8000                        # the smallest that rounds up: a carry into bit 16
        if t < 15:                                                  # ... that runs through three digits into the top one
            w[f"top{t}_ripple"] = (t << 28) | 0x0FFF8000            # (t = 15: carry_out)
    return w


def pack_samples(n, count, seed=0):
    """int32 [count][n+1]: mask column m of sample i holds word (i + 7 m) mod W of pack_mask_words (W = 53 words, 7 coprime
    to it: every column meets every word within any 53 consecutive samples, at slots that differ from column to column, and
    a sample's columns hold different words); the b column is random"""
    words = np.array(list(pack_mask_words().values()), np.int64)
    i, m = np.arange(count)[:, None], np.arange(n)[None, :]
    out = np.zeros((count, n + 1), np.int64)
    out[:, :n] = words[(i + 7 * m) % words.size]
    out[:, n] = np.random.default_rng(n * 100003 + count + seed).integers(-2**31, 2**31, count)
    return np.ascontiguousarray(_i32(out))


# A chunk of 16 key indices converts at most 64 rows x 8 x N x 2^31 = 2^50.  With every key word K, all N
# samples' mask words at all digits -8 and n = 16 (one full chunk) the 64 x N terms align at coefficient N - 1:
# 2^19 |K|.  K = -2^31 gives 2^50 exactly, the CLOSED end of the documented bound; K = -3 x 2^29 gives 1.5 x 2^49, the middle
# of the highest binade the operation reaches below it.
PACK_FULL_SCALE = dict(n=16, K=-3 * 2**29, lo=2.0**49, hi=2.0**50)


def pack_full_scale_samples():
    """int32 [N][17]: every mask word at all digits -8, b = 0"""
    out = np.full((N, PACK_FULL_SCALE["n"] + 1), pack_mask_words()["digits_min"], np.int64)
    out[:, -1] = 0
    return np.ascontiguousarray(_i32(out))


def constant_packing_blob(blob, K):
    """a copy of the EOCPKS1 blob `blob` (uint8 array: 52-byte header, then the rows as int32) with every row word K"""
    out = np.array(blob, np.uint8, copy=True)
    out[52:].view(np.int32)[:] = K
    return out


# -- k_tvpack_cols -----------------------------------------------------------------------------------------------------------
TV_WORDS = (-2**31, 2**31 - 1, 0, -1)          # INT32_MIN is its own negation, INT32_MAX + 1 wraps, -0 = 0, -(-1) = 1
TV_SHAPES = (63, 64)                           # n + 1 = 64: b is the last column of the only tile; 65: alone in the second
TV_ROWS = (1, 3)


def tv_values(n, p, rows, seed=0):
    """int32 [2][p][rows][n+1] (two functions): random words with TV_WORDS laid over mask and b columns -- sample 0 of every
    (function, row), the one k_tvpack_cols negates in its last window, has them at columns 0 .. 3, at the last mask columns
    and (one per (function, row), cycling) as its b word; the other samples carry them at shifted columns"""
    rng = np.random.default_rng(7000 + 100 * n + 10 * p + rows + seed)
    v = rng.integers(-2**31, 2**31, (2, p, rows, n + 1))
    for f in range(2):
        for j in range(p):
            for s in range(rows):
                k = f * rows + s + j
                for t, w in enumerate(TV_WORDS):
                    v[f, j, s, (j + t) % n] = w
                    v[f, j, s, n - 1 - ((j + t) % n)] = TV_WORDS[(t + 1) % 4]
                v[f, j, s, n] = TV_WORDS[k % 4]
    return np.ascontiguousarray(_i32(v))

