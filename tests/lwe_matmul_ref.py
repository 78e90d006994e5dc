"""Reference of the public int8 matrix on LWE samples (include/eoc_tfhe_lwe.h): four lines of numpy in int64,
which holds 2^16 * 127 * 2^32 without overflow; the inputs the tests share (random words mixed with limb-edge words, random
weights mixed with +-127, +-1 and 0); and both limb rules restated in numpy.  Test-side only."""
import numpy as np

MASK = 0xFFFFFFFF
FLIP = 0x80808080
EDGE_WORDS = np.array([0, 1, -1, 2**31, 2**31 - 1, 0x7F, 0x80, 0x7F80, 0x8000, 0x807F807F, 0x80808080, 0x7F7F7F7F],
                      np.int64).astype(np.uint32).view(np.int32)
EDGE_WEIGHTS = np.array([127, -127, 1, -1, 0], np.int8)


def lwe_matmul(w, cts, bias=None):
    """w [rows][cols] int8, cts [batch][cols][width] int32, bias [rows] int32 or None -> [batch][rows][width] int32"""
    w, cts = np.asarray(w), np.asarray(cts, np.int32)
    out = (w.astype(np.int64) @ cts.view(np.uint32).astype(np.int64)) & MASK
    if bias is not None:
        out[..., -1] = (out[..., -1] + np.asarray(bias, np.int32).astype(np.int64)) & MASK     # the body is the last word
    return out.astype(np.uint32).view(np.int32)


def words(rng, shape):
    """random words, every third one a limb-edge word"""
    v = rng.integers(-2**31, 2**31, shape).astype(np.int32)
    v.reshape(-1)[::3] = np.resize(EDGE_WORDS, v.reshape(-1)[::3].size)
    return v


def weights(rng, rows, cols):
    """random weights in [-127, 127], every fourth one of +-127, +-1, 0"""
    w = rng.integers(-127, 128, (rows, cols)).astype(np.int8)
    w.reshape(-1)[::4] = np.resize(EDGE_WEIGHTS, w.reshape(-1)[::4].size)
    return w


def image_bytes(rows, cols):
    """the documented size of the weight image: fragments [ceil(rows / 32)][ceil(cols / 32)][64][16 B], then 32 ceil(rows /
    32) int32 corrections; 0 for a refused shape"""
    if not (1 <= rows <= 2**20 and 1 <= cols <= 2**16):
        return 0
    rt, ks = -(-rows // 32), -(-cols // 32)
    return rt * (1024 * ks + 128)


# ---- the limb rules: v == sum_j limb_j 2^(8 j) + constant (mod 2^32), every limb a signed byte --------------------------------
def limbs_carry(v):
    """the carry rule of the key-switch limb image: l = ((v + 128) & 255) - 128, v <- (v - l) >> 8; constant 0"""
    v = np.asarray(v, np.int32).astype(np.int64)
    out = []
    for _ in range(4):
        l = ((v + 128) & 255) - 128
        v = (((v - l) & MASK) ^ 0x80000000) - 0x80000000 >> 8      # wrapped to int32, then the arithmetic shift
        out.append(l)
    return np.stack(out), 0


def limbs_carry_free(v):
    """the kernel's rule: t_j = the signed byte j of v ^ 0x80808080; constant 0x80808080"""
    u = np.asarray(v, np.int32).view(np.uint32).astype(np.int64) ^ FLIP
    t = np.stack([(u >> (8 * j)) & 255 for j in range(4)])
    return np.where(t >= 128, t - 256, t), FLIP


def lwe_matmul_by_limbs(w, cts, rule):
    """the kernel's arithmetic: four int8 products with int32 accumulators (asserted), recombined with shifts, plus the
    constant times the row sums of the weights"""
    w = np.asarray(w).astype(np.int64)
    limbs, const = rule(cts)
    assert limbs.min() >= -128 and limbs.max() <= 127
    acc = [w @ l for l in limbs]
    assert all(np.abs(a).max() < 2**31 for a in acc)
    out = sum(a << (8 * j) for j, a in enumerate(acc)) + const * w.sum(1)[:, None]
    return (out & MASK).astype(np.uint32).view(np.int32)
