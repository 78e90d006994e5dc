"""Reference of eoc_tv_pack_exact_device (include/eoc_tfhe_gpu.h) in plain numpy integers: the rule as the
header states it -- p + 1 samples (the p values and value 0 negated), their key switch to constant-slot samples against the
packing key's int32 rows, and the negacyclic window sums -- every step in int64 reduced mod 2^32.  No transform, no chunk:
this is the exact value of the rule whose FFT evaluation pack_oracle.pack_list is.  Test-side only."""
import numpy as np

import pack_oracle as po

N = 1024


def _wrap(x):
    return (np.asarray(x, np.int64) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)


def windows(p):
    """[(lo, hi)] of Win_s = X^lo + .. + X^(hi-1), s = 0 .. p"""
    h, w = N // (2 * p), N // p
    return [(0, h)] + [(s * w - h, s * w + h) for s in range(1, p)] + [(N - h, N)]


def samples(vals):
    """[..][p][n+1] -> [..][p + 1][n+1]: u_s = v_s, u_p = v_0 negated word by word"""
    vals = np.asarray(vals, np.int32)
    neg = _wrap(0 - vals[..., :1, :].astype(np.int64))
    return np.concatenate([vals, neg], axis=-2)


def const_slot(n, rows, u):
    """S [M][2][N] int32 of samples u [M][n+1]: (0, b X^0) - sum_m sum_j d_(m,j) Row(m, j), rows [n][4][2][N]"""
    u = np.asarray(u, np.int32).reshape(-1, n + 1)
    d = po.digits(u[:, :n])                                             # [4][M][n]
    A = d.transpose(1, 2, 0).reshape(u.shape[0], n * 4)                 # K order (m, j): the rows' own order
    R = np.asarray(rows, np.int32).astype(np.int64).reshape(n * 4, 2 * N)
    # the integer product through two float64 products of 16-bit halves (numpy multiplies int64 matrices without BLAS):
    # every sum is an integer below 4 n 8 2^16 < 2^53, so both are exact; tests/test_lut_tree_cpu.py holds the result
    # against int64 schoolbook products (pack_oracle.pack_list_exact)
    assert 4 * n * 8 * 65536 < 2**53
    Af = A.astype(np.float64)
    lo, hi = (Af @ (R & 0xFFFF).astype(np.float64)).astype(np.int64), (Af @ (R >> 16).astype(np.float64)).astype(np.int64)
    S = -(lo + (hi << 16))
    S[:, N] += u[:, n].astype(np.int64)
    return _wrap(S).reshape(-1, 2, N)


def spread(S, p):
    """list [2][N] int32 = sum_s Win_s(X) S_s (negacyclic), S [p + 1][2][N]"""
    S = np.asarray(S, np.int32).astype(np.int64)
    k = np.arange(N)
    out = np.zeros((2, N), np.int64)
    for s, (lo, hi) in enumerate(windows(p)):
        E = np.cumsum(np.concatenate([-S[s], S[s]], axis=1), axis=1)    # E[:, t + N] = sum_(u = -N .. t) S~[u]
        out += E[:, k - lo + N] - E[:, k - hi + N]
    return _wrap(out)


def tv_pack_exact(n, rows, vals, p):
    """eoc_tv_pack_exact_device: vals [n_funcs][p][count][n+1] -> lists [n_funcs][count][2][N]"""
    vals = np.asarray(vals, np.int32)
    F, _, C, _ = vals.shape
    u = samples(vals.transpose(0, 2, 1, 3))                             # [F][C][p + 1][n+1]
    S = const_slot(n, rows, u).reshape(F * C, p + 1, 2, N)
    return np.stack([spread(x, p) for x in S]).reshape(F, C, 2, N)
