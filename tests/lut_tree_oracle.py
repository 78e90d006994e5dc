"""d-digit table lookups composed from the references that exist: level 1 is lut2_oracle.level1 (the `_tv` /
many-LUT path), every pack tv_pack_exact_oracle.tv_pack_exact, every further level lut2_oracle.lut_enc_batch with one list
per job; and the Python twin of eoc_lut_tree_test_polynomials.  Test-side only."""
import numpy as np

import lut2_oracle as l2
import tv_pack_exact_oracle as tpe

N = 1024


def torus_table(F, p, d, p_out=None):
    """Torus32 output values [p]^d of F: Z_p^d -> Z_p_out in the integer encoding, table[x_1]..[x_d]"""
    p_out = p if p_out is None else p_out
    t = np.zeros((p,) * d, np.uint64)
    for idx in np.ndindex(*t.shape):
        t[idx] = ((int(F(*idx)) % p_out) << 32) // (2 * p_out)
    return t.astype(np.uint32).view(np.int32)


def test_polynomials(eoc, p, d, table, T=1):
    """the twin: level-1 table J = j_2 + p j_3 + p^2 j_4 (j_2 fastest) is x_1 -> table[x_1][j_2]..[j_d]; polynomial g holds the
    tables J = g T .. g T + T - 1 as lut_test_polynomial (T = 1) / lut_many_test_polynomial lay them out"""
    table = np.asarray(table, np.int32).reshape((p,) * d)
    cols = []
    for J in range(p ** (d - 1)):
        js = tuple((J // p ** k) % p for k in range(d - 1))            # (j_2, .., j_d)
        cols.append(table[(slice(None),) + js])
    cols = np.stack(cols)                                               # [p^(d-1)][p]
    if T == 1:
        return np.stack([eoc.lut_test_polynomial(p, c) for c in cols])
    return np.stack([eoc.lut_many_test_polynomial(p, cols[g:g + T]) for g in range(0, len(cols), T)])


def lut_tree_batch(orc, pk_rows, p, d, T, tv0, digits, parts=False):
    """eoc_lut_tree_batch_device: tv0 [n_funcs][p^(d-1) / T][N], digits [d][count][n+1] -> [n_funcs][count][n+1];
    parts: also the list of every pack's lists"""
    n = orc.n
    digits = np.asarray(digits, np.int32).reshape(d, -1, n + 1)
    S = digits.shape[1]
    tv0 = np.asarray(tv0, np.int32).reshape(-1, p ** (d - 1) // T, N)
    n_funcs = tv0.shape[0]
    vals = l2.level1(orc, p, T, tv0.reshape(-1, p // T, N), digits[0])  # [n_funcs p^(d-2)][p][S][n+1]
    packs = []
    for k in range(1, d):
        lists = tpe.tv_pack_exact(n, pk_rows, vals, p)                  # [groups][S][2][N]
        packs.append(lists)
        out = l2.lut_enc_batch(orc, lists, digits[k], True)             # [groups][S][n+1]
        if k + 1 < d:
            vals = out.reshape(-1, p, S, n + 1)
    out = out.reshape(n_funcs, S, n + 1)
    return (out, packs) if parts else out
