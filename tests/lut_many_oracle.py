"""Many-LUT bootstrapping composed from the CPU oracle's pieces (oracle/tfhe_oracle.h), as tests/lut_oracle.py does for one
table: the byte-for-byte reference of eoc_lut_many_batch_device.  The mod switch rounded to the grid of T (restated here in
numpy; T = 1 is orc_modswitch_sample), ACC = (0, X^(2N - barb) tv), orc_blind_rotate_step for every non-zero rotation
amount, sample extraction at indices 0 .. T - 1, orc_keyswitch of each.  Test-side only."""
import ctypes as C

import numpy as np

from lut_oracle import N, rotate


def modswitch_coarse(t, n_tables=1):
    """every word of the samples `t` [..][n+1] -> a multiple of T = n_tables in [0, 2N): round(t 2N / 2^32) on the T-grid,
    ((t + 2^(20 + theta)) >> (21 + theta)) << theta with T = 2^theta.  Returns int32 [..][n+1] (barb last)."""
    theta = int(n_tables).bit_length() - 1
    assert 1 << theta == n_tables
    u = np.asarray(t, np.int64) & 0xFFFFFFFF
    return ((((u + (1 << (20 + theta))) & 0xFFFFFFFF) >> (21 + theta)) << theta).astype(np.int32) & (2 * N - 1)


def extract(acc, j):
    """tLweExtractLweSampleIndex at j: u_i = ACC_0[j - i] (i <= j), -ACC_0[N + j - i] (i > j); b = ACC_1[j]"""
    a = acc[:N].astype(np.int64)
    ext = np.concatenate([a, -a])                                         # the signed 2N-periodic image
    u = np.zeros(N + 1, np.int32)
    u[:N] = (ext[(2 * N + j - np.arange(N)) & (2 * N - 1)] & 0xFFFFFFFF).astype(np.uint32).view(np.int32)
    u[N] = acc[N + j]
    return u


def bootstrap_many(orc, tv, t, n_tables):
    """the T key-switched samples [T][n+1] of one blind rotation of the packed polynomial `tv` on sample t"""
    L, p = orc.L, orc.p
    n = orc.n
    bar = modswitch_coarse(t, n_tables)
    bara, barb = bar[:n], int(bar[n])
    acc = np.zeros(2 * N, np.int32)
    acc[N:] = rotate(tv, (2 * N - barb) & (2 * N - 1))
    step = orc.kpl * 2 * N
    base = orc.bkfft.ctypes.data
    for i in range(n):
        if bara[i]:
            L.orc_blind_rotate_step(C.byref(p), C.c_void_p(base + i * step * 8), None, int(bara[i]), acc, 1)
    return np.stack([orc.keyswitch(extract(acc, j)) for j in range(n_tables)])


def lut_many_batch(orc, tvs, cts, n_tables):
    """[n_luts][T][count][n+1]: every packed polynomial of `tvs` on every row of `cts`"""
    cts = np.asarray(cts, np.int32).reshape(-1, orc.n + 1)
    per = [np.stack([bootstrap_many(orc, tv, c, n_tables) for c in cts]) for tv in np.asarray(tvs).reshape(-1, N)]
    return np.stack(per).transpose(0, 2, 1, 3)                            # [g][row][j] -> [g][j][row]
