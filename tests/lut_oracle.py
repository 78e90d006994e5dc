"""Programmable bootstrapping composed from the CPU oracle's pieces (oracle/tfhe_oracle.h): the byte-for-byte reference of
eoc_lut_batch_device.  orc_modswitch_sample, ACC = (0, X^(2N - barb) tv), orc_blind_rotate_step for every non-zero
rotation amount, tLweExtractLweSample (index 0), orc_keyswitch.  Test-side only."""
import ctypes as C

import numpy as np

N = 1024


def rotate(poly, a):
    """X^a * poly in Z[X]/(X^N + 1), a in [0, 2N) (the oracle's rot_coef, coefficient by coefficient)"""
    idx = (np.arange(N) - a) & (2 * N - 1)
    v = np.asarray(poly, np.int64)[idx & (N - 1)]
    return np.where(idx & N, -v, v).astype(np.int64).astype(np.uint32).view(np.int32)


def int_table(f, p, p_out):
    """Torus32 output values of f: Z_p -> Z_p_out in the integer encoding (f(m) mod p_out at phase . / (2 p_out))"""
    return np.array([((int(f(m)) % p_out) << 32) // (2 * p_out) for m in range(p)], np.uint64).astype(np.uint32).view(np.int32)


def bootstrap(orc, tv, t):
    """KeySwitch(BlindRotate(t, tv)) on the oracle: t [n+1] -> [n+1]"""
    L, p = orc.L, orc.p
    n = orc.n
    bara = np.zeros(n, np.int32)
    barb = np.zeros(1, np.int32)
    L.orc_modswitch_sample(C.byref(p), np.ascontiguousarray(t, np.int32), bara, barb)
    acc = np.zeros(2 * N, np.int32)
    acc[N:] = rotate(tv, (2 * N - int(barb[0])) & (2 * N - 1))
    step = orc.kpl * 2 * N
    base = orc.bkfft.ctypes.data
    for i in range(n):
        if bara[i]:
            L.orc_blind_rotate_step(C.byref(p), C.c_void_p(base + i * step * 8), None, int(bara[i]), acc, 1)
    u = np.zeros(N + 1, np.int32)
    u[0] = acc[0]
    u[1:N] = (0 - acc[N - np.arange(1, N)].astype(np.int64)).astype(np.uint32).view(np.int32)  # -ACC_0[N - j]
    u[N] = acc[N]
    return orc.keyswitch(u)


def lut_batch(orc, tvs, cts):
    """[n_luts][count][n+1]: every test polynomial of `tvs` on every row of `cts`"""
    cts = np.asarray(cts, np.int32).reshape(-1, orc.n + 1)
    return np.stack([np.stack([bootstrap(orc, tv, c) for c in cts]) for tv in np.asarray(tvs).reshape(-1, N)])
