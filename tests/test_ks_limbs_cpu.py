"""The arithmetic behind k_keyswitch_mfma (kernels.hip.h), restated in numpy and held against the oracle's lweKeySwitch:
split every key word into four signed byte limbs, multiply the one-hot digit matrix of the operand by each limb plane with
int32 accumulators, recombine `b - sum_k (acc_k << 8k)` in wrapping 32-bit arithmetic.  No GPU: the device side is
tests/test_gpu_ks_mfma.py."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as ol

N = 1024
T, BASEBIT = 8, 2


def limbs_of(words):
    """l_k = ((v_k + 128) & 255) - 128, v_{k+1} = (v_k - l_k) >> 8: four planes of int8, v == sum l_k 2^(8k) (mod 2^32)"""
    v = np.asarray(words, np.int32).astype(np.int64)
    out = []
    for _ in range(4):
        l = ((v + 128) & 255) - 128
        out.append(l.astype(np.int8))
        v = (v - l) >> 8
        v = ((v + 2**31) % 2**32) - 2**31          # the device keeps v in an int32 register
    return out


def limb_planes(ksk, n):
    """[4][N t 4][n + 1] int8 in the kernel's K order k = (i t + j) 4 + d, the d = 0 slot all zero"""
    rows = np.asarray(ksk, np.int32).reshape(N * T, 3, n + 1)
    planes = np.zeros((4, N * T, 4, n + 1), np.int8)
    for k, l in enumerate(limbs_of(rows)):
        planes[k, :, 1:, :] = l
    return planes.reshape(4, N * T * 4, n + 1)


def one_hot(u):
    """[rows][N t 4] int8: the digit d of (i, j) of ubar = u + 2^(31 - t basebit) sets slot (i t + j) 4 + d"""
    a = np.asarray(u, np.int32)[:, :N].astype(np.int64) & 0xFFFFFFFF
    ubar = (a + (1 << (32 - (1 + BASEBIT * T)))) & 0xFFFFFFFF
    j = np.arange(T)
    dig = (ubar[:, :, None] >> (30 - 2 * j)[None, None, :]) & 3          # [rows][N][t]
    oh = np.zeros((a.shape[0], N * T, 4), np.int8)
    r, g = np.meshgrid(np.arange(a.shape[0]), np.arange(N * T), indexing="ij")
    oh[r, g, dig.reshape(a.shape[0], N * T)] = 1
    return oh.reshape(a.shape[0], N * T * 4), dig


def keyswitch_by_limbs(planes, u, n):
    oh, _ = one_hot(u)
    out = np.zeros((u.shape[0], n + 1), np.int64)
    for k in range(4):
        acc = oh.astype(np.int32) @ planes[k].astype(np.int32)
        assert np.abs(acc).max() <= 1 << 20                  # <= N t terms of magnitude <= 128: no int32 overflow
        out += acc.astype(np.int64) << (8 * k)
    out = -out
    out[:, n] += np.asarray(u, np.int32)[:, N].astype(np.int64)
    return (((out + 2**31) % 2**32) - 2**31).astype(np.int32)


def edge_operands(rng, rows):
    u = rng.integers(-2**31, 2**31, (rows, N + 1)).astype(np.int32)
    u[0, :N] = 0                 # every digit 0: nothing is subtracted
    u[1, :N] = -65536            # ubar = 0xFFFF8000: every digit 3 (the accumulator bound)
    u[2, :N] = -32769            # ubar = 0xFFFFFFFF
    u[3, :N] = 32767             # one below the rounding offset's carry
    u[4, :N] = -2**31
    u[5, :N] = 2**31 - 1
    return u


def test_limbs_recombine_on_edge_words():
    w = np.array([0, 1, -1, 127, 128, -128, -129, 255, 256, 0x7FFFFFFF, -2**31, 0x7FFFFF80, 0x7FFFFF7F, -2**31 + 127,
                  0x00800000, 0x007FFFFF, -0x00800000, -0x00800001, 32767, 32768, -32768, -32769], np.int64).astype(np.int32)
    w = np.concatenate([w, np.random.default_rng(1).integers(-2**31, 2**31, 100000).astype(np.int32)])
    ls = limbs_of(w)
    assert all(l.dtype == np.int8 for l in ls)
    tot = sum(l.astype(np.int64) << (8 * k) for k, l in enumerate(ls))
    assert np.array_equal((tot - w.astype(np.int64)) % 2**32, np.zeros(len(w), np.int64))


def test_one_hot_product_equals_the_wrapping_row_sum_on_a_synthetic_key_with_edge_words():
    n = 40
    rng = np.random.default_rng(3)
    ksk = rng.integers(-2**31, 2**31, (N * T * 3, n + 1)).astype(np.int32)
    ksk[::7, ::3] = 0x7FFFFFFF
    ksk[1::7, 1::3] = -2**31
    ksk[2::7, 2::3] = 0x7FFFFF80
    ksk[3::7, ::5] = -129
    u = edge_operands(rng, 9)
    _, dig = one_hot(u)
    rows = ksk.reshape(N * T, 3, n + 1).astype(np.int64)
    want = np.zeros((u.shape[0], n + 1), np.int64)
    want[:, n] = u[:, N]
    for c in range(u.shape[0]):
        d = dig[c].reshape(N * T)
        nz = d > 0
        want[c] -= rows[np.nonzero(nz)[0], d[nz] - 1].sum(axis=0)
    want = (((want + 2**31) % 2**32) - 2**31).astype(np.int32)
    assert np.array_equal(keyswitch_by_limbs(limb_planes(ksk, n), u, n), want)


@pytest.mark.parametrize("pset", [0, 1], ids=["setA", "setB"])
def test_limb_product_equals_the_oracle_key_switch(oracle_mod, pset):
    orc = ol.Oracle(pset, 5, with_bk=False)
    p = orc.p
    assert (p.ks_t, p.ks_basebit) == (T, BASEBIT)
    orc.ksk = np.zeros((N * T * 3, p.n + 1), np.int32)
    orc.L.orc_keygen_ksk(C.byref(p), orc.seed, orc.lwe_key, orc.tlwe_key, orc.ksk)
    u = edge_operands(np.random.default_rng(11 + pset), 10)
    got = keyswitch_by_limbs(limb_planes(orc.ksk, p.n), u, p.n)
    want = np.stack([orc.keyswitch(x) for x in u])
    assert np.array_equal(got, want)
    assert not want[0, :p.n].any() and want[0, p.n] == u[0, N]          # all-zero digits: (0, ..., 0, b)
