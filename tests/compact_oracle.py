"""Restatement of compact public-key encryption (include/eoc_tfhe_gpu.h) on the oracle's streams: the public
key (stream tag 6), compact lists (tag 7), slot extraction and the expansion through orc_keyswitch.  Test-side only."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import oracle_lib as ol

N = 1024
TAG_PUBLIC_KEY, TAG_COMPACT_ENC = 6, 7


def _rotsum(ones, P):
    """u * P in Z_2^32[X]/(X^N + 1) for binary u with ones at `ones` (int64, not reduced)"""
    P = np.asarray(P, np.int64)
    acc = np.zeros(N, np.int64)
    for m in ones:
        acc += np.concatenate((-P[N - m:], P[:N - m]))
    return acc


def _u32(x):
    return (np.asarray(x, np.int64) & 0xFFFFFFFF).astype(np.uint32)


def _gauss(L, key, ctr0, bk_stdev):
    return np.array([L.orc_gaussian32(key, ctr0 + 2 * j, 0, bk_stdev) for j in range(N)], np.int64)


def public_key(seed, tlwe_key, bk_stdev):
    """(A, B) uint32 [N] of the reproducible secret key `seed`"""
    L = ol.lib()
    key = L.orc_stream_key(seed, TAG_PUBLIC_KEY, 0)
    A = np.array([L.orc_rng_u64(key, j) >> 32 for j in range(N)], np.int64)
    e = _gauss(L, key, N, bk_stdev)
    B = e + _rotsum(np.flatnonzero(np.asarray(tlwe_key)), A)
    return _u32(A), _u32(B)


def encrypt(A, B, enc_seed, first_list, msgs, bk_stdev):
    """lists [L][2][N] int32 of Torus32 messages `msgs` (slots past the end encrypt 0)"""
    L = ol.lib()
    msgs = np.asarray(msgs, np.int64)
    n_lists = -(-len(msgs) // N)
    out = np.zeros((n_lists, 2, N), np.uint32)
    for li in range(n_lists):
        key = L.orc_stream_key(enc_seed, TAG_COMPACT_ENC, first_list + li)
        ones = [i for i in range(N) if L.orc_rng_u64(key, i) >> 63]
        M = np.zeros(N, np.int64)
        part = msgs[li * N:(li + 1) * N]
        M[:len(part)] = part
        out[li, 0] = _u32(_gauss(L, key, N, bk_stdev) + _rotsum(ones, A))
        out[li, 1] = _u32(_gauss(L, key, 3 * N, bk_stdev) + _rotsum(ones, B) + M)
    return out.view(np.int32)


def bit_msgs(bits):
    return np.where(np.asarray(bits) != 0, 1 << 29, -(1 << 29)).astype(np.int64)


def int_msgs(values, p):
    return (np.asarray(values, np.int64) << 32) // (2 * p)


def extract(lists, idx):
    """LWE samples [len(idx)][N+1] under s' of samples idx (slot s mod N of list s / N): a'_i = c0[j - i] (i <= j),
    -c0[N + j - i] (i > j), b' = c1[j]"""
    lists = np.asarray(lists, np.int64).reshape(-1, 2, N)
    idx = np.asarray(idx, np.int64)
    j = idx % N
    i = np.arange(N)[None, :]
    c0 = lists[idx // N, 0]
    a = np.take_along_axis(c0, (j[:, None] - i) % N, 1)
    a = np.where(i <= j[:, None], a, -a)
    out = np.empty((len(idx), N + 1), np.int64)
    out[:, :N] = a
    out[:, N] = lists[idx // N, 1, j]
    return _u32(out).view(np.int32)


def phases(lists, idx, tlwe_key, chunk=2048):
    """phases (int64, wrapped to [-2^31, 2^31)) of the extracted samples under s'"""
    s1 = np.asarray(tlwe_key, np.int64)
    idx = np.asarray(idx, np.int64)
    out = np.empty(len(idx), np.int64)
    for lo in range(0, len(idx), chunk):
        x = extract(lists, idx[lo:lo + chunk]).astype(np.int64)
        out[lo:lo + chunk] = x[:, N] - x[:, :N] @ s1
    return ((out + 2**31) % 2**32) - 2**31


def ksk(orc):
    """the oracle's key-switch key for orc's secret key (without generating the bootstrapping key)"""
    if orc.ksk is None:
        p = orc.p
        orc.ksk = np.zeros((N * p.ks_t * ((1 << p.ks_basebit) - 1), p.n + 1), np.int32)
        orc.L.orc_keygen_ksk(ol.C.byref(p), orc.seed, orc.lwe_key, orc.tlwe_key, orc.ksk)
    return orc.ksk


def expand(orc, lists, idx, threads=16):
    """[len(idx)][n+1]: orc_keyswitch of every extracted sample (ctypes releases the GIL: a thread pool runs them side by
    side)"""
    k = ksk(orc)
    u = extract(lists, idx)
    out = np.zeros((len(idx), orc.n + 1), np.int32)

    def one(r):
        orc.L.orc_keyswitch(ol.C.byref(orc.p), k, np.ascontiguousarray(u[r]), out[r])
    with ThreadPoolExecutor(threads) as ex:
        list(ex.map(one, range(len(idx))))
    return out
