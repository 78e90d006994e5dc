"""Reference of the packing key switch (include/eoc_tfhe_gpu.h) on the oracle: the packing key's rows restated
on the oracle's streams (tag 9), the chunked operation through tests/c/pack_ref.c (compiled here with gcc -ffp-contract=off
against liboracle.so), the digits and the exact wrapping-integer evaluation in numpy.  Test-side only."""
import atexit
import ctypes as C
import os
import shutil
import subprocess
import tempfile
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import compact_oracle as co
import oracle_lib as ol

N = 1024
TAG_PACK_KSK = 9
PACK_T, PACK_BASEBIT, PACK_CHUNK = 4, 4, 16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_lib = None


def lib():
    global _lib
    if _lib is None:
        so_oracle = ol.build_oracle()
        tmp = tempfile.mkdtemp(prefix="pack_ref_")
        atexit.register(shutil.rmtree, tmp, ignore_errors=True)
        so = os.path.join(tmp, "libpack_ref.so")
        subprocess.check_call(["gcc", "-std=c11", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-shared", "-fPIC",
                               "-I" + ol.ORACLE_DIR, os.path.join(ROOT, "tests", "c", "pack_ref.c"), "-o", so, so_oracle,
                               "-Wl,-rpath," + ol.ORACLE_DIR, "-lm"])
        ol.lib()                                            # liboracle.so first: the reference resolves against it
        L = C.CDLL(so)
        i32p = np.ctypeslib.ndpointer(np.int32, flags="C")
        f64p = np.ctypeslib.ndpointer(np.float64, flags="C")
        L.pack_ref_key_fft.argtypes = [i32p, C.c_size_t, f64p]
        L.pack_ref_key_fft.restype = None
        L.pack_ref_list.argtypes = [C.c_int, f64p, i32p, C.c_int, C.c_int, C.c_int, i32p]
        L.pack_ref_list.restype = None
        _lib = L
    return _lib


def _u32(x):
    return (np.asarray(x, np.int64) & 0xFFFFFFFF).astype(np.uint32)


def n_chunks(n):
    return (int(n) + PACK_CHUNK - 1) // PACK_CHUNK


def key_row(seed, lwe_key, tlwe_key, bk_stdev, m, j):
    """Row (m, j), j = 1 .. 4, of the reproducible secret key `seed`: [2][N] int32"""
    L = ol.lib()
    key = L.orc_stream_key(seed, TAG_PACK_KSK, m * PACK_T + (j - 1))
    a = np.array([L.orc_rng_u64(key, k) >> 32 for k in range(N)], np.int64)
    e = np.array([L.orc_gaussian32(key, N + 2 * k, 0, bk_stdev) for k in range(N)], np.int64)
    b = e + co._rotsum(np.flatnonzero(np.asarray(tlwe_key)), a)
    if lwe_key[m]:
        b[0] += 1 << (32 - PACK_BASEBIT * j)
    return np.stack([_u32(a), _u32(b)]).view(np.int32)


def blob_rows(blob, n):
    """the rows [n][4][2][N] int32 of an EOCPKS1 blob (header: magic 8 | params 36 | t, basebit 8)"""
    return np.frombuffer(bytes(blob[52:]), np.int32).reshape(n, PACK_T, 2, N)


def key_fft(rows):
    """[n][4][2][N] int32 -> [n][4][2][N] float64, orc_fft_fwd of every polynomial (unscaled)"""
    rows = np.ascontiguousarray(rows, np.int32)
    out = np.zeros(rows.shape, np.float64)
    lib().pack_ref_key_fft(rows.reshape(-1), rows.size // N, out.reshape(-1))
    return out


def digits(a):
    """the four signed base-16 digits of mask words `a` (any shape) -> [4][...] int64 in [-8, 8): a rounding decomposition"""
    off = (1 << (31 - PACK_T * PACK_BASEBIT)) + sum(8 << (32 - PACK_BASEBIT * p) for p in range(1, PACK_T + 1))
    x = (_u32(a).astype(np.int64) + off) & 0xFFFFFFFF
    return np.stack([((x >> (32 - PACK_BASEBIT * j)) & 15) - 8 for j in range(1, PACK_T + 1)])


def pack_list(n, kfft, samples, chunk_lo=0, chunk_hi=None):
    """one list [2][N] of `samples` [filled <= N][n+1] through the reference (chunks [chunk_lo, chunk_hi) only)"""
    samples = np.ascontiguousarray(samples, np.int32).reshape(-1, n + 1)
    assert samples.shape[0] <= N
    out = np.zeros((2, N), np.int32)
    src = samples if samples.shape[0] else np.zeros((1, n + 1), np.int32)
    lib().pack_ref_list(int(n), kfft.reshape(-1), src.reshape(-1), samples.shape[0], chunk_lo,
                        n_chunks(n) if chunk_hi is None else chunk_hi, out.reshape(-1))
    return out


def pack(n, kfft, samples, threads=16):
    """[ceil(count / N)][2][N]: sample i in slot i mod N of list i / N"""
    samples = np.ascontiguousarray(samples, np.int32).reshape(-1, n + 1)
    parts = [samples[k:k + N] for k in range(0, samples.shape[0], N)]
    with ThreadPoolExecutor(threads) as ex:
        out = list(ex.map(lambda s: pack_list(n, kfft, s), parts))
    return np.stack(out) if out else np.zeros((0, 2, N), np.int32)


def _negacyclic(d, row):
    full = np.convolve(d, row)                              # |.| < 8 * 2^31 * 2^10: exact in int64
    r = full[:N].copy()
    r[:N - 1] -= full[N:]
    return r


def pack_list_exact(n, rows, samples, chunk_lo, chunk_hi):
    """the same list in EXACT wrapping-integer arithmetic (int64 schoolbook products), chunks [chunk_lo, chunk_hi) only"""
    samples = np.asarray(samples, np.int64).reshape(-1, n + 1)
    rows = np.asarray(rows, np.int64)
    out = np.zeros((2, N), np.int64)
    out[1, :samples.shape[0]] = samples[:, n]
    for m in range(chunk_lo * PACK_CHUNK, min(chunk_hi * PACK_CHUNK, n)):
        col = np.zeros(N, np.int64)
        col[:samples.shape[0]] = samples[:, m]
        d = digits(col)
        for j in range(PACK_T):
            for q in range(2):
                out[q] -= _negacyclic(d[j], rows[m, j, q])
    return _u32(out).view(np.int32)


def list_phases(lists, tlwe_key):
    """phases c1 - c0 s' of every slot, [L][N] int64 wrapped to [-2^31, 2^31)"""
    lists = np.asarray(lists, np.int64).reshape(-1, 2, N)
    ones = np.flatnonzero(np.asarray(tlwe_key))
    ph = np.stack([li[1] - co._rotsum(ones, li[0]) for li in lists])
    return ((ph + 2**31) % 2**32) - 2**31
