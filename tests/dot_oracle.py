"""Reference of the inner product with public integer weights (include/eoc_tfhe_gpu.h) on the oracle: the
chunked operation through tests/c/dot_ref.c (compiled here with gcc -ffp-contract=off against liboracle.so) and the exact
wrapping-integer evaluation in numpy.  Test-side only."""
import atexit
import ctypes as C
import os
import shutil
import subprocess
import tempfile
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import oracle_lib as ol

N = 1024
DOT_CHUNK = 8
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_lib = None


def lib():
    global _lib
    if _lib is None:
        so_oracle = ol.build_oracle()
        tmp = tempfile.mkdtemp(prefix="dot_ref_")
        atexit.register(shutil.rmtree, tmp, ignore_errors=True)
        so = os.path.join(tmp, "libdot_ref.so")
        subprocess.check_call(["gcc", "-std=c11", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-shared", "-fPIC",
                               "-I" + ol.ORACLE_DIR, os.path.join(ROOT, "tests", "c", "dot_ref.c"), "-o", so, so_oracle,
                               "-Wl,-rpath," + ol.ORACLE_DIR, "-lm"])
        ol.lib()                                            # liboracle.so first: the reference resolves against it
        L = C.CDLL(so)
        i8p = np.ctypeslib.ndpointer(np.int8, flags="C")
        i32p = np.ctypeslib.ndpointer(np.int32, flags="C")
        L.dot_ref_sample.argtypes = [i8p, C.c_int, i32p, C.c_int32, C.c_int, C.c_int, i32p, C.POINTER(C.c_double)]
        L.dot_ref_sample.restype = None
        _lib = L
    return _lib


def _u32(x):
    return (np.asarray(x, np.int64) & 0xFFFFFFFF).astype(np.uint32)


def n_lists(cols):
    return (int(cols) + N - 1) // N


def n_chunks(cols):
    return (n_lists(cols) + DOT_CHUNK - 1) // DOT_CHUNK


def padded(weights):
    """[rows][cols] -> [rows][L N] int8, zero past cols"""
    w = np.asarray(weights)
    assert w.ndim == 2 and np.abs(w.astype(np.int64)).max() <= 127
    out = np.zeros((w.shape[0], n_lists(w.shape[1]) * N), np.int8)
    out[:, :w.shape[1]] = w
    return out


def sample(wrow, lists, bias=0, chunk_lo=0, chunk_hi=None, hwm=None):
    """one output sample [N+1] through the reference: wrow [L N] int8 (padded), lists [L][2][N]; chunks [chunk_lo, chunk_hi)
    of the mask only; hwm: a one-element float64 array that keeps the high-water mark before conversion"""
    wrow = np.ascontiguousarray(wrow, np.int8)
    lists = np.ascontiguousarray(lists, np.int32).reshape(-1, 2, N)
    L = lists.shape[0]
    assert wrow.shape == (L * N,)
    out = np.zeros(N + 1, np.int32)
    lib().dot_ref_sample(wrow, L, lists.reshape(-1), int(np.int32(bias)), chunk_lo,
                         (L + DOT_CHUNK - 1) // DOT_CHUNK if chunk_hi is None else chunk_hi, out,
                         None if hwm is None else hwm.ctypes.data_as(C.POINTER(C.c_double)))
    return out


def dot(weights, lists, bias=None, threads=16):
    """[batch][rows][N+1]: weights [rows][cols] in [-127, 127], lists [batch][L][2][N], bias [rows] Torus32 or None"""
    w = padded(weights)
    rows = w.shape[0]
    lists = np.ascontiguousarray(lists, np.int32).reshape(-1, w.shape[1] // N, 2, N)
    bias = np.zeros(rows, np.int32) if bias is None else np.asarray(bias, np.int32)
    jobs = [(b, r) for b in range(lists.shape[0]) for r in range(rows)]
    with ThreadPoolExecutor(threads) as ex:
        out = list(ex.map(lambda br: sample(w[br[1]], lists[br[0]], bias[br[1]]), jobs))
    return np.stack(out).reshape(lists.shape[0], rows, N + 1) if out else np.zeros((0, rows, N + 1), np.int32)


def weight_poly(wl):
    """V of one list's weights wl [N]: V[0] = w[0], V[N - k] = -w[k]"""
    wl = np.asarray(wl, np.int64)
    V = np.zeros(N, np.int64)
    V[0] = wl[0]
    V[N - np.arange(1, N)] = -wl[1:]
    return V


def _negacyclic(a, b):
    full = np.convolve(a, b)                                # |.| < 127 * 2^31 * 2^10: exact in int64
    r = full[:N].copy()
    r[:N - 1] -= full[N:]
    return r


def sample_exact(wrow, lists, bias=0, chunk_lo=0, chunk_hi=None):
    """the same sample in EXACT wrapping-integer arithmetic: int64 schoolbook products of the weight polynomials with c0,
    chunks [chunk_lo, chunk_hi) of the mask only, and the integer body"""
    wrow = np.asarray(wrow, np.int64)
    lists = np.asarray(lists, np.int64).reshape(-1, 2, N)
    L = lists.shape[0]
    hi = (L + DOT_CHUNK - 1) // DOT_CHUNK if chunk_hi is None else chunk_hi
    P0 = np.zeros(N, np.int64)
    for l in range(chunk_lo * DOT_CHUNK, min(hi * DOT_CHUNK, L)):
        P0 += _negacyclic(weight_poly(wrow[l * N:(l + 1) * N]), lists[l, 0])
    out = np.empty(N + 1, np.int64)
    out[0] = P0[0]
    out[1:N] = -P0[N - np.arange(1, N)]
    out[N] = int(bias) + int(np.dot(wrow, lists[:, 1].reshape(-1)))    # < 2^20 * 127 * 2^31 < 2^63
    return _u32(out).view(np.int32)


def lsb_deviation(a, b):
    """largest |a - b| over the words, as wrapped int32 differences"""
    d = (_u32(a).astype(np.int64) - _u32(b).astype(np.int64) + 2**31) % 2**32 - 2**31
    return int(np.abs(d).max())


def plain_sum(weights, msgs):
    """sum_k w[r][k] msgs[b][k] for msgs [batch][cols] Torus32, wrapped to [-2^31, 2^31): [batch][rows]"""
    s = np.asarray(msgs, np.int64) @ np.asarray(weights, np.int64).T
    return ((s + 2**31) % 2**32) - 2**31
