"""Reference of the convolution with public int8 kernels (include/eoc_tfhe_gpu.h) on the oracle: the chunked
operation through tests/c/conv_ref.c (compiled here with dot_oracle.py's build line against liboracle.so) and the exact
wrapping-integer evaluation in numpy (int64 schoolbook products).  Test-side only."""
import atexit
import ctypes as C
import os
import shutil
import subprocess
import tempfile
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import dot_oracle as do
import oracle_lib as ol

N = 1024
CONV_CHUNK = do.DOT_CHUNK
ROOT = do.ROOT

_lib = None


def lib():
    global _lib
    if _lib is None:
        so_oracle = ol.build_oracle()
        tmp = tempfile.mkdtemp(prefix="conv_ref_")
        atexit.register(shutil.rmtree, tmp, ignore_errors=True)
        so = os.path.join(tmp, "libconv_ref.so")
        subprocess.check_call(["gcc", "-std=c11", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-shared", "-fPIC",
                               "-I" + ol.ORACLE_DIR, os.path.join(ROOT, "tests", "c", "conv_ref.c"), "-o", so, so_oracle,
                               "-Wl,-rpath," + ol.ORACLE_DIR, "-lm"])
        ol.lib()                                            # liboracle.so first: the reference resolves against it
        L = C.CDLL(so)
        i8p = np.ctypeslib.ndpointer(np.int8, flags="C")
        i32p = np.ctypeslib.ndpointer(np.int32, flags="C")
        L.conv_ref_lists.argtypes = [i8p, C.c_int, i32p, C.c_int32, C.c_int, C.c_int, i32p, C.POINTER(C.c_double)]
        L.conv_ref_lists.restype = None
        _lib = L
    return _lib


def out_list(wrow, lists, bias=0, chunk_lo=0, chunk_hi=None, hwm=None):
    """one output list [2][N] through the reference: wrow [L N] int8 (padded), lists [L][2][N]; chunks [chunk_lo, chunk_hi)
    only; hwm: a one-element float64 array that keeps the high-water mark before conversion"""
    wrow = np.ascontiguousarray(wrow, np.int8)
    lists = np.ascontiguousarray(lists, np.int32).reshape(-1, 2, N)
    L = lists.shape[0]
    assert wrow.shape == (L * N,)
    out = np.zeros((2, N), np.int32)
    lib().conv_ref_lists(wrow, L, lists.reshape(-1), int(np.int32(bias)), chunk_lo,
                         (L + CONV_CHUNK - 1) // CONV_CHUNK if chunk_hi is None else chunk_hi, out.reshape(-1),
                         None if hwm is None else hwm.ctypes.data_as(C.POINTER(C.c_double)))
    return out


def conv(weights, lists, bias=None, threads=16):
    """[batch][rows][2][N]: weights [rows][cols] in [-127, 127], lists [batch][L][2][N], bias [rows] Torus32 or None"""
    w = do.padded(weights)
    rows = w.shape[0]
    lists = np.ascontiguousarray(lists, np.int32).reshape(-1, w.shape[1] // N, 2, N)
    bias = np.zeros(rows, np.int32) if bias is None else np.asarray(bias, np.int32)
    jobs = [(b, r) for b in range(lists.shape[0]) for r in range(rows)]
    with ThreadPoolExecutor(threads) as ex:
        out = list(ex.map(lambda br: out_list(w[br[1]], lists[br[0]], bias[br[1]]), jobs))
    return np.stack(out).reshape(lists.shape[0], rows, 2, N) if out else np.zeros((0, rows, 2, N), np.int32)


def out_list_exact(wrow, lists, bias=0, chunk_lo=0, chunk_hi=None):
    """the same list in EXACT wrapping-integer arithmetic: int64 schoolbook products of the weight polynomials with c0 and
    with c1 (|.| < 2^20 * 127 * 2^31 < 2^63), chunks [chunk_lo, chunk_hi) only"""
    wrow = np.asarray(wrow, np.int64)
    lists = np.asarray(lists, np.int64).reshape(-1, 2, N)
    L = lists.shape[0]
    hi = (L + CONV_CHUNK - 1) // CONV_CHUNK if chunk_hi is None else chunk_hi
    P = np.zeros((2, N), np.int64)
    for l in range(chunk_lo * CONV_CHUNK, min(hi * CONV_CHUNK, L)):
        V = do.weight_poly(wrow[l * N:(l + 1) * N])
        for p in range(2):
            P[p] += do._negacyclic(V, lists[l, p])
    P[1] += int(bias)
    return do._u32(P).view(np.int32)


def to_dot_mask(c0):
    """the word map to the inner product's sample: mask word i of eoc_dot_device's sample is word (N - i) mod N of the
    convolution's c0, negated for i > 0"""
    c0 = np.asarray(c0, np.int64)
    out = np.empty(c0.shape, np.int64)
    out[..., 0] = c0[..., 0]
    out[..., 1:] = -c0[..., :0:-1]
    return do._u32(out).view(np.int32)


def shifted_rows(w_row, slots):
    """[len(slots)][L N] int64: the effective inner-product rows of slots `slots` of one output channel, written out without
    noise.conv_row: row t holds w[m - t] at m >= t and -w[m - t + N] below, per list"""
    w = np.asarray(w_row, np.int64).reshape(-1, N)
    out = np.empty((len(slots), w.shape[0], N), np.int64)
    for i, t in enumerate(slots):
        out[i] = np.concatenate((-w[:, N - t:], w[:, :N - t]), axis=1) if t else w
    return out.reshape(len(slots), -1)
