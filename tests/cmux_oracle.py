"""Reference of the leveled operations (include/eoc_tfhe_gpu.h) on the oracle: selector encryption restated on
the oracle's streams (tag 8), the CMux through tests/c/cmux_ref.c (compiled here with gcc -ffp-contract=off against
liboracle.so), and the composed table read -- the levels in the engine's order, numpy slot extraction as in
tests/compact_oracle.py, orc_keyswitch.  Test-side only."""
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
TAG_TGSW_ENC = 8
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_lib = None


def lib():
    global _lib
    if _lib is None:
        so_oracle = ol.build_oracle()
        tmp = tempfile.mkdtemp(prefix="cmux_ref_")
        atexit.register(shutil.rmtree, tmp, ignore_errors=True)
        so = os.path.join(tmp, "libcmux_ref.so")
        subprocess.check_call(["gcc", "-std=c11", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-shared", "-fPIC",
                               "-I" + ol.ORACLE_DIR, os.path.join(ROOT, "tests", "c", "cmux_ref.c"), "-o", so, so_oracle,
                               "-Wl,-rpath," + ol.ORACLE_DIR, "-lm"])
        ol.lib()                                            # liboracle.so first: the reference resolves against it
        L = C.CDLL(so)
        i32p = np.ctypeslib.ndpointer(np.int32, flags="C")
        L.cmux_ref_extprod.argtypes = [C.POINTER(ol.OrcParams), np.ctypeslib.ndpointer(np.float64, flags="C"), i32p, i32p]
        L.cmux_ref_extprod.restype = None
        _lib = L
    return _lib


def orc_params(params):
    """OrcParams of an eoc Params (or of an OrcParams)"""
    p = ol.OrcParams()
    for f, _ in ol.OrcParams._fields_:
        setattr(p, f, getattr(params, f))
    return p


def _u32(x):
    return (np.asarray(x, np.int64) & 0xFFFFFFFF).astype(np.uint32)


def tgsw_encrypt(params, tlwe_key, enc_seed, first_idx, bits):
    """eoc_tgsw_encrypt_bits restated: [len(bits)][2l][2][N] int32"""
    L = ol.lib()
    l, Bgbit, kpl = int(params.l), int(params.Bgbit), 2 * int(params.l)
    ones = np.flatnonzero(np.asarray(tlwe_key))
    out = np.zeros((len(bits), kpl, 2, N), np.uint32)
    for s, bit in enumerate(bits):
        for row in range(kpl):
            key = L.orc_stream_key(enc_seed, TAG_TGSW_ENC, (first_idx + s) * kpl + row)
            a = np.array([L.orc_rng_u64(key, j) >> 32 for j in range(N)], np.int64)
            e = np.array([L.orc_gaussian32(key, N + 2 * j, 0, params.bk_stdev) for j in range(N)], np.int64)
            b = e + co._rotsum(ones, a)
            if bit:
                (b if row // l else a)[0] += 1 << (32 - (row % l + 1) * Bgbit)
            out[s, row, 0], out[s, row, 1] = _u32(a), _u32(b)
    return out.view(np.int32)


def to_fft(sel):
    """orc_bk_to_fft on selectors [...][N] int32 -> [...][N] float64 (unscaled: the device form carries an exact 2^-9)"""
    sel = np.ascontiguousarray(sel, np.int32)
    flat = sel.reshape(-1, N)
    out = np.zeros(flat.shape, np.float64)
    for k in range(flat.shape[0]):
        ol.lib().orc_fft_fwd(flat[k], out[k])
    return out.reshape(sel.shape)


def rotate(tlwe, rot):
    """X^rot * (c0, c1), rot in [0, 2N)"""
    tlwe = np.asarray(tlwe, np.int64).reshape(2, N)
    idx = (np.arange(N) - rot) % (2 * N)
    v = tlwe[:, idx % N]
    return np.where(idx >= N, -v, v)


def extprod(p, sel_fft, D):
    r = np.zeros((2, N), np.int32)
    lib().cmux_ref_extprod(C.byref(p), np.ascontiguousarray(sel_fft, np.float64), _u32(D).view(np.int32).reshape(2, N).copy(), r)
    return r


def cmux(p, sel_fft, A, B, rot=0):
    """A + C (x) (X^rot B - A), [2][N] int32"""
    A = np.asarray(A, np.int64).reshape(2, N)
    D = rotate(B, rot) - A
    return _u32(A + extprod(p, sel_fft, D).astype(np.int64)).view(np.int32)


def extprod_exact(params, sel, D):
    """the exact integer schoolbook external product mod 2^32 (what the FFT path approximates): sel in torus form"""
    l, Bgbit = int(params.l), int(params.Bgbit)
    Bg = 1 << Bgbit
    off = sum((Bg >> 1) << (32 - pp * Bgbit) for pp in range(1, l + 1))
    u = (_u32(D).astype(np.int64).reshape(2, N) + off) & 0xFFFFFFFF
    sel = np.asarray(sel, np.int64).reshape(2 * l, 2, N)
    r = np.zeros((2, N), np.int64)
    for q in range(2):
        for pp in range(1, l + 1):
            dec = ((u[q] >> (32 - pp * Bgbit)) & (Bg - 1)) - (Bg >> 1)
            for c in range(2):
                full = np.convolve(dec, sel[q * l + pp - 1, c])          # |.| < 2^9 2^31 2^10: exact in int64
                r[c] += full[:N]
                r[c, :N - 1] -= full[N:]
    return _u32(r).view(np.int32)


def table_read_tlwe(p, table, log2_lists, log2_width, sel_fft):
    """the TLWE sample [2][N] behind the last CMux of one query: sel_fft [r + d][2l][2][N] float64, index bits LSB first;
    tree first (level v under bit r + v, nodes (2j, 2j + 1) -> j), then rotation i by X^(2N - W 2^i) under bit i"""
    d, r, W = int(log2_lists), 10 - int(log2_width), 1 << int(log2_width)
    cur = [np.asarray(t, np.int32) for t in np.asarray(table).reshape(1 << d, 2, N)]
    for v in range(d):
        cur = [cmux(p, sel_fft[r + v], cur[2 * j], cur[2 * j + 1]) for j in range(len(cur) // 2)]
    x = cur[0]
    for i in range(r):
        x = cmux(p, sel_fft[i], x, x, rot=2 * N - (W << i))
    return x


def table_read(orc, p, table, log2_lists, log2_width, sel_fft, threads=16):
    """the composed read of every query: sel_fft [queries][r + d][2l][2][N] -> [queries][W][n+1] (slots 0 .. W-1 of the
    query's sample extracted as in compact_oracle.extract, then orc_keyswitch); also returns the samples [queries][2][N]"""
    W = 1 << int(log2_width)
    with ThreadPoolExecutor(threads) as ex:
        tl = list(ex.map(lambda s: table_read_tlwe(p, table, log2_lists, log2_width, s), sel_fft))
    tl = np.stack(tl) if len(tl) else np.zeros((0, 2, N), np.int32)
    idx = (np.arange(len(tl))[:, None] * N + np.arange(W)[None, :]).ravel()
    out = co.expand(orc, tl, idx, threads).reshape(len(tl), W, orc.n + 1)
    return out, tl
