"""Reference of the encrypted-index table update (include/eoc_tfhe_gpu.h), composed on tests/cmux_oracle.py:
the rotations are its cmux, the demultiplexer is its extprod (the CMux's external product with in0 = 0, in1 = x, rot = 0
before the add), the accumulation is a wrapping integer sum.  Test-side only; no new C."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import cmux_oracle as cx

N = 1024


def wrap_i32(x):
    return cx._u32(x).view(np.int32)


def demux(p, sel_fft, x):
    """(child 2j, child 2j + 1) = (x - E, E), E = C (x) x: [2][N] int32 each"""
    x = np.asarray(x, np.int32).reshape(2, N)
    E = cx.extprod(p, sel_fft, x.astype(np.int64))
    return wrap_i32(x.astype(np.int64) - E.astype(np.int64)), E


def rotated(p, log2_width, sel_fft, value):
    """the value behind the r rotations: x <- x + C_i (x) (X^(W 2^i) x - x), i ascending"""
    r, W = 10 - int(log2_width), 1 << int(log2_width)
    x = np.asarray(value, np.int32).reshape(2, N)
    for i in range(r):
        x = cx.cmux(p, sel_fft[i], x, x, rot=W << i)
    return x


def leaves(p, log2_lists, log2_width, sel_fft, value):
    """the 2^d leaves [2^d][2][N] int32 of one query: sel_fft [r + d][2l][2][N] float64 (index bits LSB first), stage t under
    bit r + (d - 1 - t), parent j -> children 2j (x - E) and 2j + 1 (E)"""
    d, r = int(log2_lists), 10 - int(log2_width)
    cur = [rotated(p, log2_width, sel_fft, value)]
    for t in range(d):
        nxt = []
        for x in cur:
            nxt.extend(demux(p, sel_fft[r + d - 1 - t], x))
        cur = nxt
    return np.stack(cur)


def table_update(p, table, log2_lists, log2_width, sel_fft, values, threads=16):
    """table [2^d][2][N] int32 with table[idx_q] += values[q] for every query, as a new array; sel_fft [queries][r + d]...
    (None or empty at r + d = 0)"""
    table = np.asarray(table, np.int32).reshape(1 << int(log2_lists), 2, N)
    values = np.asarray(values, np.int32).reshape(-1, 2, N)
    acc = table.astype(np.int64)
    depth = int(log2_lists) + 10 - int(log2_width)
    with ThreadPoolExecutor(threads) as ex:                     # ctypes drops the GIL inside the references
        for lv in ex.map(lambda q: leaves(p, log2_lists, log2_width, sel_fft[q] if depth else None, values[q]),
                         range(len(values))):
            acc += lv
    return wrap_i32(acc)
