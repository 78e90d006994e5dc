"""Reference of the leveled calls in ROUNDING mode (include/eoc_tfhe_gpu.h), by the identity that defines the
mode: a rounding external product is the truncating one (cmux_oracle.extprod, tests/c/cmux_ref.c) of D + h, h = 2^(31 - l Bgbit)
added to every coefficient word of both polynomials (0 where l Bgbit = 32).  Everything else -- rotations, tree and stage order,
accumulation, slot extraction, key switch -- is restated from tests/cmux_oracle.py, tests/table_update_oracle.py and
tests/automaton_oracle.py around that one product, with their helpers.  No arithmetic of its own.  Test-side only."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import automaton_oracle as ao
import cmux_oracle as cx
import compact_oracle as co
import table_update_oracle as tu

N = 1024


def half(p):
    """h: half of what the gadget of p drops from a word, 0 where it drops nothing"""
    lb = int(p.l) * int(p.Bgbit)
    return 1 << (31 - lb) if lb < 32 else 0


def extprod(p, sel_fft, D):
    """C (x)_r D = C (x) (D + h)"""
    return cx.extprod(p, sel_fft, np.asarray(D, np.int64).reshape(2, N) + half(p))


def extprod_exact(params, sel, D):
    """the exact schoolbook product with ROUNDED digits (cmux_oracle.extprod_exact of D + h): sel in torus form"""
    return cx.extprod_exact(params, sel, np.asarray(D, np.int64).reshape(2, N) + half(params))


def cmux(p, sel_fft, A, B, rot=0):
    """A + C (x)_r (X^rot B - A), [2][N] int32"""
    A = np.asarray(A, np.int64).reshape(2, N)
    return tu.wrap_i32(A + extprod(p, sel_fft, cx.rotate(B, rot) - A).astype(np.int64))


# ---- table read (cmux_oracle.table_read_tlwe / table_read) -------------------------------------------------------------------
def table_read_tlwe(p, table, log2_lists, log2_width, sel_fft):
    d, r, W = int(log2_lists), 10 - int(log2_width), 1 << int(log2_width)
    cur = [np.asarray(t, np.int32) for t in np.asarray(table).reshape(1 << d, 2, N)]
    for v in range(d):
        cur = [cmux(p, sel_fft[r + v], cur[2 * j], cur[2 * j + 1]) for j in range(len(cur) // 2)]
    x = cur[0]
    for i in range(r):
        x = cmux(p, sel_fft[i], x, x, rot=2 * N - (W << i))
    return x


def table_read(orc, p, table, log2_lists, log2_width, sel_fft, threads=16):
    """[queries][W][n+1] and the samples [queries][2][N]"""
    W = 1 << int(log2_width)
    with ThreadPoolExecutor(threads) as ex:
        tl = list(ex.map(lambda s: table_read_tlwe(p, table, log2_lists, log2_width, s), sel_fft))
    tl = np.stack(tl) if len(tl) else np.zeros((0, 2, N), np.int32)
    idx = (np.arange(len(tl))[:, None] * N + np.arange(W)[None, :]).ravel()
    return co.expand(orc, tl, idx, threads).reshape(len(tl), W, orc.n + 1), tl


# ---- table update (table_update_oracle.demux / rotated / leaves / table_update) ----------------------------------------------
def demux(p, sel_fft, x):
    """(x - E, E), E = C (x)_r x"""
    x = np.asarray(x, np.int32).reshape(2, N)
    E = extprod(p, sel_fft, x.astype(np.int64))
    return tu.wrap_i32(x.astype(np.int64) - E.astype(np.int64)), E


def leaves(p, log2_lists, log2_width, sel_fft, value):
    d, r, W = int(log2_lists), 10 - int(log2_width), 1 << int(log2_width)
    x = np.asarray(value, np.int32).reshape(2, N)
    for i in range(r):
        x = cmux(p, sel_fft[i], x, x, rot=W << i)
    cur = [x]
    for t in range(d):
        nxt = []
        for y in cur:
            nxt.extend(demux(p, sel_fft[r + d - 1 - t], y))
        cur = nxt
    return np.stack(cur)


def table_update(p, table, log2_lists, log2_width, sel_fft, values, threads=16):
    table = np.asarray(table, np.int32).reshape(1 << int(log2_lists), 2, N)
    values = np.asarray(values, np.int32).reshape(-1, 2, N)
    acc = table.astype(np.int64)
    depth = int(log2_lists) + 10 - int(log2_width)
    with ThreadPoolExecutor(threads) as ex:
        for lv in ex.map(lambda q: leaves(p, log2_lists, log2_width, sel_fft[q] if depth else None, values[q]), range(len(values))):
            acc += lv
    return tu.wrap_i32(acc)


# ---- automata (automaton_oracle.step / run_tlwe / run) -----------------------------------------------------------------------
def step(p, trans, prev, sel_fft, states=None):
    prev = np.asarray(prev, np.int32).reshape(-1, 2, N)
    rec = ao.records(trans)
    states = range(len(rec)) if states is None else states
    return np.stack([cmux(p, sel_fft, ao.successor(prev, int(rec[q][0]), int(rec[q][1])),
                          ao.successor(prev, int(rec[q][2]), int(rec[q][3]))) for q in states])


def run_tlwe(p, trans, final, sel_fft, starts):
    V = np.asarray(final, np.int32).reshape(-1, 2, N)
    steps = len(sel_fft)
    for t in range(steps - 1, -1, -1):
        V = step(p, trans, V, sel_fft[t], starts if t == 0 else None)
    return V if steps else V[list(starts)]


def run(orc, p, trans, final, sel_fft, starts, log2_width, threads=16):
    W, ns = 1 << int(log2_width), len(starts)
    with ThreadPoolExecutor(threads) as ex:
        tl = list(ex.map(lambda s: run_tlwe(p, trans, final, s, starts), sel_fft))
    tl = np.stack(tl).reshape(-1, 2, N) if len(tl) else np.zeros((0, 2, N), np.int32)
    idx = (np.arange(len(tl))[:, None] * N + np.arange(W)[None, :]).ravel()
    out = co.expand(orc, tl, idx, threads).reshape(len(sel_fft), ns, W, orc.n + 1)
    return out, tl.reshape(len(sel_fft), ns, 2, N)
