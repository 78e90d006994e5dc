"""Reference of the automaton evaluation (include/eoc_tfhe_gpu.h), composed from tests/cmux_oracle.py: a step is
cmux_oracle.cmux of the two successors, each turned by cmux_oracle.rotate; a run is the steps from the last bit to the first,
numpy slot extraction as in tests/compact_oracle.py, orc_keyswitch.  No arithmetic of its own.  Test-side only."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import cmux_oracle as cx
import compact_oracle as co

N = 1024


def records(trans):
    """[states][4] int32 = (next0, w0, next1, w1) of an Automaton or an array-like"""
    return np.ascontiguousarray(getattr(trans, "trans", trans), np.int32).reshape(-1, 4)


def successor(prev, nxt, w):
    """X^(-w) prev[nxt] as int32 words"""
    return cx._u32(cx.rotate(prev[nxt], (2 * N - int(w)) % (2 * N))).view(np.int32)


def step_state(p, trans, prev, sel_fft, q):
    """next[q] = A + C (x) (B - A), A = X^(-w0) prev[next0], B = X^(-w1) prev[next1]"""
    n0, w0, n1, w1 = (int(x) for x in records(trans)[q])
    return cx.cmux(p, sel_fft, successor(prev, n0, w0), successor(prev, n1, w1))


def step(p, trans, prev, sel_fft, states=None):
    """one backward step of one query: prev [states][2][N] -> [len(states)][2][N] (every state by default)"""
    prev = np.asarray(prev, np.int32).reshape(-1, 2, N)
    states = range(len(records(trans))) if states is None else states
    return np.stack([step_state(p, trans, prev, sel_fft, q) for q in states])


def run_tlwe(p, trans, final, sel_fft, starts):
    """the TLWE samples [len(starts)][2][N] of one query: sel_fft [steps][2l][2][N] float64, selector t = input bit t; the
    steps run from the last bit to the first and the one under bit 0 computes the start states alone"""
    V = np.asarray(final, np.int32).reshape(-1, 2, N)
    steps = len(sel_fft)
    for t in range(steps - 1, -1, -1):
        V = step(p, trans, V, sel_fft[t], starts if t == 0 else None)
    return V if steps else V[list(starts)]


def run(orc, p, trans, final, sel_fft, starts, log2_width, threads=16):
    """the composed run of every query: sel_fft [queries][steps][2l][2][N] -> [queries][len(starts)][W][n+1] (slots 0 .. W-1 of
    each start state's sample extracted as in compact_oracle.extract, then orc_keyswitch); also the samples
    [queries][len(starts)][2][N]"""
    W, ns = 1 << int(log2_width), len(starts)
    with ThreadPoolExecutor(threads) as ex:
        tl = list(ex.map(lambda s: run_tlwe(p, trans, final, s, starts), sel_fft))
    tl = np.stack(tl).reshape(-1, 2, N) if len(tl) else np.zeros((0, 2, N), np.int32)
    idx = (np.arange(len(tl))[:, None] * N + np.arange(W)[None, :]).ravel()
    out = co.expand(orc, tl, idx, threads).reshape(len(sel_fft), ns, W, orc.n + 1)
    return out, tl.reshape(len(sel_fft), ns, 2, N)
