"""Rows and references of the rounding twins' instance tests (numpy and the CPU oracle only; shared by
tests/test_leveled_round_cpu.py, which computes every reference here ahead of the device, and
tests/test_gpu_leveled_round_instances.py).

A twin k_rcmux / k_rdemux / k_rstep<L,B> decomposes D + h, h = 2^(31 - l Bgbit) (leveled_round_oracle.half).  Per shape:
  unshifted rows  the truncating instance files' rows as they are (leveled_edge_inputs.cmux_inputs / cmux_differences,
                  automaton_edge_inputs.edge_automaton), then test_leveled_round_cpu.low_part_words with seeds 0 and 1 (the
                  dropped part 0, q/2 - 1, q/2, q - 1) and the all-0xFFFFFFFF row (+ h carries through every digit and wraps)
  shifted rows    every truncating row minus h in every word of both polynomials, wrapping: the twin then decomposes exactly
                  the truncating row, and its output is the TRUNCATING reference's (the CMux: of the unshifted pair; the
                  demultiplexer: out1 the same, out0 less h) -- a route that does not pass through leveled_round_oracle
  full scale      the constant selector on digits_min - h and digits_max - h: the decomposed words are digits_min and
                  digits_max, the recorded maximum lies in the instance's [lo, hi)
Every reference is computed under test_gpu_br_instances.reference, which asserts the conversion contract (|v| < 2^51), and
the truncating references are keyed as tests/test_gpu_cmux_instances.py and tests/test_gpu_demux_instances.py key theirs: in one
session they are computed once.  No arithmetic of its own: the products are cmux_oracle's and leveled_round_oracle's."""
from types import SimpleNamespace

import numpy as np

import automaton_edge_inputs as aei
import cmux_oracle as cx
import leveled_edge_inputs as lei
import leveled_round_oracle as lr
import oracle_lib as ol
import table_update_oracle as tu
from test_gpu_br_instances import reference
from test_gpu_cmux_instances import pool_map
from test_leveled_round_cpu import low_part_words

N = 1024
QUERIES = 3                                    # tests/test_gpu_automaton_instances.py: vectors of other random words
ALT = (4, 7)                                   # the one shape at which an <4,0> twin's rounding term is not 0: h = 8
# truncating kernel name -> its full-scale row; the twins' names are made from these
SHAPES = lei.cmux_full_scale


def half(l, Bgbit):
    return lr.half(SimpleNamespace(l=l, Bgbit=Bgbit))


def tag_of(name, l, Bgbit):
    """the key of a shape's references: the truncating kernel's name, marked where the shape is not the instance file's own"""
    cfg = SHAPES[name]
    return name if (l, Bgbit) == (cfg["l"], cfg["Bgbit"]) else f"{name}@({l},{Bgbit})"


def extra_rows(l, Bgbit):
    """[(name, uint32 [2][N])]: the dropped-part rows (where something is dropped) and the all-ones row"""
    out = []
    if l * Bgbit < 32:
        out += [("low_parts", low_part_words(l, Bgbit)), ("low_parts_shifted", low_part_words(l, Bgbit, seed=1))]
    return out + [("all_ones", np.full((2, N), 0xFFFFFFFF, np.uint32))]


def minus(x, h):
    """x - h in every word, wrapping, int32"""
    return np.ascontiguousarray(lei._i32(np.asarray(x).astype(np.int64) - h))


# ---- k_rcmux -----------------------------------------------------------------------------------------------------------------
def cmux_rows(l, Bgbit):
    """(names [items], in0, in1 int32 [items][2][N], items_t): item 2 s + b is sample s under the selector of bit b; the first
    items_t items are those of tests/test_gpu_cmux_instances.py, the extra rows follow"""
    ins = lei.cmux_inputs(l, Bgbit)
    names = [nm for nm, (a, _) in ins.items() for _ in range(a.shape[0])]
    in0, in1 = [a for a, _ in ins.values()], [b for _, b in ins.values()]
    items_t = 2 * len(names)
    rng = np.random.default_rng(2100 + 10 * l + Bgbit)
    for nm, D in extra_rows(l, Bgbit):
        a = rng.integers(-2**31, 2**31, (1, 2, N))
        names.append(nm), in0.append(lei._i32(a)), in1.append(lei._i32(a + D.astype(np.int64)))
    in0, in1 = (np.ascontiguousarray(np.repeat(np.concatenate(x), 2, axis=0)) for x in (in0, in1))
    return names, in0, in1, items_t


def cmux_truncating(tag, op, fft, in0, in1, items_t):
    """the truncating reference of the truncating rows, keyed and computed as tests/test_gpu_cmux_instances.py does"""
    return reference(("cmux", tag, "edges"),
                     lambda: np.stack(pool_map(lambda k: cx.cmux(op, fft[k % 2], in0[k], in1[k]), items_t)))


def cmux_rounding(tag, op, fft, in0, in1):
    return reference(("rcmux", tag, "edges"),
                     lambda: np.stack(pool_map(lambda k: lr.cmux(op, fft[k % 2], in0[k], in1[k]), len(in0))))


def cmux_full_scale(name, op, kfft, l, Bgbit):
    """(f0, f1, want): digits_min and digits_max, in1 less h"""
    cfg = SHAPES[name]
    ins = lei.cmux_inputs(l, Bgbit)
    f0 = np.concatenate([ins["digits_min"][0], ins["digits_max"][0]])
    f1 = minus(np.concatenate([ins["digits_min"][1], ins["digits_max"][1]]), half(l, Bgbit))

    def full_scale():
        L = ol.lib()
        out = np.stack([lr.cmux(op, kfft, f0[k], f1[k]) for k in range(2)])
        mx = L.orc_dbg_max_conv(0)                              # reference() reset it and asserts the contract behind this
        assert cfg["lo"] <= mx < cfg["hi"], (name, np.log2(mx))
        return out
    return f0, f1, reference(("rcmux", name, "full scale"), full_scale)


# ---- k_rdemux ----------------------------------------------------------------------------------------------------------------
def demux_rows(l, Bgbit):
    """(names [items], x int32 [items][2][N], items_t), laid out as cmux_rows: the differences taken as x itself"""
    diffs = lei.cmux_differences(l, Bgbit)
    names = [nm for nm, a in diffs.items() for _ in range(a.shape[0])]
    rows = [a.view(np.int32) for a in diffs.values()]
    items_t = 2 * len(names)
    for nm, D in extra_rows(l, Bgbit):
        names.append(nm), rows.append(D.view(np.int32)[None])
    return names, np.ascontiguousarray(np.repeat(np.concatenate(rows), 2, axis=0)), items_t


def demux_truncating(tag, op, fft, x, items_t):
    """[items_t][2 outputs][2][N], keyed and computed as tests/test_gpu_demux_instances.py does"""
    return reference(("demux", tag.replace("k_cmux", "k_demux"), "edges"),
                     lambda: np.stack(pool_map(lambda k: np.stack(tu.demux(op, fft[k % 2], x[k])), items_t)))


def demux_rounding(tag, op, fft, x):
    return reference(("rdemux", tag, "edges"),
                     lambda: np.stack(pool_map(lambda k: np.stack(lr.demux(op, fft[k % 2], x[k])), len(x))))


def demux_full_scale(name, op, kfft, l, Bgbit):
    """(fx, want [2][2 outputs][2][N])"""
    cfg = SHAPES[name]
    diffs = lei.cmux_differences(l, Bgbit)
    fx = minus(np.concatenate([diffs["digits_min"], diffs["digits_max"]]).view(np.int32), half(l, Bgbit))

    def full_scale():
        L = ol.lib()
        out = np.stack([np.stack(lr.demux(op, kfft, fx[k])) for k in range(2)])
        mx = L.orc_dbg_max_conv(0)
        assert cfg["lo"] <= mx < cfg["hi"], (name, np.log2(mx))
        return out
    return fx, reference(("rdemux", name, "full scale"), full_scale)


# ---- k_rstep -----------------------------------------------------------------------------------------------------------------
def step_vectors(l, Bgbit):
    """QUERIES edge automata (trans, prev, names) with the extra rows behind the derived ones"""
    return [aei.edge_automaton(l, Bgbit, seed=s, extra=extra_rows(l, Bgbit)) for s in range(QUERIES)]


def step_edges(tag, op, fft, vectors):
    """(cut, want_of): cut[s, c] the first c states of vector s, closed; want_of(s, b, c) [c][2][N] their successors under the
    selector of bit b -- the plan of tests/test_gpu_automaton_instances.py on leveled_round_oracle.step"""
    trans, _, names = vectors[0]
    counts = aei.COUNTS + (len(names),)
    cut = {(s, c): aei.truncated(trans, vectors[s][1], c) for s in range(QUERIES) for c in counts}
    jobs = [(s, b, c, q) for s in range(QUERIES) for b in range(2) for c in counts for q in range(c)]
    at = {(s, b, c): i for i, (s, b, c, q) in enumerate(jobs) if q == 0}
    edges = reference(("rstep", tag, "edges"), lambda: np.stack(pool_map(
        lambda i: lr.step(op, *cut[jobs[i][0], jobs[i][2]], fft[jobs[i][1]], [jobs[i][3]])[0], len(jobs))))
    return cut, lambda s, b, c: edges[at[s, b, c]:at[s, b, c] + c]


def step_full_scale(name, op, kfft, l, Bgbit):
    """(trans, prev, names, want): the digits_min and digits_max pairs built from D - h.  The state of D decomposes D itself;
    its negation decomposes -D + 2 h -- one more in the last digit than the truncating file's -D.  Every state is held to the
    instance's [lo, hi), as there"""
    cfg = SHAPES[name]
    ft, fprev, fnames = aei.full_scale_states(l, Bgbit, shift=half(l, Bgbit))

    def full_scale():
        L = ol.lib()
        out = []
        for q in range(len(fnames)):                            # read and reset per state
            out.append(lr.step(op, ft, fprev, kfft, [q])[0])
            mx = L.orc_dbg_max_conv(1)
            assert cfg["lo"] <= mx < cfg["hi"] <= 2.0**51, (name, fnames[q], np.log2(mx))
        return np.stack(out)
    return ft, fprev, fnames, reference(("rstep", name, "full scale"), full_scale)
