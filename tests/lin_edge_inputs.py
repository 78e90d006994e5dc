"""Edge inputs for the linear stage and the mod switch in front of every blind rotation (numpy only; shared by
tests/test_lin_edge_inputs_cpu.py and tests/test_gpu_linear_stage_paths.py; the cells are those of tests/br_edge_inputs.py).

The stage computes t = sum_k w_k in_k + (0, ..., 0, cst) in wrapping 32-bit arithmetic and rounds every word onto the
rotation grid, ((t + 2^(20+theta)) >> (21+theta)) << theta & 2047 -- in prepare_row, k_prepare, k_modswitch_coarse and
k_lin_modswitch (eoc_tfhe_amd/csrc/kernels.hip.h).  A random word sits on the end of a rounding cell with probability 2^-20;
here EVERY word of the wanted row t* does, and the operands are solved so that the stage yields exactly t*: what the gate
computes then depends on t* alone, and one oracle reference per set of target rows serves every opcode and code path.

  targets(n, rows, even, seed, n_tables=1)   int32 [rows][n+1]: every word the smallest or the largest word of the cell of
                    an amount of br_edge_inputs.edge_amounts(T); both ends of all eight amounts occur among the mask words
                    and in word n.  even: the largest word is the largest EVEN word of the cell (the doubling opcodes
                    reach even words only); a step of 2 outwards still rounds elsewhere.
  solve(op, t_star, seed[, t_star2])   operand rows (a, b[, c]) of opcode `op` whose linear stage is t_star (MUX: AND(a, b) =
                    t_star and ANDNY(a, c) = t_star2, one shared a).  One operand (two for MAJ / XOR3) is drawn over the whole
                    int32 range, the last is solved; on half the words of the +-1 opcodes the draw is confined to the
                    values that make the exact integer sum leave [-2^31, 2^31).  The factor 2 of XOR / XNOR / XOR3 drops
                    the solved operand's top bit, which is random.
  solve_node(weights, cst, t_star, seed)   the same for an integer-circuit node of 1 .. 4 terms: the last weight is +-1.
  free_gate_rows(n, rows, seed)   rows of 0, -1, 1, INT32_MIN, INT32_MAX and random words for NOT / COPY.
"""
import numpy as np

import br_edge_inputs as bei

# gate_lin of kernels.hip.h, restated: opcode -> (cst in eighths, s0, s1); gate_lin3: sign of all three
GATE_LIN = {0: (1, -1, -1), 1: (-1, 1, 1), 2: (1, 1, 1), 3: (-1, -1, -1), 4: (2, 2, 2), 5: (-2, -2, -2),
            6: (-1, -1, 1), 7: (-1, 1, -1), 8: (1, -1, 1), 9: (1, 1, -1)}
GATE_LIN3 = {15: 1, 16: -2}
OP_MUX, OP_NOT, OP_COPY, OP_CONST0, OP_CONST1, OP_MAJ, OP_XOR3 = 10, 11, 12, 13, 14, 15, 16
TWO_INPUT = tuple(range(10))
DOUBLING = (4, 5, 16)
NODE_WEIGHTS = (-2**31, 2**31 - 1, -3, 2, 0x10001)
INT32_MIN, INT32_MAX = -2**31, 2**31 - 1


def wrap32(x):
    """int64 (or Python ints) -> the int32 with the same low 32 bits"""
    return (np.asarray(x, np.int64) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)


def _random_words(rng, shape):
    return rng.integers(INT32_MIN, INT32_MAX + 1, shape, dtype=np.int64)


def target_cells(n, rows, even, seed, n_tables=1):
    """(t_star int32 [rows][n+1], amount int64 [rows][n+1], end [rows][n+1]: 0 = smallest word of the cell, 1 = largest)"""
    rng = np.random.default_rng(seed)
    combo = rng.integers(0, 16, (rows, n + 1))                  # amount index * 2 + end
    assert rows >= 16 or n >= 16
    if n >= 16:
        for r in range(rows):
            combo[r, (5 * r + np.arange(16)) % n] = rng.permutation(16)
    else:
        combo[:, :n] = ((np.arange(rows)[:, None] * 5 + np.arange(n)[None, :] + seed) % 16)
    combo[:, n] = (3 * np.arange(rows) + seed) % 16 if rows >= 16 else rng.integers(0, 16, rows)
    amount = bei.edge_amounts(n_tables)[combo >> 1]
    end = combo & 1
    lo, hi = bei.cell_words(amount, n_tables)
    hi = hi.astype(np.int64) - (1 if even else 0)
    t = np.where(end == 0, lo.astype(np.int64), hi)
    return np.ascontiguousarray(wrap32(t)), amount, end


def targets(n, rows, even, seed, n_tables=1):
    """int32 [rows][n+1]: see the module docstring"""
    return target_cells(n, rows, even, seed, n_tables)[0]


def _confined_draw(rng, s0, s1, tp):
    """for |s0| = |s1| = 1: values a (int64, in int32 range) for which no int32 b makes s0 a + s1 b = tp WITHOUT a wrap --
    s0 a + s1 b = tp + k 2^32 with k = +1 (tp < 0) or -1 -- and a mask of the words where such values exist"""
    k = np.where(tp < 0, 1, -1).astype(np.int64)
    goal = tp + (k << 32)
    a_lo, a_hi = (INT32_MIN, INT32_MAX) if s0 > 0 else (-INT32_MAX, -INT32_MIN)      # range of A = s0 a
    b_lo, b_hi = (INT32_MIN, INT32_MAX) if s1 > 0 else (-INT32_MAX, -INT32_MIN)      # range of B = s1 b
    w_lo, w_hi = np.maximum(a_lo, goal - b_hi), np.minimum(a_hi, goal - b_lo)
    ok = w_lo <= w_hi
    A = w_lo + (rng.random(tp.shape) * (np.where(ok, w_hi - w_lo, 0) + 1)).astype(np.int64)
    A = np.minimum(A, np.where(ok, w_hi, A))
    return s0 * A, ok


def _solve_last(rng, s, rest):
    """int32 x with s x = rest (mod 2^32), s in {1, -1, 2, -2}; for |s| = 2 rest must be even and x's top bit is random"""
    rest = np.asarray(rest, np.int64) & 0xFFFFFFFF
    if abs(s) == 1:
        return wrap32(s * rest)
    assert (rest & 1).sum() == 0, "the doubling opcodes reach even words only"
    half = rest >> 1                                             # 2 half = rest; bit 31 of x is free
    x = (half if s > 0 else -half) & 0x7FFFFFFF
    return wrap32(x | (rng.integers(0, 2, rest.shape, dtype=np.int64) << 31))


def _cst_row(shape, cst):
    c = np.zeros(shape, np.int64)
    c[..., -1] = cst
    return c


def solve(op, t_star, seed, t_star2=None):
    """operand rows (int32, like t_star) of opcode op: (a, b), or (a, b, c) for MAJ / XOR3 / MUX"""
    rng = np.random.default_rng(seed)
    t = np.asarray(t_star, np.int32).astype(np.int64)
    if op in GATE_LIN3:
        s = GATE_LIN3[op]
        a, b = _random_words(rng, t.shape), _random_words(rng, t.shape)
        return wrap32(a), wrap32(b), _solve_last(rng, s, t - s * (a + b))
    if op == OP_MUX:
        t2 = np.asarray(t_star2, np.int32).astype(np.int64)
        a, b = solve(1, t_star, seed)
        c8, s0, s1 = GATE_LIN[6]
        c = _solve_last(rng, s1, t2 - _cst_row(t.shape, c8 << 29) - s0 * a.astype(np.int64))
        return a, b, c
    c8, s0, s1 = GATE_LIN[op]
    tp = t - _cst_row(t.shape, c8 << 29)
    a = _random_words(rng, t.shape)
    if abs(s1) == 1:
        forced, ok = _confined_draw(rng, s0, s1, tp)
        a = np.where(ok & (rng.random(t.shape) < 0.5), forced, a)
    return wrap32(a), _solve_last(rng, s1, tp - s0 * a)


def exact_sum(op, ops_rows):
    """the linear stage of opcode op (0 .. 9, MAJ, XOR3) on the operand rows in exact integers (int64)"""
    rows = [np.asarray(x, np.int32).astype(np.int64) for x in ops_rows]
    if op in GATE_LIN3:
        return GATE_LIN3[op] * (rows[0] + rows[1] + rows[2])
    c8, s0, s1 = GATE_LIN[op]
    return s0 * rows[0] + s1 * rows[1] + _cst_row(rows[0].shape, c8 << 29)


def linear(op, ops_rows):
    """the same, wrapped to int32: what the kernels compute"""
    return wrap32(exact_sum(op, ops_rows))


def wrapped(exact):
    """mask of the words whose exact sum leaves [-2^31, 2^31)"""
    return (exact < INT32_MIN) | (exact > INT32_MAX)


def node_cst(which, seed):
    """the four constants of the node tests: INT32_MIN, -1, 2^29, a random word"""
    return (INT32_MIN, -1, 1 << 29, int(np.random.default_rng(seed).integers(INT32_MIN, INT32_MAX + 1)))[which % 4]


def node_weights(terms, seed):
    """terms - 1 weights of NODE_WEIGHTS (all five over a few seeds) and a last weight +-1"""
    rng = np.random.default_rng(seed)
    return [int(NODE_WEIGHTS[(seed + k) % len(NODE_WEIGHTS)]) for k in range(terms - 1)] + [int(rng.choice((-1, 1)))]


def solve_node(weights, cst, t_star, seed):
    """operand rows [terms] of a node sum_k w_k x_k + (0, ..., 0, cst) = t_star; the last weight is +1 or -1"""
    assert 1 <= len(weights) <= 4 and abs(int(weights[-1])) == 1
    rng = np.random.default_rng(seed)
    t = np.asarray(t_star, np.int32).astype(np.int64)
    xs = [_random_words(rng, t.shape) for _ in weights[:-1]]
    rest = t - _cst_row(t.shape, int(cst))
    for w, x in zip(weights, xs):
        rest = (rest - (int(w) * x & 0xFFFFFFFF)) & 0xFFFFFFFF    # every product fits int64: |w x| <= 2^62
    return [wrap32(x) for x in xs] + [_solve_last(rng, int(weights[-1]), rest)]


def node_exact(weights, cst, xs):
    """exact integer sum of a node in Python ints (object array: a product of two full-range words leaves int64)"""
    tot = _cst_row(np.asarray(xs[0]).shape, int(cst)).astype(object)
    for w, x in zip(weights, xs):
        tot = tot + int(w) * np.asarray(x, np.int32).astype(object)
    return tot


def node_linear(weights, cst, xs):
    """the wrapping sum, as tests/int_circuit_oracle.py::linear does it"""
    acc = np.zeros(np.asarray(xs[0]).shape, np.uint32)
    for w, x in zip(weights, xs):
        acc = acc + np.uint32(int(w) & 0xFFFFFFFF) * np.asarray(x, np.int32).view(np.uint32)
    acc[..., -1] += np.uint32(int(cst) & 0xFFFFFFFF)
    return acc.view(np.int32)


def free_gate_rows(n=260, rows=35, seed=5):
    """int32 [rows][n+1]: a third random words, the rest 0, -1, 1, INT32_MIN, INT32_MAX; every special value occurs in word 0,
    in word n - 1 and in word n (the b word)"""
    rng = np.random.default_rng(seed)
    special = np.array([0, -1, 1, INT32_MIN, INT32_MAX], np.int64)
    pick = rng.integers(0, 8, (rows, n + 1))
    out = np.where(pick < 5, special[np.minimum(pick, 4)], _random_words(rng, (rows, n + 1)))
    assert rows >= 15
    for j, col in enumerate((0, n - 1, n)):
        out[(np.arange(5) * 3 + j) % rows, col] = special
    return np.ascontiguousarray(wrap32(out))
