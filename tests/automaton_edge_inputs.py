"""Edge inputs for k_automaton_step (numpy only; shared by tests/test_automaton_edge_inputs_cpu.py and
tests/test_gpu_automaton_instances.py).

A step decomposes BOTH polynomials of X^(-w1) prev[next1] - X^(-w0) prev[next0]; pseudo-random state vectors meet neither a
rounding-cell end nor an all-end-digits word, and the weight is applied by index arithmetic twice, in the load phase and in
the store phase.  The automata made here put the named differences of leveled_edge_inputs.cmux_differences under the
decomposition THROUGH the two rotations, and every weight in [0, 2N) on both branches.  Nothing of the gadget is restated:
the differences, the alternating pair, the full-scale table and the constant selector are leveled_edge_inputs', the rotation
is automaton_oracle.successor.

  edge_automaton(l, Bgbit)    (trans, prev, names): states 2k / 2k + 1 decompose D_k / -D_k, every row D_k of cmux_differences,
                              under weight pairs that cycle through W_ALL x W_ALL; the alternating INT32_MIN / INT32_MAX pair
                              under the seven weight pairs of ALT_WEIGHTS.
  truncated(trans, prev, c)   the first c states made closed (an odd c ends in a self-loop); COUNTS are the counts to run.
  weight_sweep()              2 048 states: every weight once as w0 and once as w1, w0 != w1, no successor pair read twice.
  full_scale                  per k_automaton_step instance (l, Bgbit, K, [lo, hi)): leveled_edge_inputs.cmux_full_scale.
  full_scale_states(l, Bgbit) the digits_min and digits_max pairs of edge_automaton alone, a closed 4-state automaton: D and -D
                              of both rows.
"""
import numpy as np

import leveled_edge_inputs as lei
from automaton_oracle import successor
from leveled_edge_inputs import constant_selector  # noqa: F401  (re-used, not restated: the tests reach it here)

N = 1024
W_ALL = (0, 1, 63, 64, N - 1, N, N + 1, 2 * N - 1)
# the alternating pair is not derived from its difference (the subtraction itself must wrap), so its weights are listed:
# (0,0): the wrapping +-1 words; (N,0): all -1; (1,0): all 0 -- only because -INT32_MIN wraps at the turned coefficient;
# (0,1) and (2N-1,0): +-2 at exactly two coefficients
ALT_WEIGHTS = ((0, 0), (1, 0), (0, 1), (N, 0), (N + 1, 0), (2 * N - 1, 0), (63, 64))
# kCmuxItemsPerWG = 2: a dead pair in the only workgroup, a full workgroup, a dead pair in the last one, a longer odd grid;
# the tests add `all`
COUNTS = (1, 2, 3, 33)
full_scale = {name.replace("k_cmux", "k_automaton_step"): cfg for name, cfg in lei.cmux_full_scale.items()}


def weight_pair(k):
    """pair k of the walk through W_ALL x W_ALL: 11 is coprime to 64, so 64 consecutive k meet every pair once; the first
    16 (no gadget has fewer rows) meet every weight as w0 and as w1, and k = 4 is (1, 1).  k = 0 is (64, N): the zero row is turned too."""
    m = (11 * k + 29) % 64
    return W_ALL[m // 8], W_ALL[m % 8]


def derived_rows(l, Bgbit, extra=(), shift=0):
    """[(name, D_k)]: every row of cmux_differences but `alternating`, in the order edge_automaton lays the pairs out, then the
    rows of `extra` ((name, uint32 [2][N]) pairs); every word minus `shift`, wrapping (tests/leveled_round_cases.py: the
    rounding twins add it back)"""
    rows = [(f"{nm}[{i}]", row) for nm, D in lei.cmux_differences(l, Bgbit).items() if nm != "alternating"
            for i, row in enumerate(D)] + [(nm, np.asarray(row, np.uint32)) for nm, row in extra]
    return [(nm, lei._i32(row.astype(np.int64) - shift).view(np.uint32)) for nm, row in rows] if shift else rows


def _turn(poly, w):
    """X^w (c0, c1) as int32 words"""
    return successor(poly[None], 0, (2 * N - w) % (2 * N))


def edge_automaton(l, Bgbit, seed=0, extra=(), shift=0):
    """(trans [Q][4] int32, prev [Q][2][N] int32, names [Q]).  Pair k = states (2k, 2k + 1) holds (P0, P1) with
    X^(-w1) P1 - X^(-w0) P0 = D_k in wrapping arithmetic: P0 random full-range words, P1 = X^(w1) (D_k + X^(-w0) P0).
    State 2k = (2k, w0, 2k+1, w1) decomposes D_k, state 2k+1 = (2k+1, w1, 2k, w0) decomposes -D_k.  `seed` changes the random
    words only: the differences are the same.  `extra` and `shift`: derived_rows; the rows of `extra` follow the derived ones,
    ahead of the alternating pairs, and draw their random words after them."""
    rng = np.random.default_rng(17000 + 1000 * l + Bgbit + seed)
    trans, prev, names = [], [], []

    def pair(P0, P1, w0, w1, name):
        k = len(prev) // 2
        trans.extend([(2 * k, w0, 2 * k + 1, w1), (2 * k + 1, w1, 2 * k, w0)])
        prev.extend([P0, P1])
        names.extend([name, name + " negated"])

    for k, (name, D) in enumerate(derived_rows(l, Bgbit, extra, shift)):
        w0, w1 = weight_pair(k)
        P0 = lei._i32(rng.integers(-2**31, 2**31, (2, N)))
        P1 = _turn(lei._i32(D.astype(np.int64) + successor(P0[None], 0, w0)), w1)
        pair(P0, P1, w0, w1, name)
    a0, a1 = lei.cmux_inputs(l, Bgbit)["alternating"]
    for w0, w1 in ALT_WEIGHTS:
        pair(a0[0], a1[0], w0, w1, f"alternating({w0},{w1})")
    return np.array(trans, np.int32), np.ascontiguousarray(np.stack(prev), np.int32), names


def truncated(trans, prev, count):
    """(trans, prev) of the first `count` states, closed: an even count keeps whole pairs; an odd count replaces the last
    state, whose partner is cut off, by the self-loop (q, w, q, w') with w != w'"""
    trans = np.array(trans[:count], np.int32)
    if count & 1:
        q, w0, w1 = count - 1, int(trans[-1, 1]), int(trans[-1, 3])
        trans[-1] = (q, w0, q, w1 if w1 != w0 else (w0 + N + 1) % (2 * N))
    assert (trans[:, [0, 2]] < count).all()
    return trans, np.ascontiguousarray(prev[:count])


def weight_sweep(seed=0):
    """(trans [2048][4], prev [2048][2][N]): w0(q) = q, w1 a permutation of [0, 2N) of the other parity, next0 and next1
    permutations of the states (odd multipliers), so no two states read the same pair of successors"""
    q = np.arange(2 * N)
    trans = np.stack([(7 * q + 1) % (2 * N), q, (11 * q + 5) % (2 * N), (2 * N - 1 - q + N * (q & 1)) % (2 * N)], axis=1)
    prev = np.random.default_rng(17900 + seed).integers(-2**31, 2**31, (2 * N, 2, N))
    return trans.astype(np.int32), np.ascontiguousarray(lei._i32(prev))


def full_scale_states(l, Bgbit, seed=0, shift=0):
    """(trans [4][4], prev [4][2][N], names [4]): the digits_min and digits_max pairs of edge_automaton, renumbered"""
    trans, prev, names = edge_automaton(l, Bgbit, seed, shift=shift)
    keep = [q for q, nm in enumerate(names) if nm.startswith(("digits_min", "digits_max"))]
    assert len(keep) == 4
    new = {q: i for i, q in enumerate(keep)}
    t = np.array([(new[int(a)], w0, new[int(b)], w1) for a, w0, b, w1 in trans[keep]], np.int32)
    return t, np.ascontiguousarray(prev[keep]), [names[q] for q in keep]
