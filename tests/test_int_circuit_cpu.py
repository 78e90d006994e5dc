"""Integer circuits, host side (no GPU): the leveliser and its argument checks, the builders' plain evaluation, the range
and noise checker, and the linear stage + coarse mod switch restated in numpy.  GPU side: tests/test_gpu_int_circuit.py."""
import ctypes as C

import numpy as np
import pytest

import lut_many_oracle as lmo
from eoc_tfhe_amd import noise

EOC_ERR_ARG = -1


@pytest.fixture(scope="module")
def eoc(built_lib):
    import eoc_tfhe_amd
    return eoc_tfhe_amd


def node(eoc, T, out, tv, terms, cst=0, garbage=None):
    q = eoc.INode()
    q.n_tables, q.out, q.tv, q.n_terms, q.cst = T, out, tv, len(terms), cst
    for k in range(4):
        q.in_[k], q.w[k] = (garbage, garbage) if garbage is not None else (0, 0)
    for k, (w, x) in enumerate(terms):
        q.in_[k], q.w[k] = x, w
    return q


def levels_rc(eoc, nodes, n_wires, n_tv):
    arr = (eoc.INode * max(1, len(nodes)))(*nodes)
    lev = (C.c_int32 * max(1, len(nodes)))()
    boots = C.c_int64(-7)
    rc = eoc.lib().eoc_int_netlist_levels(C.addressof(arr), len(nodes), n_wires, n_tv, C.addressof(lev), C.addressof(boots))
    return rc, list(lev[:len(nodes)]), boots.value


def hand_written(eoc, garbage=None):
    """wires 0..2 inputs; levels written next to the nodes"""
    n = lambda *a, **k: node(eoc, *a, garbage=garbage, **k)
    return [
        n(1, 3, 0, [(1, 0)]),                        # level 1
        n(0, 4, 0, [(1, 0), (-1, 1)], cst=5),        # free, reads inputs only: pre-pass of level 1
        n(2, 5, 1, [(1, 4), (1, 2)]),                # level 1 (a free operand costs nothing): wires 5, 6
        n(0, 7, 0, [(2, 6), (1, 3)]),                # free behind level 1: pre-pass of level 2
        n(0, 8, 0, [(1, 7)]),                        # free behind a free node of the same pre-pass: still level 2
        n(1, 9, 0, [(1, 8), (1, 5), (1, 6)]),        # level 2: BOTH wires of the many-LUT node are there
        n(4, 10, 2, [(1, 9)]),                       # level 3: wires 10 .. 13
        n(0, 14, 0, [(1, 13), (1, 0)]),              # free behind the last level: the last pre-pass (level 4)
        n(0, 15, 0, [(1, 1)]),                       # free on an input: pre-pass of level 1
    ], 16, 3


def test_levels_of_a_hand_written_netlist(eoc):
    nodes, n_wires, n_tv = hand_written(eoc)
    rc, lev, boots = levels_rc(eoc, nodes, n_wires, n_tv)
    assert rc == 3 and boots == 4
    assert lev == [1, 1, 1, 2, 2, 2, 3, 4, 1]
    assert eoc.int_netlist_levels(nodes, n_wires, n_tv) == (lev, 3, 4)
    arr = (eoc.INode * len(nodes))(*nodes)
    assert eoc.lib().eoc_int_netlist_levels(C.addressof(arr), len(nodes), n_wires, n_tv, None, None) == 3
    assert eoc.lib().eoc_int_netlist_levels(None, 0, 0, 0, None, None) == 0


def test_garbage_in_unused_slots_is_ignored(eoc):
    for garbage in (-1, 2**31 - 1, -2**31, 99999):
        nodes, n_wires, n_tv = hand_written(eoc, garbage)
        rc, lev, boots = levels_rc(eoc, nodes, n_wires, n_tv)
        assert (rc, lev, boots) == (3, [1, 1, 1, 2, 2, 2, 3, 4, 1], 4), garbage


BAD = {
    "input wire out of range": lambda n: [n(1, 3, 0, [(1, 16)])],
    "negative input wire": lambda n: [n(1, 3, 0, [(1, 0), (1, -1)])],
    "output wire out of range": lambda n: [n(1, 16, 0, [(1, 0)])],
    "negative output wire": lambda n: [n(0, -1, 0, [(1, 0)])],
    "tv out of range": lambda n: [n(1, 3, 3, [(1, 0)])],
    "negative tv": lambda n: [n(2, 3, -1, [(1, 0)])],
    "no terms": lambda n: [n(1, 3, 0, [])],
    "five terms": lambda n: [n(1, 3, 0, [(1, 0)] * 5)],
    "three tables": lambda n: [n(3, 3, 0, [(1, 0)])],
    "sixteen tables": lambda n: [n(16, 0, 0, [(1, 0)])],
    "negative tables": lambda n: [n(-1, 3, 0, [(1, 0)])],
    "many-LUT outputs past the end": lambda n: [n(4, 13, 0, [(1, 0)])],
    "a wire written twice": lambda n: [n(1, 3, 0, [(1, 0)]), n(0, 3, 0, [(1, 1)])],
    "a wire written twice, inside a many-LUT range": lambda n: [n(4, 3, 0, [(1, 0)]), n(1, 5, 0, [(1, 1)])],
    "reads its own output": lambda n: [n(1, 3, 0, [(1, 3)])],
    "reads its own second output": lambda n: [n(2, 3, 0, [(1, 4)])],
    "reads a later node's output": lambda n: [n(1, 3, 0, [(1, 4)]), n(1, 4, 0, [(1, 0)])],
}


@pytest.mark.parametrize("case", sorted(BAD))
def test_malformed_netlists_are_refused(eoc, case):
    def n(T, out, tv, terms, cst=0):
        q = node(eoc, T, out, tv, terms[:4], cst)
        q.n_terms = len(terms)
        return q
    rc, _, _ = levels_rc(eoc, BAD[case](n), 16, 3)
    assert rc == EOC_ERR_ARG, case
    assert eoc.lib().eoc_last_error()
    with pytest.raises(eoc.EocError):
        eoc.int_netlist_levels(BAD[case](n), 16, 3)


def test_tables_without_polynomials_and_null_netlists_are_refused(eoc):
    q = node(eoc, 1, 3, 0, [(1, 0)])
    assert levels_rc(eoc, [q], 16, 0)[0] == EOC_ERR_ARG                       # n_tv = 0: every tv index is out of range
    assert levels_rc(eoc, [node(eoc, 0, 3, 77, [(1, 0)])], 16, 0)[0] == 0     # a free node's tv is ignored
    assert eoc.lib().eoc_int_netlist_levels(None, 3, 16, 3, None, None) == EOC_ERR_ARG


def test_2000_random_malformed_netlists_return(eoc):
    rng = np.random.default_rng(2024)
    L = eoc.lib()
    seen = set()
    for _ in range(2000):
        n_nodes, n_wires, n_tv = int(rng.integers(0, 12)), int(rng.integers(0, 20)), int(rng.integers(0, 4))
        raw = rng.integers(-3, 24, (max(1, n_nodes), C.sizeof(eoc.INode) // 4)).astype(np.int32)
        if rng.integers(0, 4) == 0:
            raw[rng.integers(0, raw.shape[0]), rng.integers(0, raw.shape[1])] = rng.integers(-2**31, 2**31)
        lev = np.zeros(max(1, n_nodes), np.int32)
        boots = C.c_int64(0)
        rc = L.eoc_int_netlist_levels(raw.ctypes.data, n_nodes, n_wires, n_tv, lev.ctypes.data, C.addressof(boots))
        assert rc == EOC_ERR_ARG or 0 <= rc <= n_nodes, rc
        if rc >= 0:
            assert 0 <= boots.value <= n_nodes and (n_nodes == 0 or (lev[:n_nodes] >= 1).all())
        seen.add(rc >= 0)
    assert seen == {True, False}                                              # both outcomes occur in the sample


def test_run_device_without_an_engine_is_an_argument_error(eoc):
    nodes, n_wires, n_tv = hand_written(eoc)
    arr = (eoc.INode * len(nodes))(*nodes)
    buf = np.zeros(8, np.int32)
    L = eoc.lib()
    assert L.eoc_int_circuit_run_device(None, C.addressof(arr), len(nodes), buf.ctypes.data, n_tv, buf.ctypes.data,
                                        n_wires, 1, None) == EOC_ERR_ARG
    assert L.eoc_int_circuit_run_device(None, None, 0, None, 0, None, 0, 0, None) == EOC_ERR_ARG


# ---- builders ------------------------------------------------------------------------------------------------------------
def digits(x, n):
    return [(x >> i) & 1 for i in range(n)]


def test_radix_add_plain_exhaustive_at_3_digits(eoc):
    c = eoc.IntCircuit()
    A = [c.input(4, 1) for _ in range(3)]
    B = [c.input(4, 1) for _ in range(3)]
    S, carry = eoc.radix_add(c, A, B)
    x = np.arange(64)
    a, b = x & 7, x >> 3
    v = c.evaluate_plain(digits(a, 3) + digits(b, 3))
    assert np.array_equal(sum(v[w] << i for i, w in enumerate(S + [carry])), a + b)
    lev, nlev, boots = c.levels()
    assert (nlev, boots) == (3, 3) and lev == [1, 2, 3]                       # n bootstraps on n levels
    assert all(q.n_tables == 2 for q in c.nodes())
    # with a carry in: 2^7 cases
    c = eoc.IntCircuit()
    A = [c.input(4, 1) for _ in range(3)]
    B = [c.input(4, 1) for _ in range(3)]
    k = c.input(4, 1)
    S, carry = eoc.radix_add(c, A, B, carry_in=k)
    x = np.arange(128)
    a, b, ci = x & 7, (x >> 3) & 7, x >> 6
    v = c.evaluate_plain(digits(a, 3) + digits(b, 3) + [ci])
    assert np.array_equal(sum(v[w] << i for i, w in enumerate(S + [carry])), a + b + ci)


def test_bit_function2_all_16_functions(eoc):
    for code in range(16):
        f = lambda a, b, code=code: (code >> (2 * a + b)) & 1
        c = eoc.IntCircuit()
        a, b = c.input(4, 1), c.input(4, 1)
        out = eoc.bit_function2(c, a, b, f)
        v = c.evaluate_plain([np.array([0, 0, 1, 1]), np.array([0, 1, 0, 1])])
        assert list(v[out]) == [f(0, 0), f(0, 1), f(1, 0), f(1, 1)], code
        assert c.levels()[1:] == (1, 1)


def test_radix_less_than_plain_exhaustive_at_3_digits(eoc):
    c = eoc.IntCircuit()
    A = [c.input(4, 1) for _ in range(3)]
    B = [c.input(4, 1) for _ in range(3)]
    lt = eoc.radix_less_than(c, A, B)
    x = np.arange(64)
    a, b = x & 7, x >> 3
    v = c.evaluate_plain(digits(a, 3) + digits(b, 3))
    assert np.array_equal(v[lt], (a < b).astype(np.int64))
    assert c.levels()[1:] == (3, 3)


def test_plain_evaluation_of_the_padding_half_negates(eoc):
    c = eoc.IntCircuit()
    a = c.input(4)
    b = c.input(4)
    out = c.lut([a, b], lambda m: m + 1, 4, 4, allow_padding=True)            # a + b reaches 6: [4, 8) is -f(m - 4)
    v = c.evaluate_plain([np.array([1, 3, 3]), np.array([1, 1, 3])])
    assert list(v[out]) == [3, 8 - 1, 8 - 3]                                  # phases in eighths: -f is the step 2p - f
    assert list(v[out] % 4) == [3, (-(0 + 1)) % 4, (-(2 + 1)) % 4]            # what decrypt_ints reads
    assert c.check(eoc.default_params(0), np.ones(630, np.int32), np.ones(1024, np.int32))["nodes"][0][0] is False


# ---- the checker ---------------------------------------------------------------------------------------------------------
def test_range_checker(eoc):
    c = eoc.IntCircuit()
    a, b, k, d = (c.input(4, 1) for _ in range(4))
    c.lut([a, b, k], lambda m: m, 4, 4)                                       # a + b + c <= 3 at p = 4
    with pytest.raises(ValueError, match=r"node 1 .*\[0, 4\].*\[0, 3\]"):
        c.lut([a, b, k, d], lambda m: m, 4, 4)                                # a fourth unit term: 4 > p - 1
    assert len(c.nodes()) == 1                                                # the refused node was not recorded
    c.lut([a, b, k, d], lambda m: m, 4, 4, allow_padding=True)
    with pytest.raises(ValueError, match="node 2"):
        c.lut([(1, a), (-1, b)], lambda m: m, 4, 4)                           # a - b reaches -1
    c.lut([(1, a), (-1, b)], lambda m: m, 4, 4, cst=eoc.int_circuits.units(1, 4))         # a - b + 1 in [0, 2]
    with pytest.raises(ValueError, match="node 3"):
        c.lut([(1, a), (-1, b)], lambda m: m, 4, 4, cst=eoc.int_circuits.units(3, 4))     # a - b + 3 reaches 4
    with pytest.raises(ValueError, match="share p"):
        c.lut([a, c.input(8, 1)], lambda m: m, 4, 4)
    # a table's output bound is max f over the input interval
    w = c.lut([a, b], lambda m: [0, 1, 1, 3][m], 4, 4)                        # a + b in [0, 2]: f <= 1
    assert c.wire_range(w) == (4, 0, 1)
    c.lut([w, w, w], lambda m: m, 4, 4)                                       # 3 w <= 3
    free = c.lin([(1, a), (-1, b)], cst=eoc.int_circuits.units(1, 4))
    assert c.wire_range(free) == (4, 0, 2)
    with pytest.raises(ValueError):
        c.lut([free, free], lambda m: m, 4, 4)                                # 2 (a - b + 1) reaches 4


@pytest.mark.parametrize("pset", [0, 1], ids=["setA", "setB"])
def test_noise_checker(eoc, pset):
    P = eoc.default_params(pset)
    sk = eoc.SecretKey(P, 1, with_cloud_key=False)
    keys = (P, sk.lwe_key, sk.tlwe_key)
    v_out = noise.predict(*keys)["total_var"]
    c = eoc.IntCircuit()
    A = [c.input(4, 1) for _ in range(2)]
    B = [c.input(4, 1) for _ in range(2)]
    eoc.radix_add(c, A, B)
    chk = c.check(*keys)
    want = noise.lut_margin_sigma(*keys, 4, 2, inputs=3)
    assert chk["nodes"][1][0] is True and abs(chk["nodes"][1][1] / want - 1) < 1e-12
    assert abs(chk["nodes"][0][1] / noise.lut_margin_sigma(*keys, 4, 2, inputs=2) - 1) < 1e-12
    assert chk["worst"] == 1 and chk["worst_sigma"] == chk["nodes"][1][1]
    assert abs(noise.lut_margin_sigma_var(4, 2, 3 * v_out, sk.lwe_key) / want - 1) < 1e-12
    # 2a + b: sum of w^2 = 5
    c = eoc.IntCircuit()
    a, b = c.input(4, 1), c.input(4, 1)
    eoc.bit_function2(c, a, b, lambda x, y: x ^ y)
    formula = (1 / 16) / np.sqrt(5 * v_out + noise.modswitch_var(sk.lwe_key, 1))
    assert abs(c.check(*keys)["nodes"][0][1] / formula - 1) < 1e-12
    # a fresh input carries ks_stdev^2, a free node sum w^2 V
    c = eoc.IntCircuit()
    a, b = c.input(4, 1, fresh=True), c.input(4, 1)
    f = c.lin([(2, a), (-1, b)], cst=eoc.int_circuits.units(1, 4))
    c.lut([f], lambda m: m, 4, 4)
    chk = c.check(*keys)
    v_free = 4 * float(P.ks_stdev) ** 2 + v_out
    assert abs(chk["wire_var"][f] / v_free - 1) < 1e-12
    assert abs(chk["nodes"][1][1] / noise.lut_margin_sigma_var(4, 1, v_free, sk.lwe_key) - 1) < 1e-12
    # the base-4 adder digit at p = 8, T = 2 sums three inputs: below the weakest shape DESIGN.md 10.1 supports
    c = eoc.IntCircuit()
    a, b, k = c.input(8, 3), c.input(8, 3), c.input(8, 1)
    c.lut_many([a, b, k], [lambda m: m % 4, lambda m: m // 4], 8, 8)
    ok, sigma = c.check(*keys)["nodes"][0]
    assert ok and sigma < noise.lut_margin_sigma(*keys, 8, 2, inputs=2)
    with pytest.raises(ValueError, match="min_sigma"):
        c.run({}, min_sigma=sigma + 0.01, params=P, lwe_key=sk.lwe_key, tlwe_key=sk.tlwe_key)


def test_linear_stage_and_coarse_modswitch_in_numpy(eoc):
    """k_lin_modswitch's arithmetic restated: wrapping weighted sum, constant on the last word, rounding onto the 2^theta-grid
    = lut_many_oracle.modswitch_coarse of the numpy sum"""
    rng = np.random.default_rng(7)
    n = 630
    rows = rng.integers(-2**31, 2**31, (4, 5, n + 1)).astype(np.int32)
    for theta in range(4):
        for terms in range(1, 5):
            w = rng.integers(-3, 4, terms)
            cst = int(rng.integers(-2**31, 2**31))
            t = np.zeros((5, n + 1), np.uint32)
            for k in range(terms):
                t = t + np.uint32(int(w[k]) & 0xFFFFFFFF) * rows[k].view(np.uint32)               # uint32 arithmetic wraps
            t[:, n] += np.uint32(cst & 0xFFFFFFFF)
            bara = (((t + np.uint32(1 << (20 + theta))) >> np.uint32(21 + theta)) << np.uint32(theta)) & np.uint32(2047)
            exact = sum(int(w[k]) * rows[k].astype(np.int64) for k in range(terms))
            exact[:, n] += cst
            assert np.array_equal(bara.astype(np.int32), lmo.modswitch_coarse(exact, 1 << theta)), (theta, terms)


def test_bit_out_nodes(eoc):
    """bit_out tables hold +-2^29 (a gate sample); plain evaluation gives the bit, flipped on the padding half; such a wire
    is no operand of an integer node"""
    c = eoc.IntCircuit()
    a, b = c.input(4), c.input(4, 1)
    one = c.lut_bit_out([a], lambda m: m >= 2, 4)
    many = c.lut_many_bit_out([a, b], [lambda m: m % 2, lambda m: m == 3], 4, allow_padding=True)
    tabs = c.tables()
    assert tabs[0].tolist() == [[-2**29, -2**29, 2**29, 2**29]]
    assert tabs[1].tolist() == [[-2**29, 2**29, -2**29, 2**29], [-2**29, -2**29, -2**29, 2**29]]
    assert [q.n_tables for q in c.nodes()] == [1, 2] and c.wire_range(one)[0] == "bit"
    v = c.evaluate_plain([np.array([0, 1, 2, 3, 3]), np.array([0, 0, 0, 0, 1])])
    assert list(v[one]) == [0, 0, 1, 1, 1]
    assert list(v[many[0]]) == [0, 1, 0, 1, 1 - 0]            # 3 + 1 = 4: the padding half, -f(0)
    assert list(v[many[1]]) == [0, 0, 0, 1, 1 - 0]
    with pytest.raises(ValueError, match="bit_out"):
        c.lut([one], lambda m: m, 4, 4)
    with pytest.raises(ValueError):
        c.lut_many_bit_out([a], [lambda m: m], 4)               # one function: lut_bit_out
