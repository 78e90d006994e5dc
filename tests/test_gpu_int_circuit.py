"""Integer circuits on the MI355X: eoc_int_circuit_run_device against the CPU oracle (tests/int_circuit_oracle.py) byte for
byte -- a mixed two-level circuit on both sets and both rotation-amount read-back forms, radix_add, a wide level with a pair
remainder inside a node's rows, a ragged last slice, the global context, argument errors, and the existing table-lookup and
gate paths around an integer-circuit call.  Host side: tests/test_int_circuit_cpu.py.

Decrypt assertions are limited to wires behind nodes that IntCircuit.check prices at >= 6 sigma (two-sided tail 2e-9 per
lookup, fewer than 1e4 lookups in this file); bit-exactness against the oracle is asserted for every wire."""
import ctypes as C

import numpy as np
import pytest

import int_circuit_oracle as ico
import lut_oracle as lo
import oracle_lib as ol
from gpu_util import dev_empty, sync, to_dev, torch_cuda

pytestmark = pytest.mark.gpu
N = 1024
EOC_ERR_ARG = -1
MIN_SIGMA = 6.0


@pytest.fixture(scope="module")
def eoc(built_lib):
    torch_cuda()
    import eoc_tfhe_amd
    return eoc_tfhe_amd


_KEYS = {}


def keys(eoc, pset, seed=1):
    if (pset, seed) not in _KEYS:
        p = eoc.default_params(pset)
        _KEYS[(pset, seed)] = (p, eoc.SecretKey(p, seed), ol.Oracle(pset, seed))
    return _KEYS[(pset, seed)]


def engine(eoc, monkeypatch, pset, readback="default", slice_rows=None):
    if readback == "scalar-abar":
        monkeypatch.setenv("EOC_TFHE_SCALAR_ABAR", "1")       # read at engine creation: the SABAR instances
    if slice_rows:
        monkeypatch.setenv("EOC_TFHE_INT_SLICE_ROWS", str(slice_rows))
    params, sk, orc = keys(eoc, pset)
    eng = eoc.Engine(params)
    eng.load_cloud_key(sk)
    return params, sk, orc, eng


def inputs(eoc, sk, p, rows, enc_seed, shift=0):
    """as test_gpu_lut_many.py::inputs: rows cycling through every m in Z_p and, every fourth row, a padding-half phase m in
    [p, 2p); `shift` moves the cycle so that the wires of one circuit differ"""
    m = (np.arange(rows) + shift) % (2 * p)
    m[np.arange(rows) % 4 != 3] %= p
    cts = np.empty((rows, sk.n + 1), np.int32)
    for r in range(rows):
        mu = np.int64((int(m[r]) << 32) // (2 * p)).astype(np.uint32).view(np.int32)
        assert eoc.lib().eoc_lwe_encrypt(sk.h, enc_seed, r, int(mu), sk.params.ks_stdev, cts[r].ctypes.data) == 0
    return m, cts


def mixed_circuit(eoc):
    """two levels: level 1 = three T = 1 nodes (one term; weights (2, 1); three unit terms and a constant) and a T = 2 node;
    level 2 = a T = 1 node on two level-1 outputs, a T = 4 node, a T = 1 node behind two chained free nodes (x - y + cst over
    a level-1 output and an input, then a free node on that one: two launches of one pre-pass) and a bit_out node; last, a free
    node nobody reads.  Inputs carry every phase, the padding half included, so
    the nodes whose declared range leaves [0, p - 1] are built with allow_padding."""
    u = eoc.int_circuits.units
    c = eoc.IntCircuit()
    x = [c.input(4, fresh=True) for _ in range(4)]
    n1 = c.lut([x[0]], lambda m: (3 * m + 1) % 4, 4, 4)
    n2 = c.lut([(2, x[0]), (1, x[1])], lambda m: (m + 2) % 4, 4, 4, allow_padding=True)
    n3 = c.lut([x[1], x[2], x[3]], lambda m: [1, 0, 0, 1][m], 4, 4, cst=u(1, 4), allow_padding=True)
    n4 = c.lut_many([x[2]], [lambda m: m % 2, lambda m: m // 2], 4, 4)
    n5 = c.lut([n1, n2], lambda m: 3 - m, 4, 4, allow_padding=True)
    n6 = c.lut_many([n3], [lambda m: m, lambda m: (m + 1) % 4, lambda m: (2 * m) % 4, lambda m: 3 - m], 4, 4)
    f7 = c.lin([(1, n4[0]), (-1, x[3])], cst=u(3, 4))
    f7b = c.lin([(1, f7), (2, n4[1])], cst=u(1, 4))           # reads a free node of its own pre-pass
    n8 = c.lut([f7b], lambda m: (m + 3) % 4, 4, 4, allow_padding=True)
    nb = c.lut_bit_out([n1], lambda m: m >= 2, 4)             # +-1/8: a gate sample
    f9 = c.lin([(1, n5), (2, n6[0])], cst=u(1, 4))
    groups = 4                                                # (1, T=1), (1, T=2), (2, T=1), (2, T=4)
    return c, x, groups, dict(n1=n1, n2=n2, n3=n3, n4=n4, n5=n5, n6=n6, f7=f7, f7b=f7b, n8=n8, nb=nb, f9=f9)


def circuit_inputs(eoc, sk, c, x, rows, seed):
    ms, wires = [], np.zeros((c.n_wires, rows, sk.n + 1), np.int32)
    for k, w in enumerate(x):
        m, wires[w] = inputs(eoc, sk, 4, rows, seed + k, shift=3 * k)
        ms.append(m)
    return ms, wires


def run_device(eoc, eng, c, wires):
    d_tv, d_w = to_dev(c.test_polynomials()), to_dev(wires)
    eng.int_circuit_run_device(c.nodes(), d_tv.data_ptr(), d_tv.shape[0], d_w.data_ptr(), wires.shape[0], wires.shape[1])
    sync()
    return d_w.cpu().numpy()


def trusted_wires(c, chk, min_sigma=MIN_SIGMA):
    """wires whose value rests only on lookups priced at min_sigma or more (inputs and free nodes add no decision)"""
    ok = [True] * c.n_wires
    for k, q in enumerate(c.nodes()):
        good = all(ok[q.in_[a]] for a in range(q.n_terms)) and (q.n_tables == 0 or chk["nodes"][k][1] >= min_sigma)
        for w in c.node_outputs(k):
            ok[w] = good
    return ok


def assert_decrypts(sk, c, got, plain, ok, p=4):
    checked = 0
    for k in range(len(c.nodes())):
        for w in c.node_outputs(k):
            if ok[w]:
                bit = c.wire_range(w)[0] == "bit"
                dec = sk.decrypt_bits(got[w]) if bit else sk.decrypt_ints(got[w], p)
                want = np.asarray(plain[w]) % (2 if bit else p)
                assert np.array_equal(dec, want), (w, np.flatnonzero(dec != want)[:8])
                checked += 1
    return checked


_REF = {}


def mixed_reference(eoc, pset, rows=16):
    """the mixed circuit's inputs and its oracle result, once per parameter set"""
    if pset not in _REF:
        params, sk, orc = keys(eoc, pset)
        c, x, groups, names = mixed_circuit(eoc)
        ms, wires = circuit_inputs(eoc, sk, c, x, rows, 9800)
        ref = ico.run(orc, c.nodes(), c.test_polynomials(), wires)
        ref.setflags(write=False)
        _REF[pset] = (ms, wires, ref)
    return _REF[pset]


@pytest.mark.parametrize("readback", ["default", "scalar-abar"])
@pytest.mark.parametrize("pset", [0, 1], ids=["setA", "setB"])
def test_mixed_two_level_circuit_bit_exact(eoc, monkeypatch, pset, readback):
    """16 instances.  One blind rotation per (level, T) group -- one launch on Set A; on Set B every blind rotation is two
    launches (the step range is cut in two through acc_state, as test_gpu_lut_many.py asserts for its levels).
    check: every node is at 6 sigma or more on Set A; on Set B the T = 4 node at p = 4 is at 5.92 sigma (DESIGN.md 10.1's
    table: 5.9), so its four outputs and the free node behind them are compared with the oracle only."""
    params, sk, orc, eng = engine(eoc, monkeypatch, pset, readback)
    c, x, groups, names = mixed_circuit(eoc)
    ms, wires, ref = mixed_reference(eoc, pset)
    rows = wires.shape[1]
    lev, nlev, boots = c.levels()
    assert (nlev, boots) == (2, 8) and lev == [1, 1, 1, 1, 2, 2, 2, 2, 2, 2, 3]
    before = eng.stats()
    got = run_device(eoc, eng, c, wires)
    st = eng.stats()
    parts = 1 if pset == 0 else 2
    assert st["br_launches"] - before["br_launches"] == groups * parts
    assert st["br_wide_launches"] == before["br_wide_launches"]
    assert st["bootstraps"] - before["bootstraps"] == 8 * rows            # nodes x rows
    assert st["keyswitches"] - before["keyswitches"] == (6 + 2 + 4) * rows  # output slots x rows
    for w in range(c.n_wires):
        assert np.array_equal(got[w], ref[w]), w
    chk = c.check(params, sk.lwe_key, sk.tlwe_key)
    for k, (range_ok, sigma) in chk["nodes"].items():
        print(f"pset {pset} node {k}: range_ok {range_ok}, margin {sigma:.2f} sigma")
    below = [k for k, (_, sigma) in chk["nodes"].items() if sigma < MIN_SIGMA]
    assert below == ([] if pset == 0 else [5]), below
    ok = trusted_wires(c, chk)
    plain = c.evaluate_plain(ms)
    assert assert_decrypts(sk, c, got, plain, ok) == (15 if pset == 0 else 10)
    eng.close()


@pytest.mark.parametrize("pset", [0, 1], ids=["setA", "setB"])
def test_radix_add_four_digits(eoc, monkeypatch, pset):
    """4 digits x 16 instances: four levels, one blind rotation each; every written wire equals the oracle, all sums decrypt"""
    params, sk, orc, eng = engine(eoc, monkeypatch, pset)
    c = eoc.IntCircuit()
    A = [c.input(4, 1, fresh=True) for _ in range(4)]
    B = [c.input(4, 1, fresh=True) for _ in range(4)]
    S, carry = eoc.radix_add(c, A, B)
    assert c.levels()[1:] == (4, 4)
    rows = 16
    rng = np.random.default_rng(31)
    a, b = rng.integers(0, 16, rows), rng.integers(0, 16, rows)
    a[:2], b[:2] = [15, 0], [15, 0]
    wires = np.zeros((c.n_wires, rows, sk.n + 1), np.int32)
    for i in range(4):
        wires[A[i]] = sk.encrypt_ints(((a >> i) & 1).astype(np.uint8), 4, 9900 + i)
        wires[B[i]] = sk.encrypt_ints(((b >> i) & 1).astype(np.uint8), 4, 9910 + i)
    before = eng.stats()
    got = run_device(eoc, eng, c, wires)
    st = eng.stats()
    assert st["br_launches"] - before["br_launches"] == 4 * (1 if pset == 0 else 2)
    assert st["bootstraps"] - before["bootstraps"] == 4 * rows and st["keyswitches"] - before["keyswitches"] == 8 * rows
    ref = ico.run(orc, c.nodes(), c.test_polynomials(), wires)
    for w in range(c.n_wires):
        assert np.array_equal(got[w], ref[w]), w
    assert c.check(params, sk.lwe_key, sk.tlwe_key)["worst_sigma"] >= MIN_SIGMA
    total = np.zeros(rows, np.int64)
    for i, w in enumerate(S + [carry]):
        total |= sk.decrypt_ints(got[w], 4).astype(np.int64) << i
    assert np.array_equal(total, a + b), np.flatnonzero(total != a + b)[:8]
    eng.close()


def test_set_a_wide_level_and_pair_remainder_inside_a_node(eoc, monkeypatch):
    """one level of three T = 1 nodes x 700 instances = 2 100 jobs: one full wide launch (8 x CUs) and a pair-kernel remainder
    whose first job lies inside node 2's rows (as test_set_a_wide_and_pair_remainder_inside_a_polynomial).  Every row
    decrypts; the rows on both sides of the cut and the first four rows of every node equal the oracle byte for byte"""
    params, sk, orc, eng = engine(eoc, monkeypatch, 0)
    c = eoc.IntCircuit()
    x = [c.input(4, fresh=True) for _ in range(3)]
    outs = [c.lut([x[0]], lambda m: (m + 1) % 4, 4, 4),
            c.lut([(2, x[0]), (1, x[1])], lambda m: (3 * m) % 4, 4, 4, allow_padding=True),
            c.lut([x[0], x[1], x[2]], lambda m: 3 - m, 4, 4, allow_padding=True)]
    rows = 700
    ms, wires = circuit_inputs(eoc, sk, c, x, rows, 9950)
    jobs, Rw = 3 * rows, eng.resident_jobs()
    n_wide, rem = divmod(jobs, Rw)
    assert n_wide >= 1 and 0 < rem <= Rw // 2 and (n_wide * Rw) % rows != 0, (jobs, Rw)
    before = eng.stats()
    got = run_device(eoc, eng, c, wires)
    st = eng.stats()
    assert st["br_wide_launches"] - before["br_wide_launches"] == n_wide
    assert st["br_launches"] - before["br_launches"] == n_wide + 1
    assert st["bootstraps"] - before["bootstraps"] == jobs and st["keyswitches"] - before["keyswitches"] == jobs
    chk = c.check(params, sk.lwe_key, sk.tlwe_key)
    assert chk["worst_sigma"] >= MIN_SIGMA
    assert assert_decrypts(sk, c, got, c.evaluate_plain(ms), trusted_wires(c, chk)) == 3
    g_cut, r_cut = divmod(n_wide * Rw, rows)
    assert g_cut == 2
    side = np.r_[0:4, r_cut - 6:r_cut + 6]
    ref = ico.run(orc, c.nodes(), c.test_polynomials(), wires[:, side])
    for w in outs:
        assert np.array_equal(got[w][side], ref[w]), w
    eng.close()


def test_slice_boundary_ragged_last_slice(eoc, monkeypatch):
    """the mixed circuit on 40 instances in slices of 16 rows (EOC_TFHE_INT_SLICE_ROWS: 16 + 16 + 8) equals the unsliced run
    byte for byte; the first 16 rows are the oracle-checked ones of the first test"""
    params, sk, orc = keys(eoc, 0)
    c, x, groups, names = mixed_circuit(eoc)
    ms16, wires16, ref16 = mixed_reference(eoc, 0)
    ms, wires = circuit_inputs(eoc, sk, c, x, 40, 9800)
    assert np.array_equal(wires[:, :16], wires16)
    _, _, _, whole = engine(eoc, monkeypatch, 0)
    _, _, _, sliced = engine(eoc, monkeypatch, 0, slice_rows=16)
    monkeypatch.delenv("EOC_TFHE_INT_SLICE_ROWS")
    a = run_device(eoc, whole, c, wires)
    before = sliced.stats()
    b = run_device(eoc, sliced, c, wires)
    st = sliced.stats()
    assert st["br_launches"] - before["br_launches"] == 3 * groups            # three slices
    assert whole.stats()["br_launches"] == groups
    assert st["bootstraps"] - before["bootstraps"] == 8 * 40 and st["keyswitches"] - before["keyswitches"] == 12 * 40
    assert np.array_equal(a, b)
    assert np.array_equal(a[:, :16], ref16)
    chk = c.check(params, sk.lwe_key, sk.tlwe_key)
    assert assert_decrypts(sk, c, b, c.evaluate_plain(ms), trusted_wires(c, chk)) == 15
    whole.close()
    sliced.close()


def bad_netlists(eoc):
    def node(T, out, tv, terms):
        q = eoc.INode()
        q.n_tables, q.out, q.tv, q.n_terms = T, out, tv, len(terms)
        for k, x in enumerate(terms[:4]):
            q.in_[k], q.w[k] = x, 1
        return q
    return {
        "input wire out of range": [node(1, 4, 0, [99])],
        "output wire out of range": [node(1, 99, 0, [0])],
        "tv out of range": [node(1, 4, 9, [0])],
        "no terms": [node(1, 4, 0, [])],
        "five terms": [node(1, 4, 0, [0, 1, 2, 3, 0])],
        "three tables": [node(3, 4, 0, [0])],
        "many-LUT outputs past the end": [node(4, 10, 0, [0])],
        "a wire written twice": [node(1, 4, 0, [0]), node(0, 4, 0, [1])],
        "reads its own output": [node(1, 4, 0, [4])],
        "reads a later node's output": [node(1, 4, 0, [5]), node(1, 5, 0, [0])],
    }


def test_global_context_cloud_key_only_and_argument_errors(eoc, monkeypatch):
    params, sk, orc, eng = engine(eoc, monkeypatch, 0)
    c, x, groups, names = mixed_circuit(eoc)
    ms, wires, ref = mixed_reference(eoc, 0)
    dev = run_device(eoc, eng, c, wires)
    L = eoc.lib()
    # engine layer: malformed netlists and null pointers are refused before anything runs
    torch = torch_cuda()
    d_tv, d_w = to_dev(c.test_polynomials()), dev_empty((12, 4, params.n + 1), torch.int32)
    before = eng.stats()
    for name, nodes in bad_netlists(eoc).items():
        arr = (eoc.INode * len(nodes))(*nodes)
        assert L.eoc_int_circuit_run_device(eng.h, C.addressof(arr), len(nodes), d_tv.data_ptr(), d_tv.shape[0],
                                            d_w.data_ptr(), 12, 4, None) == EOC_ERR_ARG, name
    good = (eoc.INode * len(c.nodes()))(*c.nodes())
    assert L.eoc_int_circuit_run_device(eng.h, None, 3, d_tv.data_ptr(), 1, d_w.data_ptr(), 12, 4, None) == EOC_ERR_ARG
    assert L.eoc_int_circuit_run_device(eng.h, C.addressof(good), len(c.nodes()), None, d_tv.shape[0], d_w.data_ptr(),
                                        c.n_wires, 4, None) == EOC_ERR_ARG
    assert L.eoc_int_circuit_run_device(eng.h, C.addressof(good), len(c.nodes()), d_tv.data_ptr(), d_tv.shape[0], None,
                                        c.n_wires, 4, None) == EOC_ERR_ARG
    assert L.eoc_int_circuit_run_device(eng.h, C.addressof(good), len(c.nodes()), d_tv.data_ptr(), d_tv.shape[0],
                                        d_w.data_ptr(), c.n_wires, 0, None) == 0                  # no instance: a no-op
    assert eng.stats() == before
    nokey = eoc.Engine(params)
    assert L.eoc_int_circuit_run_device(nokey.h, C.addressof(good), len(c.nodes()), d_tv.data_ptr(), d_tv.shape[0],
                                        d_w.data_ptr(), c.n_wires, 4, None) == -4                 # EOC_ERR_NO_KEY
    nokey.close()
    eng.close()
    try:
        eoc.gpu_shutdown()
        bk, ksk = np.ascontiguousarray(sk.bk), np.ascontiguousarray(sk.ksk)
        eoc.gpu_init(params, devices=[0, 0])                      # two engines on one device: two blocks of instances
        assert L.eoc_upload_cloud_key_arrays(bk.ctypes.data, ksk.ctypes.data) == 0
        assert eoc.global_key_mode() == 0
        assert np.array_equal(eoc.int_circuit_run(c.nodes(), c.tables(), wires), dev)
        assert np.array_equal(c.run(dict(zip(x, wires[x]))), dev)
        tabs = np.zeros(64, np.int32)
        ps, Ts = np.array([4] * 3, np.int32), np.array([1] * 3, np.int32)
        host = np.zeros((12, 4, params.n + 1), np.int32)
        call = lambda arr, n, tb, pp, tt, n_tv, w: L.eoc_int_circuit_run(
            arr, n, None if tb is None else tb.ctypes.data, None if pp is None else pp.ctypes.data,
            None if tt is None else tt.ctypes.data, n_tv, None if w is None else w.ctypes.data, 12, 4)
        for name, nodes in bad_netlists(eoc).items():
            arr = (eoc.INode * len(nodes))(*nodes)
            assert call(C.addressof(arr), len(nodes), tabs, ps, Ts, 3, host) == EOC_ERR_ARG, name
        one = bad_netlists(eoc)["tv out of range"]
        one[0].tv = 0
        arr = (eoc.INode * 1)(*one)
        assert call(C.addressof(arr), 1, tabs, ps, Ts, 3, None) == EOC_ERR_ARG
        assert call(C.addressof(arr), 1, None, ps, Ts, 3, host) == EOC_ERR_ARG
        assert call(None, 1, tabs, ps, Ts, 3, host) == EOC_ERR_ARG
        assert call(C.addressof(arr), 1, tabs, np.array([3, 4, 4], np.int32), Ts, 3, host) == EOC_ERR_ARG     # p = 3
        assert call(C.addressof(arr), 1, tabs, ps, np.array([2, 1, 1], np.int32), 3, host) == EOC_ERR_ARG     # node T != entry T
        assert call(C.addressof(arr), 1, tabs, np.array([8, 4, 4], np.int32), np.array([4, 1, 1], np.int32), 3,
                    host) == EOC_ERR_ARG                                                                       # p T = 32
        assert eoc.stats()["bootstraps"] == 2 * 8 * wires.shape[1]                # nothing ran for the refused calls
    finally:
        eoc.gpu_shutdown()


def test_existing_paths_give_the_same_bytes_around_an_integer_circuit(eoc, monkeypatch):
    """eoc_lut_batch_device, eoc_lut_many_batch_device and a 64-gate NAND batch before and after an integer-circuit call on
    the same engine: the workspace (descriptor ring, mixed-batch area, rotation amounts) is shared"""
    torch = torch_cuda()
    params, sk, orc, eng = engine(eoc, monkeypatch, 0)
    c, x, groups, names = mixed_circuit(eoc)
    ms, wires, ref = mixed_reference(eoc, 0)
    rows = 64
    cts = to_dev(sk.encrypt_ints((np.arange(rows) % 4).astype(np.uint8), 4, 9990))
    tv1 = to_dev(np.stack([eoc.lut_test_polynomial(4, lo.int_table(lambda m: (m + k) % 4, 4, 4)) for k in range(2)]))
    tvm = to_dev(eoc.lut_many_test_polynomial(4, [lo.int_table(lambda m: m % 2, 4, 4), lo.int_table(lambda m: m // 2, 4, 4)]))
    ba, bb = to_dev(sk.encrypt_bits((np.arange(rows) & 1).astype(np.uint8), 9991)), \
        to_dev(sk.encrypt_bits(((np.arange(rows) >> 1) & 1).astype(np.uint8), 9992))
    ops = (np.arange(rows) % 10).astype(np.uint8)              # a mixed batch too: it uses the mixed-batch area

    def old_paths():
        o1 = dev_empty((2, rows, params.n + 1), torch.int32)
        o2 = dev_empty((1, 2, rows, params.n + 1), torch.int32)
        o3 = dev_empty((rows, params.n + 1), torch.int32)
        o4 = dev_empty((rows, params.n + 1), torch.int32)
        eng.lut_batch_device(tv1.data_ptr(), 2, cts.data_ptr(), o1.data_ptr(), rows)
        eng.lut_many_batch_device(2, tvm.data_ptr(), 1, cts.data_ptr(), o2.data_ptr(), rows)
        eng.gate_batch_device(eoc.OPS["NAND"], ba.data_ptr(), bb.data_ptr(), None, o3.data_ptr(), rows)
        eng.gate_batch_device(0, ba.data_ptr(), bb.data_ptr(), None, o4.data_ptr(), rows, ops=ops)
        sync()
        return [o.cpu().numpy() for o in (o1, o2, o3, o4)]

    first = old_paths()
    assert np.array_equal(sk.decrypt_bits(first[2]), 1 - ((np.arange(rows) & 1) & ((np.arange(rows) >> 1) & 1)))
    got = run_device(eoc, eng, c, wires)
    assert np.array_equal(got, ref)
    second = old_paths()
    for a, b in zip(first, second):
        assert np.array_equal(a, b)
    assert np.array_equal(run_device(eoc, eng, c, wires), ref)  # and the circuit after the old paths
    eng.close()


def test_wide_group_wraps_the_descriptor_ring(eoc, monkeypatch):
    """One level of 64 T = 8 nodes (bit_out tables on every other one): 128 descriptor slots of linear stages and 512 of
    key-switch outputs travel in ONE push of 640, with 7 slots of polynomial indices ahead of it, through a ring of 1 024.
    First call: slots [7, 647), compared with the oracle.  Then a lookup call of 378 tables wraps the ring to [0, 378), the
    circuit's indices take [378, 385), and its 640 descriptors wrap again: sent as two pushes, 128 to [385, 513) and then
    512 wrapped to [0, 512), the second would overwrite the first before the kernel that reads it ran.  Same bytes each time."""
    torch = torch_cuda()
    params, sk, orc, eng = engine(eoc, monkeypatch, 0)
    c = eoc.IntCircuit()
    x = c.input(2, fresh=True)
    for k in range(64):
        fs = [lambda m, k=k, j=j: (m + (k >> (j % 6)) + j) % 2 for j in range(8)]
        (c.lut_many_bit_out if k & 1 else c.lut_many)([x], fs, 2, *(() if k & 1 else (2,)))
    assert c.levels()[1:] == (1, 64)
    rows = 2
    vals = np.arange(rows, dtype=np.uint8) % 2
    wires = np.zeros((c.n_wires, rows, sk.n + 1), np.int32)
    wires[x] = sk.encrypt_ints(vals, 2, 9970)
    first = run_device(eoc, eng, c, wires)
    assert np.array_equal(first, ico.run(orc, c.nodes(), c.test_polynomials(), wires))
    chk = c.check(params, sk.lwe_key, sk.tlwe_key)
    assert chk["worst_sigma"] >= MIN_SIGMA
    assert assert_decrypts(sk, c, first, c.evaluate_plain([vals]), trusted_wires(c, chk), p=2) == 512
    n_fill = 378
    tvs = to_dev(np.tile(eoc.lut_test_polynomial(2, lo.int_table(lambda m: m, 2, 2)), (n_fill, 1)))
    d_in, d_out = to_dev(wires[x][:1]), dev_empty((n_fill, 1, sk.n + 1), torch.int32)
    grows = eng.L.eoc_engine_workspace_grows(eng.h)
    for _ in range(3):
        eng.lut_batch_device(tvs.data_ptr(), n_fill, d_in.data_ptr(), d_out.data_ptr(), 1)
        assert np.array_equal(run_device(eoc, eng, c, wires), first)
    assert eng.L.eoc_engine_workspace_grows(eng.h) == grows     # the ring kept its 1 024 slots: the positions above hold
    eng.close()


def test_group_cut_into_several_launches(eoc, monkeypatch):
    """4 097 T = 8 nodes on one level, one row: 32 776 output slots are more than a grid dimension takes, so the group runs as
    4 096 nodes + 1, the second part's polynomials starting at staged entry 4 096.  Node k uses table set k mod 3 (4 096 mod 3
    = 1: not the set of entry 0), so every node's outputs equal those of node k mod 3, which are compared with the oracle"""
    params, sk, orc, eng = engine(eoc, monkeypatch, 0)
    c = eoc.IntCircuit()
    x = c.input(2, fresh=True)
    sets = [[lambda m, a=a, j=j: (m * (j + a) + (a * (j + 1) >> 1)) % 2 for j in range(8)] for a in range(3)]
    outs = [c.lut_many([x], sets[k % 3], 2, 2) for k in range(4097)]
    wires = np.zeros((c.n_wires, 1, sk.n + 1), np.int32)
    wires[x] = sk.encrypt_ints(np.array([1], np.uint8), 2, 9980)
    before = eng.stats()
    got = run_device(eoc, eng, c, wires)
    st = eng.stats()
    assert st["bootstraps"] - before["bootstraps"] == 4097 and st["keyswitches"] - before["keyswitches"] == 8 * 4097
    assert st["batches"] - before["batches"] == 2
    small = eoc.IntCircuit()
    xs = small.input(2, fresh=True)
    for a in range(3):
        small.lut_many([xs], sets[a], 2, 2)
    ref = ico.run(orc, small.nodes(), small.test_polynomials(), wires[:small.n_wires])
    assert len({ref[1 + 8 * a:9 + 8 * a].tobytes() for a in range(3)}) == 3
    for k, o in enumerate(outs):
        a = k % 3
        assert np.array_equal(got[o[0]:o[0] + 8], ref[1 + 8 * a:9 + 8 * a]), k
    eng.close()
