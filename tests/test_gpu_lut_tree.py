"""d-digit table lookups on the MI355X: eoc_lut_tree_batch_device against the composed reference
(tests/lut_tree_oracle.py: the `_tv` / many-LUT level, the exact pack, the encrypted-seed levels) byte for byte at d = 2, 3 and
4, every input combination decrypted at d = 3, row slices, a captured graph, the global context, the counters and the errors.
Host side: tests/test_lut_tree_cpu.py; the pack alone: tests/test_gpu_tvpack_mm.py."""
import numpy as np
import pytest

import capture_cases as cc
import lut2_oracle as l2
import lut_tree_oracle as lt
import pack_oracle as po
from gpu_util import dev_empty, sync, to_dev, torch_cuda
from test_gpu_capture import assert_words, capture, side_stream, still_poisoned

pytestmark = pytest.mark.gpu
N = 1024
EOC_OK, EOC_ERR_ARG, EOC_ERR_NO_KEY = 0, -1, -4
ENV_KNOBS = ("EOC_TFHE_BR_WIDE", "EOC_TFHE_BR_TABLES_LDS", "EOC_TFHE_SCALAR_ABAR", "EOC_TFHE_BR_SLICE", "EOC_TFHE_BR_PARTS",
             "EOC_TFHE_PACK_WS_BYTES", "EOC_TFHE_SLICE_SAMPLES")


@pytest.fixture(scope="module")
def eoc(built_lib):
    torch_cuda()
    import eoc_tfhe_amd
    return eoc_tfhe_amd


def functions(p):
    """two functions of any number of digits: a weighted sum and the largest digit"""
    return [lambda *x: (sum((k + 1) * v for k, v in enumerate(x)) + 1) % p, lambda *x: max(x)]


def engine(eoc, monkeypatch, pset, env=None):
    for k in ENV_KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)                                          # read at engine creation
    params, sk, blob = l2.keys(eoc, pset)[:3]
    eng = eoc.Engine(params)
    eng.load_cloud_key(sk)
    eng.load_packing_key(blob)
    return eng


def polynomials(eoc, p, d, T):
    return np.stack([eoc.lut_tree_test_polynomials(p, d, lt.torus_table(f, p, d), T) for f in functions(p)])


def tree_device(eng, p, d, T, tv0, digits):
    F, S = tv0.shape[0], digits.shape[1]
    d_tv, d_dig = to_dev(tv0), to_dev(digits)
    d_out = dev_empty((F, S, digits.shape[2]), torch_cuda().int32)
    eng.lut_tree_batch_device(p, d, T, d_tv.data_ptr(), F, d_dig.data_ptr(), d_out.data_ptr(), S)
    sync()
    return d_out.cpu().numpy()


def digit_rows(p, d, rows):
    """digit values [d][rows]: every combination (rows None), or the first `rows` of a fixed shuffle of them"""
    xs = np.array(list(np.ndindex(*(p,) * d)), np.uint8)
    if rows is not None:
        xs = xs[np.random.default_rng(10 * p + d).permutation(len(xs))[:rows]]
    return np.ascontiguousarray(xs.T)


def shared_case(eoc, pset, p, d, T, rows):
    """inputs (fixed seeds), level-1 polynomials and the reference's words, computed once"""
    def make():
        params, sk, blob, _, orc = l2.keys(eoc, pset)
        xs = digit_rows(p, d, rows)
        digits = np.stack([sk.encrypt_ints(xs[k], p, 6400 + 100 * pset + 10 * p + k) for k in range(d)])
        tv0 = polynomials(eoc, p, d, T)
        out = lt.lut_tree_batch(orc, po.blob_rows(blob, params.n), p, d, T, tv0, digits)
        want = np.array([[f(*(int(v) for v in col)) % p for col in xs.T] for f in functions(p)], np.uint8)
        return dict(xs=xs, digits=digits, tv0=tv0, out=out, want=want)
    return l2.cached(("tree", pset, p, d, T, rows), make)


def counts(p, d, T):
    """(bootstraps, keyswitches) per row and function"""
    return p ** (d - 1) // T + sum(p ** (d - k) for k in range(2, d + 1)), sum(p ** (d - k) for k in range(1, d + 1))


# -- bit-exact -------------------------------------------------------------------------------------------------------------------
CASES = [(0, 4, 2, 1), (0, 2, 3, 1), (1, 2, 3, 1), (0, 2, 4, 2), (0, 4, 3, 4)]


@pytest.mark.parametrize("pset,p,d,T", CASES, ids=[f"set{'AB'[c[0]]}-p{c[1]}-d{c[2]}-T{c[3]}" for c in CASES])
def test_tree_bit_exact_against_the_composed_reference(eoc, monkeypatch, pset, p, d, T):
    """two functions, 3 rows; the counters are the formulas of include/eoc_tfhe_gpu.h"""
    params, sk = l2.keys(eoc, pset)[:2]
    case = shared_case(eoc, pset, p, d, T, 3)
    eng = engine(eoc, monkeypatch, pset)
    before = eng.stats()
    got = tree_device(eng, p, d, T, case["tv0"], case["digits"])
    st = eng.stats()
    eng.close()
    boots, kss = counts(p, d, T)
    assert st["bootstraps"] - before["bootstraps"] == 2 * 3 * boots
    assert st["keyswitches"] - before["keyswitches"] == 2 * 3 * kss
    assert st["pack_launches"] - before["pack_launches"] == d - 1
    assert st["packed_samples"] - before["packed_samples"] == 2 * 3 * sum(p ** (d - k) for k in range(1, d))
    bad = np.argwhere((got != case["out"]).any(axis=-1))
    assert bad.size == 0, (pset, p, d, T, len(bad), bad[:8].tolist())
    if T == 1:                                                            # fresh inputs: every level far above 6 sigma
        for f in range(2):
            assert np.array_equal(sk.decrypt_ints(got[f], p), case["want"][f]), (pset, p, d, T, f)


def test_counter_formulas():
    assert counts(4, 2, 1) == (5, 5) and counts(4, 2, 4) == (2, 5)        # eoc_lut2_batch_device's p / T + 1 and p + 1
    assert counts(2, 3, 1) == (7, 7) and counts(2, 4, 2) == (4 + 7, 15) and counts(4, 3, 4) == (4 + 5, 21)


@pytest.mark.parametrize("p,rows", [(2, 8), (4, 64)])
def test_every_input_combination_decrypts(eoc, monkeypatch, p, rows):
    """Set A, d = 3, T = 1, two functions, all p^3 combinations of fresh digits"""
    d = 3
    params, sk = l2.keys(eoc, 0)[:2]
    xs = digit_rows(p, d, None)
    assert xs.shape == (d, rows)
    digits = np.stack([sk.encrypt_ints(xs[k], p, 6900 + 10 * p + k) for k in range(d)])
    eng = engine(eoc, monkeypatch, 0)
    got = tree_device(eng, p, d, 1, polynomials(eoc, p, d, 1), digits)
    eng.close()
    for f, F in enumerate(functions(p)):
        want = np.array([F(*(int(v) for v in col)) % p for col in xs.T], np.uint8)
        assert np.array_equal(sk.decrypt_ints(got[f], p), want), (p, f)


def test_row_slices_give_the_unsliced_words(eoc, monkeypatch):
    """EOC_TFHE_SLICE_SAMPLES = 16 at 2 functions x 4 level-1 tables: slices of 2 rows, 3 rows as 2 + 1"""
    case = shared_case(eoc, 0, 2, 3, 1, 3)
    eng = engine(eoc, monkeypatch, 0, env={"EOC_TFHE_SLICE_SAMPLES": "16"})
    before = eng.stats()
    got = tree_device(eng, 2, 3, 1, case["tv0"], case["digits"])
    st = eng.stats()
    eng.close()
    assert st["pack_launches"] - before["pack_launches"] == 2 * 2          # two packs per slice
    assert np.array_equal(got, case["out"])


# -- a captured graph ------------------------------------------------------------------------------------------------------------
ROW_SETS = ([0, 1], [2, 3], [4, 7], [5, 6], [7, 0])             # rows of the all-combinations p = 2, d = 3 case per input set


class LutTree(cc.Case):
    """p = 2, d = 3, T = 1, both functions on 2 rows: three levels and two exact packs in one call"""
    rows = 2
    expect = dict(pack_launches=2)

    def setup(self):
        eoc = self.eoc
        self.p, self.sk, blob = l2.keys(eoc, 0)[:3]
        self.case = shared_case(eoc, 0, 2, 3, 1, None)
        with cc.knobs({}):
            self.eng2 = eoc.Engine(self.p)
        self.eng2.load_cloud_key(self.sk)
        self.eng2.load_packing_key(blob)
        self.fresh(self.p).load_cloud_key(self.sk)
        self.eng.load_packing_key(blob)
        self.d_tv = to_dev(self.case["tv0"])
        self.keep.append(self.d_tv)

    def alloc(self):
        return dict(x=self.new((3, self.rows, self.p.n + 1)), out=self.new((2, self.rows, self.p.n + 1)))

    def load(self, b, k):
        b["x"].copy_(to_dev(self.case["digits"][:, ROW_SETS[k]]))

    def tree(self, eng, b, n_funcs, rows, st):
        eng.lut_tree_batch_device(2, 3, 1, self.d_tv.data_ptr(), n_funcs, b["x"].data_ptr(), b["out"].data_ptr(), rows, stream=st)

    def call(self, eng, b, st):
        self.tree(eng, b, 2, self.rows, st)

    def ref(self, k):
        return dict(out=self.case["out"][:, ROW_SETS[k]])

    def other(self):
        self.tree(self.eng, self.dbufs[0], 1, 1, None)            # one function, one row: it reads [3][1][n+1], any words do

    def close(self):
        cc.Case.close(self)
        self.eng2.close()


def test_captured_tree_replays_the_reference_words(eoc):
    """the protocol of tests/test_gpu_capture.py: eager (sizes every buffer), capture, two replays on new inputs behind
    disturbing eager calls, each compared with the reference and with a second engine's eager call"""
    torch, L = torch_cuda(), eoc.lib()
    c = LutTree(eoc)
    eng = c.eng
    st = side_stream(torch)
    c.set_inputs(0)
    c.poison()
    sync()
    st.wait_stream(torch.cuda.current_stream())
    before = eng.stats()
    with torch.cuda.stream(st):
        c.run(st.cuda_stream)
    st.synchronize()
    after = eng.stats()
    for counter, delta in c.expect.items():
        assert after[counter] - before[counter] == delta, counter
    assert_words(c.fetch(), c.want(0), c, "eager")
    c.set_inputs(0)
    sync()
    grows = L.eoc_engine_workspace_grows(eng.h)
    g = capture(torch, st, c.run)
    assert L.eoc_engine_workspace_grows(eng.h) == grows
    got = {}
    for k in (1, 2):
        c.set_inputs(k)
        c.disturb()
        c.poison()
        sync()
        assert L.eoc_engine_workspace_grows(eng.h) == grows, "a call after the capture grew a buffer: the graph is void"
        g.replay()
        sync()
        got[k] = c.fetch()
        assert not still_poisoned(c), (k, still_poisoned(c))
        assert_words(got[k], c.want(k), c, f"replay {k}")
    for k in (1, 2):
        second = c.second(k)
        assert cc.bytes_equal(got[k]["out"], second["out"]), k
    del g
    c.close()


# -- the global context ----------------------------------------------------------------------------------------------------------
def test_global_context_agrees_with_the_device_call(eoc):
    params, sk, blob = l2.keys(eoc, 0)[:3]
    case = shared_case(eoc, 0, 2, 3, 1, 3)
    tabs = np.stack([lt.torus_table(f, 2, 3) for f in functions(2)])
    digits = case["digits"]
    L = eoc.lib()
    try:
        eoc.gpu_shutdown()
        eoc.gpu_init(params, devices=[0])
        eoc.upload_cloud_key(sk)
        out = np.zeros((2,) + digits.shape[1:], np.int32)
        args = (tabs.ctypes.data, 2, digits.ctypes.data, out.ctypes.data)
        assert L.eoc_lut_tree_batch(2, 3, 1, *args, 3) == EOC_ERR_NO_KEY                   # no packing key yet
        assert not out.any()
        eoc.global_import_packing_key_blob(blob)
        one = eoc.lut_tree_batch(2, 3, tabs, digits)
        assert L.eoc_lut_tree_batch(2, 3, 1, *args, 0) == EOC_OK and not out.any()         # count 0 touches nothing
        for p, d, T in [(3, 3, 1), (2, 1, 1), (2, 5, 1), (8, 4, 1), (2, 3, 4), (2, 3, -1)]:
            assert L.eoc_lut_tree_batch(p, d, T, *args, 3) == EOC_ERR_ARG, (p, d, T)
        assert L.eoc_lut_tree_batch(2, 3, 1, None, 2, digits.ctypes.data, out.ctypes.data, 3) == EOC_ERR_ARG
        eoc.gpu_shutdown()
        eoc.gpu_init(params, devices=[0, 0])                                                # two engines: two row blocks
        eoc.upload_cloud_key(sk)
        eoc.global_import_packing_key_blob(blob)
        two = eoc.lut_tree_batch(2, 3, tabs, digits)
    finally:
        eoc.gpu_shutdown()
    assert np.array_equal(one, case["out"]) and np.array_equal(two, case["out"])


# -- errors ------------------------------------------------------------------------------------------------------------------------
def test_device_errors_and_missing_keys(eoc, monkeypatch):
    torch = torch_cuda()
    L = eoc.lib()
    params, sk, blob = l2.keys(eoc, 0)[:3]
    eng = engine(eoc, monkeypatch, 0)
    buf = torch.full((1 << 17,), 7, dtype=torch.int32, device="cuda")
    a = buf.data_ptr()
    bad = [(p, 3, 1) for p in (0, 1, 3, 16)] + [(4, 1, 1), (4, 5, 1), (8, 4, 1), (2, 3, 4), (4, 3, 8), (8, 3, 4), (4, 3, 3), (4, 3, -1)]
    for p, d, T in bad:
        assert L.eoc_lut_tree_batch_device(eng.h, p, d, T, a, 1, a, a, 4, None) == EOC_ERR_ARG, (p, d, T)
    assert L.eoc_lut_tree_batch_device(eng.h, 4, 3, 1, a, 0, a, a, 4, None) == EOC_ERR_ARG
    assert L.eoc_lut_tree_batch_device(eng.h, 4, 3, 1, a, 2049, a, a, 4, None) == EOC_ERR_ARG        # n_funcs p^2 > 32 768
    for k in range(3):
        ptrs = [a, a, a]
        ptrs[k] = None
        assert L.eoc_lut_tree_batch_device(eng.h, 4, 3, 1, ptrs[0], 1, ptrs[1], ptrs[2], 4, None) == EOC_ERR_ARG, k
    assert L.eoc_lut_tree_batch_device(eng.h, 4, 3, 1, a, 1, a, a, 0, None) == EOC_OK                # count 0 touches nothing
    sync()
    st = eng.stats()
    assert bool((buf == 7).all()) and st["bootstraps"] == 0 and st["pack_launches"] == 0
    eng.close()
    no_pack = eoc.Engine(params)                                           # the cloud key alone
    no_pack.load_cloud_key(sk)
    assert L.eoc_lut_tree_batch_device(no_pack.h, 2, 3, 1, a, 1, a, a, 2, None) == EOC_ERR_NO_KEY
    no_pack.close()
    no_cloud = eoc.Engine(params)                                          # the packing key alone
    no_cloud.load_packing_key(blob)
    assert L.eoc_lut_tree_batch_device(no_cloud.h, 2, 3, 1, a, 1, a, a, 2, None) == EOC_ERR_NO_KEY
    no_cloud.close()
    sync()
    assert bool((buf == 7).all())
