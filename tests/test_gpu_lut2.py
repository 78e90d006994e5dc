"""Two-input table lookups on the MI355X: eoc_tv_pack_device, eoc_lut_enc_batch_device and
eoc_lut2_batch_device against the composed reference (tests/lut2_oracle.py) byte for byte -- Set A's pair and wide kernels,
Set B's two-part launch --, the column budget's slicing in a fresh process, compositions with the existing lookups and the
packing key switch, the global context on one and two engines and in key mode 2, errors, and the output noise at 4 096 rows.
Decode assertions only where noise.lut2_margin_sigma gives 6 sigma or more on both levels (lut2_oracle.decodable).  Host side
and the shared inputs' own decryption on the reference: tests/test_lut2_cpu.py."""
import numpy as np
import pytest

import lut2_oracle as l2
import lut_oracle as lo
import pack_oracle as po
from eoc_tfhe_amd import noise
from gpu_util import dev_empty, sync, to_dev, torch_cuda
from test_gpu_pack import child

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


def engine(eoc, monkeypatch, pset, env=None, cloud=True):
    for k in ENV_KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)                                          # read at engine creation
    params, sk, blob = l2.keys(eoc, pset)[:3]
    eng = eoc.Engine(params)
    if cloud:
        eng.load_cloud_key(sk)
    eng.load_packing_key(blob)
    return eng


def tv_pack_device(eng, p, vals):
    F, _, S, _ = vals.shape
    d_vals = to_dev(vals)
    d_lists = dev_empty((F, S, 2, N), torch_cuda().int32)
    eng.tv_pack_device(p, d_vals.data_ptr(), F, S, d_lists.data_ptr())
    sync()
    return d_lists.cpu().numpy()


def lut_enc_device(eng, lists, n_groups, per_row, cts):
    d_lists, d_in = to_dev(lists), to_dev(cts)
    d_out = dev_empty((n_groups, cts.shape[0], cts.shape[1]), torch_cuda().int32)
    eng.lut_enc_batch_device(d_lists.data_ptr(), n_groups, per_row, d_in.data_ptr(), d_out.data_ptr(), cts.shape[0])
    sync()
    return d_out.cpu().numpy()


def lut2_device(eng, p, T, tv0, x, y):
    tv0 = np.ascontiguousarray(tv0, np.int32)
    F = tv0.size // ((p // max(T, 1)) * N)
    d_tv, d_x, d_y = to_dev(tv0), to_dev(x), to_dev(y)
    d_out = dev_empty((F, x.shape[0], x.shape[1]), torch_cuda().int32)
    eng.lut2_batch_device(p, T, d_tv.data_ptr(), F, d_x.data_ptr(), d_y.data_ptr(), d_out.data_ptr(), x.shape[0])
    sync()
    return d_out.cpu().numpy()


def pack_inputs(eoc, pset, p, count):
    """fresh encryptions [2][p][count][n+1] (the pack is linear in nothing the test relies on: any samples do) and the
    reference lists, shared by the tests that need them"""
    def make():
        params, sk, _, kfft, _ = l2.keys(eoc, pset)
        vals = sk.encrypt_ints(np.random.default_rng(p + count).integers(0, p, 2 * p * count).astype(np.uint8), p,
                               5000 + 100 * pset + 10 * p + count).reshape(2, p, count, params.n + 1)
        return vals, l2.tv_pack(params.n, kfft, vals, p)
    return l2.cached(("pack_inputs", pset, p, count), make)


# -- the pack ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pset", [0, 1], ids=["setA", "setB"])
@pytest.mark.parametrize("p", [2, 4, 8])
@pytest.mark.parametrize("count", [1, 3])
def test_tv_pack_equals_the_reference(eoc, monkeypatch, pset, p, count):
    """n_funcs = 2; n = 500 and n = 630 both end in a short chunk.  Lists of (function, row) hold value j in window j"""
    params, sk = l2.keys(eoc, pset)[:2]
    eng = engine(eoc, monkeypatch, pset, cloud=False)
    vals, want = pack_inputs(eoc, pset, p, count)
    before = eng.stats()
    got = tv_pack_device(eng, p, vals)
    st = eng.stats()
    eng.close()
    assert np.array_equal(got, want), (pset, p, count)
    assert st["pack_launches"] - before["pack_launches"] == 1
    assert st["packed_samples"] - before["packed_samples"] == 2 * count * p        # the samples read
    assert st["keyswitches"] == before["keyswitches"] and st["bootstraps"] == before["bootstraps"]
    ph = sk.list_phases(got.reshape(-1, 2, N)).astype(np.int64).reshape(2, count, N)
    for j in range(p):                                                    # the middle of window j decrypts as sample j does
        assert np.array_equal(((ph[:, :, j * (N // p)] * 2 * p + (1 << 31)) >> 32) % p,
                              sk.decrypt_ints(vals[:, j].reshape(-1, params.n + 1), p).reshape(2, count))


SLICE_BODY = """
    import lut2_oracle as l2
    from test_gpu_lut2 import tv_pack_device
    params, sk, blob = l2.keys(eoc, 0)[:3]
    eng = eoc.Engine(params)
    eng.load_packing_key(blob)
    np.save(%r, tv_pack_device(eng, 4, np.load(%r)))
    out['launches'] = eng.stats()['pack_launches']
"""


def test_column_budget_slices_the_lists_without_changing_a_word(eoc, monkeypatch, tmp_path):
    """EOC_TFHE_PACK_WS_BYTES (read at engine creation) at one list's columns and a little: the 3 lists of one function run
    as 1 + 1 + 1, the same words as the unsliced call"""
    params = l2.keys(eoc, 0)[0]
    vals, want = pack_inputs(eoc, 0, 4, 3)
    a, b = str(tmp_path / "vals.npy"), str(tmp_path / "sliced.npy")
    np.save(a, vals[:1])
    sliced = child(SLICE_BODY % (b, a), env={"EOC_TFHE_PACK_WS_BYTES": str(params.n * N * 4 + 100)})
    assert sliced["launches"] == 3
    assert np.array_equal(np.load(b), want[:1])


# -- level 2 alone -----------------------------------------------------------------------------------------------------------
def test_lut_enc_on_packed_lists_and_on_a_trivial_list(eoc, monkeypatch):
    """packed lists of the shared p = 4 case in both per_row modes, and a public table as a trivial list (c0 = 0): the
    encrypted-seed kernel then computes what the _tv kernel computes from the same polynomial"""
    torch = torch_cuda()
    params, sk, _, _, orc = l2.keys(eoc, 0)
    case = l2.shared_case(eoc, 0, 4, 1)
    eng = engine(eoc, monkeypatch, 0)
    lists, y = case["lists"], case["y"]                                    # [2][16][2][N]
    before = eng.stats()
    got_rows = lut_enc_device(eng, lists, 2, True, y)
    st = eng.stats()
    assert st["bootstraps"] - before["bootstraps"] == 32 == st["keyswitches"] - before["keyswitches"]
    assert st["br_launches"] - before["br_launches"] == 1
    assert np.array_equal(got_rows, case["out"])
    # one list per group: the lists of rows 0 and 5 of function 0, each against all 16 rows of y
    groups = np.ascontiguousarray(lists[0, [0, 5]])
    got = lut_enc_device(eng, groups, 2, False, y)
    want = l2.cached(("enc_groups",), lambda: l2.lut_enc_batch(orc, groups, y, False))
    assert np.array_equal(got, want)
    for g, r in enumerate((0, 5)):                                        # list of row r holds F(x_r, .): row s gives F(x_r, y_s)
        assert np.array_equal(sk.decrypt_ints(got[g], 4), [l2.PROD_LO(int(case["xv"][r]), int(b)) for b in case["yv"]])
    # a trivial list
    tv = eoc.lut_test_polynomial(4, lo.int_table(lambda m: (3 * m + 1) % 4, 4, 4))
    triv = eoc.trivial_table(tv)
    assert triv.shape == (1, 2, N) and not triv[0, 0].any()
    got_t = lut_enc_device(eng, triv, 1, False, y)
    d_tv, d_y = to_dev(tv), to_dev(y)
    d_out = dev_empty((1, 16, params.n + 1), torch.int32)
    eng.lut_batch_device(d_tv.data_ptr(), 1, d_y.data_ptr(), d_out.data_ptr(), 16)
    sync()
    assert np.array_equal(got_t, d_out.cpu().numpy())
    assert np.array_equal(got_t, lo.lut_batch(orc, tv, y))
    eng.close()


# -- the composed call -------------------------------------------------------------------------------------------------------
CASES = [(0, 4, 1, None), (0, 4, 2, None), (0, 4, 4, None), (0, 2, 2, None), (0, 8, 1, 8), (1, 4, 1, None), (1, 4, 4, None)]


@pytest.mark.parametrize("pset,p,T,rows", CASES, ids=[f"set{'AB'[c[0]]}-p{c[1]}-T{c[2]}" for c in CASES])
def test_lut2_bit_exact_against_the_reference(eoc, monkeypatch, pset, p, T, rows):
    """n_funcs = 2, every (x, y) pair (8 of the 64 at p = 8).  Set B: every blind rotation is two launches"""
    params, sk = l2.keys(eoc, pset)[:2]
    case = l2.shared_case(eoc, pset, p, T, rows)
    S = len(case["xv"])
    eng = engine(eoc, monkeypatch, pset, env={"EOC_TFHE_BR_WIDE": "0"})
    before = eng.stats()
    got = lut2_device(eng, p, T, case["tv0"].reshape(-1, N), case["x"], case["y"])
    st = eng.stats()
    eng.close()
    assert got.shape == (2, S, params.n + 1)
    assert st["bootstraps"] - before["bootstraps"] == 2 * S * (p // T + 1)
    assert st["keyswitches"] - before["keyswitches"] == 2 * S * (p + 1)
    assert st["br_launches"] - before["br_launches"] == 2 * (1 + pset) and st["br_wide_launches"] == before["br_wide_launches"]
    assert st["pack_launches"] - before["pack_launches"] == 1
    bad = np.argwhere((got != case["out"]).any(axis=-1))
    assert bad.size == 0, (pset, p, T, len(bad), bad[:8].tolist())
    if l2.decodable(eoc, noise, pset, p, T):
        for f in range(2):
            assert np.array_equal(sk.decrypt_ints(got[f], p), case["want"][f]), (pset, p, T, f)


def test_lut2_with_the_wide_kernels_inside_the_composed_call(eoc, monkeypatch):
    """Set A once more with EOC_TFHE_BR_WIDE=1: level 1 on k_blind_rotate_wide_tv, level 2 on k_br_enc_wide, the same words"""
    case = l2.shared_case(eoc, 0, 4, 1)
    eng = engine(eoc, monkeypatch, 0, env={"EOC_TFHE_BR_WIDE": "1"})
    before = eng.stats()
    got = lut2_device(eng, 4, 1, case["tv0"].reshape(-1, N), case["x"], case["y"])
    st = eng.stats()
    eng.close()
    assert st["br_launches"] - before["br_launches"] == 2 == st["br_wide_launches"] - before["br_wide_launches"]
    assert np.array_equal(got, case["out"])


def test_row_slices_of_the_composed_call_are_the_unsliced_words(eoc, monkeypatch):
    """n_tables = 0 is T = 1; and a sub-range of rows gives those rows' words (every row is computed on its own)"""
    case = l2.shared_case(eoc, 0, 4, 1)
    eng = engine(eoc, monkeypatch, 0)
    got = lut2_device(eng, 4, 0, case["tv0"].reshape(-1, N), case["x"][5:8], case["y"][5:8])
    eng.close()
    assert np.array_equal(got, case["out"][:, 5:8])


# -- compositions ------------------------------------------------------------------------------------------------------------
def test_a_lut2_output_feeds_a_lookup_and_the_packing_key_switch(eoc, monkeypatch):
    torch = torch_cuda()
    params, sk, _, kfft, orc = l2.keys(eoc, 0)
    case = l2.shared_case(eoc, 0, 4, 1)
    eng = engine(eoc, monkeypatch, 0)
    out = lut2_device(eng, 4, 1, case["tv0"].reshape(-1, N), case["x"], case["y"])
    assert np.array_equal(out, case["out"])
    f = lambda m: (2 * m + 3) % 4                                          # noqa: E731
    tv = eoc.lut_test_polynomial(4, lo.int_table(f, 4, 4))
    d_tv, d_in = to_dev(tv), to_dev(out[0])
    d_out = dev_empty((1, 16, params.n + 1), torch.int32)
    d_lists = dev_empty((1, 2, N), torch.int32)
    eng.lut_batch_device(d_tv.data_ptr(), 1, d_in.data_ptr(), d_out.data_ptr(), 16)
    eng.pack_device(d_in.data_ptr(), 16, d_lists.data_ptr())
    sync()
    eng.close()
    got = d_out.cpu().numpy()
    assert np.array_equal(got, l2.cached(("feeds",), lambda: lo.lut_batch(orc, tv, case["out"][0])))
    assert np.array_equal(sk.decrypt_ints(got[0], 4), [f(int(v)) for v in case["want"][0]])      # >= 6 sigma: test_lut2_cpu.py
    lists = d_lists.cpu().numpy()
    assert np.array_equal(lists, po.pack(params.n, kfft, case["out"][0]))
    assert np.array_equal(sk.decrypt_list_ints(lists, 4, 16), case["want"][0])


# -- the global context ------------------------------------------------------------------------------------------------------
def test_global_context_one_and_two_engines_and_key_mode_2(eoc, tmp_path):
    params, sk, blob = l2.keys(eoc, 0)[:3]
    case = l2.shared_case(eoc, 0, 4, 2)
    tabs = np.stack([l2.lut2_tables(f, 4) for f in l2.functions(4)])
    x, y = case["x"], case["y"]
    L = eoc.lib()
    try:
        eoc.gpu_shutdown()
        eoc.gpu_init(params, devices=[0])
        eoc.upload_cloud_key(sk)
        out = np.zeros((2,) + x.shape, np.int32)
        args = (tabs.ctypes.data, 2, x.ctypes.data, y.ctypes.data, out.ctypes.data)
        assert L.eoc_lut2_batch(4, 2, *args, 16) == EOC_ERR_NO_KEY                  # no packing key yet
        assert not out.any()
        eoc.global_import_packing_key_blob(blob)
        one = eoc.lut2_batch(4, tabs, x, y, n_tables=2)
        assert L.eoc_lut2_batch(4, 2, *args, 0) == EOC_OK and not out.any()          # count 0 touches nothing
        for p, T in [(3, 1), (16, 1), (4, 3), (4, 8), (8, 4), (2, 4), (4, -1)]:
            assert L.eoc_lut2_batch(p, T, *args, 16) == EOC_ERR_ARG, (p, T)
        assert L.eoc_lut2_batch(4, 2, None, 2, x.ctypes.data, y.ctypes.data, out.ctypes.data, 16) == EOC_ERR_ARG
        assert L.eoc_lut2_batch(4, 2, tabs.ctypes.data, 0, x.ctypes.data, y.ctypes.data, out.ctypes.data, 16) == EOC_ERR_ARG
        eoc.gpu_shutdown()
        eoc.gpu_init(params, devices=[0, 0])                                        # two engines: two row blocks
        eoc.upload_cloud_key(sk)
        eoc.global_import_packing_key_blob(blob)
        two = eoc.lut2_batch(4, tabs, x, y, n_tables=2)
        per = [int(L.eoc_engine_packed_samples(L.eoc_global_engine_at(i))) for i in range(2)]
    finally:
        eoc.gpu_shutdown()
    assert np.array_equal(one, case["out"]) and np.array_equal(two, case["out"])
    assert per == [2 * 8 * 4, 2 * 8 * 4]
    # a server that holds the cloud key alone (key mode 2) and is given the packing key
    for name, a in (("x", x), ("y", y), ("tabs", tabs)):
        np.save(tmp_path / f"{name}.npy", a)
    blob.tofile(tmp_path / "pks.bin")
    server = child("""
        sk = eoc.SecretKey(eoc.default_params(0), 1)
        ck = sk.export_cloud_key()
        del sk
        eoc.global_import_cloud_key_blob(ck)
        out['mode'] = eoc.global_key_mode()
        d = %r
        x, y, tabs = (np.load(os.path.join(d, n + '.npy')) for n in ('x', 'y', 'tabs'))
        o = np.zeros((2,) + x.shape, np.int32)
        out['before'] = eoc.lib().eoc_lut2_batch(4, 2, tabs.ctypes.data, 2, x.ctypes.data, y.ctypes.data, o.ctypes.data, 16)
        eoc.global_import_packing_key_blob(np.fromfile(os.path.join(d, 'pks.bin'), np.uint8))
        np.save(os.path.join(d, 'got.npy'), eoc.lut2_batch(4, tabs, x, y, n_tables=2))
        eoc.Tfhe.resetGateKey()
    """ % str(tmp_path))
    assert server == {"mode": 2, "before": EOC_ERR_NO_KEY}
    assert np.array_equal(np.load(tmp_path / "got.npy"), case["out"])


def test_device_errors_and_missing_keys(eoc, monkeypatch):
    torch = torch_cuda()
    L = eoc.lib()
    params, sk, blob = l2.keys(eoc, 0)[:3]
    eng = engine(eoc, monkeypatch, 0)
    buf = torch.full((1 << 16,), 7, dtype=torch.int32, device="cuda")
    a = buf.data_ptr()
    bad = [(p, T) for p in (0, 1, 3, 16) for T in (1, 2)] + [(2, 4), (2, 8), (4, 8), (8, 4), (8, 8), (4, 3), (8, 16), (4, -1)]
    for p, T in bad:
        assert L.eoc_lut2_batch_device(eng.h, p, T, a, 1, a, a, a, 4, None) == EOC_ERR_ARG, (p, T)
    assert L.eoc_lut2_batch_device(eng.h, 4, 1, a, 0, a, a, a, 4, None) == EOC_ERR_ARG
    assert L.eoc_lut2_batch_device(eng.h, 4, 1, a, 8193, a, a, a, 4, None) == EOC_ERR_ARG          # n_funcs p > 32 768
    for k in range(4):
        ptrs = [a, a, a, a]
        ptrs[k] = None
        assert L.eoc_lut2_batch_device(eng.h, 4, 1, ptrs[0], 1, ptrs[1], ptrs[2], ptrs[3], 4, None) == EOC_ERR_ARG, k
    assert L.eoc_lut2_batch_device(eng.h, 4, 1, a, 1, a, a, a, 0, None) == EOC_OK                  # count 0 touches nothing
    for p in (0, 3, 16):
        assert L.eoc_tv_pack_device(eng.h, p, a, 1, 1, a, None) == EOC_ERR_ARG
    assert L.eoc_tv_pack_device(eng.h, 4, a, 0, 1, a, None) == EOC_ERR_ARG
    assert L.eoc_tv_pack_device(eng.h, 4, None, 1, 1, a, None) == EOC_ERR_ARG
    assert L.eoc_tv_pack_device(eng.h, 4, a, 1, 0, a, None) == EOC_OK
    assert L.eoc_lut_enc_batch_device(eng.h, a, 0, 0, a, a, 4, None) == EOC_ERR_ARG
    assert L.eoc_lut_enc_batch_device(eng.h, a, 32769, 0, a, a, 4, None) == EOC_ERR_ARG
    assert L.eoc_lut_enc_batch_device(eng.h, None, 1, 0, a, a, 4, None) == EOC_ERR_ARG
    assert L.eoc_lut_enc_batch_device(eng.h, a, 1, 1, a, a, 0, None) == EOC_OK
    sync()
    st = eng.stats()
    assert bool((buf == 7).all()) and st["bootstraps"] == 0 and st["pack_launches"] == 0
    eng.close()
    no_pack = eoc.Engine(params)                                           # the cloud key alone
    no_pack.load_cloud_key(sk)
    assert L.eoc_lut2_batch_device(no_pack.h, 4, 1, a, 1, a, a, a, 4, None) == EOC_ERR_NO_KEY
    assert L.eoc_tv_pack_device(no_pack.h, 4, a, 1, 1, a, None) == EOC_ERR_NO_KEY
    no_pack.close()
    no_cloud = engine(eoc, monkeypatch, 0, cloud=False)                    # the packing key alone
    assert L.eoc_lut2_batch_device(no_cloud.h, 4, 1, a, 1, a, a, a, 4, None) == EOC_ERR_NO_KEY
    assert L.eoc_lut_enc_batch_device(no_cloud.h, a, 1, 0, a, a, 4, None) == EOC_ERR_NO_KEY
    no_cloud.close()
    sync()
    assert bool((buf == 7).all())


# -- noise on the device -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pset,T", [(0, 4), (1, 1)], ids=["setA-T4", "setB-T1"])
def test_output_noise_matches_lut2_var(eoc, monkeypatch, pset, T):
    """4 096 rows, p = 4, random (x, y): the variance of the output error within 1 +- 3.5 sqrt(2 / 4095) of noise.lut2_var, the
    mean within 4 standard errors of noise.lut2_mean (the sampling spread; the second witness of tests/test_lut2_cpu.py's
    figure at a larger sample).  F is the digit sum (lut2_oracle.SUM_LO)"""
    S, p = 4096, 4
    params, sk = l2.keys(eoc, pset)[:2]
    rng = np.random.default_rng(7000 + pset)
    xv, yv = rng.integers(0, p, S).astype(np.uint8), rng.integers(0, p, S).astype(np.uint8)
    x, y = sk.encrypt_ints(xv, p, 7100 + pset), sk.encrypt_ints(yv, p, 7200 + pset)
    tv0 = eoc.lut2_test_polynomials(p, l2.lut2_tables(l2.SUM_LO, p), T)
    eng = engine(eoc, monkeypatch, pset)
    got = lut2_device(eng, p, T, tv0, x, y)[0]
    eng.close()
    want = np.array([l2.SUM_LO(int(a), int(b)) for a, b in zip(xv, yv)], np.uint8)
    g = got.astype(np.int64)
    ph = g[:, -1] - g[:, :-1] @ sk.lwe_key.astype(np.int64)
    err = ((((ph - ((want.astype(np.int64) << 32) // (2 * p))) + 2**31) % 2**32) - 2**31) / 2.0**32
    var_pred = noise.lut2_var(params, sk.lwe_key, sk.tlwe_key, sk.ksk)
    mean_pred = noise.lut2_mean(params, sk.lwe_key, sk.tlwe_key, sk.ksk)
    ratio = err.var(ddof=1) / var_pred
    z = (err.mean() - mean_pred) / (err.std(ddof=1) / np.sqrt(S))
    print(f"pset {pset} T {T}: sigma {err.std():.4e} predicted {np.sqrt(var_pred):.4e} variance ratio {ratio:.4f}; mean "
          f"{err.mean():.3e} predicted {mean_pred:.3e} ({z:+.2f} se); max |err| {np.abs(err).max():.4f}")
    assert abs(ratio - 1) <= 3.5 * np.sqrt(2.0 / (S - 1)), ratio
    assert abs(z) <= 4, z
    if l2.decodable(eoc, noise, pset, p, T):
        assert np.array_equal(sk.decrypt_ints(got, p), want)
