"""Many-LUT bootstrapping on the MI355X: eoc_lut_many_batch_device against the composed CPU-oracle bootstrap
(tests/lut_many_oracle.py) byte for byte on the Set A pair kernel, the Set A wide kernel with a pair remainder and Set B's
two-part launch, in both rotation-amount read-back forms; launch counts; 16 384 rows per supported (T, p); output noise per
slot; the global context; argument errors; an 8-bit ripple addition in the integer encoding.  Host side:
tests/test_lut_many_cpu.py."""
import numpy as np
import pytest

import lut_many_oracle as lmo
import lut_oracle as lo
import oracle_lib as ol
from eoc_tfhe_amd import noise
from gpu_util import br_segments, dev_empty, sync, to_dev, torch_cuda

pytestmark = pytest.mark.gpu
N = 1024
EOC_ERR_ARG = -1
SUPPORTED = [(T, p) for T in (2, 4, 8) for p in (2, 4, 8) if p * T <= 16]
SHAPES = [(2, 8), (4, 4), (8, 2)]          # every T, each with the largest p it supports


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


def engine(eoc, monkeypatch, pset, readback="default"):
    if readback == "scalar-abar":
        monkeypatch.setenv("EOC_TFHE_SCALAR_ABAR", "1")       # read at engine creation: the SABAR instances
    params, sk, orc = keys(eoc, pset)
    eng = eoc.Engine(params)
    eng.load_cloud_key(sk)
    return params, sk, orc, eng


def inputs(eoc, sk, p, rows, enc_seed):
    """rows cycling through every m in Z_p and, every fourth row, a padding-half phase m in [p, 2p)"""
    m = np.arange(rows) % (2 * p)
    m[np.arange(rows) % 4 != 3] %= p
    cts = np.empty((rows, sk.n + 1), np.int32)
    for r in range(rows):
        mu = np.int64((int(m[r]) << 32) // (2 * p)).astype(np.uint32).view(np.int32)
        assert eoc.lib().eoc_lwe_encrypt(sk.h, enc_seed, r, int(mu), sk.params.ks_stdev, cts[r].ctypes.data) == 0
    return m, cts


def tables_for(T, p, n_luts):
    """n_luts x T functions Z_p -> Z_p, all different"""
    fs = [[(lambda m, a=2 * (g * T + j) + 1, c=g + j: (a * m + c) % p) for j in range(T)] for g in range(n_luts)]
    return fs, [[lo.int_table(f, p, p) for f in row] for row in fs]


def packed(eoc, p, tabs):
    return np.stack([eoc.lut_many_test_polynomial(p, row) for row in tabs])


def run_device(eoc, eng, T, tvs, cts):
    torch = torch_cuda()
    tvs = np.ascontiguousarray(np.asarray(tvs, np.int32).reshape(-1, N))
    d_tv, d_in = to_dev(tvs), to_dev(cts)
    d_out = dev_empty((tvs.shape[0], T, cts.shape[0], cts.shape[1]), torch.int32)
    eng.lut_many_batch_device(T, d_tv.data_ptr(), tvs.shape[0], d_in.data_ptr(), d_out.data_ptr(), cts.shape[0])
    sync()
    return d_out.cpu().numpy()


def check_decrypts(sk, got, fs, m, p):
    for g, row in enumerate(fs):
        for j, f in enumerate(row):
            dec = sk.decrypt_ints(got[g, j], p)
            exp = np.array([f(x) if x < p else (-f(x - p)) % p for x in m])
            assert np.array_equal(dec, exp), (g, j, np.flatnonzero(dec != exp)[:8])


@pytest.mark.parametrize("readback", ["default", "scalar-abar"])
@pytest.mark.parametrize("T,p", SHAPES)
def test_set_a_pair_kernel_bit_exact(eoc, monkeypatch, readback, T, p):
    """2 polynomials x 32 rows = 64 jobs: one pair-kernel launch; every slot of every row equals the composed oracle"""
    params, sk, orc, eng = engine(eoc, monkeypatch, 0, readback)
    fs, tabs = tables_for(T, p, 2)
    tvs = packed(eoc, p, tabs)
    rows = 32
    m, cts = inputs(eoc, sk, p, rows, 9000 + T)
    before = eng.stats()
    got = run_device(eoc, eng, T, tvs, cts)
    st = eng.stats()
    assert st["br_launches"] - before["br_launches"] == 1 and st["br_wide_launches"] == before["br_wide_launches"]
    assert st["bootstraps"] - before["bootstraps"] == 2 * rows                 # one blind rotation per (polynomial, row)
    assert st["keyswitches"] - before["keyswitches"] == 2 * T * rows
    check_decrypts(sk, got, fs, m, p)
    assert np.array_equal(got, lmo.lut_many_batch(orc, tvs, cts, T))
    eng.close()


@pytest.mark.parametrize("readback", ["default", "scalar-abar"])
@pytest.mark.parametrize("T,p", SHAPES)
def test_set_a_wide_and_pair_remainder_inside_a_polynomial(eoc, monkeypatch, readback, T, p):
    """3 polynomials x 700 rows = 2 100 jobs: one full wide launch (8 x CUs) and a pair-kernel remainder whose job0 lies
    inside polynomial 2's rows.  Every slot decrypts; the rows on both sides of the cut and the first rows of every
    polynomial equal the composed oracle byte for byte"""
    params, sk, orc, eng = engine(eoc, monkeypatch, 0, readback)
    fs, tabs = tables_for(T, p, 3)
    tvs = packed(eoc, p, tabs)
    rows = 700
    m, cts = inputs(eoc, sk, p, rows, 9100 + T)
    jobs, Rw = 3 * rows, eng.resident_jobs()
    n_wide, rem = divmod(jobs, Rw)
    assert n_wide >= 1 and 0 < rem <= Rw // 2 and (n_wide * Rw) % rows != 0, (jobs, Rw)
    before = eng.stats()
    got = run_device(eoc, eng, T, tvs, cts)
    st = eng.stats()
    assert st["br_wide_launches"] - before["br_wide_launches"] == n_wide
    assert st["br_launches"] - before["br_launches"] == n_wide + 1
    assert st["bootstraps"] - before["bootstraps"] == jobs
    check_decrypts(sk, got, fs, m, p)
    g_cut, r_cut = divmod(n_wide * Rw, rows)
    side = np.r_[r_cut - 6:r_cut + 6]
    assert np.array_equal(got[g_cut][:, side], lmo.lut_many_batch(orc, tvs[g_cut], cts[side], T)[0])
    assert np.array_equal(got[g_cut][:, rows - 2:], lmo.lut_many_batch(orc, tvs[g_cut], cts[rows - 2:], T)[0])
    for g in range(3):
        assert np.array_equal(got[g][:, :2], lmo.lut_many_batch(orc, tvs[g], cts[:2], T)[0]), g
    eng.close()


@pytest.mark.parametrize("readback", ["default", "scalar-abar"])
@pytest.mark.parametrize("T,p", SHAPES)
def test_set_b_two_part_segment_cut_inside_a_polynomial(eoc, monkeypatch, readback, T, p):
    """Set B, 3 polynomials x 500 rows = 1 500 jobs: two even segments of two launches each (acc_state hand-off), the
    second starting inside polynomial 1's rows"""
    params, sk, orc, eng = engine(eoc, monkeypatch, 1, readback)
    fs, tabs = tables_for(T, p, 3)
    tvs = packed(eoc, p, tabs)
    rows = 500
    m, cts = inputs(eoc, sk, p, rows, 9200 + T)
    segs = br_segments(3 * rows, eng.resident_jobs())
    assert len(segs) == 2 and segs[1] % rows != 0, segs
    before = eng.stats()
    got = run_device(eoc, eng, T, tvs, cts)
    st = eng.stats()
    assert st["br_launches"] - before["br_launches"] == 2 * len(segs)
    assert st["br_wide_launches"] == before["br_wide_launches"]
    assert st["bootstraps"] - before["bootstraps"] == 3 * rows
    assert st["keyswitches"] - before["keyswitches"] == 3 * T * rows
    check_decrypts(sk, got, fs, m, p)
    g_cut, r_cut = divmod(segs[1], rows)
    side = np.r_[r_cut - 6:r_cut + 6]
    assert np.array_equal(got[g_cut][:, side], lmo.lut_many_batch(orc, tvs[g_cut], cts[side], T)[0])
    for g in range(3):
        assert np.array_equal(got[g][:, [0, rows - 1]], lmo.lut_many_batch(orc, tvs[g], cts[[0, rows - 1]], T)[0]), g
    eng.close()


@pytest.mark.parametrize("pset", [0, 1], ids=["setA", "setB"])
@pytest.mark.parametrize("T,p", SUPPORTED)
def test_16384_rows_decrypt(eoc, monkeypatch, pset, T, p):
    params, sk, orc, eng = engine(eoc, monkeypatch, pset)
    fs, tabs = tables_for(T, p, 1)
    rows = 16384
    m, cts = inputs(eoc, sk, p, rows, 9300 + 10 * T + p)
    got = run_device(eoc, eng, T, packed(eoc, p, tabs), cts)
    check_decrypts(sk, got, fs, m, p)
    eng.close()


@pytest.mark.parametrize("pset", [0, 1], ids=["setA", "setB"])
def test_output_noise_per_slot_matches_prediction(eoc, monkeypatch, pset):
    """T = 8, p = 2, 16 384 rows: in every slot the output-error variance is the gate bootstrap's, within 5 % of
    noise.predict()['total_var'] (tests/test_gpu_lut.py's tolerance): the grid widens only the input's rounding"""
    T, p = 8, 2
    params, sk, orc, eng = engine(eoc, monkeypatch, pset)
    rows = 16384
    vals = (np.arange(rows) % p).astype(np.uint8)
    cts = sk.encrypt_ints(vals, p, 9401 + pset)
    fs, tabs = tables_for(T, p, 1)
    got = run_device(eoc, eng, T, packed(eoc, p, tabs), cts)[0]
    pred = noise.predict(params, sk.lwe_key, sk.tlwe_key, sk.ksk)
    s = sk.lwe_key.astype(np.int64)
    for j in range(T):
        g = got[j].astype(np.int64)
        ph = (g[:, -1] - g[:, :-1] @ s) & 0xFFFFFFFF
        want = tabs[0][j][vals].astype(np.int64)
        err = (((ph - want) + 2**31) % 2**32 - 2**31) / 2.0**32
        ratio = err.var() / pred["total_var"]
        print(f"pset {pset} slot {j}: measured var {err.var():.4e}, predicted {pred['total_var']:.4e}, ratio {ratio:.4f}")
        assert abs(ratio - 1) < 0.05, (j, ratio)
    eng.close()


def test_global_context_two_engines_and_cloud_key_only(eoc, monkeypatch):
    T, p = 2, 4
    params, sk, orc, eng = engine(eoc, monkeypatch, 0)
    rows = 700
    vals = (np.arange(rows) % p).astype(np.uint8)
    cts = sk.encrypt_ints(vals, p, 9501)
    fs, tabs = tables_for(T, p, 2)
    dev = run_device(eoc, eng, T, packed(eoc, p, tabs), cts)
    eng.close()
    try:
        eoc.gpu_shutdown()
        eoc.gpu_init(params, devices=[0, 0])                      # two engines on one device: two row blocks
        eoc.upload_cloud_key(sk)
        two = eoc.lut_many_batch(p, tabs, cts)
        assert two.shape == (2, T, rows, params.n + 1)
        assert np.array_equal(two, dev)
        one_poly = eoc.lut_many_batch(p, tabs[1], cts)            # [T][p]: one polynomial
        assert np.array_equal(one_poly[0], dev[1])
        eoc.gpu_shutdown()
        bk, ksk = np.ascontiguousarray(sk.bk), np.ascontiguousarray(sk.ksk)
        eoc.gpu_init(params, devices=[0])
        assert eoc.lib().eoc_upload_cloud_key_arrays(bk.ctypes.data, ksk.ctypes.data) == 0
        assert eoc.global_key_mode() == 0
        assert np.array_equal(eoc.lut_many_batch(p, tabs, cts), dev)
        L = eoc.lib()
        tb = np.ascontiguousarray(np.zeros((1, 8, 8), np.int32))
        out = np.empty((8,) + cts.shape, np.int32)
        assert L.eoc_lut_many_batch(8, 4, tb.ctypes.data, 1, cts.ctypes.data, out.ctypes.data, rows) == EOC_ERR_ARG
        assert L.eoc_lut_many_batch(4, 3, tb.ctypes.data, 1, cts.ctypes.data, out.ctypes.data, rows) == EOC_ERR_ARG
        assert L.eoc_lut_many_batch(4, 2, tb.ctypes.data, 0, cts.ctypes.data, out.ctypes.data, rows) == EOC_ERR_ARG
        assert L.eoc_lut_many_batch(4, 2, None, 1, cts.ctypes.data, out.ctypes.data, rows) == EOC_ERR_ARG
        assert L.eoc_lut_many_batch(4, 2, tb.ctypes.data, 1, None, out.ctypes.data, rows) == EOC_ERR_ARG
        assert L.eoc_lut_many_batch(4, 2, tb.ctypes.data, 1, cts.ctypes.data, None, rows) == EOC_ERR_ARG
    finally:
        eoc.gpu_shutdown()


def test_device_errors(eoc, monkeypatch):
    torch = torch_cuda()
    params, sk, orc, eng = engine(eoc, monkeypatch, 0)
    L = eoc.lib()
    d_tv = dev_empty((1, N), torch.int32)
    d_in = dev_empty((4, params.n + 1), torch.int32)
    d_out = dev_empty((1, 8, 4, params.n + 1), torch.int32)
    a, b, c = d_tv.data_ptr(), d_in.data_ptr(), d_out.data_ptr()
    for T in (0, 1, 3, 16):
        assert L.eoc_lut_many_batch_device(eng.h, T, a, 1, b, c, 4, None) == EOC_ERR_ARG, T
    assert L.eoc_lut_many_batch_device(eng.h, 2, a, 0, b, c, 4, None) == EOC_ERR_ARG          # n_luts = 0
    assert L.eoc_lut_many_batch_device(eng.h, 2, a, 16385, b, c, 4, None) == EOC_ERR_ARG      # n_luts T > 32 768
    assert L.eoc_lut_many_batch_device(eng.h, 8, a, 4097, b, c, 4, None) == EOC_ERR_ARG
    assert L.eoc_lut_many_batch_device(eng.h, 2, None, 1, b, c, 4, None) == EOC_ERR_ARG
    assert L.eoc_lut_many_batch_device(eng.h, 2, a, 1, None, c, 4, None) == EOC_ERR_ARG
    assert L.eoc_lut_many_batch_device(eng.h, 2, a, 1, b, None, 4, None) == EOC_ERR_ARG
    assert eng.stats()["bootstraps"] == 0
    eng.close()


def test_ripple_addition_one_many_lut_level_per_bit(eoc, monkeypatch):
    """8-bit a + b over 1 024 pairs in the integer encoding: bits are p = 4 ints, s_i = a_i + b_i + c_i is added on the
    device, and ONE lut_many_batch_device call with T = 2 (s mod 2, s >= 2) gives the sum bit and the next carry"""
    torch = torch_cuda()
    T, p, nbits, pairs = 2, 4, 8, 1024
    params, sk, orc, eng = engine(eoc, monkeypatch, 0)
    rng = np.random.default_rng(12)
    a = rng.integers(0, 256, pairs)
    b = rng.integers(0, 256, pairs)
    bits = lambda x, i: ((x >> i) & 1).astype(np.uint8)
    d_a = [to_dev(sk.encrypt_ints(bits(a, i), p, 9600 + i)) for i in range(nbits)]
    d_b = [to_dev(sk.encrypt_ints(bits(b, i), p, 9700 + i)) for i in range(nbits)]
    tv = to_dev(eoc.lut_many_test_polynomial(p, [lo.int_table(lambda s: s % 2, p, p), lo.int_table(lambda s: s >= 2, p, p)]))
    out = dev_empty((T, pairs, params.n + 1), torch.int32)
    sums, carry = [], None
    before = eng.stats()
    for i in range(nbits):
        s = d_a[i] + d_b[i] if carry is None else d_a[i] + d_b[i] + carry      # wrapping int32 additions
        eng.lut_many_batch_device(T, tv.data_ptr(), 1, s.data_ptr(), out.data_ptr(), pairs)
        sums.append(out[0].clone())
        carry = out[1].clone()
    sync()
    st = eng.stats()
    assert st["bootstraps"] - before["bootstraps"] == nbits * pairs
    got = np.zeros(pairs, np.int64)
    for i, d in enumerate(sums + [carry]):
        got |= sk.decrypt_ints(d.cpu().numpy(), p).astype(np.int64) << i
    assert np.array_equal(got, a + b), np.flatnonzero(got != a + b)[:8]
    eng.close()
