"""Programmable bootstrapping on the MI355X: eoc_lut_batch_device against the composed CPU-oracle bootstrap
(tests/lut_oracle.py) byte for byte on the pair kernel, the wide kernel and Set B's two-part launch; 4 tables x 16 384 rows;
bit outputs fed to the gates; output noise against noise.predict; the global context (two engines, cloud key only);
argument errors.  Host side: tests/test_lut_cpu.py."""
import numpy as np
import pytest

import lut_oracle as lo
import oracle_lib as ol
from eoc_tfhe_amd import noise
from gpu_util import br_segments, dev_empty, sync, to_dev, torch_cuda

pytestmark = pytest.mark.gpu
N = 1024
EOC_ERR_ARG = -1


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


def inputs(eoc, sk, p, rows, enc_seed):
    """rows cycling through every m in Z_p and, every fourth row, a padding-half phase m in [p, 2p)"""
    m = np.arange(rows) % (2 * p)
    m[np.arange(rows) % 4 != 3] %= p
    cts = np.empty((rows, sk.n + 1), np.int32)
    for r in range(rows):
        mu = np.int64((int(m[r]) << 32) // (2 * p)).astype(np.uint32).view(np.int32)
        assert eoc.lib().eoc_lwe_encrypt(sk.h, enc_seed, r, int(mu), sk.params.ks_stdev, cts[r].ctypes.data) == 0
    return m, cts


def run_device(eoc, eng, tvs, cts):
    torch = torch_cuda()
    tvs = np.ascontiguousarray(np.asarray(tvs, np.int32).reshape(-1, N))
    d_tv, d_in = to_dev(tvs), to_dev(cts)
    d_out = dev_empty((tvs.shape[0], cts.shape[0], cts.shape[1]), torch.int32)
    eng.lut_batch_device(d_tv.data_ptr(), tvs.shape[0], d_in.data_ptr(), d_out.data_ptr(), cts.shape[0])
    sync()
    return d_out.cpu().numpy()


def tables_for(p):
    fs = [lambda m: m, lambda m: (3 * m + 1) % p, lambda m: (m * m) % p]
    return fs, [lo.int_table(f, p, p) for f in fs]


@pytest.mark.parametrize("shape", ["setA-pair", "setA-pair-scalar-abar", "setA-wide", "setB-two-part"])
@pytest.mark.parametrize("p", [2, 4, 8])
def test_lut_bit_exact_against_composed_oracle(eoc, monkeypatch, shape, p):
    pset = 1 if shape.startswith("setB") else 0
    if shape.endswith("scalar-abar"):
        monkeypatch.setenv("EOC_TFHE_SCALAR_ABAR", "1")       # read at engine creation: the SABAR instances
    params, sk, orc = keys(eoc, pset)
    eng = eoc.Engine(params)
    eng.load_cloud_key(sk)
    fs, tabs = tables_for(p)
    tvs = np.stack([eoc.lut_test_polynomial(p, t) for t in tabs])
    # the wide kernel takes a level of more than 4 x CUs jobs (3 x 400 = 1200 > 1024)
    rows = 400 if shape == "setA-wide" else 32
    m, cts = inputs(eoc, sk, p, rows, 7000 + 10 * p + pset)
    before = eng.stats()
    got = run_device(eoc, eng, tvs, cts)
    st = eng.stats()
    if shape == "setA-wide":
        assert st["br_wide_launches"] > before["br_wide_launches"]
    else:
        assert st["br_wide_launches"] == before["br_wide_launches"]
    if shape == "setB-two-part":
        assert st["br_launches"] - before["br_launches"] == 2            # one level, two launches (acc_state hand-off)
    check = np.arange(rows) if rows <= 32 else np.r_[0:12, rows // 2:rows // 2 + 8, rows - 12:rows]
    want = lo.lut_batch(orc, tvs, cts[check])
    assert np.array_equal(got[:, check], want)
    for t, f in enumerate(fs):
        dec = sk.decrypt_ints(got[t], p)
        exp = np.array([f(x) if x < p else (-f(x - p)) % p for x in m])
        assert np.array_equal(dec, exp), (t, np.flatnonzero(dec != exp)[:8])


def _lut_engine(eoc, monkeypatch, pset, readback):
    if readback == "scalar-abar":
        monkeypatch.setenv("EOC_TFHE_SCALAR_ABAR", "1")       # read at engine creation: the SABAR instances
    params, sk, orc = keys(eoc, pset)
    eng = eoc.Engine(params)
    eng.load_cloud_key(sk)
    return params, sk, orc, eng


def _check_decrypts(sk, got, fs, m, p):
    for t, f in enumerate(fs):
        dec = sk.decrypt_ints(got[t], p)
        exp = np.array([f(x) if x < p else (-f(x - p)) % p for x in m])
        assert np.array_equal(dec, exp), (t, np.flatnonzero(dec != exp)[:8])


@pytest.mark.parametrize("readback", ["default", "scalar-abar"])
def test_lut_set_b_segment_starts_inside_a_table(eoc, monkeypatch, readback):
    """Set B, 3 tables x 500 rows = 1 500 jobs: the launch policy cuts them into two even segments (750 + 750 at 1 024
    resident jobs) of two launches each, so the second segment's kernels start at job0 = 750 -- row 250 of table 1 -- and
    take the table index (job0 + job) / tv_rows inside a launch.  Every output decrypts; the rows around the cut, and the
    first and last rows, of every table equal the composed oracle byte for byte."""
    p, rows = 4, 500
    params, sk, orc, eng = _lut_engine(eoc, monkeypatch, 1, readback)
    fs, tabs = tables_for(p)
    tvs = np.stack([eoc.lut_test_polynomial(p, t) for t in tabs])
    m, cts = inputs(eoc, sk, p, rows, 7400)
    segs = br_segments(3 * rows, eng.resident_jobs())
    assert len(segs) == 2 and segs[1] % rows != 0, segs                 # the cut lies inside a table
    before = eng.stats()
    got = run_device(eoc, eng, tvs, cts)
    st = eng.stats()
    assert st["br_launches"] - before["br_launches"] == 2 * len(segs)   # two segments x two parts
    assert st["br_wide_launches"] == before["br_wide_launches"]
    _check_decrypts(sk, got, fs, m, p)
    cut = segs[1] % rows
    check = np.r_[0:4, cut - 10:cut + 10, rows - 4:rows]
    assert np.array_equal(got[:, check], lo.lut_batch(orc, tvs, cts[check]))
    eng.close()


@pytest.mark.parametrize("readback", ["default", "scalar-abar"])
def test_lut_set_a_pair_remainder_inside_a_table(eoc, monkeypatch, readback):
    """Set A, 3 tables x 700 rows = 2 100 jobs: one full wide launch (8 x CUs = 2 048 jobs) and a pair-kernel remainder at
    job0 = 2 048 -- row 648 of table 2 -- on the _tv kernels.  Every output decrypts; the remainder's rows and the rows
    just before it in table 2, and the first rows of tables 0 and 1, equal the composed oracle byte for byte."""
    p, rows = 4, 700
    params, sk, orc, eng = _lut_engine(eoc, monkeypatch, 0, readback)
    fs, tabs = tables_for(p)
    tvs = np.stack([eoc.lut_test_polynomial(p, t) for t in tabs])
    m, cts = inputs(eoc, sk, p, rows, 7500)
    jobs, Rw = 3 * rows, eng.resident_jobs()
    n_wide, rem = divmod(jobs, Rw)
    assert n_wide >= 1 and 0 < rem <= Rw // 2 and (n_wide * Rw) % rows != 0, (jobs, Rw)
    before = eng.stats()
    got = run_device(eoc, eng, tvs, cts)
    st = eng.stats()
    assert st["br_wide_launches"] - before["br_wide_launches"] == n_wide
    assert st["br_launches"] - before["br_launches"] == n_wide + 1     # the wide launches + one pair-kernel launch
    _check_decrypts(sk, got, fs, m, p)
    t_cut, r_cut = divmod(n_wide * Rw, rows)
    tail = np.r_[r_cut - 8:rows]
    assert np.array_equal(got[t_cut, tail], lo.lut_batch(orc, tvs[t_cut], cts[tail])[0])
    for t in range(t_cut):
        assert np.array_equal(got[t, :4], lo.lut_batch(orc, tvs[t], cts[:4])[0]), t
    eng.close()


def test_lut_scale_and_bits_into_gates(eoc):
    """4 tables x 16 384 rows at p = 4; two of the tables output bits (+-1/8), which then go through bootsAND"""
    torch = torch_cuda()
    p = 4
    params, sk, orc = keys(eoc, 0)
    eng = eoc.Engine(params)
    eng.load_cloud_key(sk)
    rows = 16384
    rng = np.random.default_rng(5)
    vals = rng.integers(0, p, rows).astype(np.uint8)
    cts = sk.encrypt_ints(vals, p, 8101)
    bit = lambda g: np.array([(1 << 29) if g(m) else -(1 << 29) for m in range(p)], np.int32)
    tabs = [lo.int_table(lambda m: m + 1, p, p), lo.int_table(lambda m: 3 - m, p, p),
            bit(lambda m: m >= 2), bit(lambda m: m & 1)]
    tvs = np.stack([eoc.lut_test_polynomial(p, t) for t in tabs])
    got = run_device(eoc, eng, tvs, cts)
    assert np.array_equal(sk.decrypt_ints(got[0], p), (vals + 1) % p)
    assert np.array_equal(sk.decrypt_ints(got[1], p), 3 - vals)
    hi, lo_bit = sk.decrypt_bits(got[2]), sk.decrypt_bits(got[3])
    assert np.array_equal(hi, vals >= 2) and np.array_equal(lo_bit, vals & 1)
    d_a, d_b = to_dev(got[2]), to_dev(got[3])
    d_o = dev_empty((rows, params.n + 1), torch.int32)
    eng.gate_batch_device(eoc.OPS["AND"], d_a.data_ptr(), d_b.data_ptr(), None, d_o.data_ptr(), rows)
    sync()
    assert np.array_equal(sk.decrypt_bits(d_o.cpu().numpy()), vals == 3)
    idx = np.r_[0:4, rows - 4:rows]
    assert np.array_equal(got[:, idx], lo.lut_batch(orc, tvs, cts[idx]))


@pytest.mark.parametrize("pset", [0, 1], ids=["setA", "setB"])
def test_lut_output_noise_matches_prediction(eoc, pset):
    """p = 8, 16 384 lookups: the variance of the output phase around table[m] (f(m)'s phase) is the gate bootstrap's (blind rotation +
    key switch), within 5 % of noise.predict()['total_var']"""
    p = 8
    params, sk, _ = keys(eoc, pset)
    eng = eoc.Engine(params)
    eng.load_cloud_key(sk)
    rows = 16384
    vals = (np.arange(rows) % p).astype(np.uint8)
    cts = sk.encrypt_ints(vals, p, 8201 + pset)
    f = lambda m: (5 * m + 3) % p
    tab = lo.int_table(f, p, p)
    got = run_device(eoc, eng, eoc.lut_test_polynomial(p, tab), cts)[0]
    assert np.array_equal(sk.decrypt_ints(got, p), np.array([f(m) for m in vals]))
    s = sk.lwe_key.astype(np.int64)
    g = got.astype(np.int64)
    ph = (g[:, -1] - g[:, :-1] @ s) & 0xFFFFFFFF
    err = (((ph - tab[vals].astype(np.int64)) + 2**31) % 2**32 - 2**31) / 2.0**32      # table[m] = f(m)'s phase
    pred = noise.predict(params, sk.lwe_key, sk.tlwe_key, sk.ksk)
    ratio = err.var() / pred["total_var"]
    print(f"pset {pset}: measured var {err.var():.4e}, predicted {pred['total_var']:.4e}, ratio {ratio:.4f}, "
          f"std {err.std():.5f}")
    assert abs(ratio - 1) < 0.05, ratio


def test_lut_global_context_two_engines_and_cloud_key_only(eoc):
    p = 4
    params, sk, _ = keys(eoc, 0)
    rows = 700
    vals = (np.arange(rows) % p).astype(np.uint8)
    cts = sk.encrypt_ints(vals, p, 8301)
    fs, tabs = tables_for(p)
    try:
        eoc.gpu_shutdown()
        eoc.gpu_init(params, devices=[0])
        eoc.upload_cloud_key(sk)
        one = eoc.lut_batch(p, tabs, cts)
        eoc.gpu_shutdown()
        eoc.gpu_init(params, devices=[0, 0])                      # two engines on one device: two row blocks
        eoc.upload_cloud_key(sk)
        two = eoc.lut_batch(p, tabs, cts)
        assert np.array_equal(one, two)
        assert eoc.lib().eoc_worker_wakeups(1) >= 1
        eoc.gpu_shutdown()
        # server: the global context gets the cloud key's arrays alone, no secret key anywhere in it
        bk, ksk = np.ascontiguousarray(sk.bk), np.ascontiguousarray(sk.ksk)
        eoc.gpu_init(params, devices=[0])
        assert eoc.lib().eoc_upload_cloud_key_arrays(bk.ctypes.data, ksk.ctypes.data) == 0
        assert eoc.global_key_mode() == 0
        srv = eoc.lut_batch(p, tabs, cts)
        assert np.array_equal(srv, one)
        for t, f in enumerate(fs):
            assert np.array_equal(sk.decrypt_ints(one[t], p), [f(v) for v in vals])
        # errors of the global entry point
        L = eoc.lib()
        tb = np.ascontiguousarray(np.zeros((1, 16), np.int32))
        out = np.empty((1,) + cts.shape, np.int32)
        assert L.eoc_lut_batch(16, tb.ctypes.data, 1, cts.ctypes.data, out.ctypes.data, rows) == EOC_ERR_ARG
        assert L.eoc_lut_batch(p, tb.ctypes.data, 0, cts.ctypes.data, out.ctypes.data, rows) == EOC_ERR_ARG
        assert L.eoc_lut_batch(p, None, 1, cts.ctypes.data, out.ctypes.data, rows) == EOC_ERR_ARG
        assert L.eoc_lut_batch(p, tb.ctypes.data, 1, None, out.ctypes.data, rows) == EOC_ERR_ARG
        assert L.eoc_lut_batch(p, tb.ctypes.data, 1, cts.ctypes.data, None, rows) == EOC_ERR_ARG
    finally:
        eoc.gpu_shutdown()


def test_lut_device_errors(eoc):
    torch = torch_cuda()
    params, sk, _ = keys(eoc, 0)
    eng = eoc.Engine(params)
    eng.load_cloud_key(sk)
    L = eoc.lib()
    d_tv = dev_empty((1, N), torch.int32)
    d_in = dev_empty((4, params.n + 1), torch.int32)
    d_out = dev_empty((1, 4, params.n + 1), torch.int32)
    a, b, c = d_tv.data_ptr(), d_in.data_ptr(), d_out.data_ptr()
    assert L.eoc_lut_batch_device(eng.h, a, 0, b, c, 4, None) == EOC_ERR_ARG          # n_luts = 0
    assert L.eoc_lut_batch_device(eng.h, a, 40000, b, c, 4, None) == EOC_ERR_ARG      # beyond one grid dimension
    assert L.eoc_lut_batch_device(eng.h, None, 1, b, c, 4, None) == EOC_ERR_ARG
    assert L.eoc_lut_batch_device(eng.h, a, 1, None, c, 4, None) == EOC_ERR_ARG
    assert L.eoc_lut_batch_device(eng.h, a, 1, b, None, 4, None) == EOC_ERR_ARG
    assert L.eoc_lut_test_polynomial(16, np.zeros(16, np.int32).ctypes.data, np.zeros(N, np.int32).ctypes.data) == EOC_ERR_ARG
