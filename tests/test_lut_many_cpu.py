"""Many-LUT bootstrapping, host side (no GPU): the packed test-polynomial rule, argument checks, the coarse mod switch against
the oracle's and its noise, a many-LUT bootstrap composed on the CPU oracle, and the noise margins that bound p T.  GPU side:
tests/test_gpu_lut_many.py."""
import numpy as np
import pytest

import lut_many_oracle as lmo
import lut_oracle as lo
import oracle_lib as ol
from eoc_tfhe_amd import noise

N = 1024
EOC_ERR_ARG = -1
SUPPORTED = [(T, p) for T in (2, 4, 8) for p in (2, 4, 8) if p * T <= 16]


@pytest.fixture(scope="module")
def eoc(built_lib):
    import eoc_tfhe_amd
    return eoc_tfhe_amd


def F(table, p, x):
    """DESIGN.md 10.1's F_j at x in [0, 2N), extended negacyclically: table[(x p + N/2) / N] below N - N/(2p), -table[0]
    up to N, and -F(x - N) on the padding half -- as an unsigned word"""
    if x >= N:
        return (-np.int64(F(table, p, x - N))) & 0xFFFFFFFF
    v = np.int64(table[(x * p + N // 2) // N]) if x < N - N // (2 * p) else -np.int64(table[0])
    return v & 0xFFFFFFFF


@pytest.mark.parametrize("T,p", SUPPORTED)
def test_packed_rule_is_the_single_table_rule_sampled_on_the_grid(eoc, T, p):
    rng = np.random.default_rng(10 * T + p)
    tables = rng.integers(-2**31, 2**31, (T, p)).astype(np.int32)
    tv = eoc.lut_many_test_polynomial(p, tables)
    singles = [eoc.lut_test_polynomial(p, tables[j]) for j in range(T)]
    for k in range(N // T):
        for j in range(T):
            assert tv[k * T + j] == singles[j][k * T], (k, j)
    # coefficient j of X^(-kT) tv is F_j(kT) for every multiple of T in [0, 2N): the last region and the padding half too
    for k in range(2 * N // T):
        b = k * T
        rot = lo.rotate(tv, (2 * N - b) % (2 * N))
        for j in range(T):
            assert np.int64(rot[j]) & 0xFFFFFFFF == F(tables[j], p, b), (T, p, b, j)


def test_arguments_are_refused(eoc):
    L = eoc.lib()
    tabs = np.zeros(64, np.int32)
    tv = np.zeros(N, np.int32)
    for T, p in [(0, 2), (1, 2), (3, 2), (16, 2), (2, 3), (2, 16), (4, 8), (8, 4), (8, 8), (2, 0)]:
        assert L.eoc_lut_many_test_polynomial(p, T, tabs.ctypes.data, tv.ctypes.data) == EOC_ERR_ARG, (T, p)
    assert L.eoc_lut_many_test_polynomial(4, 2, None, tv.ctypes.data) == EOC_ERR_ARG
    assert L.eoc_lut_many_test_polynomial(4, 2, tabs.ctypes.data, None) == EOC_ERR_ARG
    assert L.eoc_lut_many_test_polynomial(4, 2, tabs.ctypes.data, tv.ctypes.data) == 0
    with pytest.raises(eoc.EocError):
        eoc.lut_many_test_polynomial(8, np.zeros((4, 8), np.int32))           # p T = 32
    with pytest.raises(eoc.EocError):
        eoc.lut_many_test_polynomial(4, np.zeros((2, 3), np.int32))           # rows are not [p]
    # the engine entry point checks its arguments before it needs a device
    cts = np.zeros((4, 501), np.int32)
    assert L.eoc_lut_many_batch_device(None, 2, tv.ctypes.data, 1, cts.ctypes.data, cts.ctypes.data, 4, None) == EOC_ERR_ARG


def test_coarse_mod_switch_is_the_oracles_at_t1_and_on_the_grid_above(eoc):
    L = ol.lib()
    orc = ol.Oracle(0, 1, with_bk=False)
    rng = np.random.default_rng(4)
    t = rng.integers(-2**31, 2**31, (64, orc.n + 1)).astype(np.int32)
    t[0, :8] = [0, -1, 1 << 20, (1 << 20) - 1, -(1 << 20), 2**31 - 1, -2**31, (1 << 21) + (1 << 20)]   # rounding edges
    bara, barb = np.zeros(orc.n, np.int32), np.zeros(1, np.int32)
    for r in range(t.shape[0]):
        L.orc_modswitch_sample(ol.C.byref(orc.p), np.ascontiguousarray(t[r]), bara, barb)
        got = lmo.modswitch_coarse(t[r], 1)
        assert np.array_equal(got[:orc.n].astype(np.int32).tobytes(), bara.tobytes()), r
        assert int(got[orc.n]) == int(barb[0])
    for T in (2, 4, 8):
        got = lmo.modswitch_coarse(t, T).astype(np.int64)
        assert np.all(got % T == 0) and got.min() >= 0 and got.max() < 2 * N
        want = np.floor((t.astype(np.int64) & 0xFFFFFFFF) * (2 * N / T) / 2.0**32 + 0.5).astype(np.int64) * T % (2 * N)
        assert np.array_equal(got, want), T


@pytest.mark.parametrize("pset", [0, 1], ids=["setA", "setB"])
def test_coarse_mod_switch_noise_is_t_squared(eoc, pset):
    """16 384 fresh encryptions: the phase error the coarse mod switch adds (phase of (abar, barb) under the LWE key, in
    units of 1/(2N), against the sample's phase) has variance (1 + |s|) T^2 / (48 N^2), within the output-noise tests' 5 %"""
    params = eoc.default_params(pset)
    sk = eoc.SecretKey(params, 5, with_cloud_key=False)
    count = 16384
    vals = (np.arange(count) % 4).astype(np.uint8)
    cts = sk.encrypt_ints(vals, 4, 6100 + pset)
    s = sk.lwe_key.astype(np.int64)
    c = cts.astype(np.int64)
    ph = ((c[:, -1] - c[:, :-1] @ s) & 0xFFFFFFFF) / 2.0**32
    for T in (1, 2, 4, 8):
        bar = lmo.modswitch_coarse(cts, T).astype(np.int64)
        phs = ((bar[:, -1] - bar[:, :-1] @ s) % (2 * N)) / (2.0 * N)
        err = (phs - ph + 0.5) % 1.0 - 0.5
        pred = noise.modswitch_var(sk.lwe_key, T)
        ratio = err.var() / pred
        print(f"pset {pset} T {T}: var {err.var():.4e} predicted {pred:.4e} ratio {ratio:.4f}")
        assert abs(ratio - 1) < 0.05, (T, ratio)
        assert abs(err.mean()) < 5 * err.std() / np.sqrt(count), (T, err.mean())


@pytest.mark.parametrize("pset", [0, 1], ids=["setA", "setB"])
@pytest.mark.parametrize("T,p", [(2, 8), (4, 4), (8, 2)])
def test_composed_oracle_many_lut_bootstrap_applies_every_table(eoc, pset, T, p):
    """the packed polynomial through the coarse mod switch, the oracle's blind-rotation steps, extraction at 0 .. T - 1 and
    the key switch (small n) gives table j's value in slot j for every m, and -table j for padding-half inputs"""
    params = eoc.default_params(pset)
    params.n = 40
    sk = eoc.SecretKey(params, 11, with_cloud_key=False)
    orc = ol.Oracle(pset, 11, n_override=40)
    fs = [lambda m, j=j: (m + j) % p if j % 2 == 0 else (3 * m + j) % p for j in range(T)]
    tv = eoc.lut_many_test_polynomial(p, [lo.int_table(f, p, p) for f in fs])
    rows = np.zeros((2 * p, params.n + 1), np.int32)
    for m in range(2 * p):                                                          # m in [p, 2p): the padding half
        mu = np.int64((m << 32) // (2 * p)).astype(np.uint32).view(np.int32)
        assert eoc.lib().eoc_lwe_encrypt(sk.h, 970 + p, m, int(mu), params.ks_stdev, rows[m].ctypes.data) == 0
    out = lmo.lut_many_batch(orc, tv, rows, T)[0]
    assert out.shape == (T, 2 * p, params.n + 1)
    for j, f in enumerate(fs):
        got = sk.decrypt_ints(out[j], p)
        assert got[:p].tolist() == [f(m) for m in range(p)], j
        assert got[p:].tolist() == [(-f(m)) % p for m in range(p)], j
    # at T = 1 the composition is tests/lut_oracle.py's single-table bootstrap, byte for byte
    tv1 = eoc.lut_test_polynomial(p, lo.int_table(fs[1], p, p))
    for r in (0, p - 1, p + 1):
        assert np.array_equal(lmo.bootstrap_many(orc, tv1, rows[r], 1)[0], lo.bootstrap(orc, tv1, rows[r]))


def test_margins_reproduce_section_10_and_bound_p_times_t(eoc):
    """noise.lut_margin_sigma at T = 1 is DESIGN.md 10's table (key 1, which states two digits: 5 %); every supported (T, p)
    keeps 5 sigma or more with one input on both sets, and p T = 32 would not"""
    sec10 = {0: {2: (26, 20), 4: (13, 9.8), 8: (6.6, 4.9), 16: (3.3, 2.5)},
             1: {2: (29, 23), 4: (15, 11), 8: (7.3, 5.7), 16: (3.7, 2.8)}}
    for pset in (0, 1):
        params = eoc.default_params(pset)
        sk = eoc.SecretKey(params, 1, with_cloud_key=False)
        args = (params, sk.lwe_key, sk.tlwe_key)
        for p, (one, two) in sec10[pset].items():
            assert noise.lut_margin_sigma(*args, p) == pytest.approx(one, rel=0.05), (pset, p)
            assert noise.lut_margin_sigma(*args, p, inputs=2) == pytest.approx(two, rel=0.05), (pset, p)
        for T, p in SUPPORTED:
            m = noise.lut_margin_sigma(*args, p, n_tables=T)
            assert 5.0 <= m < noise.lut_margin_sigma(*args, p), (pset, T, p, m)
        assert noise.lut_margin_sigma(*args, 8, n_tables=4) < 3.5
