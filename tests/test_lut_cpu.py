"""Programmable bootstrapping, host side (no GPU): the test-polynomial rule, the small-integer encoding, a bootstrap
composed on the CPU oracle from the library's test polynomial, argument checks.  GPU side: tests/test_gpu_lut.py."""
import ctypes as C

import numpy as np
import pytest

import lut_oracle as lo
import oracle_lib as ol

N = 1024
EOC_ERR_ARG = -1


@pytest.fixture(scope="module")
def eoc(built_lib):
    import eoc_tfhe_amd
    return eoc_tfhe_amd


def const_coef_after_rotation(tv, b):
    """constant coefficient of X^(-b) tv, b in [0, 2N), as an unsigned word: tv[b], or -tv[b - N] in the negacyclic half"""
    return (np.int64(tv[b]) if b < N else -np.int64(tv[b - N])) & 0xFFFFFFFF


@pytest.mark.parametrize("p", [2, 4, 8])
def test_test_polynomial_rule(eoc, p):
    """every rotation the mod switch makes of the error-free phase m / (2p), shifted by up to N / (2p) - 1 steps either
    way, reads table[m] (m < p) or -table[m - p] (padding half)"""
    rng = np.random.default_rng(p)
    table = rng.integers(-2**31, 2**31, p).astype(np.int32)
    tv = eoc.lut_test_polynomial(p, table)
    half = N // (2 * p)
    assert np.array_equal(tv[N - half:], (-table[0].astype(np.int64)).astype(np.uint32).view(np.int32).repeat(half))
    for m in range(2 * p):
        want = (np.int64(table[m]) if m < p else -np.int64(table[m - p])) & 0xFFFFFFFF
        centre = m * N // p
        for d in range(-(half - 1), half):
            b = (centre + d) % (2 * N)
            assert const_coef_after_rotation(tv, b) == want, (p, m, d)
            # the same through a full polynomial rotation (the oracle's coefficient rule)
            if d in (-(half - 1), 0, half - 1):
                assert np.int64(lo.rotate(tv, (2 * N - b) % (2 * N))[0]) & 0xFFFFFFFF == want


@pytest.mark.parametrize("p", [2, 4, 8])
def test_encrypt_ints_roundtrip_and_oracle_bytes(eoc, p):
    params = eoc.default_params(0)
    sk = eoc.SecretKey(params, 3, with_cloud_key=False)
    orc = ol.Oracle(0, 3, with_bk=False)
    assert np.array_equal(sk.lwe_key, orc.lwe_key)
    vals = np.tile(np.arange(p), 40).astype(np.uint8)
    cts = sk.encrypt_ints(vals, p, 77, first_idx=5)
    assert np.array_equal(sk.decrypt_ints(cts, p), vals)
    assert np.array_equal(sk.encrypt_ints(vals, p, 77, first_idx=5), cts)              # reproducible stream
    L = orc.L
    for s in range(0, len(vals), 7):
        mu = (int(vals[s]) << 32) // (2 * p)
        mu = mu - (1 << 32) if mu >= 1 << 31 else mu
        ref = np.zeros(orc.n + 1, np.int32)
        L.orc_lwe_encrypt(C.byref(orc.p), orc.lwe_key, 77, 5 + s, mu, params.ks_stdev, ref)
        assert np.array_equal(cts[s], ref), s                                          # same stream, same bytes
        ph = L.orc_lwe_phase(C.byref(orc.p), orc.lwe_key, cts[s])
        assert ph == sk.phase(cts[s])
        err = ((ph - mu + 2**31) % 2**32) - 2**31
        assert abs(err) < 2**32 // (4 * p) // 8                                        # fresh noise: far inside the margin


@pytest.mark.parametrize("pset", [0, 1], ids=["setA", "setB"])
@pytest.mark.parametrize("p", [2, 4, 8])
def test_composed_oracle_bootstrap_applies_the_table(eoc, pset, p):
    """the library's test polynomial through the oracle's mod switch, blind-rotation steps, extraction and key switch
    (small n) gives f(m) for every m, and -f(m - p) for padding-half inputs"""
    params = eoc.default_params(pset)
    params.n = 40
    sk = eoc.SecretKey(params, 11, with_cloud_key=False)
    orc = ol.Oracle(pset, 11, n_override=40)
    assert np.array_equal(sk.lwe_key, orc.lwe_key)
    f = lambda m: (3 * m + 1) % p
    tv = eoc.lut_test_polynomial(p, lo.int_table(f, p, p))
    vals = np.arange(p, dtype=np.uint8)
    cts = sk.encrypt_ints(vals, p, 900 + p)
    pad = np.zeros((p, params.n + 1), np.int32)                                        # m in [p, 2p): the padding half
    for m in range(p, 2 * p):
        mu = np.int64((m << 32) // (2 * p)).astype(np.uint32).view(np.int32)
        assert eoc.lib().eoc_lwe_encrypt(sk.h, 950 + p, m, int(mu), params.ks_stdev, pad[m - p].ctypes.data) == 0
    out = lo.lut_batch(orc, tv, np.concatenate([cts, pad]))[0]
    got = sk.decrypt_ints(out, p)
    assert got[:p].tolist() == [f(m) for m in range(p)]
    assert got[p:].tolist() == [(-f(m)) % p for m in range(p)]


def test_arguments_are_refused(eoc):
    L = eoc.lib()
    sk = eoc.SecretKey(eoc.default_params(0), 3, with_cloud_key=False)
    table = np.zeros(16, np.int32)
    tv = np.zeros(N, np.int32)
    vals = np.zeros(4, np.uint8)
    cts = np.zeros((4, sk.n + 1), np.int32)
    for p in (0, 1, 3, 16, 32):
        assert L.eoc_lut_test_polynomial(p, table.ctypes.data, tv.ctypes.data) == EOC_ERR_ARG
        assert L.eoc_encrypt_ints(sk.h, 1, 0, p, vals.ctypes.data, 4, cts.ctypes.data) == EOC_ERR_ARG
        assert L.eoc_decrypt_ints(sk.h, p, cts.ctypes.data, 4, vals.ctypes.data) == EOC_ERR_ARG
    assert L.eoc_lut_test_polynomial(4, None, tv.ctypes.data) == EOC_ERR_ARG
    assert L.eoc_lut_test_polynomial(4, table.ctypes.data, None) == EOC_ERR_ARG
    assert L.eoc_encrypt_ints(None, 1, 0, 4, vals.ctypes.data, 4, cts.ctypes.data) == EOC_ERR_ARG
    assert L.eoc_encrypt_ints(sk.h, 1, 0, 4, None, 4, cts.ctypes.data) == EOC_ERR_ARG
    assert L.eoc_decrypt_ints(sk.h, 4, None, 4, vals.ctypes.data) == EOC_ERR_ARG
    before = cts.copy()
    bad = np.array([0, 1, 4, 2], np.uint8)                                             # 4 is not in Z_4
    assert L.eoc_encrypt_ints(sk.h, 1, 0, 4, bad.ctypes.data, 4, cts.ctypes.data) == EOC_ERR_ARG
    assert np.array_equal(cts, before)                                                  # nothing written
    with pytest.raises(eoc.EocError):
        eoc.lut_test_polynomial(16, np.zeros(16, np.int32))
    # the engine entry point checks its arguments before it needs a device
    assert L.eoc_lut_batch_device(None, tv.ctypes.data, 1, cts.ctypes.data, cts.ctypes.data, 4, None) == EOC_ERR_ARG
