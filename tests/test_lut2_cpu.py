"""Two-input table lookups, host side (no GPU): the level-1 test polynomials and their refusals, the composed
reference (tests/lut2_oracle.py) on exactly the keys, seeds and inputs the GPU tests compare with, its output noise against
noise.lut2_var / lut2_mean, and the model's statement about a following lookup.  GPU side: tests/test_gpu_lut2.py,
tests/test_gpu_lut2_instances.py; registers: tests/test_isa_lut2.py."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import lut2_oracle as l2
import lut_oracle as lo
from eoc_tfhe_amd import noise

N = 1024
EOC_OK, EOC_ERR_ARG = 0, -1
ALLOWED = [(p, T) for p in (2, 4, 8) for T in (1, 2, 4, 8) if p % T == 0 and (T == 1 or p * T <= 16)]


@pytest.fixture(scope="module")
def eoc(built_lib):
    import eoc_tfhe_amd
    return eoc_tfhe_amd


def test_allowed_shapes_are_what_the_issue_lists():
    assert ALLOWED == [(2, 1), (2, 2), (4, 1), (4, 2), (4, 4), (8, 1), (8, 2)]


@pytest.mark.parametrize("p,T", ALLOWED)
def test_level1_polynomials_against_a_numpy_restatement(eoc, p, T):
    rng = np.random.default_rng(10 * p + T)
    table = rng.integers(-2**31, 2**31, (p, p)).astype(np.int32)
    tv = eoc.lut2_test_polynomials(p, table, T)
    assert tv.shape == (p // T, N) and tv.dtype == np.int32
    k = np.arange(N)
    top = N - N // (2 * p)
    for g in range(p // T):
        for j in range(T):
            col = table[:, g * T + j].astype(np.int64)                   # x -> F(x, y), y = g T + j
            kk = (k // T) * T                                            # the rule sampled on the T-grid, in coefficient kT + j
            want = np.where(kk < top, col[np.minimum((kk * p + N // 2) // N, p - 1)], -col[0])
            sel = k % T == j
            assert np.array_equal(tv[g][sel].astype(np.int64) & 0xFFFFFFFF, want[sel] & 0xFFFFFFFF), (g, j)
    # the layouts the issue names: eoc_lut_test_polynomial at T = 1, eoc_lut_many_test_polynomial above
    for g in range(p // T):
        cols = [table[:, g * T + j] for j in range(T)]
        ref = eoc.lut_test_polynomial(p, cols[0]) if T == 1 else eoc.lut_many_test_polynomial(p, cols)
        assert np.array_equal(tv[g], ref), g
    # n_tables = 0 means one table per rotation, as 1 does
    assert np.array_equal(eoc.lut2_test_polynomials(p, table, 0), eoc.lut2_test_polynomials(p, table, 1))


def test_refusals(eoc):
    L = eoc.lib()
    tab, tv = np.zeros(64, np.int32), np.zeros(8 * N, np.int32)
    bad = [(p, T) for p in (0, 1, 3, 16) for T in (1, 2)] + [(2, 4), (2, 8), (4, 8), (8, 4), (8, 8), (4, 3), (8, 16), (4, -1)]
    for p, T in bad:
        assert L.eoc_lut2_test_polynomials(p, T, tab.ctypes.data, tv.ctypes.data) == EOC_ERR_ARG, (p, T)
    assert L.eoc_lut2_test_polynomials(4, 1, None, tv.ctypes.data) == EOC_ERR_ARG
    assert L.eoc_lut2_test_polynomials(4, 1, tab.ctypes.data, None) == EOC_ERR_ARG
    for p, T in ALLOWED:
        assert L.eoc_lut2_test_polynomials(p, T, tab.ctypes.data, tv.ctypes.data) == EOC_OK, (p, T)
    with pytest.raises(eoc.EocError):
        eoc.lut2_test_polynomials(4, np.zeros((4, 3), np.int32))
    with pytest.raises(eoc.EocError):
        eoc.lut2_test_polynomials(8, np.zeros((8, 8), np.int32), 4)
    # the engine entry points check their arguments before they need a device
    x = np.zeros((4, 501), np.int32)
    a = x.ctypes.data
    assert L.eoc_lut2_batch_device(None, 4, 1, a, 1, a, a, a, 4, None) == EOC_ERR_ARG
    assert L.eoc_lut_enc_batch_device(None, a, 1, 0, a, a, 4, None) == EOC_ERR_ARG
    assert L.eoc_tv_pack_device(None, 4, a, 1, 4, a, None) == EOC_ERR_ARG


def test_tv_batch_is_the_test_polynomial_rule_on_samples(eoc):
    """row k of the N-row batch is sample j(k), the last N / (2p) rows sample 0 negated: column m of the batch is
    eoc_lut_test_polynomial of the column's p words"""
    rng = np.random.default_rng(5)
    for p in (2, 4, 8):
        vals = rng.integers(-2**31, 2**31, (p, 7)).astype(np.int32)
        vals[0, 0], vals[0, 1] = -2**31, 0                                # words that are their own negation
        batch = l2.tv_batch(vals, p)
        assert batch.shape == (N, 7)
        for m in range(7):
            assert np.array_equal(batch[:, m], eoc.lut_test_polynomial(p, vals[:, m])), (p, m)
        j, neg = l2.tv_slots(p)
        assert neg.sum() == N // (2 * p) and (np.flatnonzero(np.diff(j)) + 1).tolist() == \
            [b for b in range(N // (2 * p), N, N // p)] and all(b % 64 == 0 for b in range(N // (2 * p), N, N // p))


@pytest.mark.parametrize("pset", [0, 1], ids=["setA", "setB"])
@pytest.mark.parametrize("T", [1, 2])
def test_all_16_pairs_decrypt_on_the_reference(eoc, pset, T):
    """the shared inputs of the GPU tests, on the reference alone: every row of both functions (the digit product's low and
    high base-4 digit) decrypts to F(x, y), every stage decrypts to what it should hold"""
    assert l2.decodable(eoc, noise, pset, 4, T), (pset, T)
    params, sk, _, _, orc = l2.keys(eoc, pset)
    case = l2.shared_case(eoc, pset, 4, T)
    assert case["out"].shape == (2, 16, params.n + 1) and sorted(zip(case["xv"], case["yv"])) == [(x, y) for x in range(4) for y in range(4)]
    for f, F in enumerate(l2.functions(4)):
        want = np.array([F(int(x), int(y)) for x, y in zip(case["xv"], case["yv"])], np.uint8)
        assert np.array_equal(case["want"][f], want)
        assert np.array_equal(sk.decrypt_ints(case["out"][f], 4), want), (pset, T, f)
        for y in range(4):                                                # level 1: value y of row s is F(x_s, y)
            assert np.array_equal(sk.decrypt_ints(case["vals"][f, y], 4), [F(int(x), y) for x in case["xv"]]), (f, y)
        ph = sk.list_phases(case["lists"][f]).astype(np.int64)            # the lists: windows of N / 4 coefficients
        dec = ((ph * 8 + (1 << 31)) >> 32) % 4
        for y in range(4):
            mid = y * (N // 4)
            assert np.array_equal(dec[:, mid], [F(int(x), y) for x in case["xv"]]), (f, y)
    assert l2.PROD_LO(3, 3) == 1 and l2.PROD_HI(3, 3) == 2


def test_case_below_six_sigma_is_not_decoded(eoc):
    """DESIGN.md 10.1's table: (T, p) = (4, 4) on Set B is below the decode rule's bound, on Set A above it"""
    assert not l2.decodable(eoc, noise, 1, 4, 4)
    assert l2.decodable(eoc, noise, 0, 4, 4) and l2.decodable(eoc, noise, 0, 4, 1) and l2.decodable(eoc, noise, 1, 4, 1)


def _errors(sk, out, want, p):
    ph = (np.asarray(out, np.int64)[:, -1] - np.asarray(out, np.int64)[:, :-1] @ sk.lwe_key.astype(np.int64))
    msg = (want.astype(np.int64) << 32) // (2 * p)
    return ((((ph - msg) + 2**31) % 2**32) - 2**31) / 2.0**32


@pytest.mark.parametrize("pset", [0, 1], ids=["setA", "setB"])
def test_reference_noise_matches_lut2_var(eoc, pset):
    """S = 256 reference samples, p = 4, T = 1, random (x, y): the output error's variance within 1 +- 3.5 sqrt(2 / (S - 1)) of
    noise.lut2_var and its mean within 4 standard errors of noise.lut2_mean -- the sampling spread, not tolerances.  F is the
    digit sum: lut2_oracle.SUM_LO says why not the product"""
    S, p = 256, 4
    params, sk, _, kfft, orc = l2.keys(eoc, pset)
    rng = np.random.default_rng(900 + pset)
    xv, yv = rng.integers(0, p, S).astype(np.uint8), rng.integers(0, p, S).astype(np.uint8)
    x, y = sk.encrypt_ints(xv, p, 3100 + pset), sk.encrypt_ints(yv, p, 3200 + pset)
    tv0 = eoc.lut2_test_polynomials(p, l2.lut2_tables(l2.SUM_LO, p), 1)[None]
    out = l2.lut2_batch(orc, kfft, p, 1, tv0, x, y)[0]                    # pooled over threads inside
    want = np.array([l2.SUM_LO(int(a), int(b)) for a, b in zip(xv, yv)], np.uint8)
    assert np.array_equal(sk.decrypt_ints(out, p), want)
    err = _errors(sk, out, want, p)
    var_pred = noise.lut2_var(params, sk.lwe_key, sk.tlwe_key, sk.ksk)
    mean_pred = noise.lut2_mean(params, sk.lwe_key, sk.tlwe_key, sk.ksk)
    ratio = err.var(ddof=1) / var_pred
    z = (err.mean() - mean_pred) / (err.std(ddof=1) / np.sqrt(S))
    print(f"pset {pset}: sigma {err.std():.4e} predicted {np.sqrt(var_pred):.4e} variance ratio {ratio:.4f}; mean {err.mean():.3e} "
          f"predicted {mean_pred:.3e} ({z:+.2f} se)")
    assert abs(ratio - 1) <= 3.5 * np.sqrt(2.0 / (S - 1)), ratio
    assert abs(z) <= 4, z


@pytest.mark.parametrize("pset", [0, 1], ids=["setA", "setB"])
def test_model_a_lut2_output_feeds_a_single_input_lookup(eoc, pset):
    """from the model alone: a lut2 output at p = 4 keeps >= 6 sigma as the single input of a p = 4 lookup; its variance is
    about twice a gate output's, and step 0 counts as a regular step"""
    params = eoc.default_params(pset)
    sk = eoc.SecretKey(params, l2.KEY_SEED, with_cloud_key=False)
    args = (params, sk.lwe_key, sk.tlwe_key)
    pr = noise.predict(*args)
    v2 = noise.lut2_var(*args)
    m = noise.lut_margin_sigma_var(4, 1, v2, sk.lwe_key)
    print(f"pset {pset}: lut2 sigma {np.sqrt(v2):.4e} = {np.sqrt(v2 / pr['total_var']):.3f} x a gate output's; a following p = 4 "
          f"lookup keeps {m:.2f} sigma")
    assert m >= 6.0
    assert 1.9 < v2 / pr["total_var"] < 2.2
    assert noise.br_enc_var(*args) > pr["br_var"]                         # the regular step 0
    assert noise.br_enc_var(*args) < pr["br_var"] * (1 + 2.0 / params.n)
    assert v2 == pytest.approx(pr["total_var"] + noise.pack_var(params, sk.lwe_key, N) + noise.br_enc_var(*args) + pr["ks_var"])
    l1, l2m = noise.lut2_margin_sigma(4, 2, *args)
    assert l1 == pytest.approx(noise.lut_margin_sigma(*args, 4, n_tables=2)) and l2m == pytest.approx(noise.lut_margin_sigma(*args, 4))
