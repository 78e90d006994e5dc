"""Inner products with public integer weights, host side (include/eoc_tfhe_gpu.h): the new symbols, compact
lists of arbitrary Torus32 messages, the chunked reference (tests/c/dot_ref.c) against exact wrapping-integer arithmetic,
the output noise against noise.linear_var / linear_offset, and the network model of eoc_tfhe_amd/dinn.py.
GPU side: tests/test_gpu_dot.py; registers: tests/test_isa_dot.py."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import compact_oracle as co
import dot_oracle as do
from eoc_tfhe_amd import dinn, noise

N = 1024
EOC_OK, EOC_ERR_ARG = 0, -1
INT32_MIN, INT32_MAX = -(2**31), 2**31 - 1


@pytest.fixture(scope="module")
def eoc(built_lib):
    import eoc_tfhe_amd
    return eoc_tfhe_amd


def test_symbols_and_argument_errors(eoc):
    L = eoc.lib()
    new = {"eoc_weights_image_bytes", "eoc_weights_to_device", "eoc_dot_device", "eoc_linear_device", "eoc_engine_dot_launches",
           "eoc_linear", "eoc_pk_encrypt_torus", "eoc_pk_encrypt_torus_keyed"}
    assert new <= set(eoc.abi_symbols()) and all(hasattr(L, s) for s in new)
    assert all(hasattr(eoc.Engine, m) for m in ("weights_to_device", "dot_device", "linear_device", "dot_launches"))
    assert callable(eoc.linear) and hasattr(eoc.PublicKey, "encrypt_torus") and L.eoc_engine_dot_launches(None) == 0
    # [rows][L][512] complex spectra + the zero-padded int8 weights; refused shapes have no image
    assert L.eoc_weights_image_bytes(1, 1) == 8192 + 1024 and L.eoc_weights_image_bytes(5, N + 3) == 5 * 2 * (8192 + 1024)
    assert L.eoc_weights_image_bytes(0, 4) == 0 and L.eoc_weights_image_bytes(4, 0) == 0
    assert L.eoc_weights_image_bytes(2**20 + 1, 4) == 0 and L.eoc_weights_image_bytes(4, 2**20 + 1) == 0
    x = np.zeros(8, np.int32)
    ptr = x.ctypes.data                                                    # never followed: every call below is refused first
    for call in (lambda: L.eoc_weights_to_device(None, ptr, 1, 1, ptr, None), lambda: L.eoc_dot_device(None, ptr, 1, 1, ptr, 1, None, ptr, None),
                 lambda: L.eoc_linear_device(None, ptr, 1, 1, ptr, 1, None, ptr, None), lambda: L.eoc_linear(None, 1, 1, ptr, 1, None, ptr),
                 lambda: L.eoc_linear(ptr, 1, 1, None, 1, None, ptr), lambda: L.eoc_linear(ptr, 1, 1, ptr, 1, None, None)):
        assert call() == EOC_ERR_ARG
    with pytest.raises(eoc.EocError):
        eoc.linear(np.full((1, 4), -128), np.zeros((1, 1, 2, N), np.int32))
    with pytest.raises(eoc.EocError):
        eoc.linear(np.ones((1, 4), np.int8), np.zeros((1, 2, 2, N), np.int32))


@pytest.mark.parametrize("pset", [0, 1])
def test_torus_lists_equal_the_bit_and_integer_lists(eoc, pset):
    """the same streams, u, e1 and e2: the messages of _bits (+-2^29) and of _ints give their lists byte for byte, keyed or
    seeded, and the oracle-stream restatement gives the same words for arbitrary messages"""
    p = eoc.default_params(pset)
    sk = eoc.SecretKey(p, 5, with_cloud_key=False)
    pk = eoc.PublicKey(sk.public_key_bytes())
    rng = np.random.default_rng(1)
    bits = rng.integers(0, 2, N + 7).astype(np.uint8)
    assert np.array_equal(pk.encrypt_torus(co.bit_msgs(bits), 21, 3), pk.encrypt_bits(bits, 21, 3))
    vals = rng.integers(0, 8, N + 7).astype(np.uint8)
    assert np.array_equal(pk.encrypt_torus(co.int_msgs(vals, 8), 22), pk.encrypt_ints(vals, 8, 22))
    L = eoc.lib()
    key = np.arange(32, dtype=np.uint8)
    a, b = np.empty((2, 2, N), np.int32), np.empty((2, 2, N), np.int32)
    m = np.ascontiguousarray(co.bit_msgs(bits), np.int32)
    assert L.eoc_pk_encrypt_torus_keyed(pk.blob, len(pk.blob), key.ctypes.data, 4, m.ctypes.data, m.size, a.ctypes.data) == EOC_OK
    assert L.eoc_pk_encrypt_bits_keyed(pk.blob, len(pk.blob), key.ctypes.data, 4, bits.ctypes.data, bits.size, b.ctypes.data) == EOC_OK
    assert np.array_equal(a, b)
    msgs = rng.integers(INT32_MIN, INT32_MAX, 40, endpoint=True)
    A, B = co.public_key(5, sk.tlwe_key, p.bk_stdev)
    lists = pk.encrypt_torus(msgs, 23, 1)
    assert np.array_equal(lists, co.encrypt(A, B, 23, 1, msgs, p.bk_stdev))
    # list_phases returns the messages plus noise (slots past the end: 0 plus noise)
    err = (sk.list_phases(lists).astype(np.int64)[0] - np.r_[msgs, np.zeros(N - 40, np.int64)] + 2**31) % 2**32 - 2**31
    assert np.abs(err / 2.0**32).max() < 8 * np.sqrt(noise.compact_var(p, sk.tlwe_key, pk))
    assert pk.encrypt_torus(msgs).shape == (1, 2, N)                       # secure mode: a fresh key per call
    bad = np.zeros(4, np.int32)
    assert L.eoc_pk_encrypt_torus(pk.blob, len(pk.blob), 1, 0, None, 4, bad.ctypes.data) == EOC_ERR_ARG
    assert L.eoc_pk_encrypt_torus(pk.blob[:100], 100, 1, 0, bad.ctypes.data, 4, bad.ctypes.data) == EOC_ERR_ARG


def _check_chunks(w, lists, chunks, label):
    """body word for word; per converted chunk the mask within 8 LSB of exact arithmetic; returns (worst LSB, high water)"""
    hwm = np.zeros(1)
    worst = 0
    for c in range(chunks):
        ref = do.sample(w, lists, 12345, c, c + 1, hwm)
        exact = do.sample_exact(w, lists, 12345, c, c + 1)
        assert ref[N] == exact[N], label
        d = do.lsb_deviation(ref[:N], exact[:N])
        print(f"{label}: chunk {c}: max |reference - exact| = {d} LSB")
        assert d <= 8, (label, c, d)
        worst = max(worst, d)
    print(f"{label}: high-water mark before conversion 2^{np.log2(max(hwm[0], 1.0)):.2f}")
    assert hwm[0] < 2.0**51
    return worst, hwm[0]


def test_reference_against_exact_arithmetic():
    """one full chunk (L = 8), L = 9 (a chunk of one list behind a full one) and the full-scale chunk: every weight +127
    against list words all INT32_MIN, then all INT32_MAX.  Bound: 8 LSB per converted chunk (DESIGN.md 13's bound for the same
    conversion); measured here: 1 LSB in every chunk, high-water mark 2^44.9 (random) / 2^50.99 (full scale)"""
    rng = np.random.default_rng(2)
    for L in (8, 9):
        w = rng.integers(-127, 128, L * N).astype(np.int8)
        w[:4] = (127, -127, 0, 1)
        lists = rng.integers(INT32_MIN, INT32_MAX, (L, 2, N), endpoint=True).astype(np.int32)
        _check_chunks(w, lists, (L + 7) // 8, f"L = {L}")
        # the chunks add up: the whole sample is the word-wise sum of its chunks' masks, the body is whole in each
        full = do.sample(w, lists, 12345).astype(np.int64)
        parts = sum(do.sample(w, lists, 12345, c, c + 1).astype(np.int64)[:N] for c in range((L + 7) // 8))
        assert np.array_equal((full[:N] - parts) % 2**32, np.zeros(N, np.int64))
        assert np.array_equal(full, do.sample(w, lists, 12345, 0, (L + 7) // 8).astype(np.int64))
    w = np.full(8 * N, 127, np.int8)
    for word in (INT32_MIN, INT32_MAX):
        _, hw = _check_chunks(w, np.full((8, 2, N), word, np.int32), 1, f"full scale, words {word}")
        assert hw > 2.0**49                                                # the shape does reach the top of the range
    # the batch form and the plain sum agree with the single-sample form
    w2 = rng.integers(-127, 128, (3, N + 5))
    lists = rng.integers(INT32_MIN, INT32_MAX, (2, 2, 2, N), endpoint=True).astype(np.int32)
    bias = rng.integers(INT32_MIN, INT32_MAX, 3).astype(np.int32)
    out = do.dot(w2, lists, bias)
    assert out.shape == (2, 3, N + 1)
    assert np.array_equal(out[1, 2], do.sample(do.padded(w2)[2], lists[1], bias[2]))


_NOISE = {}


def _noise_run(eoc, pset, rows, M=4096):
    """M (vector, row) samples through the reference, every vector one fresh list of 1 024 messages: rows = 1 pairs every
    vector with the ONE row w[0]; rows = M pairs vector b with row b, M independent rows of 1 024 random int8 weights.
    (params, sk, pk, w [rows][N], the M errors = output phase minus the plain sum, torus units); once per (set, rows)"""
    if (pset, rows) not in _NOISE:
        p = eoc.default_params(pset)
        sk = eoc.SecretKey(p, 5, with_cloud_key=False)
        pk = eoc.PublicKey(sk.public_key_bytes())
        rng = np.random.default_rng(10 + pset + rows)
        w = rng.integers(-127, 128, (rows, N)).astype(np.int8)
        msgs = rng.integers(-(2**20), 2**20, (M, N))
        lists = pk.encrypt_torus(msgs, 31 + pset + rows).reshape(M, 1, 2, N)
        with ThreadPoolExecutor(16) as ex:
            out = np.stack(list(ex.map(lambda b: do.sample(w[b % rows], lists[b]), range(M)))).astype(np.int64)
        phase = out[:, N] - out[:, :N] @ np.asarray(sk.tlwe_key, np.int64)
        plain = (w.astype(np.int64)[np.arange(M) % rows] * msgs).sum(1)
        err = ((phase - plain + 2**31) % 2**32 - 2**31) / 2.0**32
        _NOISE[(pset, rows)] = (p, sk, pk, w, err)
    return _NOISE[(pset, rows)]


@pytest.mark.parametrize("pset", [0, 1])
def test_output_noise_matches_the_model(eoc, pset):
    """M = 4 096 (vector, row) samples, each one row of 1 024 random int8 weights on one fresh list: the output phase minus the
    plain sum, less the row's noise.linear_offset and over the square root of the row's noise.linear_var(compact_var), has
    variance 1 within 4 sqrt(2 / (M - 1)) = 0.088 and mean 0 within 4 standard errors.
    Why every sample has a row of its own: linear_var = ||w||^2 compact_var is the variance over lists AND rows of independent
    zero-mean weights -- the slots of one list share u and e1, and for ONE fixed row the cross terms do not vanish (the next
    test: noise.linear_var_row, 0.66 - 2.10 of linear_var over 200 rows, standard deviation 0.29).  Pooled over R independent
    rows the model's own deviation is 0.29 / sqrt(R): 0.0045 at R = M, a twentieth of the tolerance, and the M samples are
    independent, which is what the tolerance's 2 / (M - 1) assumes.  Measured: DESIGN.md 18."""
    M = 4096
    p, sk, pk, w, err = _noise_run(eoc, pset, M)
    cv = noise.compact_var(p, sk.tlwe_key, pk)
    want_var = np.array([noise.linear_var(p, r, cv) for r in w])
    want_mean = w.astype(np.float64) @ noise.compact_offset(sk.tlwe_key, pk)
    for r in (0, M - 1):                                                   # the offset of a row, both ways of naming the key
        assert noise.linear_offset(p, sk, w[r]) == noise.linear_offset(p, pk, w[r], sk.tlwe_key)
        assert abs(noise.linear_offset(p, sk, w[r]) - want_mean[r]) <= 1e-12 * np.abs(w[r].astype(np.float64)).sum()
    z = (err - want_mean) / np.sqrt(want_var)
    ratio = z.var(ddof=1)
    t = z.mean() / (z.std(ddof=1) / np.sqrt(M))
    print(f"pset {pset}: variance of the normalised errors {ratio:.4f}; mean {t:+.2f} standard errors; sigma of a sum "
          f"{np.sqrt(want_var.mean()):.3e}, |offset| up to {np.abs(want_mean).max():.3e}")
    assert err.size >= 4096 and abs(t) <= 4, t
    assert abs(ratio - 1) <= 4 * np.sqrt(2.0 / (M - 1)), ratio


@pytest.mark.parametrize("pset", [0, 1])
def test_output_noise_of_one_row_matches_the_exact_row_model(eoc, pset):
    """ONE row of 1 024 random int8 weights on M = 4 096 fresh lists against noise.linear_var_row, the variance of THIS row
    under THIS key (nothing fitted), within 4 sqrt(2 / (M - 1)), and the mean against noise.linear_offset within 4 standard
    errors; and over rows of random weights linear_var is linear_var_row's mean (200 rows: within 4 standard errors of the
    row-to-row spread)"""
    p, sk, pk, w, err = _noise_run(eoc, pset, 1)
    M = err.size
    row = noise.linear_var_row(p, w[0], sk.tlwe_key, pk)
    ratio = err.var(ddof=1) / row
    t = (err.mean() - noise.linear_offset(p, sk, w[0])) / (err.std(ddof=1) / np.sqrt(M))
    print(f"pset {pset}: measured var / linear_var_row = {ratio:.4f}; linear_var_row / linear_var = "
          f"{row / noise.linear_var(p, w[0], noise.compact_var(p, sk.tlwe_key, pk)):.4f}; mean {t:+.2f} standard errors")
    assert abs(ratio - 1) <= 4 * np.sqrt(2.0 / (M - 1)), ratio
    assert abs(t) <= 4, t
    rng = np.random.default_rng(77)
    cv = noise.compact_var(p, sk.tlwe_key, pk)
    r = np.array([noise.linear_var_row(p, wr, sk.tlwe_key, pk) / noise.linear_var(p, wr, cv) for wr in rng.integers(-127, 128, (200, N))])
    print(f"pset {pset}: linear_var_row / linear_var over 200 rows: mean {r.mean():.4f}, std {r.std():.4f}, range [{r.min():.3f}, {r.max():.3f}]")
    assert abs(r.mean() - 1) <= 4 * r.std(ddof=1) / np.sqrt(r.size)


# ---- the network model -------------------------------------------------------------------------------------------------------
def _net(rng, delta=1 << 24, mu=(1 << 32) // 36):
    l1 = dinn.DenseLayer(rng.integers(-3, 4, (8, 32)), None, dinn.sign_test_polynomial(mu))
    l2 = dinn.DenseLayer(rng.choice([-1, 1], (2, 8)), None, dinn.sign_test_polynomial(1 << 29))
    return dinn.Network([l1, l2], delta)


def test_test_polynomials_and_plain_evaluation():
    mu = 1 << 26
    assert np.array_equal(dinn.sign_test_polynomial(mu), np.full(N, mu, np.int32))
    assert np.array_equal(dinn.staircase_test_polynomial(1, mu), dinn.sign_test_polynomial(mu))
    st = dinn.staircase_test_polynomial(4, 7 * 1000)
    assert np.array_equal(st, st[::-1]) and sorted(set(st.tolist())) == [1000, 3000, 5000, 7000] and st[0] == 1000 and st[N // 2 - 1] == 7000
    x = np.array([1, (1 << 30) // 4 - (1 << 21), (1 << 30) // 4 + (1 << 21), (1 << 30) - (1 << 22)], np.int64)
    assert dinn.apply_test_polynomial(st, x).tolist() == [1000, 1000, 3000, 7000]
    assert np.array_equal(dinn.apply_test_polynomial(st, -x - (1 << 21)), -dinn.apply_test_polynomial(st, x))   # odd inside (-1/4, 1/4)
    assert sorted(dinn.decision_boundaries(dinn.sign_test_polynomial(mu)).tolist()) == [-(1 << 20), (1 << 31) - (1 << 20)]
    # evaluate_plain against numpy: sign(W2 sign(W1 x)) with the torus scaling written out
    rng = np.random.default_rng(3)
    net = _net(rng)
    x = rng.choice([-1, 1], (50, 32))
    W1, W2 = (ly.weights.astype(np.int64) for ly in net.layers)
    s1 = x @ W1.T
    h = np.where(s1 * (1 << 24) + (1 << 20) >= 0, 1, -1)                    # the mod switch rounds to the nearest 1 / 2N
    s2 = h @ W2.T
    want = np.where(s2 * ((1 << 32) // 36) + (1 << 20) >= 0, 1, -1) * (1 << 29)
    got, pres = net.evaluate_plain(x, return_pre=True)
    assert np.array_equal(got, want) and np.array_equal(pres[0], s1 << 24) and np.array_equal(pres[1], s2 * ((1 << 32) // 36))
    lin = dinn.Network([dinn.DenseLayer(W1, np.arange(8) * 1000)], 1 << 20)  # no activation: the sums themselves
    assert np.array_equal(lin.evaluate_plain(x), (s1 << 20) + np.arange(8) * 1000)
    with pytest.raises(ValueError):
        dinn.Network([dinn.DenseLayer(W1), dinn.DenseLayer(W2)], 1)          # a hidden layer needs an activation
    with pytest.raises(ValueError):
        dinn.DenseLayer(np.full((1, 2), 128))


def test_check_refuses_wide_ranges_and_small_margins(eoc):
    p = eoc.default_params(0)
    sk = eoc.SecretKey(p, 5, with_cloud_key=False)
    keys = (p, sk.lwe_key, sk.tlwe_key)
    rng = np.random.default_rng(4)
    net = _net(rng)
    x = rng.choice([-1, 1], (400, 32))
    chk = net.check(*keys, x=x, pk=eoc.PublicKey(sk.public_key_bytes()))
    sig = chk["layers"][0]["sigma"]
    assert chk["layers"][0]["range"] < 0.25 and chk["layers"][1]["range"] == pytest.approx(8 / 36, abs=1e-6)
    assert 0.002 < sig.min() and sig.max() < 0.006 and 0.008 < chk["layers"][1]["sigma"].max() < 0.02     # ks + mod switch; + 8 bootstraps
    # margins are distances to the boundary at -1/(4N) over sigma: a vector is priced by its worst pre-activation
    pres = net.evaluate_plain(x, return_pre=True)[1]
    d0 = np.abs(pres[0] + (1 << 20)).min(1) / 2.0**32
    assert chk["vector_sigma"].shape == (400,) and (chk["vector_sigma"] <= d0 / sig.min() + 1e-9).all()
    assert chk["worst_sigma"] == pytest.approx(chk["vector_sigma"].min())
    good = x[chk["vector_sigma"] >= 6]
    assert net.check(*keys, x=good, min_sigma=6)["worst_sigma"] >= 6 if len(good) else True
    with pytest.raises(ValueError, match="min_sigma"):
        net.check(*keys, x=x, min_sigma=6)                                  # some of 400 random vectors sit near a boundary
    with pytest.raises(ValueError, match="min_sigma"):
        net.check(*keys, min_sigma=6)                                       # without x: a sum of 0 is reachable
    wide = dinn.Network([dinn.DenseLayer(np.full((1, 32), 4), None, dinn.sign_test_polynomial(1 << 29))], 1 << 25)
    with pytest.raises(ValueError, match="1/4"):
        wide.check(*keys)                                                   # 32 x 4 / 128 = 1 >= 1/4
    edge = dinn.Network([dinn.DenseLayer(np.full((1, 32), 1), None, dinn.sign_test_polynomial(1 << 29))], 1 << 25)
    with pytest.raises(ValueError, match="1/4"):
        edge.check(*keys)                                                   # exactly 1/4 is refused too
    ok = dinn.Network([dinn.DenseLayer(np.full((1, 31), 1), [1 << 24], dinn.sign_test_polynomial(1 << 29))], 1 << 25)
    assert ok.check(*keys, min_sigma=1)["worst_sigma"] > 1                  # odd sums + half a step of bias: never near 0


def test_the_end_to_end_draw_terminates_quickly(eoc):
    """the GPU end-to-end test's draw (tests/dinn_case.py): 64 vectors at >= 6 sigma within 200 000 draws"""
    import dinn_case as dc
    p = eoc.default_params(0)
    sk = eoc.SecretKey(p, dc.KEY_SEED, with_cloud_key=False)
    net, x, draws = dc.dinn_case(eoc, p, sk)
    print(f"end-to-end draw: 64 vectors kept of {draws} drawn")
    assert x.shape == (64, 32) and draws <= 200000
    chk = net.check(p, sk.lwe_key, sk.tlwe_key, x=x, pk=eoc.PublicKey(sk.public_key_bytes()), min_sigma=6)
    assert chk["vector_sigma"].min() >= 6
