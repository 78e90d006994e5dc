"""Convolutions with public int8 kernels, host side (include/eoc_tfhe_gpu.h): the new symbols and their
refusals, the chunked reference (tests/c/conv_ref.c) against the inner product's reference under the word map and against
exact wrapping-integer arithmetic, noise.conv_row, the output noise of one slot against noise.linear_var_row / linear_offset,
and the convolution layers of eoc_tfhe_amd/dinn.py.  GPU side: tests/test_gpu_conv.py; registers: tests/test_isa_conv.py."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import compact_oracle as co
import conv_case as cc
import conv_oracle as cv
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
    new = {"eoc_conv_slots_to_device", "eoc_conv_device", "eoc_conv_linear_device", "eoc_conv_extract_device",
           "eoc_engine_conv_launches", "eoc_conv_linear"}
    assert new <= set(eoc.abi_symbols()) and all(hasattr(L, s) for s in new)
    assert all(hasattr(eoc.Engine, m) for m in ("conv_slots_to_device", "conv_device", "conv_linear_device",
                                                "conv_extract_device", "conv_launches"))
    assert callable(eoc.conv_linear) and L.eoc_engine_conv_launches(None) == 0
    x = np.zeros(8, np.int32)
    ptr = x.ctypes.data                                                    # never followed: every call below is refused first
    for call in (lambda: L.eoc_conv_slots_to_device(None, ptr, 1, 1, ptr, None),
                 lambda: L.eoc_conv_device(None, ptr, 1, 1, ptr, 1, None, ptr, None),
                 lambda: L.eoc_conv_linear_device(None, ptr, 1, 1, ptr, 1, None, ptr, 1, ptr, None),
                 lambda: L.eoc_conv_extract_device(None, ptr, 1, 1, ptr, 1, ptr, None),
                 lambda: L.eoc_conv_linear(None, 1, 1, ptr, 1, None, ptr, 1, ptr),
                 lambda: L.eoc_conv_linear(ptr, 1, 1, None, 1, None, ptr, 1, ptr),
                 lambda: L.eoc_conv_linear(ptr, 1, 1, ptr, 1, None, None, 1, ptr),
                 lambda: L.eoc_conv_linear(ptr, 1, 1, ptr, 1, None, ptr, 1, None)):
        assert call() == EOC_ERR_ARG
    lists = np.zeros((1, 1, 2, N), np.int32)
    with pytest.raises(eoc.EocError):
        eoc.conv_linear(np.full((1, 4), -128), lists, [0])
    with pytest.raises(eoc.EocError):
        eoc.conv_linear(np.ones((1, 4), np.int8), np.zeros((1, 2, 2, N), np.int32), [0])
    with pytest.raises(eoc.EocError):
        eoc.conv_linear(np.ones((2, 4), np.int8), lists, [0, 2 * N])         # a slot behind the last output channel
    with pytest.raises(eoc.EocError):
        eoc.conv_linear(np.ones((1, 4), np.int8), lists, [0], bias=[1, 2])


def _rand(rng, L):
    w = rng.integers(-127, 128, L * N).astype(np.int8)
    w[:4] = (127, -127, 0, 1)
    return w, rng.integers(INT32_MIN, INT32_MAX, (L, 2, N), endpoint=True).astype(np.int32)


def test_c0_is_the_inner_products_mask_under_the_word_map():
    """word j of the reference's c0 is mask word (N - j) mod N of dot_oracle.sample, negated for j > 0: byte for byte, at one
    list, one full chunk and a one-list chunk behind it; the body of that sample is slot 0 of c1"""
    rng = np.random.default_rng(1)
    for L in (1, 8, 9):
        w, lists = _rand(rng, L)
        out = cv.out_list(w, lists, 12345)
        smp = do.sample(w, lists, 12345)
        assert cv.to_dot_mask(out[0]).tobytes() == smp[:N].tobytes(), L
        # the bodies: the inner product's is an exact integer sum, slot 0 of c1 went through the transform
        assert do.lsb_deviation(out[1, :1], smp[N:]) <= 8 * cv.do.n_chunks(L * N), L


def _check_chunks(w, lists, chunks, label):
    """per converted chunk both polynomials within 8 LSB of exact arithmetic; returns (worst LSB, high water)"""
    hwm = np.zeros(1)
    worst = 0
    for c in range(chunks):
        ref = cv.out_list(w, lists, 12345, c, c + 1, hwm)
        exact = cv.out_list_exact(w, lists, 12345, c, c + 1)
        for p in range(2):
            d = do.lsb_deviation(ref[p], exact[p])
            print(f"{label}: chunk {c}, polynomial {p}: max |reference - exact| = {d} LSB")
            assert d <= 8, (label, c, p, d)
            worst = max(worst, d)
    print(f"{label}: high-water mark before conversion 2^{np.log2(max(hwm[0], 1.0)):.2f}")
    assert hwm[0] < 2.0**51
    return worst, hwm[0]


def test_reference_against_exact_arithmetic():
    """L = 1, one full chunk (L = 8), L = 9 (a chunk of one list behind a full one) and the full-scale chunk (every weight +127
    against list words all INT32_MIN, then all INT32_MAX), BOTH polynomials.  Bound: 8 LSB per converted chunk, the project's
    bound for this conversion; measured here: 1 LSB in every chunk and polynomial"""
    rng = np.random.default_rng(2)
    worst = 0
    for L in (1, 8, 9):
        w, lists = _rand(rng, L)
        worst = max(worst, _check_chunks(w, lists, (L + 7) // 8, f"L = {L}")[0])
        full = cv.out_list(w, lists, 12345).astype(np.int64)
        parts = sum(cv.out_list(w, lists, 0 if c else 12345, c, c + 1).astype(np.int64) for c in range((L + 7) // 8))
        assert np.array_equal((full - parts) % 2**32, np.zeros((2, N), np.int64))       # the chunks add up, the bias enters once
    w = np.full(8 * N, 127, np.int8)
    for word in (INT32_MIN, INT32_MAX):
        d, hw = _check_chunks(w, np.full((8, 2, N), word, np.int32), 1, f"full scale, words {word}")
        worst = max(worst, d)
        assert hw > 2.0**49                                                # the shape does reach the top of the range
    print(f"largest deviation of any chunk and polynomial: {worst} LSB")
    # the batch form agrees with the single-list form
    w2 = rng.integers(-127, 128, (3, N + 5))
    lists = rng.integers(INT32_MIN, INT32_MAX, (2, 2, 2, N), endpoint=True).astype(np.int32)
    bias = rng.integers(INT32_MIN, INT32_MAX, 3).astype(np.int32)
    out = cv.conv(w2, lists, bias)
    assert out.shape == (2, 3, 2, N)
    assert np.array_equal(out[1, 2], cv.out_list(do.padded(w2)[2], lists[1], bias[2]))


def test_conv_row_is_the_inner_product_row_of_a_slot():
    """slot t of the exact convolution is the exact inner product with noise.conv_row(w, t), mask and body, word for word, at
    t = 0, 1 and N - 1 (every tap but the first wraps), over two lists; conv_row pads a short row and refuses a bad slot"""
    rng = np.random.default_rng(3)
    w, lists = _rand(rng, 2)
    out = cv.out_list_exact(w, lists, 777)
    for t in (0, 1, N - 1):
        row = noise.conv_row(w, t)
        assert row.shape == (2 * N,) and np.array_equal(row.reshape(2, N), cv.shifted_rows(w, [t])[0].reshape(2, N))
        want = do.sample_exact(row.astype(np.int8), lists, 777)
        assert np.array_equal(co.extract(out[None], [t])[0], want), t
    assert np.array_equal(noise.conv_row([1, 2, 3], 2)[:6], [0, 0, 1, 2, 3, 0]) and noise.conv_row([1, 2, 3], 2).size == N
    assert np.array_equal(noise.conv_row(np.r_[np.zeros(N - 1), 5], 2)[:3], [0, -5, 0])
    for bad in (-1, N):
        with pytest.raises(ValueError):
            noise.conv_row(w, bad)


@pytest.mark.parametrize("pset", [0, 1])
def test_output_noise_of_a_slot_matches_the_row_model(eoc, pset):
    """K = 9 fixed random taps, one channel, slot t = 500 on M = 4 096 fresh lists through the reference, key seed 5: the
    variance of (phase - plain correlation) over noise.linear_var_row(noise.conv_row(w, t)) is 1 within the project's
    4 sqrt(2 / (M - 1)) = 0.088, and the mean less noise.linear_offset(noise.conv_row(w, t)) is 0 within 4 standard errors;
    nothing fitted.  Measured: DESIGN.md 20."""
    M, K, t = 4096, 9, 500
    p = eoc.default_params(pset)
    sk = eoc.SecretKey(p, 5, with_cloud_key=False)
    pk = eoc.PublicKey(sk.public_key_bytes())
    rng = np.random.default_rng(40 + pset)
    w = np.zeros(N, np.int8)
    w[:K] = rng.integers(-127, 128, K)
    msgs = rng.integers(-(2**20), 2**20, (M, N))
    lists = pk.encrypt_torus(msgs, 41 + pset).reshape(M, 1, 2, N)
    with ThreadPoolExecutor(16) as ex:
        out = np.stack(list(ex.map(lambda b: cv.out_list(w, lists[b]), range(M))))
    phase = sk.list_phases(out).astype(np.int64)[:, t]
    plain = (msgs[:, t:t + K] * w[:K].astype(np.int64)).sum(1)
    err = ((phase - plain + 2**31) % 2**32 - 2**31) / 2.0**32
    row = noise.conv_row(w, t)
    assert np.array_equal(np.flatnonzero(row), t + np.flatnonzero(w))
    var = noise.linear_var_row(p, row, sk.tlwe_key, pk)
    ratio = err.var(ddof=1) / var
    z = (err.mean() - noise.linear_offset(p, sk, row)) / (err.std(ddof=1) / np.sqrt(M))
    print(f"pset {pset}: slot {t}: measured var / linear_var_row(conv_row) = {ratio:.4f}; mean - linear_offset = {z:+.2f} "
          f"standard errors; linear_var_row / linear_var = "
          f"{var / noise.linear_var(p, row, noise.compact_var(p, sk.tlwe_key, pk)):.4f}")
    assert abs(ratio - 1) <= 4 * np.sqrt(2.0 / (M - 1)), ratio
    assert abs(z) <= 4, z


def test_conv_layer_equals_the_dense_layer_of_its_shifted_rows():
    """ConvLayer against the DenseLayer whose rows are the shifted copies of the filters, written out in
    conv_oracle.shifted_rows: pre-activations and outputs of evaluate_plain, two input channels, a bias, slots that wrap; and
    a conv -> dense network against dense -> dense on the unpadded weights"""
    rng = np.random.default_rng(5)
    taps = rng.integers(-3, 4, (2, 2, 3, 3))
    w = dinn.conv2d_weights(taps, 8)
    assert w.shape == (2, 2 * N) and w[1, N + 2 * 8 + 1] == taps[1, 1, 2, 1] and np.count_nonzero(w) == np.count_nonzero(taps)
    slots = np.r_[dinn.conv_slots(8, 8, 3, 3), N - 1, N - 10]                              # the last two wrap
    assert dinn.conv_slots(8, 8, 3, 3).tolist() == [y * 8 + x for y in range(6) for x in range(6)]
    assert dinn.conv_slots(8, 8, 3, 3, stride=2).tolist() == [y * 8 + x for y in (0, 2, 4) for x in (0, 2, 4)]
    bias = np.array([1 << 20, -(1 << 21)])
    mu = 1 << 24
    conv = dinn.ConvLayer(w, slots, bias, dinn.sign_test_polynomial(mu))
    rows = np.concatenate([cv.shifted_rows(w[c], slots) for c in range(2)])
    dense = dinn.DenseLayer(rows, np.repeat(bias, slots.size), dinn.sign_test_polynomial(mu))
    assert conv.n_out == dense.rows == 2 * slots.size and conv.slot_table().tolist() == [c * N + t for c in range(2) for t in slots]
    x = rng.choice([-1, 1], (7, 2, N))                                                    # every slot filled: the wrap counts
    xin = conv.pad_input(x)
    a, pa = dinn.Network([conv], 1 << 22).evaluate_plain(xin, return_pre=True)
    b, pb = dinn.Network([dense], 1 << 22).evaluate_plain(xin, return_pre=True)
    assert np.array_equal(pa[0], pb[0]) and np.array_equal(a, b) and len(np.unique(pa[0])) > 10
    w2 = rng.choice([-1, 0, 1], (3, conv.n_out))
    padded = dinn.pad_dense_weights(w2, 2, slots.size)
    assert padded.shape == (3, 2 * N) and np.array_equal(padded[:, N:N + slots.size], w2[:, slots.size:])
    two = dinn.Network([conv, dinn.DenseLayer(padded, None, dinn.sign_test_polynomial(1 << 29))], 1 << 22)
    ref = dinn.Network([dense, dinn.DenseLayer(w2, None, dinn.sign_test_polynomial(1 << 29))], 1 << 22)
    assert np.array_equal(two.evaluate_plain(xin), ref.evaluate_plain(xin))
    with pytest.raises(ValueError):
        dinn.Network([conv, dinn.DenseLayer(w2, None, None)], 1)                          # cols must be channels * N
    with pytest.raises(ValueError):
        dinn.ConvLayer(w[:, :N + 1], slots)
    with pytest.raises(ValueError):
        dinn.ConvLayer(w, [N])
    with pytest.raises(ValueError):
        dinn.conv2d_weights(taps, 2)


def test_check_prices_the_end_to_end_network_at_six_sigma(eoc):
    """the GPU end-to-end network (tests/conv_case.py): all 16 drawn vectors at >= 6 predicted sigma, none rejected; the conv
    layer's sigma is per channel, its offset per slot the correlation of the taps with compact_offset"""
    p = eoc.default_params(0)
    sk = eoc.SecretKey(p, cc.KEY_SEED, with_cloud_key=False)
    pk = eoc.PublicKey(sk.public_key_bytes())
    net, x, xin = cc.conv_case()
    assert x.shape == (cc.VECTORS, 1, 64) and xin.shape == (cc.VECTORS, N)
    chk = net.check(p, sk.lwe_key, sk.tlwe_key, x=xin, pk=pk, min_sigma=cc.MIN_SIGMA)
    for i, e in enumerate(chk["layers"]):
        print(f"layer {i}: range {e['range']:.4f}, sigma {e['sigma'].min():.3e} .. {e['sigma'].max():.3e}, "
              f"smallest margin {e['margin_sigma']:.2f} sigma")
    print("vector_sigma", np.round(chk["vector_sigma"], 2).tolist())
    assert chk["vector_sigma"].shape == (cc.VECTORS,) and chk["vector_sigma"].min() >= 6
    assert chk["layers"][0]["range"] < 0.25 and chk["layers"][1]["range"] < 0.25
    conv = net.layers[0]
    sig = chk["layers"][0]["sigma"].reshape(2, 36)
    assert (sig == sig[:, :1]).all()                                        # one sigma per channel
    # layer 0's offsets: the slot's own inner-product row, priced by the inner product's formula
    sg, mean = net.layer_sigma(p, sk.lwe_key, sk.tlwe_key, pk)[0]
    ksm = noise.predict(p, sk.lwe_key, sk.tlwe_key)["ks_mean"]
    for c, i in ((0, 0), (1, 35)):
        row = noise.conv_row(conv.weights[c], conv.slots[i])
        assert mean[c * 36 + i] == pytest.approx(abs(noise.linear_offset(p, pk, row, sk.tlwe_key) + ksm), rel=1e-9, abs=1e-15)
        want = noise.linear_var_row(p, row, sk.tlwe_key, pk) + noise.predict(p, sk.lwe_key, sk.tlwe_key)["ks_var"] + noise.modswitch_var(sk.lwe_key)
        assert sg[c * 36 + i] == pytest.approx(np.sqrt(want), rel=1e-9)
    # without the public key: ||taps||^2 V_slot per channel
    s0 = net.layer_sigma(p, sk.lwe_key, sk.tlwe_key)[0][0]
    pr = noise.predict(p, sk.lwe_key, sk.tlwe_key)
    assert s0[0] == pytest.approx(np.sqrt(9 * noise.compact_var(p, sk.tlwe_key) + pr["ks_var"] + noise.modswitch_var(sk.lwe_key)))
    # the pre-activations are odd multiples of their steps
    pres = net.evaluate_plain(xin, return_pre=True)[1]
    assert (np.abs(pres[0]) % (2 * cc.DELTA_IN) == cc.DELTA_IN).all() and (np.abs(pres[1]) % (2 * cc.MU1) == cc.MU1).all()
