"""Packing key switch, host side (include/eoc_tfhe_gpu.h): the packing key's rows against the oracle-stream
restatement, the chunked reference (tests/c/pack_ref.c) against exact wrapping-integer arithmetic, decryption of packed
lists, the added noise against noise.pack_var, the EOCPKS1 blob and its refusals, and the model's margin statement.
GPU side: tests/test_gpu_pack.py; registers: tests/test_isa_pack.py."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as ol
import pack_oracle as po
from eoc_tfhe_amd import noise

N = 1024
EOC_OK, EOC_ERR_ARG, EOC_ERR_NO_KEY = 0, -1, -4


@pytest.fixture(scope="module")
def eoc(built_lib):
    import eoc_tfhe_amd
    return eoc_tfhe_amd


_KEYS = {}


def key(eoc, pset, seed=5):
    """(params, secret key, packing-key rows [n][4][2][N], their reference spectra), once per (set, seed)"""
    if (pset, seed) not in _KEYS:
        p = eoc.default_params(pset)
        sk = eoc.SecretKey(p, seed, with_cloud_key=False)
        rows = po.blob_rows(sk.packing_key_bytes(), p.n)
        _KEYS[(pset, seed)] = (p, sk, rows, po.key_fft(rows))
    return _KEYS[(pset, seed)]


def lwe_phases(cts, lwe_key):
    cts = np.asarray(cts, np.int64)
    ph = cts[:, -1] - cts[:, :-1] @ np.asarray(lwe_key, np.int64)
    return ((ph + 2**31) % 2**32) - 2**31


@pytest.mark.parametrize("pset", [0, 1])
def test_key_rows_equal_the_oracle_stream_restatement(eoc, pset):
    p, sk, rows, _ = key(eoc, pset)
    blob = sk.packing_key_bytes()
    assert len(blob) == 8 + 36 + 8 + p.n * 4 * 2 * N * 4 == eoc.lib().eoc_packing_key_blob_bytes(C.byref(p))
    assert bytes(blob[:8]) == b"EOCPKS1\0" and np.frombuffer(bytes(blob[44:52]), np.int32).tolist() == [4, 4]
    assert np.array_equal(sk.packing_key_bytes(), blob)                   # the same key gives the same packing key
    orc = ol.Oracle(pset, 5, with_bk=False)
    assert np.array_equal(orc.lwe_key, sk.lwe_key) and np.array_equal(orc.tlwe_key, sk.tlwe_key)
    one, zero = int(np.flatnonzero(orc.lwe_key)[3]), int(np.flatnonzero(orc.lwe_key == 0)[3])
    for m in sorted({0, 1, one, zero, p.n - 1}):                           # word for word: both key-bit values, both ends
        for j in range(1, 5):
            assert np.array_equal(rows[m, j - 1], po.key_row(5, orc.lwe_key, orc.tlwe_key, p.bk_stdev, m, j)), (m, j)
    # every row: a TLWE sample under s' whose phase is s_m 2^(32 - 4j) on the constant coefficient plus the row's noise
    ph = sk.list_phases(rows.reshape(-1, 2, N)).astype(np.int64).reshape(p.n, 4, N)
    assert np.array_equal(ph[0], po.list_phases(rows[0], orc.tlwe_key))   # eoc_list_phases against numpy
    msg = np.zeros((p.n, 4, N), np.int64)
    msg[:, :, 0] = np.asarray(orc.lwe_key, np.int64)[:, None] * (1 << (32 - 4 * np.arange(1, 5)))[None, :]
    e = (((ph - msg) + 2**31) % 2**32 - 2**31) / 2.0**32
    assert np.abs(e).max() < 7 * p.bk_stdev and 0.98 < e.std() / p.bk_stdev < 1.02, (np.abs(e).max(), e.std())


def test_other_keys_of_the_same_secret_key_are_unchanged(eoc):
    """tag 9 is a stream of its own: exporting the packing key moves no word of the public key, and the key-switch and
    bootstrapping keys are the oracle's as before"""
    p = eoc.default_params(0)
    p.n = 16
    a = eoc.SecretKey(p, 7)
    pk0, bk0, ksk0 = a.public_key_bytes(), a.bk.copy(), a.ksk.copy()
    a.packing_key_bytes()
    b = eoc.SecretKey(p, 7)
    assert a.public_key_bytes() == pk0 == b.public_key_bytes()
    assert np.array_equal(a.bk, bk0) and np.array_equal(b.bk, bk0) and np.array_equal(b.ksk, ksk0)
    orc = ol.Oracle(0, 7, n_override=16)
    assert np.array_equal(orc.bk.ravel(), np.asarray(bk0).ravel()) and np.array_equal(orc.ksk.ravel(), np.asarray(ksk0).ravel())


def test_digits_round_to_sixteen_bits(eoc):
    rng = np.random.default_rng(1)
    a = np.r_[rng.integers(0, 2**32, 4096), 0, 2**15 - 1, 2**15, 2**32 - 2**15, 2**32 - 2**15 - 1, 2**31].astype(np.int64)
    d = po.digits(a)
    assert d.min() >= -8 and d.max() < 8
    approx = sum(d[j] << (32 - 4 * (j + 1)) for j in range(4))
    err = ((a - approx) + 2**31) % 2**32 - 2**31
    assert err.min() >= -2**15 and err.max() < 2**15                      # round to nearest multiple of 2^16
    assert (po.digits(np.zeros(4, np.int64)) == 0).all()                  # an absent sample contributes nothing


@pytest.mark.parametrize("pset", [0, 1])
def test_reference_against_exact_arithmetic(eoc, pset):
    """the first two chunks and the short last chunk of one full list: bound 8 LSB per converted chunk (the project's
    contract for one converted product), 24 here; the whole list's bound is chunks x 8 = 256 (Set A) / 320 (Set B)"""
    p, sk, rows, kfft = key(eoc, pset)
    cts = sk.encrypt_bits(np.random.default_rng(2).integers(0, 2, N), 11)
    nch = po.n_chunks(p.n)
    assert nch == (32, 40)[pset] and p.n - 16 * (nch - 1) == (4, 6)[pset]
    worst = 0
    for lo, hi in ((0, 2), (nch - 1, nch)):
        ref = po.pack_list(p.n, kfft, cts, lo, hi)
        exact = po.pack_list_exact(p.n, rows, cts, lo, hi)
        d = int(np.abs(((ref.astype(np.int64) - exact) + 2**31) % 2**32 - 2**31).max())
        print(f"pset {pset}: chunks [{lo}, {hi}): max |reference - exact| = {d} LSB")
        assert d <= 8 * (hi - lo), (lo, hi, d)
        worst = max(worst, d)
    assert ol.lib().orc_dbg_max_conv(0) < 2.0**51
    # the chunks add up: the whole list is (0, B) minus every chunk's part
    full = po.pack_list(p.n, kfft, cts).astype(np.int64)
    start = po.pack_list(p.n, kfft, cts, 0, 0).astype(np.int64)
    parts = sum(start - po.pack_list(p.n, kfft, cts, c, c + 1).astype(np.int64) for c in range(nch))
    assert np.array_equal((full - (start - parts)) % 2**32, np.zeros((2, N), np.int64))


@pytest.mark.parametrize("pset", [0, 1])
def test_packed_lists_decrypt(eoc, pset):
    p, sk, _, kfft = key(eoc, pset)
    rng = np.random.default_rng(3 + pset)
    for count in (N, 1, N + 3):
        bits = rng.integers(0, 2, count).astype(np.uint8)
        lists = po.pack(p.n, kfft, sk.encrypt_bits(bits, 20 + count))
        assert lists.shape == (-(-count // N), 2, N)
        assert np.array_equal(sk.decrypt_list_bits(lists, count), bits), count
        ph = sk.list_phases(lists).ravel().astype(np.int64)
        assert np.abs(ph[count:]).max(initial=0) < 2**20                  # unfilled slots: samples (0, 0), phase ~ 0
        vals = rng.integers(0, 8, count).astype(np.uint8)
        lists = po.pack(p.n, kfft, sk.encrypt_ints(vals, 8, 40 + count))
        assert np.array_equal(sk.decrypt_list_ints(lists, 8, count), vals), count
    with pytest.raises(eoc.EocError):
        sk.decrypt_list_bits(lists, 3 * N)                                # more than the lists hold
    assert eoc.lib().eoc_decrypt_list_ints(sk.h, 3, lists.ctypes.data, 4, np.zeros(4, np.uint8).ctypes.data) == EOC_ERR_ARG
    assert eoc.lib().eoc_decrypt_list_bits(sk.h, None, 4, np.zeros(4, np.uint8).ctypes.data) == EOC_ERR_ARG
    assert eoc.lib().eoc_list_phases(None, lists.ctypes.data, 1, lists.ctypes.data) == EOC_ERR_ARG


@pytest.mark.parametrize("pset", [0, 1])
def test_added_noise_matches_pack_var(eoc, pset):
    """the ADDED error, output phase minus input phase sample by sample, over 16 full lists = 16 384 samples: variance within
    5 % of noise.pack_var (sampling error of a variance at 16 384 samples: 1.1 %), mean within 4 standard errors of zero"""
    p, sk, rows, kfft = key(eoc, pset)
    rng = np.random.default_rng(30 + pset)
    cts = sk.encrypt_bits(rng.integers(0, 2, 16 * N), 99)
    lists = po.pack(p.n, kfft, cts)
    d = sk.list_phases(lists).ravel().astype(np.int64) - lwe_phases(cts, sk.lwe_key)
    err = (((d + 2**31) % 2**32) - 2**31) / 2.0**32
    pv = noise.pack_var(p, sk.lwe_key, N)
    ratio, se = err.var() / pv, err.mean() / (err.std() / np.sqrt(len(err)))
    print(f"pset {pset}: added sigma {err.std():.4e}, pack_var sigma {np.sqrt(pv):.4e}, variance ratio {ratio:.4f}, "
          f"mean {err.mean():.3e} ({se:+.2f} se)")
    assert len(err) >= 16384 and abs(ratio - 1) < 0.05, ratio
    assert abs(se) < 4 and noise.pack_mean(p, sk.lwe_key) == 0.0, se
    # one key's slots carry the fixed offsets of noise.pack_offset (the digits' mean is -1/2): derived from the key alone and
    # removed slot by slot, the mean stays within 4 standard errors and the offsets explain their share of the variance
    off = noise.pack_offset(sk.list_phases(rows.reshape(-1, 2, N)).reshape(p.n, 4, N), sk.lwe_key, N)
    res = err - np.tile(off, 16)
    se_res = res.mean() / (res.std() / np.sqrt(len(res)))
    print(f"pset {pset}: slot offsets: mean {off.mean():.3e}, sigma {off.std():.3e} (expected over keys "
          f"{0.5 * np.sqrt(4 * p.n * N) * p.bk_stdev:.3e}); mean with them removed {res.mean():.3e} ({se_res:+.2f} se), "
          f"variance ratio {res.var() / pv:.4f}")
    assert abs(se_res) < 4, se_res
    assert res.var() < err.var()


@pytest.mark.parametrize("pset", [0, 1])
def test_noise_of_a_sparse_list_scales_with_the_filled_slots(eoc, pset):
    """`filled` enters the rows' term: with 64 occupied slots the added error is the model's at filled = 64 (the rounding
    term, which does not shrink, then dominates).  64 slots x 16 lists = 1 024 samples: sampling error 4.4 %, bound 4 sigma"""
    p, sk, _, kfft = key(eoc, pset)
    cts = sk.encrypt_bits(np.random.default_rng(40 + pset).integers(0, 2, 16 * 64), 98)
    lists = np.stack([po.pack_list(p.n, kfft, cts[k * 64:(k + 1) * 64]) for k in range(16)])
    d = sk.list_phases(lists)[:, :64].ravel().astype(np.int64) - lwe_phases(cts, sk.lwe_key)
    err = (((d + 2**31) % 2**32) - 2**31) / 2.0**32
    pv = noise.pack_var(p, sk.lwe_key, 64)
    assert pv < noise.pack_var(p, sk.lwe_key, N)
    assert abs(err.var() / pv - 1) < 4 * np.sqrt(2.0 / len(err)), err.var() / pv


@pytest.mark.parametrize("pset", [0, 1])
def test_model_packing_is_far_below_a_gate_output(eoc, pset):
    """sigma ~9e-5 (Set A) / ~3e-4 (Set B) for a full list against a gate output's 0.004 / 0.003: a packed gate output, and
    one expanded again, keeps every margin stated for gate outputs"""
    p, sk, _, _ = key(eoc, pset)
    pred = noise.predict(p, sk.lwe_key, sk.tlwe_key)
    pv = noise.pack_var(p, sk.lwe_key, N)
    print(f"pset {pset}: pack sigma {np.sqrt(pv):.3e}, gate output sigma {np.sqrt(pred['total_var']):.5f}")
    assert 0.7 < np.sqrt(pv) / (9e-5, 3e-4)[pset] < 1.3                  # the issue's round figures; exactly 8.2e-5 / 2.3e-4
    assert pv < 0.02 * pred["total_var"]
    assert noise.pack_var(p, sk.lwe_key, 1) < pv


def test_blob_round_trip_and_refusals(eoc):
    L = eoc.lib()
    p = eoc.default_params(0)
    p.n = 24
    sk = eoc.SecretKey(p, 5, with_cloud_key=False)
    blob = sk.packing_key_bytes().tobytes()
    q = eoc.Params()
    assert L.eoc_packing_key_blob_params(blob, len(blob), C.byref(q)) == EOC_OK
    assert (q.n, q.l, q.Bgbit, q.ks_t, q.ks_basebit, q.ks_stdev, q.bk_stdev) == \
        (24, p.l, p.Bgbit, p.ks_t, p.ks_basebit, p.ks_stdev, p.bk_stdev)
    i32 = lambda *v: np.array(v, np.int32).tobytes()
    bad = {
        "magic": b"EOCPKS2\0" + blob[8:],
        "public key magic": b"EOCPK1\0\0" + blob[8:],
        "truncated": blob[:-4],
        "longer": blob + b"\0\0\0\0",
        "header only": blob[:52],
        "short": blob[:20],
        "empty": b"",
        "t": blob[:44] + i32(3, 4) + blob[52:],
        "basebit": blob[:44] + i32(4, 2) + blob[52:],
        "t and basebit": blob[:44] + i32(8, 2) + blob[52:],
        "n": blob[:8] + i32(25) + blob[12:],
        "public key": sk.public_key_bytes(),
    }
    for name, b in bad.items():
        assert L.eoc_packing_key_blob_params(b, len(b), C.byref(q)) == EOC_ERR_ARG, name
    assert L.eoc_packing_key_blob_params(None, 0, C.byref(q)) == EOC_ERR_ARG
    assert L.eoc_packing_key_blob_params(blob, len(blob), None) == EOC_ERR_ARG
    small = np.zeros(len(blob) - 1, np.uint8)
    assert L.eoc_packing_key_export(sk.h, small.ctypes.data, small.size) == EOC_ERR_ARG and not small.any()
    assert L.eoc_packing_key_export(None, small.ctypes.data, small.size) == EOC_ERR_ARG
    # a secure-mode key has a packing key of its own, deterministic per key
    m1 = bytes(range(32))
    a = eoc.SecretKey(p, None, with_cloud_key=False, master=m1).packing_key_bytes()
    b = eoc.SecretKey(p, None, with_cloud_key=False, master=m1).packing_key_bytes()
    assert np.array_equal(a, b) and not np.array_equal(a, np.frombuffer(blob, np.uint8))


def test_global_context_client_calls(eoc):
    import base64
    L = eoc.lib()
    p = eoc.default_params(0)
    p.n = 24
    sk = eoc.SecretKey(p, 5, with_cloud_key=False)
    rows = po.blob_rows(sk.packing_key_bytes(), p.n)
    bits = np.array([1, 0, 0, 1, 1], np.uint8)
    lists = po.pack(p.n, po.key_fft(rows), sk.encrypt_bits(bits, 3))
    out = np.zeros(5, np.uint8)
    ph = np.zeros((1, N), np.int32)
    assert eoc.global_key_mode() == 0
    assert L.eoc_global_decrypt_list_bits(lists.ctypes.data, 5, out.ctypes.data) == EOC_ERR_NO_KEY
    assert L.eoc_global_packing_key_export(None, 0) == 0
    blob = sk.packing_key_bytes()
    assert L.eoc_global_import_packing_key_blob(blob.ctypes.data, blob.size) == EOC_ERR_NO_KEY
    assert L.eoc_global_import_packing_key_blob(blob.ctypes.data, 40) == EOC_ERR_ARG
    assert eoc.Tfhe.importSecretKey(base64.b64encode(sk.export_bytes()).decode()) == 0
    try:
        assert L.eoc_global_decrypt_list_bits(lists.ctypes.data, 5, out.ctypes.data) == EOC_OK and np.array_equal(out, bits)
        assert L.eoc_global_list_phases(lists.ctypes.data, 1, ph.ctypes.data) == EOC_OK
        assert np.array_equal(ph, sk.list_phases(lists))
        vals = np.array([7, 0, 3], np.uint8)
        li = po.pack(p.n, po.key_fft(rows), sk.encrypt_ints(vals, 8, 4))
        assert L.eoc_global_decrypt_list_ints(8, li.ctypes.data, 3, out.ctypes.data) == EOC_OK and np.array_equal(out[:3], vals)
        need = L.eoc_global_packing_key_export(None, 0)
        assert need == blob.size
        buf = np.zeros(need, np.uint8)
        assert L.eoc_global_packing_key_export(buf.ctypes.data, need) == need and np.array_equal(buf, blob)
    finally:
        eoc.Tfhe.resetGateKey()
