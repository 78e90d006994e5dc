"""Seeded ciphertexts, selectors and cloud key, host side (no GPU): the mask streams depend on (seed, tag, idx)
only, expanded samples decrypt and carry the fresh-ciphertext noise, every seeded selector / bootstrapping-key row has the
gadget phase and drives the CMux reference, the expanded seeded cloud key drives the oracle's gates, the seeded cloud key is
an INDEPENDENT encryption (its noise is not the EOCCK1 key's), exports are deterministic, EOCCK1 is untouched, and malformed
blobs are refused.  Device side: tests/test_gpu_seeded.py."""
import ctypes as C

import numpy as np
import pytest

import cmux_oracle as cx
import oracle_lib as ol
from eoc_tfhe_amd import noise

N = 1024
EOC_OK, EOC_ERR_ARG = 0, -1
ONE8 = 1 << 29


@pytest.fixture(scope="module")
def eoc(built_lib):
    import eoc_tfhe_amd
    return eoc_tfhe_amd


@pytest.fixture(scope="module", params=[0, 1])
def keyset(request, eoc):
    """(pset, params, sk, EOCCK1 made BEFORE any seeded call, seeded blob, expanded (bk, ksk)) -- computed once per set"""
    pset = request.param
    p = eoc.default_params(pset)
    sk = eoc.SecretKey(p, 11 + pset)
    ck_before = sk.export_cloud_key().copy()
    blob = sk.seeded_cloud_key_bytes()
    bk, ksk = eoc.seeded_cloud_key_expand(blob)
    return pset, p, sk, ck_before, blob, bk, ksk


def wrap32(x):
    return ((np.asarray(x, np.int64) + 2**31) % 2**32) - 2**31


def lwe_phases(cts, key):
    cts = np.asarray(cts, np.int64)
    return wrap32(cts[:, -1] - cts[:, :-1] @ np.asarray(key, np.int64))


def row_phases(sk, rows):
    """c1 - c0 s' of TLWE rows [...][2][N] (eoc_list_phases)"""
    rows = np.ascontiguousarray(rows, np.int32)
    return sk.list_phases(rows.reshape(-1, 2, N)).astype(np.int64).reshape(rows.shape[:-2] + (N,))


def gadget_messages(p, tlwe_key, bits):
    """[len(bits)][2l][N]: row (q, pp) of bit 1 carries h = 2^(32 - pp Bgbit): -h s'(X) for q = 0, h on coefficient 0 for q = 1"""
    msg = np.zeros((len(bits), 2 * p.l, N), np.int64)
    for row in range(2 * p.l):
        q, pp = row // p.l, row % p.l + 1
        h = 1 << (32 - pp * p.Bgbit)
        one = np.zeros(N, np.int64)
        if q:
            one[0] = h
        else:
            one = -h * np.asarray(tlwe_key, np.int64)
        msg[:, row] = np.asarray(bits, np.int64)[:, None] * one[None, :]
    return msg


K1, K2 = bytes(range(32)), bytes(range(1, 33))
S1, S2 = bytes(range(100, 132)), bytes(range(101, 133))


def test_symbols(eoc):
    new = {"eoc_seeded_encrypt_bits", "eoc_seeded_encrypt_ints", "eoc_seeded_encrypt_bits_keyed", "eoc_seeded_encrypt_ints_keyed",
           "eoc_tgsw_seeded_encrypt_bits", "eoc_tgsw_seeded_encrypt_bits_keyed", "eoc_seeded_cloud_key_blob_bytes",
           "eoc_seeded_cloud_key_export", "eoc_seeded_cloud_key_blob_params", "eoc_seeded_expand_host",
           "eoc_tgsw_seeded_expand_host", "eoc_seeded_cloud_key_expand", "eoc_seeded_expand_device",
           "eoc_tgsw_seeded_to_fft_device", "eoc_engine_load_seeded_cloud_key", "eoc_engine_create_from_seeded_cloud_key_blob",
           "eoc_engine_seed_launches", "eoc_dbg_chacha20_blocks_device", "eoc_seeded_expand",
           "eoc_global_import_seeded_cloud_key_blob"}
    L = eoc.lib()
    assert new <= set(eoc.abi_symbols()) and all(hasattr(L, s) for s in new)


def test_masks_depend_on_seed_tag_and_index_only(eoc):
    p = eoc.default_params(0)
    ska, skb = eoc.SecretKey(p, 3, with_cloud_key=False), eoc.SecretKey(p, 4, with_cloud_key=False)
    bits = np.array([0, 1, 1, 0, 1], np.uint8)
    sa, ba = ska.encrypt_bits_seeded(bits, K1, S1, first_idx=7)
    sb, bb = skb.encrypt_bits_seeded(1 - bits, K2, S1, first_idx=7)
    assert sa == sb == S1 and not np.array_equal(ba, bb)
    ea, eb = eoc.seeded_expand_host(p, sa, ba, 7), eoc.seeded_expand_host(p, sb, bb, 7)
    assert np.array_equal(ea[:, :-1], eb[:, :-1])                       # two keys, two messages, one seed: the same masks
    assert np.array_equal(ea[:, -1], ba) and np.array_equal(eb[:, -1], bb)
    assert np.array_equal(eoc.seeded_expand_host(p, sa, ba, 7), ea)     # deterministic
    assert len({r.tobytes() for r in ea[:, :-1]}) == 5                  # no mask is repeated inside a batch
    # sample s of a call at first_idx is sample 0 of a call at first_idx + s; another seed gives other masks
    assert np.array_equal(eoc.seeded_expand_host(p, sa, ba[2:3], 9)[0], ea[2])
    assert not np.array_equal(eoc.seeded_expand_host(p, S2, ba, 7)[:, :-1], ea[:, :-1])
    # the mask is the documented stream: sub-key = block(seed, counter tag << 32, nonce idx)[:32], word j = odd word
    # 2 (j mod 8) + 1 of block(sub-key, counter j / 8, nonce 0)
    L = eoc.lib()

    def block(key, counter, nonce):
        out = np.zeros(64, np.uint8)
        k = np.frombuffer(key, np.uint8).copy()
        n12 = np.array([counter >> 32, nonce & 0xFFFFFFFF, nonce >> 32], np.uint32).view(np.uint8).copy()
        L.eoc_dbg_chacha20_block(k.ctypes.data, counter & 0xFFFFFFFF, n12.ctypes.data, out.ctypes.data)
        return out
    sub = block(S1, 10 << 32, 8).tobytes()[:32]                        # tag 10 (LWE samples), stream index 7 + 1
    want = np.concatenate([block(sub, b, 0).view(np.uint32)[1::2] for b in range(63)])[:p.n]
    assert np.array_equal(ea[1, :-1].view(np.uint32), want)
    # selectors: tag 13, stream index (first_idx + s) 2l + row
    sel_seed, sel_b = ska.encrypt_selector_bits_seeded([1], K1, S1, first_idx=2)
    sel = eoc.tgsw_seeded_expand_host(p, sel_seed, sel_b, 2)
    sub = block(S1, 13 << 32, 2 * 2 * p.l + 3).tobytes()[:32]
    want = np.concatenate([block(sub, b, 0).view(np.uint32)[1::2] for b in range(128)])
    assert np.array_equal(sel[0, 3, 0].view(np.uint32), want) and np.array_equal(sel[0, :, 1], sel_b[0])


@pytest.mark.parametrize("pset", [0, 1])
def test_expanded_bits_and_ints_decrypt(eoc, pset):
    p = eoc.default_params(pset)
    rng = np.random.default_rng(5 + pset)
    for sk in (eoc.SecretKey(p, 21, with_cloud_key=False), eoc.SecretKey(p, None, with_cloud_key=False)):   # test and secure keys
        bits = rng.integers(0, 2, 300).astype(np.uint8)
        seed, bodies = sk.encrypt_bits_seeded(bits)
        assert len(seed) == 32 and bodies.shape == (300,) and bodies.dtype == np.int32
        assert np.array_equal(sk.decrypt_bits(eoc.seeded_expand_host(p, seed, bodies)), bits)
        for pp in (2, 4, 8):
            vals = rng.integers(0, pp, 200).astype(np.uint8)
            seed, bodies = sk.encrypt_ints_seeded(vals, pp)
            assert np.array_equal(sk.decrypt_ints(eoc.seeded_expand_host(p, seed, bodies), pp), vals)
        with pytest.raises(eoc.EocError):
            sk.encrypt_ints_seeded([4], 4)                                  # a value >= p
        with pytest.raises(eoc.EocError):
            sk.encrypt_ints_seeded([1], 16)
        with pytest.raises(eoc.EocError):
            sk.encrypt_bits_seeded([1], first_idx=3)                        # first_idx belongs to the keyed form


def test_secure_forms_accept_and_return_distinct_seeds(eoc):
    p = eoc.default_params(0)
    sk = eoc.SecretKey(p, 2, with_cloud_key=False)
    bits = np.ones(4, np.uint8)
    (s1, b1), (s2, b2) = sk.encrypt_bits_seeded(bits), sk.encrypt_bits_seeded(bits)
    assert s1 != s2 and s1 != bytes(32) and not np.array_equal(b1, b2)
    (s3, _), (s4, _) = sk.encrypt_ints_seeded([1, 2], 4), sk.encrypt_selector_bits_seeded([1])
    assert len({s1, s2, s3, s4}) == 4
    seed, bodies = sk.encrypt_bits_seeded(np.zeros(0, np.uint8))            # an empty batch still gets its seed
    assert len(seed) == 32 and bodies.size == 0
    # the keyed form: the noise key changes the bodies and nothing else
    _, ka = sk.encrypt_bits_seeded(bits, K1, S1)
    _, kb = sk.encrypt_bits_seeded(bits, K2, S1)
    _, kc = sk.encrypt_bits_seeded(bits, K1, S1)
    assert np.array_equal(ka, kc) and not np.array_equal(ka, kb)
    L = eoc.lib()
    out = np.zeros(4, np.int32)
    assert L.eoc_seeded_encrypt_bits(sk.h, None, 4, out.ctypes.data, out.ctypes.data) == EOC_ERR_ARG
    assert L.eoc_seeded_expand_host(None, out.ctypes.data, 0, out.ctypes.data, 1, out.ctypes.data) == EOC_ERR_ARG


def test_noise_of_seeded_samples_is_the_fresh_ciphertext_noise(eoc):
    """16 384 Set A samples: the phase error's variance is ks_stdev^2 within 5 % (standard error of the estimate: 1.1 %)"""
    p = eoc.default_params(0)
    sk = eoc.SecretKey(p, None, with_cloud_key=False)
    bits = np.random.default_rng(9).integers(0, 2, 16384).astype(np.uint8)
    seed, bodies = sk.encrypt_bits_seeded(bits)
    ph = lwe_phases(eoc.seeded_expand_host(p, seed, bodies), sk.lwe_key)
    e = wrap32(ph - np.where(bits, ONE8, -ONE8)) / 2.0**32
    ratio = e.var() / p.ks_stdev**2
    print("variance / ks_stdev^2 =", ratio)
    assert abs(e.mean()) < 5 * p.ks_stdev / 128 and abs(ratio - 1) < 0.05, ratio


@pytest.mark.parametrize("pset", [0, 1])
def test_seeded_selector_rows_have_the_gadget_phase_and_drive_the_cmux(eoc, pset):
    p = eoc.default_params(pset)
    sk = eoc.SecretKey(p, 6, with_cloud_key=False)
    bits = [0, 1] * 8
    seed, bodies = sk.encrypt_selector_bits_seeded(bits)
    assert bodies.shape == (16, 2 * p.l, N)
    sel = eoc.tgsw_seeded_expand_host(p, seed, bodies)
    assert sel.shape == (16, 2 * p.l, 2, N) and np.array_equal(sel[:, :, 1], bodies)
    e = wrap32(row_phases(sk, sel) - gadget_messages(p, sk.tlwe_key, bits)) / 2.0**32
    assert np.abs(e).max() < 6.5 * p.bk_stdev
    # the sampler truncates toward zero: its variance is noise._sig2 (2.6 % below bk_stdev^2 on Set A).  2^16 draws: s.e. 0.55 %
    assert abs(e.var() / noise._sig2(p) - 1) < 0.025, e.var() / noise._sig2(p)
    assert len({r.tobytes() for r in sel[:, :, 0].reshape(-1, N)}) == 16 * 2 * p.l  # no mask is repeated
    # CMux on the reference: the selector of bit 1 picks B, of bit 0 picks A
    op = cx.orc_params(p)
    rng = np.random.default_rng(pset)
    msg = np.where(rng.integers(0, 2, (2, N)), ONE8, -ONE8).astype(np.int32)
    A, B = eoc.trivial_table(msg[0])[0], eoc.trivial_table(msg[1])[0]
    for s in (0, 1):
        out = cx.cmux(op, cx.to_fft(sel[s]), A, B)
        err = wrap32(row_phases(sk, out) - msg[s].astype(np.int64))
        assert np.abs(err).max() < 2**24, (s, np.abs(err).max())                    # far inside the 2^29 margin
        assert np.array_equal(sk.decrypt_list_bits(out[None]), (msg[s] > 0).astype(np.uint8))


def test_seeded_bk_rows_have_the_gadget_phase(eoc, keyset):
    pset, p, sk, _, blob, bk, ksk = keyset
    assert bk.shape == (p.n, 2 * p.l, 2, N) and ksk.shape == (N * p.ks_t * ((1 << p.ks_basebit) - 1), p.n + 1)
    e = wrap32(row_phases(sk, bk) - gadget_messages(p, sk.tlwe_key, sk.lwe_key)) / 2.0**32
    assert np.abs(e).max() < 6.5 * p.bk_stdev
    assert abs(e.var() / noise._sig2(p) - 1) < 0.01, e.var() / noise._sig2(p)       # 2^21 draws and more: s.e. 0.1 %
    # key-switch-key rows: message s'_i d / base^(j + 1) at ks_stdev
    nd, t, bb = (1 << p.ks_basebit) - 1, p.ks_t, p.ks_basebit
    r = np.arange(ksk.shape[0])
    d, j, i = r % nd + 1, (r // nd) % t, r // (nd * t)
    msg = np.where(sk.tlwe_key[i] != 0, d.astype(np.int64) << (32 - (j + 1) * bb), 0)
    e = wrap32(lwe_phases(ksk, sk.lwe_key) - msg) / 2.0**32
    assert np.abs(e).max() < 6 * p.ks_stdev and abs(e.var() / p.ks_stdev**2 - 1) < 0.05, e.var() / p.ks_stdev**2


def test_expanded_seeded_cloud_key_drives_the_oracle(eoc, keyset):
    pset, p, sk, _, blob, bk, ksk = keyset
    orc = ol.Oracle(pset, 11 + pset, with_bk=False)
    assert np.array_equal(orc.lwe_key, sk.lwe_key) and np.array_equal(orc.tlwe_key, sk.tlwe_key)
    orc.bk, orc.ksk = np.ascontiguousarray(bk), np.ascontiguousarray(ksk)
    orc.bkfft = np.zeros((p.n, 2 * p.l, 2, N), np.float64)
    orc.L.orc_bk_to_fft(C.byref(orc.p), orc.bk, orc.bkfft)
    a, b = np.array([0, 0, 1, 1], np.uint8), np.array([0, 1, 0, 1], np.uint8)
    ca, cb = sk.encrypt_bits(a, 31), sk.encrypt_bits(b, 32)
    assert np.array_equal(sk.decrypt_bits(orc.gate_batch(ol.OPS["NAND"], ca, cb)), 1 - (a & b))
    assert np.array_equal(sk.decrypt_bits(orc.gate_batch(ol.OPS["XOR"], ca, cb)), a ^ b)


def test_seeded_cloud_key_is_an_independent_encryption(eoc, keyset):
    """Publishing EOCCK1 and EOCCKS1 of one key must not cancel the noise: with shared noise streams b - b_seeded would be
    s (a - a_seeded) exactly, linear algebra for the key.  The phases of corresponding rows differ by e - e', two independent
    draws: variance 2 sigma^2, non-zero in essentially every word."""
    pset, p, sk, _, blob, bk, ksk = keyset
    d = wrap32(row_phases(sk, sk.bk) - row_phases(sk, bk))
    ratio = (d / 2.0**32).var() / (2 * p.bk_stdev**2)
    print("BK: var(e - e') / 2 sigma^2 =", ratio, " zero words:", (d == 0).mean())
    assert abs(ratio - 1) < 0.10, ratio
    assert (d != 0).mean() > 0.97                                                   # P(e = e') ~ 1 / (2 sqrt(pi) sigma 2^32) < 1 %
    assert not np.array_equal(sk.bk[:, :, 0], bk[:, :, 0])                          # and the masks are other masks
    d = wrap32(lwe_phases(sk.ksk, sk.lwe_key) - lwe_phases(ksk, sk.lwe_key))
    ratio = (d / 2.0**32).var() / (2 * p.ks_stdev**2)
    print("KSK: var(e - e') / 2 sigma^2 =", ratio, " zero words:", (d == 0).mean())
    assert abs(ratio - 1) < 0.10, ratio
    assert (d != 0).mean() > 0.999


def test_exports_are_deterministic_and_eocck1_is_untouched(eoc, keyset):
    pset, p, sk, ck_before, blob, bk, ksk = keyset
    assert np.array_equal(sk.seeded_cloud_key_bytes(), blob)                        # the same bytes on every export
    assert np.array_equal(eoc.SecretKey(p, 11 + pset).seeded_cloud_key_bytes(), blob)   # ... and from the same key made again
    assert np.array_equal(sk.export_cloud_key(), ck_before)                         # EOCCK1 as before the seeded calls
    words = ck_before[8 + 36:].view(np.int32)
    assert np.array_equal(words[:sk.bk.size], sk.bk.ravel()) and np.array_equal(words[sk.bk.size:], sk.ksk.ravel())
    other = eoc.SecretKey(p, 12 + pset, with_cloud_key=False).seeded_cloud_key_bytes()
    assert not np.array_equal(other[44:76], blob[44:76])                            # the seed is a function of the key
    sec = eoc.SecretKey(p, None, master=bytes(range(32)), with_cloud_key=False)     # a secure-mode key: deterministic too
    assert np.array_equal(sec.seeded_cloud_key_bytes()[:76], sec.seeded_cloud_key_bytes()[:76])
    assert sec.seeded_cloud_key_bytes()[44:76].tobytes() != bytes(range(32))        # a PRF output, not the master key


def test_blob_size_and_malformed_blobs(eoc, keyset):
    pset, p, sk, _, blob, bk, ksk = keyset
    L = eoc.lib()
    need = 8 + 36 + 32 + 4 * (p.n * 2 * p.l * N + N * p.ks_t * ((1 << p.ks_basebit) - 1))
    assert blob.size == need == L.eoc_seeded_cloud_key_blob_bytes(C.byref(p))
    assert blob[:8].tobytes() == b"EOCCKS1\0"
    assert need * 5 < L.eoc_cloud_key_blob_bytes(C.byref(p))                         # 7.9 x (Set A) / 6 x (Set B) smaller
    q = eoc.seeded_cloud_key_params(blob)
    assert (q.n, q.l, q.Bgbit, q.ks_t, q.ks_basebit, q.ks_stdev, q.bk_stdev) == \
        (p.n, p.l, p.Bgbit, p.ks_t, p.ks_basebit, p.ks_stdev, p.bk_stdev)
    out_bk, out_ksk = np.zeros(bk.size, np.int32), np.zeros(ksk.size, np.int32)
    bad_magic = blob.copy()
    bad_magic[:8] = np.frombuffer(b"EOCCK1\0\0", np.uint8)
    bad_params = blob.copy()
    bad_params[8:12] = np.array([p.n + 1], np.int32).view(np.uint8)                  # n + 1: the length no longer matches
    zero_n = blob.copy()
    zero_n[8:12] = 0                                                                # n = 0: not a parameter set
    qq = eoc.Params()
    for bad, ln in ((blob, need - 1), (blob, 75), (bad_magic, need), (bad_params, need), (zero_n, need),
                    (sk.export_cloud_key(), L.eoc_cloud_key_blob_bytes(C.byref(p)))):
        assert L.eoc_seeded_cloud_key_blob_params(bad.ctypes.data, ln, C.byref(qq)) == EOC_ERR_ARG
        assert L.eoc_seeded_cloud_key_expand(bad.ctypes.data, ln, out_bk.ctypes.data, out_ksk.ctypes.data) == EOC_ERR_ARG
        assert L.eoc_global_import_seeded_cloud_key_blob(bad.ctypes.data, ln) == EOC_ERR_ARG
        assert L.eoc_global_key_mode() == 0
        h = C.c_void_p()
        assert L.eoc_engine_create_from_seeded_cloud_key_blob(0, bad.ctypes.data, ln, C.byref(h)) == EOC_ERR_ARG and not h.value
    assert not out_bk.any() and not out_ksk.any()                                   # nothing was written
    small = np.zeros(need - 1, np.uint8)
    assert L.eoc_seeded_cloud_key_export(sk.h, small.ctypes.data, need - 1) == EOC_ERR_ARG
    # the seeded blob is not an EOCCK1 blob either
    assert L.eoc_global_import_cloud_key_blob(blob.ctypes.data, blob.size) == EOC_ERR_ARG and L.eoc_global_key_mode() == 0
