"""Compact public-key encryption, host side (include/eoc_tfhe_gpu.h): the public key and reproducible lists
against the oracle-stream restatement (tests/compact_oracle.py) bit for bit, the noise of extracted samples against
noise.compact_var, an oracle-composed expansion, the EOCPK1 blob and argument errors, the model's margin statement, and the
new kernel's registers.  GPU side: tests/test_gpu_compact.py."""
import ctypes as C
import re

import numpy as np
import pytest

import compact_oracle as co
import isa_lib
import oracle_lib as ol
from eoc_tfhe_amd import noise

N = 1024
EOC_ERR_ARG = -1


@pytest.fixture(scope="module")
def eoc(built_lib):
    import eoc_tfhe_amd
    return eoc_tfhe_amd


_KEYS = {}


def key(eoc, pset, seed=1, n=None):
    if (pset, seed, n) not in _KEYS:
        p = eoc.default_params(pset)
        if n is not None:
            p.n = n
        _KEYS[(pset, seed, n)] = (p, eoc.SecretKey(p, seed, with_cloud_key=False))
    return _KEYS[(pset, seed, n)]


@pytest.mark.parametrize("pset", [0, 1])
def test_public_key_equals_the_oracle_stream_restatement(eoc, pset):
    p, sk = key(eoc, pset, 5)
    blob = sk.public_key_bytes()
    assert len(blob) == 8 + 36 + 8 * N == eoc.lib().eoc_public_key_blob_bytes(C.byref(p)) and blob[:8] == b"EOCPK1\0\0"
    pk = eoc.PublicKey(blob)
    assert (pk.params.n, pk.params.l, pk.params.bk_stdev) == (p.n, p.l, p.bk_stdev)
    orc = ol.Oracle(pset, 5, with_bk=False)
    assert np.array_equal(orc.tlwe_key, sk.tlwe_key)
    A, B = co.public_key(5, orc.tlwe_key, p.bk_stdev)
    assert np.array_equal(pk.A.view(np.uint32), A) and np.array_equal(pk.B.view(np.uint32), B)
    assert sk.public_key_bytes() == blob
    e = noise.pk_noise(pk, sk.tlwe_key)                    # B - A s' is the key's gaussian noise
    assert 0.9 < e.std() / p.bk_stdev < 1.1


def test_secure_public_keys_are_deterministic_per_key_and_differ_between_keys(eoc):
    p = eoc.default_params(0)
    m1, m2 = bytes(range(32)), bytes(range(1, 33))
    a = eoc.SecretKey(p, None, with_cloud_key=False, master=m1).public_key_bytes()
    b = eoc.SecretKey(p, None, with_cloud_key=False, master=m1).public_key_bytes()
    c = eoc.SecretKey(p, None, with_cloud_key=False, master=m2).public_key_bytes()
    d = eoc.SecretKey(p, None, with_cloud_key=False).public_key_bytes()
    assert a == b and a != c and d not in (a, c)
    assert a[:44] == c[:44]                                # same magic and parameters, different A | B


@pytest.mark.parametrize("pset", [0, 1])
def test_reproducible_lists_equal_the_restatement(eoc, pset):
    p, sk = key(eoc, pset, 5)
    pk = eoc.PublicKey(sk.public_key_bytes())
    rng = np.random.default_rng(pset)
    A, B = pk.A.view(np.uint32), pk.B.view(np.uint32)
    bits = rng.integers(0, 2, 2 * N + 300).astype(np.uint8)          # two full lists and a partial third
    got = pk.encrypt_bits(bits, enc_seed=41, first_list=7)
    assert got.shape == (3, 2, N)
    assert np.array_equal(got, co.encrypt(A, B, 41, 7, co.bit_msgs(bits), p.bk_stdev))
    for q in (2, 4, 8):
        vals = rng.integers(0, q, N + 5).astype(np.uint8)
        got = pk.encrypt_ints(vals, q, enc_seed=42 + q, first_list=3 * q)
        assert np.array_equal(got, co.encrypt(A, B, 42 + q, 3 * q, co.int_msgs(vals, q), p.bk_stdev)), q
    # the list index is the stream index: list 1 of a call from list 0 is list 0 of a call from list 1
    assert np.array_equal(pk.encrypt_bits(bits, 9, 0)[1:2], pk.encrypt_bits(bits[N:2 * N], 9, 1))
    # the secure form draws a fresh key per call
    x, y = pk.encrypt_bits(bits[:10]), pk.encrypt_bits(bits[:10])
    assert x.shape == (1, 2, N) and not np.array_equal(x, y)


@pytest.mark.parametrize("pset", [0, 1])
def test_extracted_phases_decode_and_noise_matches_compact_var(eoc, pset):
    """16 384 samples: 16 slots (64 apart) of each of 1 024 lists, so that the correlated part of e1 s' within one list
    averages out; error = phase - message - the slot's offset (u e with mean 1/2)"""
    p, sk = key(eoc, pset, 3)
    pk = eoc.PublicKey(sk.public_key_bytes())
    rng = np.random.default_rng(10 + pset)
    bits = rng.integers(0, 2, N * N).astype(np.uint8)
    lists = pk.encrypt_bits(bits, enc_seed=77)
    L = np.arange(N)
    idx = (L[:, None] * N + (L[:, None] + 64 * np.arange(16)[None, :]) % N).ravel()
    ph = co.phases(lists, idx, sk.tlwe_key)
    assert np.array_equal((ph > 0).astype(np.uint8), bits[idx])
    off = noise.compact_offset(sk.tlwe_key, pk)
    err = (ph - co.bit_msgs(bits[idx])) / 2.0**32 - off[idx % N]
    cv = noise.compact_var(p, sk.tlwe_key, pk)
    ratio = err.var() / cv
    print(f"pset {pset}: measured var {err.var():.4e}, compact_var {cv:.4e}, ratio {ratio:.4f}, "
          f"mean {err.mean():.3e} ({err.mean() / (err.std() / np.sqrt(len(err))):.2f} se)")
    assert abs(ratio - 1) < 0.05, ratio
    # without the key's e, the model's expectation over keys is close too
    assert abs(noise.compact_var(p, sk.tlwe_key) / cv - 1) < 0.2


@pytest.mark.parametrize("pset", [0, 1])
def test_host_side_expansion_decrypts_under_the_lwe_key(eoc, pset):
    p, sk = key(eoc, pset, 5)
    orc = ol.Oracle(pset, 5, with_bk=False)
    pk = eoc.PublicKey(sk.public_key_bytes())
    rng = np.random.default_rng(20 + pset)
    bits = rng.integers(0, 2, N + 40).astype(np.uint8)
    lists = pk.encrypt_bits(bits, enc_seed=5)
    idx = np.r_[0:8, 1016:1032, N + 30:N + 40]
    out = co.expand(orc, lists, idx)
    assert np.array_equal(orc.decrypt_bits(out), bits[idx])
    vals = rng.integers(0, 8, 40).astype(np.uint8)
    out = co.expand(orc, pk.encrypt_ints(vals, 8, enc_seed=6), np.arange(40))
    assert np.array_equal(sk.decrypt_ints(out, 8), vals)


def test_blob_round_trip_and_refusals(eoc):
    L = eoc.lib()
    p, sk = key(eoc, 0, 5, n=48)
    blob = sk.public_key_bytes()
    pk = eoc.PublicKey(blob)
    assert eoc.PublicKey.from_bytes(pk.to_bytes()).to_bytes() == blob
    q = eoc.Params()
    assert L.eoc_public_key_blob_params(blob, len(blob), C.byref(q)) == 0 and q.n == 48
    bits = np.array([1, 0, 1], np.uint8)
    out = np.zeros((1, 2, N), np.int32)
    assert L.eoc_pk_encrypt_bits(blob, len(blob), 1, 0, bits.ctypes.data, 3, out.ctypes.data) == 0
    bad_magic = b"EOCPK2" + blob[6:]
    truncated = blob[:-4]
    longer = blob + b"\0\0\0\0"
    sk_full = eoc.SecretKey(p, 5)
    ck = sk_full.export_cloud_key().tobytes()
    sk1 = sk_full.export_bytes()
    sk2 = eoc.SecretKey(p, None, with_cloud_key=False).export_bytes()
    assert ck[:6] == b"EOCCK1" and sk1[:6] == b"EOCSK1" and sk2[:6] == b"EOCSK2"
    for b in (bad_magic, truncated, longer, ck, sk1, sk2, b""):
        assert L.eoc_public_key_blob_params(b, len(b), C.byref(q)) == EOC_ERR_ARG
        out[:] = 7
        assert L.eoc_pk_encrypt_bits(b, len(b), 1, 0, bits.ctypes.data, 3, out.ctypes.data) == EOC_ERR_ARG
        assert (out == 7).all()
        with pytest.raises(eoc.EocError):
            eoc.PublicKey(b)
    # a buffer too small for the export
    small = (C.c_ubyte * (len(blob) - 1))()
    assert L.eoc_public_key_export(sk.h, small, len(small)) == EOC_ERR_ARG
    assert L.eoc_public_key_export(None, small, len(small)) == EOC_ERR_ARG


def test_argument_errors_write_nothing(eoc):
    L = eoc.lib()
    _, sk = key(eoc, 0, 5, n=48)
    blob = sk.public_key_bytes()
    n = len(blob)
    key32 = np.arange(32, dtype=np.uint8)
    vals = np.array([0, 1, 3], np.uint8)
    out = np.full((1, 2, N), 7, np.int32)
    o, v, k = out.ctypes.data, vals.ctypes.data, key32.ctypes.data
    calls = [
        lambda: L.eoc_pk_encrypt_bits(None, n, 1, 0, v, 3, o),
        lambda: L.eoc_pk_encrypt_bits(blob, n, 1, 0, None, 3, o),
        lambda: L.eoc_pk_encrypt_bits(blob, n, 1, 0, v, 3, None),
        lambda: L.eoc_pk_encrypt_bits_keyed(blob, n, None, 0, v, 3, o),
        lambda: L.eoc_pk_encrypt_ints(blob, n, 1, 0, 16, v, 3, o),
        lambda: L.eoc_pk_encrypt_ints(blob, n, 1, 0, 0, v, 3, o),
        lambda: L.eoc_pk_encrypt_ints(blob, n, 1, 0, 3, v, 3, o),
        lambda: L.eoc_pk_encrypt_ints(blob, n, 1, 0, 2, v, 3, o),          # 3 >= 2
        lambda: L.eoc_pk_encrypt_ints_keyed(blob, n, k, 0, 2, v, 3, o),
        lambda: L.eoc_pk_encrypt_ints_keyed(blob, n, None, 0, 4, v, 3, o),
        lambda: L.eoc_pk_encrypt_ints_keyed(blob, n, k, 0, 5, v, 3, o),
        lambda: L.eoc_compact_expand(None, 3, o),
        lambda: L.eoc_compact_expand(o, 3, None),
    ]
    for i, f in enumerate(calls):
        assert f() == EOC_ERR_ARG, i
        assert (out == 7).all(), i
    # count 0: nothing to do, nothing written
    for f in (lambda: L.eoc_pk_encrypt_bits(blob, n, 1, 0, v, 0, o), lambda: L.eoc_pk_encrypt_ints_keyed(blob, n, k, 0, 4, v, 0, o),
              lambda: L.eoc_compact_expand(o, 0, o)):
        assert f() == 0 and (out == 7).all()
    assert L.eoc_pk_encrypt_ints_keyed(blob, n, k, 0, 4, v, 3, o) == 0 and not (out == 7).all()
    with pytest.raises(eoc.EocError):
        eoc.PublicKey(blob).encrypt_bits([1], first_list=3)      # a list index only exists in the test mode


def test_global_public_key_export(eoc):
    import base64
    _, sk = key(eoc, 0, 5, n=48)
    assert eoc.global_key_mode() == 0
    assert eoc.lib().eoc_global_public_key_export(None, 0) == 0
    assert eoc.Tfhe.importSecretKey(base64.b64encode(sk.export_bytes()).decode()) == 0
    try:
        assert eoc.global_key_mode() == 1
        assert eoc.global_public_key_export() == sk.public_key_bytes()
        small = (C.c_ubyte * 16)()
        assert eoc.lib().eoc_global_public_key_export(small, 16) == 8236
    finally:
        eoc.Tfhe.resetGateKey()


@pytest.mark.parametrize("pset", [0, 1])
def test_model_expanded_inputs_are_quieter_than_gate_outputs(eoc, pset):
    """after the key switch an expanded sample carries compact_var + ks_var; every margin stated for gate-output inputs
     assumes total_var: the model must put the first below the second"""
    p = eoc.default_params(pset)
    sk = eoc.SecretKey(p, 1)
    pk = eoc.PublicKey(sk.public_key_bytes())
    pred = noise.predict(p, sk.lwe_key, sk.tlwe_key, sk.ksk)
    cv = noise.compact_var(p, sk.tlwe_key, pk)
    expanded = cv + pred["ks_var"]
    print(f"pset {pset}: compact sigma {np.sqrt(cv):.3e}, expanded sigma {np.sqrt(expanded):.5f}, "
          f"gate output sigma {np.sqrt(pred['total_var']):.5f}")
    assert cv < 1e-3 * pred["ks_var"]                      # the public-key terms vanish behind the key switch
    assert expanded < pred["total_var"]
    assert expanded < noise.predict(p, sk.lwe_key, sk.tlwe_key)["total_var"]     # also with the average-key key switch


def test_isa_compact_expand_kernel_has_no_spill_no_scratch_vector_stores_only():
    text = isa_lib.engine_isa()
    meta = isa_lib.kernel_meta(text)
    hits = [k for k in meta if "k_compact_expand" in k]
    assert len(hits) == 1, hits
    m = meta[hits[0]]
    assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, m
    assert not any("blind_rotate" in k or "keyswitch_waves" in k for k in hits)
    parts = re.split(r"^(\S+):\s*;\s*@\S+\s*$", text, flags=re.M)
    body = [parts[i + 1] for i in range(1, len(parts), 2) if parts[i] == hits[0]][0]
    body = body[:body.find("s_endpgm")]
    ops = [ln.split()[0] for ln in body.splitlines()
           if ln.strip() and not ln.strip().startswith((".", ";")) and not ln.strip().endswith(":")]
    writes = sorted({o for o in ops if "store" in o or "atomic" in o or o.startswith("ds_write")})
    assert writes and all(o.startswith(("global_store_dword", "ds_write_b32")) for o in writes), writes
