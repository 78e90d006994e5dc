"""Leveled operations, host side (no GPU): selector encryption against a numpy restatement on the oracle's streams, the row
structure of a selector, the keyed and the refused forms, the CMux reference (tests/c/cmux_ref.c) pinned to
orc_blind_rotate_step and held to the exact schoolbook product, the composed table read on the CPU, eoc_table_trivial, the
argument errors, and the noise model of one CMux against the reference.  Device side: tests/test_gpu_cmux.py."""
import ctypes as C

import numpy as np
import pytest

import cmux_oracle as cx
import compact_oracle as co
import oracle_lib as ol
from eoc_tfhe_amd import noise

N = 1024
EOC_ERR_ARG, EOC_ERR_STATE = -1, -6


@pytest.fixture(scope="module")
def eoc(built_lib):
    import eoc_tfhe_amd
    return eoc_tfhe_amd


def custom(eoc, l, Bgbit, pset=0):
    p = eoc.default_params(pset)
    p.l, p.Bgbit = l, Bgbit
    return p


def wrap32(x):
    return ((np.asarray(x, np.int64) + 2**31) % 2**32) - 2**31


def tlwe_phase(tlwe, tlwe_key):
    """phase polynomial c1 - c0 s' of TLWE samples [...][2][N] (int64, wrapped)"""
    t = np.asarray(tlwe, np.int64).reshape(-1, 2, N)
    out = t[:, 1].copy()
    for m in np.flatnonzero(np.asarray(tlwe_key)):
        out -= np.concatenate((-t[:, 0, N - m:], t[:, 0, :N - m]), axis=1)
    return wrap32(out).reshape(np.asarray(tlwe).shape[:-2] + (N,))


@pytest.mark.parametrize("pset", [0, 1])
def test_selector_encryption_equals_the_restatement_on_the_oracle_streams(eoc, pset):
    p = eoc.default_params(pset)
    sk = eoc.SecretKey(p, 3, with_cloud_key=False)
    got = sk.encrypt_selector_bits([0, 1, 1], enc_seed=41 + pset, first_idx=5)
    assert got.shape == (3, 2 * p.l, 2, N) and got.size == 3 * eoc.lib().eoc_tgsw_len(C.byref(p))
    want = cx.tgsw_encrypt(p, sk.tlwe_key, 41 + pset, 5, [0, 1, 1])
    assert np.array_equal(got, want)
    # selector s of a call at first_idx is selector 0 of a call at first_idx + s
    assert np.array_equal(sk.encrypt_selector_bits([1], 41 + pset, first_idx=6)[0], got[1])


@pytest.mark.parametrize("pset", [0, 1])
def test_every_row_is_the_gadget_message_plus_noise(eoc, pset):
    p = eoc.default_params(pset)
    sk = eoc.SecretKey(p, 4, with_cloud_key=False)
    sel = sk.encrypt_selector_bits([0, 1] * 8, enc_seed=7)
    ph = tlwe_phase(sel, sk.tlwe_key).astype(np.int64)                     # [16][2l][N]
    a = sel[:, :, 0].astype(np.int64)
    for s in range(16):
        for row in range(2 * p.l):
            q, pp = row // p.l, row % p.l + 1
            msg = np.zeros(N, np.int64)
            if s & 1:
                # row (q, p) carries h on polynomial q: on the mask (q = 0) the phase sees -h s', on the body +h
                h = 1 << (32 - pp * p.Bgbit)
                if q:
                    msg[0] = h
                else:
                    msg = -h * sk.tlwe_key.astype(np.int64)
            ph[s, row] = wrap32(ph[s, row] - msg)
    e = ph / 2.0**32
    assert np.abs(e).max() < 6 * p.bk_stdev
    assert abs(e.var() / noise._sig2(p) - 1) < 0.02, e.var() / noise._sig2(p)   # 2^17 draws: s.e. 0.4 %
    assert len({r.tobytes() for r in a.reshape(-1, N)}) == 16 * 2 * p.l        # no mask is repeated


def test_keyed_form_and_the_refusal_for_a_secure_key(eoc):
    L = eoc.lib()
    p = eoc.default_params(0)
    sk = eoc.SecretKey(p, None, master=bytes(range(32)), with_cloud_key=False)
    bits = np.array([1, 0], np.uint8)
    out = [np.zeros((2, 2 * p.l, 2, N), np.int32) for _ in range(4)]
    k1, k2 = np.arange(32, dtype=np.uint8), np.arange(1, 33, dtype=np.uint8)
    for o, k in zip(out, (k1, k1, k2)):
        assert L.eoc_tgsw_encrypt_bits_keyed(sk.h, k.ctypes.data, 0, bits.ctypes.data, 2, o.ctypes.data) == 0
    assert np.array_equal(out[0], out[1]) and not np.array_equal(out[0][:, :, 0], out[2][:, :, 0])
    zero = np.zeros(1, np.uint8)
    assert L.eoc_tgsw_encrypt_bits_keyed(sk.h, k1.ctypes.data, 1, zero.ctypes.data, 1, out[3].ctypes.data) == 0
    assert np.array_equal(out[3][0], out[0][1])                   # the stream index is first_idx + s
    ph = tlwe_phase(out[0][1], sk.tlwe_key)                                   # bit 0: every row a TLWE sample of 0
    assert np.abs(ph).max() < 6 * p.bk_stdev * 2**32
    # the seeded (test) form is refused for a secure-mode key, nothing is written
    o = np.full((2, 2 * p.l, 2, N), 7, np.int32)
    assert L.eoc_tgsw_encrypt_bits(sk.h, 1, 0, bits.ctypes.data, 2, o.ctypes.data) == EOC_ERR_STATE
    assert (o == 7).all()
    with pytest.raises(eoc.EocError):
        sk.encrypt_selector_bits([1], enc_seed=1)
    # the wrapper's secure path: a fresh key per call
    a, b = sk.encrypt_selector_bits([1], None), sk.encrypt_selector_bits([1], None)
    assert not np.array_equal(a[:, :, 0], b[:, :, 0])
    with pytest.raises(eoc.EocError):
        sk.encrypt_selector_bits([1], None, first_idx=3)


SHAPES = [(0, None, None), (1, None, None), (0, 1, 10), (0, 4, 7)]


def shape_params(eoc, shape):
    pset, l, Bgbit = shape
    return eoc.default_params(pset) if l is None else custom(eoc, l, Bgbit, pset)


@pytest.mark.parametrize("shape", SHAPES)
def test_reference_is_pinned_to_the_oracle_step(eoc, shape):
    """D = (X^a - 1) acc: cmux_ref.c equals orc_blind_rotate_step(..., a, acc, use_fft = 1) bit for bit"""
    p = shape_params(eoc, shape)
    sk = eoc.SecretKey(p, 5, with_cloud_key=False)
    op = cx.orc_params(p)
    rng = np.random.default_rng(sum(x or 0 for x in shape))
    sel = sk.encrypt_selector_bits([1, 0], enc_seed=9)
    fft = cx.to_fft(sel)
    for k, a in enumerate((1, 1023, 1024, 2047)):
        acc = rng.integers(-2**31, 2**31, (2, N)).astype(np.int32)
        want = acc.copy()
        ol.lib().orc_blind_rotate_step(C.byref(op), fft[k & 1].ctypes.data, None, a, want, 1)
        assert np.array_equal(cx.cmux(op, fft[k & 1], acc, acc, rot=a), want), (shape, a)


@pytest.mark.parametrize("shape", SHAPES)
def test_reference_is_within_8_lsb_of_the_exact_product(eoc, shape):
    p = shape_params(eoc, shape)
    sk = eoc.SecretKey(p, 6, with_cloud_key=False)
    op = cx.orc_params(p)
    rng = np.random.default_rng(100 + sum(x or 0 for x in shape))
    sel = sk.encrypt_selector_bits([1, 0], enc_seed=10)
    fft = cx.to_fft(sel)
    for k in range(2):
        A, B = (rng.integers(-2**31, 2**31, (2, N)) for _ in range(2))
        got = cx.extprod(op, fft[k], B - A)
        exact = cx.extprod_exact(p, sel[k], B - A)
        assert np.abs(wrap32(got.astype(np.int64) - exact)).max() <= 8, shape


def table_values(d, lw):
    """ints mod 8, slot (entry e, w): neighbours in e and in w differ"""
    W, entries = 1 << lw, 1 << (d + 10 - lw)
    e, w = np.arange(entries)[:, None], np.arange(W)[None, :]
    return ((5 * e + 3 * w + e // 8 + e // 64) % 8).astype(np.uint8)


def test_composed_read_on_the_cpu_decrypts_every_index(eoc):
    d, lw = 2, 2
    p = eoc.default_params(0)
    sk = eoc.SecretKey(p, 1, with_cloud_key=False)
    orc = ol.Oracle(0, 1, with_bk=False)
    op = cx.orc_params(p)
    vals = table_values(d, lw)                                              # [1024][4]
    table = eoc.trivial_table(co.int_msgs(vals.ravel(), 8))
    assert table.shape == (4, 2, N)
    depth = d + 10 - lw
    # one selector per (bit position, bit value): index idx uses [k][idx >> k & 1]
    both = cx.to_fft(sk.encrypt_selector_bits([0, 1] * depth, enc_seed=77)).reshape(depth, 2, 2 * p.l, 2, N)
    idx = np.arange(1 << depth)
    sel = [np.stack([both[k, (i >> k) & 1] for k in range(depth)]) for i in idx]
    out, tl = cx.table_read(orc, op, table, d, lw, sel)
    got = sk.decrypt_ints(out.reshape(-1, p.n + 1), 8).reshape(len(idx), 1 << lw)
    assert np.array_equal(got, vals[idx])
    # before the key switch, slot 0's error has the mean the model derives from the index (noise.table_read_mean): the CMuxes
    # whose bit is 1 each leave -(q/2) J(1 - s') at the slot the entry occupied behind them
    err = wrap32(tlwe_phase(tl, sk.tlwe_key)[:, 0] - co.int_msgs(vals[idx, 0], 8)) / 2.0**32
    model = np.array([noise.table_read_mean(p, sk.tlwe_key, i, d, lw) for i in idx])
    res = err - model
    z = res.mean() / (res.std() / np.sqrt(len(res)))
    print(f"read error before the key switch: mean {err.mean():.3e} (model {model.mean():.3e}), residual z {z:.2f}, "
          f"residual var / (mean depth x cmux_var) {res.var() / (depth / 2 * noise.cmux_var(p, sk.tlwe_key) + depth / 2 * noise.cmux_var(p, sk.tlwe_key, 0)):.3f}")
    assert abs(z) < 4 and abs(err.mean() / model.mean() - 1) < 0.1


def test_trivial_table_layout_and_argument_errors(eoc):
    L = eoc.lib()
    msgs = np.arange(1, 1500, dtype=np.int32)
    t = eoc.trivial_table(msgs)
    assert t.shape == (2, 2, N) and not t[:, 0].any()
    assert np.array_equal(t[:, 1].ravel()[:1499], msgs) and not t[1, 1, 1499 - N:].any()
    p = eoc.default_params(0)
    sk = eoc.SecretKey(p, 2, with_cloud_key=False)
    bits = np.ones(1, np.uint8)
    o = np.zeros(eoc.lib().eoc_tgsw_len(C.byref(p)), np.int32)
    key = np.zeros(32, np.uint8)
    assert L.eoc_tgsw_encrypt_bits(None, 1, 0, bits.ctypes.data, 1, o.ctypes.data) == EOC_ERR_ARG
    assert L.eoc_tgsw_encrypt_bits(sk.h, 1, 0, None, 1, o.ctypes.data) == EOC_ERR_ARG
    assert L.eoc_tgsw_encrypt_bits(sk.h, 1, 0, bits.ctypes.data, 1, None) == EOC_ERR_ARG
    assert L.eoc_tgsw_encrypt_bits_keyed(sk.h, None, 0, bits.ctypes.data, 1, o.ctypes.data) == EOC_ERR_ARG
    assert L.eoc_tgsw_encrypt_bits_keyed(sk.h, key.ctypes.data, 0, bits.ctypes.data, 0, o.ctypes.data) == 0 and not o.any()
    assert L.eoc_table_trivial(None, 1, o.ctypes.data) == EOC_ERR_ARG
    assert L.eoc_table_trivial(msgs.ctypes.data, 1, None) == EOC_ERR_ARG
    # device entry points: null engine / null pointers are refused before anything touches a device
    assert L.eoc_tgsw_to_fft_device(None, 1, 1, 1, None) == EOC_ERR_ARG
    assert L.eoc_cmux_device(None, 1, 1, 1, 1, 1, None) == EOC_ERR_ARG
    assert L.eoc_table_read_device(None, 1, 0, 0, 1, 1, 1, None) == EOC_ERR_ARG
    assert L.eoc_engine_cmux_launches(None) == 0
    # the global read checks its shape before it looks for a key or a device
    x = np.zeros(8, np.int32)
    for d, lw in ((13, 0), (-1, 0), (0, 11), (0, -1)):
        assert L.eoc_table_read(x.ctypes.data, d, lw, x.ctypes.data, 1, x.ctypes.data) == EOC_ERR_ARG, (d, lw)
    assert L.eoc_table_read(None, 0, 0, x.ctypes.data, 1, x.ctypes.data) == EOC_ERR_ARG
    assert L.eoc_table_read(x.ctypes.data, 0, 0, x.ctypes.data, 0, x.ctypes.data) == 0          # no query: a no-op
    with pytest.raises(eoc.EocError):
        eoc.table_read(np.zeros((2, 2, N), np.int32), 2, 0, np.zeros((1, 12, 4, 2, N), np.int32))
    if L.eoc_global_key_mode() != 1:                                          # no global secret key
        assert L.eoc_global_tgsw_encrypt_bits(bits.ctypes.data, 1, o.ctypes.data) == -4
    names = set(eoc.abi_symbols())
    new = {"eoc_tgsw_len", "eoc_tgsw_encrypt_bits", "eoc_tgsw_encrypt_bits_keyed", "eoc_global_tgsw_encrypt_bits",
           "eoc_table_trivial", "eoc_tgsw_fft_bytes", "eoc_tgsw_to_fft_device", "eoc_cmux_device", "eoc_table_read_device",
           "eoc_engine_cmux_launches", "eoc_table_read"}
    assert new <= names and all(hasattr(L, s) for s in new)
    assert L.eoc_tgsw_fft_bytes(C.byref(p)) == 65536 == L.eoc_bkfft_bytes(C.byref(p)) // p.n
    assert L.eoc_tgsw_fft_bytes(C.byref(eoc.default_params(1))) == 98304


SLOTS = np.arange(16) * 64


@pytest.mark.parametrize("pset", [0, 1])
def test_cmux_noise_matches_the_model(eoc, pset):
    """16 384 samples = 16 slots x 1 024 independent (selector, input) pairs, bit 1, random full-range inputs: the error of
    slot j is phase(out)[j] - phase(in1)[j].  Its mean is cmux_mean(slot) -- the truncating decomposition's -(q/2) J(1 - s')
    -- and its variance around the slot's mean cmux_var, within 8 % (5 standard errors of a variance on 16 384 samples, 1.1 %
    each, plus the 3 % the model is held to elsewhere)."""
    p = eoc.default_params(pset)
    sk = eoc.SecretKey(p, 11, with_cloud_key=False)
    op = cx.orc_params(p)
    pairs = 1024
    rng = np.random.default_rng(200 + pset)
    sel = sk.encrypt_selector_bits(np.ones(pairs, np.uint8), enc_seed=300 + pset)
    err = np.zeros((pairs, len(SLOTS)))
    for k in range(pairs):
        A, B = (rng.integers(-2**31, 2**31, (2, N)).astype(np.int32) for _ in range(2))
        out = cx.cmux(op, cx.to_fft(sel[k]), A, B)
        err[k] = wrap32(tlwe_phase(out, sk.tlwe_key)[SLOTS] - tlwe_phase(B, sk.tlwe_key)[SLOTS]) / 2.0**32
    var = float(err.var(axis=0, ddof=1).mean())
    model = noise.cmux_var(p, sk.tlwe_key)
    z = (err.mean(0) - noise.cmux_mean(p, sk.tlwe_key, SLOTS)) / (err.std(0) / np.sqrt(pairs))
    print(f"pset {pset}: var {var:.4e} model {model:.4e} ratio {var / model:.4f}; slot means z in [{z.min():.2f}, {z.max():.2f}]; "
          f"mean at slot 0 {err[:, 0].mean():.3e} model {float(noise.cmux_mean(p, sk.tlwe_key, 0)):.3e}")
    assert abs(var / model - 1) < 0.08
    assert np.abs(z).max() < 4.5                                             # 16 slots: 4.5 sigma two-sided is 1e-4
    # a selector of 0 leaves the rows' term alone
    assert noise.cmux_var(p, sk.tlwe_key, bit=0) < model


@pytest.mark.parametrize("pset", [0, 1])
def test_a_read_output_has_less_variance_than_a_gate_output(eoc, pset):
    """from the model alone: for every supported depth (up to 22), a trivial or a public-key-encrypted table"""
    p = eoc.default_params(pset)
    sk = eoc.SecretKey(p, 12, with_cloud_key=False)
    gate = noise.predict(p, sk.lwe_key, sk.tlwe_key)["total_var"]
    enc = noise.compact_var(p, sk.tlwe_key)
    for depth in range(0, 23):
        for tv in (0.0, enc):
            v = noise.table_read_var(p, sk.lwe_key, sk.tlwe_key, depth, tv)
            assert v < gate, (depth, tv, v, gate)
    assert noise.table_read_var(p, sk.lwe_key, sk.tlwe_key, 22, enc) < 0.5 * gate
    # the deterministic part (table_read_mean) is bounded by depth (q/2) max |J (1 - s')|
    q = 2.0 ** (-p.l * p.Bgbit)
    worst = max(abs(noise.table_read_mean(p, sk.tlwe_key, idx, 12, 0)) for idx in (0, 1, 2**22 - 1, 2**22 - 1024, 1023 << 0))
    assert worst <= 22 * (q / 2) * (1 + int(sk.tlwe_key.sum())) + 1e-12
