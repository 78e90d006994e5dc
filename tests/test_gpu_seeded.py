"""Seeded ciphertexts, selectors and cloud key on the MI355X: the kernels' ChaCha20 block function against the
host's on the RFC 8439 vector, across the carry of the 64-bit block counter and with 64-bit stream indices; k_seed_masks'
LWE rows against the host twin word for word on every row length and count at which the kernel takes another path (no partial
block, 1 / 4 / 6 / 7 words in the last block, aligned and unaligned rows, one row to many workgroups, indices across 2^32),
with sentinels around the output; expanded samples as gate inputs against the oracle bit for bit; the key images of an engine
made from the EOCCKS1 blob against those of an engine loaded with the host-expanded arrays, byte for byte, with gates; seeded
selectors against the converted host-expanded ones byte for byte, and in a table read; the global context in key mode 2 and
on one and two engines.  Host side: tests/test_seeded_cpu.py."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as ol
from gpu_util import dev_empty, sync, to_dev, torch_cuda

pytestmark = pytest.mark.gpu
N = 1024
EOC_ERR_ARG = -1
ONE8 = 1 << 29
SENTINEL = 0x5EEDF00D
SEED = bytes(range(7, 39))


@pytest.fixture(scope="module")
def eoc(built_lib):
    torch_cuda()
    import eoc_tfhe_amd
    return eoc_tfhe_amd


_KEYS = {}


def keys(eoc, pset):
    """params, secret key (seed 1), its EOCCKS1 blob, the host-expanded (bk, ksk), an engine made from the blob"""
    if pset not in _KEYS:
        p = eoc.default_params(pset)
        sk = eoc.SecretKey(p, 1, with_cloud_key=False)
        blob = sk.seeded_cloud_key_bytes()
        bk, ksk = eoc.seeded_cloud_key_expand(blob)
        _KEYS[pset] = (p, sk, blob, bk, ksk, eoc.Engine.from_seeded_cloud_key_blob(blob))
    return _KEYS[pset]


def host_blocks(eoc, key, counter, nonce, n_blocks):
    """blocks ChaCha20(key, counter + i, nonce) of the host's block function: [n_blocks][16] words"""
    L = eoc.lib()
    k = np.frombuffer(key, np.uint8).copy()
    out = np.zeros((n_blocks, 64), np.uint8)
    for i in range(n_blocks):
        c = (counter + i) & (2**64 - 1)
        n12 = np.array([c >> 32, nonce & 0xFFFFFFFF, nonce >> 32], np.uint32).view(np.uint8).copy()
        L.eoc_dbg_chacha20_block(k.ctypes.data, c & 0xFFFFFFFF, n12.ctypes.data, out[i].ctypes.data)
    return out.view(np.uint32)


def device_blocks(eoc, eng, key, counter, nonce, n_blocks):
    torch = torch_cuda()
    k = np.frombuffer(key, np.uint8).copy()
    d = dev_empty((n_blocks, 16), torch.int32)
    assert eoc.lib().eoc_dbg_chacha20_blocks_device(eng.h, k.ctypes.data, counter, nonce, n_blocks, d.data_ptr(), None) == 0
    sync()
    return d.cpu().numpy().view(np.uint32)


def test_block_function_equals_the_hosts(eoc):
    eng = eoc.Engine(eoc.default_params(0))
    # RFC 8439 2.3.2: key 00 .. 1f, block counter 1, nonce 00 00 00 09 00 00 00 4a 00 00 00 00 -- in the original layout the
    # first nonce word is the high counter word
    rfc = device_blocks(eoc, eng, bytes(range(32)), 1 | (0x09000000 << 32), 0x4A000000, 1)
    assert rfc.view(np.uint8)[0, :16].tobytes().hex() == "10f1e7e4d13b5915500fdd1fa32071c4"
    assert rfc.view(np.uint8)[0, 48:].tobytes().hex() == "b5129cd1de164eb9cbd083e8a2503c4e"
    assert np.array_equal(rfc, host_blocks(eoc, bytes(range(32)), 1 | (0x09000000 << 32), 0x4A000000, 1))
    # the carry into the high counter word: counters 0xFFFFFFFE .. 0x1_0000_0001; 300 blocks: two workgroups
    for counter, nonce, n in ((0xFFFFFFFE, 0, 4), (0xFFFFFFFE, (0xDEADBEEF << 32) | 5, 4), (0, 2**64 - 1, 300),
                              (2**64 - 2, 1 << 63, 3)):
        got = device_blocks(eoc, eng, SEED, counter, nonce, n)
        assert np.array_equal(got, host_blocks(eoc, SEED, counter, nonce, n)), (hex(counter), hex(nonce))
    assert len({r.tobytes() for r in device_blocks(eoc, eng, SEED, 0xFFFFFFFE, 0, 4)}) == 4
    eng.close()


def expand_device(eoc, eng, seed, bodies, first_idx, n, misalign=1):
    """the expansion into a buffer with a sentinel word on either side; the rows start `misalign` words into the allocation"""
    torch = torch_cuda()
    count = len(bodies)
    words = count * (n + 1)
    d_b = to_dev(np.ascontiguousarray(bodies, np.int32)) if count else dev_empty((1,), torch.int32)
    d_buf = torch.full((misalign + words + 1,), SENTINEL, dtype=torch.int32, device="cuda")
    eng.seeded_expand_device(seed, d_b.data_ptr(), count, d_buf.data_ptr() + 4 * misalign, first_idx)
    sync()
    buf = d_buf.cpu().numpy()
    assert (buf[:misalign] == SENTINEL).all() and buf[-1] == SENTINEL, "a word outside the output was written"
    return buf[misalign:misalign + words].reshape(count, n + 1)


@pytest.mark.parametrize("n", [16, 17, 500, 630, 1023])
def test_lwe_expansion_equals_the_host_twin(eoc, n):
    """n mod 8 = 0, 1, 4, 6, 7 words in the last block; row strides of 17 .. 1024 words; 32 .. 8 rows per workgroup"""
    p = eoc.default_params(0)
    p.n = n
    eng = eoc.Engine(p)
    rng = np.random.default_rng(n)
    first = 2**32 - 2                                           # stream indices cross 32 bits inside every batch
    bodies = rng.integers(-2**31, 2**31, 1000).astype(np.int32)
    want = eoc.seeded_expand_host(p, SEED, bodies, first)
    launches = eng.seed_launches
    for count in (1, 2, 63, 64, 65, 1000):
        got = expand_device(eoc, eng, SEED, bodies[:count], first, n)
        assert np.array_equal(got, want[:count]), (n, count)
    assert eng.seed_launches == launches + 6
    # sample s of a call at first_idx is sample 0 of a call at first_idx + s (also across 2^32), on aligned rows too
    assert np.array_equal(expand_device(eoc, eng, SEED, bodies[5:70], first + 5, n, misalign=4), want[5:70])
    # count 0: a no-op that touches nothing
    assert expand_device(eoc, eng, SEED, bodies[:0], first, n).shape == (0, n + 1)
    assert eng.seed_launches == launches + 7
    eng.close()


def test_expansion_argument_errors(eoc):
    torch = torch_cuda()
    p = eoc.default_params(0)
    eng = eoc.Engine(p)
    L = eoc.lib()
    seed = np.frombuffer(SEED, np.uint8).copy()
    d = dev_empty((4 * (p.n + 1),), torch.int32)
    assert L.eoc_seeded_expand_device(eng.h, seed.ctypes.data, 0, d.data_ptr(), 4, d.data_ptr(), None) == EOC_ERR_ARG   # aliased
    assert L.eoc_seeded_expand_device(eng.h, seed.ctypes.data, 0, d.data_ptr() + 8, 4, d.data_ptr(), None) == EOC_ERR_ARG
    assert L.eoc_seeded_expand_device(eng.h, None, 0, d.data_ptr(), 4, d.data_ptr(), None) == EOC_ERR_ARG
    assert L.eoc_seeded_expand_device(eng.h, seed.ctypes.data, 0, None, 4, d.data_ptr(), None) == EOC_ERR_ARG
    assert L.eoc_tgsw_seeded_to_fft_device(eng.h, seed.ctypes.data, 0, None, 1, d.data_ptr(), None) == EOC_ERR_ARG
    b = keys(eoc, 1)[2]                                                                        # Set B blob, Set A engine
    assert L.eoc_engine_load_seeded_cloud_key(eng.h, b.ctypes.data, b.size) == EOC_ERR_ARG
    assert L.eoc_engine_load_seeded_cloud_key(eng.h, b.ctypes.data, b.size - 4) == EOC_ERR_ARG
    assert eng.seed_launches == 0
    eng.close()


def test_expanded_samples_feed_gates(eoc):
    torch = torch_cuda()
    p, sk, blob, bk, ksk, eng = keys(eoc, 0)
    orc = ol.Oracle(0, 1, with_bk=False)
    orc.bk, orc.ksk = np.ascontiguousarray(bk), np.ascontiguousarray(ksk)
    orc.bkfft = np.zeros((p.n, 2 * p.l, 2, N), np.float64)
    orc.L.orc_bk_to_fft(C.byref(orc.p), orc.bk, orc.bkfft)
    rng = np.random.default_rng(3)
    bits = rng.integers(0, 2, (2, 64)).astype(np.uint8)
    d_in, words = [], []
    for k in range(2):
        seed, bodies = sk.encrypt_bits_seeded(bits[k])
        d, d_b = dev_empty((64, p.n + 1), torch.int32), to_dev(bodies)
        eng.seeded_expand_device(seed, d_b.data_ptr(), 64, d.data_ptr())
        d_in.append(d)
        sync()
        words.append(d.cpu().numpy())
        assert np.array_equal(words[k], eoc.seeded_expand_host(p, seed, bodies))
    d_out = dev_empty((64, p.n + 1), torch.int32)
    eng.gate_batch_device(eoc.OPS["NAND"], d_in[0].data_ptr(), d_in[1].data_ptr(), None, d_out.data_ptr(), 64)
    sync()
    got = d_out.cpu().numpy()
    assert np.array_equal(sk.decrypt_bits(got), 1 - (bits[0] & bits[1]))
    assert np.array_equal(got, orc.gate_batch(ol.OPS["NAND"], words[0], words[1]))


@pytest.mark.parametrize("pset", [0, 1])
def test_cloud_key_images_equal_those_of_the_host_expanded_arrays(eoc, pset):
    torch = torch_cuda()
    p, sk, blob, bk, ksk, e1 = keys(eoc, pset)
    L = eoc.lib()
    e2 = eoc.Engine(p)
    e2.load_cloud_key(bk, ksk)
    nb, nk = L.eoc_bkfft_bytes(C.byref(p)), L.eoc_ksk_dev_bytes(C.byref(p))
    (b1, k1), (b2, k2) = e1.cloud_key_device(), e2.cloud_key_device()
    assert np.array_equal(e1.download(b1, nb), e2.download(b2, nb))                   # BK-FFT image
    img = e1.download(k1, nk, np.int32)
    assert np.array_equal(img, e2.download(k2, nk, np.int32))                         # padded KSK image, padding included
    stride = L.eoc_ksk_row_stride(C.byref(p))
    img = img.reshape(-1, stride)
    assert np.array_equal(img[:, :p.n + 1], ksk) and not img[:, p.n + 1:].any()
    # loading again over the installed images gives the same bytes
    e1.load_seeded_cloud_key(blob)
    assert np.array_equal(e1.download(e1.cloud_key_device()[1], nk, np.int32).reshape(-1, stride), img)
    rng = np.random.default_rng(10 + pset)
    bits = rng.integers(0, 2, (2, 64)).astype(np.uint8)
    d0, d1 = to_dev(sk.encrypt_bits(bits[0], 5)), to_dev(sk.encrypt_bits(bits[1], 6))
    outs = []
    for e in (e1, e2):
        before = L.eoc_engine_keyswitch_mfma_launches(e.h)
        d_out = dev_empty((64, p.n + 1), torch.int32)
        e.gate_batch_device(eoc.OPS["NAND"], d0.data_ptr(), d1.data_ptr(), None, d_out.data_ptr(), 64)
        sync()
        outs.append(d_out.cpu().numpy())
        assert L.eoc_engine_keyswitch_mfma_launches(e.h) > before                     # the limb image was installed
    assert np.array_equal(sk.decrypt_bits(outs[0]), 1 - (bits[0] & bits[1]))
    assert np.array_equal(outs[0], outs[1])
    e2.close()


@pytest.mark.parametrize("pset", [0, 1])
def test_seeded_selectors_equal_the_converted_host_expansion(eoc, pset):
    torch = torch_cuda()
    p, sk, _, _, _, eng = keys(eoc, pset)
    kpl = 2 * p.l
    for count, first in ((1, 0), (3, 2**32 - 1)):
        seed, bodies = sk.encrypt_selector_bits_seeded([1, 0, 1][:count], bytes(range(32)), SEED, first_idx=first)
        sel = eoc.tgsw_seeded_expand_host(p, seed, bodies, first)
        d_sel = to_dev(sel)
        want = dev_empty((count, kpl, 2, N), torch.float64)
        eng.tgsw_to_fft_device(d_sel.data_ptr(), count, want.data_ptr())
        got = torch.full((count * kpl * 2 * N + 2,), -1.0, dtype=torch.float64, device="cuda")
        launches, d_b = eng.seed_launches, to_dev(bodies)
        eng.tgsw_seeded_to_fft_device(seed, d_b.data_ptr(), count, got.data_ptr(), first)
        sync()
        g = got.cpu().numpy()
        assert g[-1] == -1.0 and g[-2] == -1.0
        assert np.array_equal(g[:-2].view(np.uint8), want.cpu().numpy().ravel().view(np.uint8)), (pset, count)
        assert eng.seed_launches == launches + 1


def test_table_read_with_seeded_selectors(eoc):
    torch = torch_cuda()
    p, sk, _, _, _, eng = keys(eoc, 0)
    d, lw, depth = 1, 0, 11                                     # 2 lists of 1 024 one-slot entries: 11 index bits
    rng = np.random.default_rng(4)
    msgs = np.where(rng.integers(0, 2, 2 * N), ONE8, -ONE8).astype(np.int32)
    d_tab = to_dev(eoc.trivial_table(msgs))
    idx = 1337
    seed, bodies = sk.encrypt_selector_bits_seeded([(idx >> k) & 1 for k in range(depth)])
    fft = [dev_empty((depth, 2 * p.l, 2, N), torch.float64) for _ in range(2)]
    d_b, d_sel = to_dev(bodies), to_dev(eoc.tgsw_seeded_expand_host(p, seed, bodies))
    eng.tgsw_seeded_to_fft_device(seed, d_b.data_ptr(), depth, fft[0].data_ptr())
    eng.tgsw_to_fft_device(d_sel.data_ptr(), depth, fft[1].data_ptr())
    sync()
    outs = []
    for f in fft:
        d_out = dev_empty((1, 1, p.n + 1), torch.int32)
        eng.table_read_device(d_tab.data_ptr(), d, lw, f.data_ptr(), 1, d_out.data_ptr())
        sync()
        outs.append(d_out.cpu().numpy().reshape(1, p.n + 1))
    assert np.array_equal(outs[0], outs[1])
    assert sk.decrypt_bits(outs[0])[0] == int(msgs[idx] > 0)


def test_global_context_in_key_mode_2_and_on_one_and_two_engines(eoc):
    p, sk, blob, bk, ksk, _ = keys(eoc, 0)
    L = eoc.lib()
    assert eoc.global_key_mode() == 0
    rng = np.random.default_rng(8)
    bits = rng.integers(0, 2, (2, 16)).astype(np.uint8)
    bodies = rng.integers(-2**31, 2**31, 3001).astype(np.int32)
    first = 2**32 - 1500
    want = eoc.seeded_expand_host(p, SEED, bodies, first)
    try:
        eoc.gpu_shutdown()
        eoc.global_import_seeded_cloud_key_blob(blob)
        assert eoc.global_key_mode() == 2
        out = eoc.global_gate_batch(eoc.OPS["NAND"], sk.encrypt_bits(bits[0], 7), sk.encrypt_bits(bits[1], 8))
        assert np.array_equal(sk.decrypt_bits(out), 1 - (bits[0] & bits[1]))
        assert np.array_equal(eoc.seeded_expand(SEED, bodies, first), want)
        ck = eoc.global_cloud_key_export()                       # EOCCK1 of the host-expanded arrays, made on demand
        assert ck.size == L.eoc_cloud_key_blob_bytes(C.byref(p)) and ck[:8].tobytes() == b"EOCCK1\0\0"
        words = ck[8 + 36:].view(np.int32)
        assert np.array_equal(words[:bk.size], bk.ravel()) and np.array_equal(words[bk.size:], ksk.ravel())
        with pytest.raises(eoc.EocError):
            eoc.global_import_seeded_cloud_key_blob(blob)        # one key per process
    finally:
        eoc.Tfhe.resetGateKey()
    assert eoc.global_key_mode() == 0
    try:                                                         # no key at all: engines of gpu_init serve the expansion
        eoc.gpu_init(p, devices=[0])
        one = eoc.seeded_expand(SEED, bodies, first)
        eoc.gpu_shutdown()
        eoc.gpu_init(p, devices=[0, 0])
        two = eoc.seeded_expand(SEED, bodies, first)
        per = [L.eoc_engine_seed_launches(L.eoc_global_engine_at(i)) for i in range(2)]
    finally:
        eoc.gpu_shutdown()
    assert np.array_equal(one, want) and np.array_equal(two, want) and per == [1, 1]
