"""Packing key switch on the MI355X: eoc_pack_device against the chunked reference (tests/c/pack_ref.c through
tests/pack_oracle.py) byte for byte, the workspace budget's slicing in a fresh process, the round trips gate outputs -> lists
-> decryption, lists -> expansion -> NAND and packed LUT outputs as the table of an encrypted-index read, the global context on
one and two engines and in key mode 2, errors and counters.  Host side: tests/test_pack_cpu.py."""
import os
import subprocess
import sys
import json
import textwrap

import numpy as np
import pytest

import cmux_oracle as cx
import compact_oracle as co
import lut_oracle as lo
import oracle_lib as ol
import pack_oracle as po
from gpu_util import dev_empty, sync, to_dev, torch_cuda

pytestmark = pytest.mark.gpu
N = 1024
EOC_ERR_ARG, EOC_ERR_NO_KEY = -1, -4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def eoc(built_lib):
    torch_cuda()
    import eoc_tfhe_amd
    return eoc_tfhe_amd


_KEYS = {}


def keys(eoc, pset, seed=1):
    """params, secret key (Set A: with the cloud key), packing-key blob, its reference spectra, engine with the keys"""
    if (pset, seed) not in _KEYS:
        p = eoc.default_params(pset)
        sk = eoc.SecretKey(p, seed, with_cloud_key=(pset == 0))
        blob = sk.packing_key_bytes()
        eng = eoc.Engine(p)
        if pset == 0:
            eng.load_cloud_key(sk)
        eng.load_packing_key(blob)
        _KEYS[(pset, seed)] = (p, sk, blob, po.key_fft(po.blob_rows(blob, p.n)), eng)
    return _KEYS[(pset, seed)]


def pack_device(eng, cts):
    torch = torch_cuda()
    cts = np.ascontiguousarray(cts, np.int32)
    d_in = to_dev(cts)
    d_out = dev_empty((-(-cts.shape[0] // N), 2, N), torch.int32)
    eng.pack_device(d_in.data_ptr(), cts.shape[0], d_out.data_ptr())
    sync()
    return d_out.cpu().numpy()


@pytest.mark.parametrize("pset,count", [(0, 1), (0, N), (0, N + 3), (1, 1), (1, N + 3)])
def test_pack_equals_the_reference(eoc, pset, count):
    """one slot, a full list, two lists with a ragged last one; n = 500 and n = 630 both end in a short chunk"""
    p, sk, _, kfft, eng = keys(eoc, pset)
    bits = np.random.default_rng(100 * pset + count).integers(0, 2, count).astype(np.uint8)
    cts = sk.encrypt_bits(bits, 50 + count)
    before = eng.stats()
    eng.set_profiling(True)
    eng.kernel_times()
    got = pack_device(eng, cts)
    times = eng.kernel_times()
    eng.set_profiling(False)
    after = eng.stats()
    assert np.array_equal(got, po.pack(p.n, kfft, cts)), (pset, count)
    assert np.array_equal(sk.decrypt_list_bits(got, count), bits)
    assert after["pack_launches"] - before["pack_launches"] == 1 and after["packed_samples"] - before["packed_samples"] == count
    assert after["keyswitches"] == before["keyswitches"] and after["bootstraps"] == before["bootstraps"]
    assert times["keyswitch"]["launches"] == 2 and times["prepare"]["launches"] == times["blind_rotate"]["launches"] == 0


def child(body, env=None, timeout=600):
    code = textwrap.dedent("""
        import json, sys, os
        import numpy as np
        sys.path.insert(0, %r)
        sys.path.insert(0, %r)
        import torch
        import eoc_tfhe_amd as eoc
        out = {}
    """ % (ROOT, os.path.join(ROOT, "tests"))) + textwrap.dedent(body) + "\nprint('RESULT' + json.dumps(out))\n"
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=timeout,
                       env=dict(os.environ, **(env or {})))
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT")][-1][len("RESULT"):])


SLICE_BODY = """
    from test_gpu_pack import pack_device
    p = eoc.default_params(0)
    sk = eoc.SecretKey(p, 1, with_cloud_key=False)
    eng = eoc.Engine(p)
    eng.load_packing_key(sk.packing_key_bytes())
    cts = sk.encrypt_bits(np.random.default_rng(7).integers(0, 2, 2 * 1024 + 3), 70)
    np.save(%r, pack_device(eng, cts))
    out['launches'] = eng.stats()['pack_launches']
    out['grows'] = int(eoc.lib().eoc_engine_workspace_grows(eng.h))
"""


def test_workspace_budget_slices_the_lists(eoc, tmp_path):
    """EOC_TFHE_PACK_WS_BYTES (read at engine creation) at one list's columns (n N 4 bytes) and a little: 2 N + 3 samples run
    as three slices of one list, the same words as the unsliced call of this process.  A budget below one list is refused."""
    p, sk, _, _, eng = keys(eoc, 0)
    cts = sk.encrypt_bits(np.random.default_rng(7).integers(0, 2, 2 * N + 3), 70)
    before = eng.stats()["pack_launches"]
    whole = pack_device(eng, cts)
    assert eng.stats()["pack_launches"] - before == 1
    a = str(tmp_path / "sliced.npy")
    sliced = child(SLICE_BODY % a, env={"EOC_TFHE_PACK_WS_BYTES": str(p.n * N * 4 + 100)})
    assert sliced["launches"] == 3 and sliced["grows"] == 1
    assert np.array_equal(np.load(a), whole)
    small = child("""
        p = eoc.default_params(0)
        eng = eoc.Engine(p)
        eng.load_packing_key(eoc.SecretKey(p, 1, with_cloud_key=False).packing_key_bytes())
        x = torch.zeros(1 << 16, dtype=torch.int32, device='cuda')
        out['rc'] = eoc.lib().eoc_pack_device(eng.h, x.data_ptr(), 1, x.data_ptr(), None)
    """, env={"EOC_TFHE_PACK_WS_BYTES": str(p.n * N * 4 - 1)})
    assert small["rc"] == EOC_ERR_ARG


def test_gate_outputs_pack_and_decrypt(eoc):
    torch = torch_cuda()
    p, sk, _, kfft, eng = keys(eoc, 0)
    rng = np.random.default_rng(200)
    count = N + 3
    a, b = (rng.integers(0, 2, count).astype(np.uint8) for _ in range(2))
    d_a, d_b = to_dev(sk.encrypt_bits(a, 201)), to_dev(sk.encrypt_bits(b, 202))
    d_g = dev_empty((count, p.n + 1), torch.int32)
    d_lists = dev_empty((2, 2, N), torch.int32)
    eng.gate_batch_device(ol.OPS["NAND"], d_a.data_ptr(), d_b.data_ptr(), None, d_g.data_ptr(), count)
    eng.pack_device(d_g.data_ptr(), count, d_lists.data_ptr())          # the same (NULL) stream: ordered behind the gates
    sync()
    lists = d_lists.cpu().numpy()
    assert np.array_equal(sk.decrypt_list_bits(lists, count), 1 - (a & b))
    assert np.array_equal(lists, po.pack(p.n, kfft, d_g.cpu().numpy()))


def test_packed_lists_expand_and_feed_a_gate(eoc):
    """pack -> eoc_compact_expand_device -> NAND, against the composition reference pack, numpy slot extraction,
    orc_keyswitch, orc_gate"""
    torch = torch_cuda()
    p, sk, _, kfft, eng = keys(eoc, 0)
    orc = ol.Oracle(0, 1)                                                # with the bootstrapping key
    bits = np.array([1, 0, 1, 1, 0, 0, 1, 0], np.uint8)
    cts = sk.encrypt_bits(bits, 300)
    d_in = to_dev(cts)
    d_lists = dev_empty((1, 2, N), torch.int32)
    d_exp = dev_empty((8, p.n + 1), torch.int32)
    d_out = dev_empty((4, p.n + 1), torch.int32)
    eng.pack_device(d_in.data_ptr(), 8, d_lists.data_ptr())
    eng.compact_expand_device(d_lists.data_ptr(), 8, d_exp.data_ptr())
    eng.gate_batch_device(ol.OPS["NAND"], d_exp[:4].data_ptr(), d_exp[4:].data_ptr(), None, d_out.data_ptr(), 4)
    sync()
    lists_ref = po.pack(p.n, kfft, cts)
    exp_ref = co.expand(orc, lists_ref, np.arange(8))
    assert np.array_equal(d_lists.cpu().numpy(), lists_ref)
    assert np.array_equal(d_exp.cpu().numpy(), exp_ref)
    assert np.array_equal(sk.decrypt_bits(exp_ref), bits)
    got = d_out.cpu().numpy()
    assert np.array_equal(got, orc.gate_batch(ol.OPS["NAND"], exp_ref[:4], exp_ref[4:]))
    assert np.array_equal(sk.decrypt_bits(got), 1 - (bits[:4] & bits[4:]))


def test_packed_lut_outputs_serve_as_the_table_of_an_encrypted_read(eoc):
    """N + 3 lookups at p = 8 -> two packed lists -> the TABLE of eoc_table_read_device at (d, W) = (1, 1) with client
    selectors: the entries read are the lookups' results, bit-exact against pack_ref + the CMux reference + extraction +
    orc_keyswitch on the device's LUT outputs.  An index past the filled slots reads a (0, 0) sample: 0."""
    torch = torch_cuda()
    p, sk, _, kfft, eng = keys(eoc, 0)
    orc = ol.Oracle(0, 1, with_bk=False)
    rng = np.random.default_rng(400)
    count, depth = N + 3, 11
    f = lambda m: (3 * m + 1) % 8
    vals = rng.integers(0, 8, count).astype(np.uint8)
    tv = eoc.lut_test_polynomial(8, lo.int_table(f, 8, 8))
    d_tv, d_x = to_dev(tv), to_dev(sk.encrypt_ints(vals, 8, 401))
    d_lut = dev_empty((1, count, p.n + 1), torch.int32)
    d_table = dev_empty((2, 2, N), torch.int32)
    eng.lut_batch_device(d_tv.data_ptr(), 1, d_x.data_ptr(), d_lut.data_ptr(), count)
    eng.pack_device(d_lut.data_ptr(), count, d_table.data_ptr())
    sync()
    want = np.array([f(int(m)) for m in vals], np.uint8)
    table = d_table.cpu().numpy()
    assert np.array_equal(sk.decrypt_list_ints(table, 8, count), want)
    assert np.array_equal(table, po.pack(p.n, kfft, d_lut.cpu().numpy()[0]))
    indices = [0, N + 2, int(rng.integers(1, N)), N + 500]
    sel = np.stack([sk.encrypt_index(i, depth, 410, first_idx=k * depth) for k, i in enumerate(indices)])
    d_sel = to_dev(sel)
    d_fft = dev_empty((sel.size,), torch.float64)                        # the converted form takes twice the bytes
    eng.tgsw_to_fft_device(d_sel.data_ptr(), len(indices) * depth, d_fft.data_ptr())
    d_out = dev_empty((len(indices), 1, p.n + 1), torch.int32)
    eng.table_read_device(d_table.data_ptr(), 1, 0, d_fft.data_ptr(), len(indices), d_out.data_ptr())
    sync()
    got = d_out.cpu().numpy()
    assert np.array_equal(sk.decrypt_ints(got[:, 0], 8), np.r_[want[indices[:3]], 0])
    op = cx.orc_params(p)
    tl = np.stack([cx.table_read_tlwe(op, table, 1, 0, cx.to_fft(s)) for s in sel])
    ref = co.expand(orc, tl, np.arange(len(indices)) * N).reshape(len(indices), 1, p.n + 1)
    assert np.array_equal(got, ref)


def test_global_context_one_and_two_engines_and_key_mode_2(eoc, tmp_path):
    p, sk, blob, _, eng = keys(eoc, 0)
    cts = sk.encrypt_bits(np.random.default_rng(500).integers(0, 2, 2 * N + 3), 501)
    ref = pack_device(eng, cts)
    L = eoc.lib()
    try:
        eoc.gpu_shutdown()
        eoc.gpu_init(p, devices=[0])
        lists = np.zeros((3, 2, N), np.int32)
        assert L.eoc_pack(cts.ctypes.data, cts.shape[0], lists.ctypes.data) == EOC_ERR_NO_KEY      # no packing key yet
        eoc.global_import_packing_key_blob(blob)
        one = eoc.pack(cts)
        eoc.gpu_shutdown()
        eoc.gpu_init(p, devices=[0, 0])
        eoc.global_import_packing_key_blob(blob)
        two = eoc.pack(cts)
        per = [int(L.eoc_engine_packed_samples(L.eoc_global_engine_at(i))) for i in range(2)]
    finally:
        eoc.gpu_shutdown()
    assert np.array_equal(one, ref) and np.array_equal(two, ref)
    assert per == [2 * N, 3]                                             # whole lists per engine: 2 + 1
    # a server that holds the cloud key alone (key mode 2) and is given the packing key
    np.save(tmp_path / "cts.npy", cts)
    blob.tofile(tmp_path / "pks.bin")
    server = child("""
        sk = eoc.SecretKey(eoc.default_params(0), 1)
        ck = sk.export_cloud_key()
        del sk
        eoc.global_import_cloud_key_blob(ck)
        out['mode'] = eoc.global_key_mode()
        cts = np.load(%r)
        lists = np.zeros((3, 2, 1024), np.int32)
        out['before'] = eoc.lib().eoc_pack(cts.ctypes.data, cts.shape[0], lists.ctypes.data)
        pks = np.fromfile(%r, np.uint8)
        out['short'] = eoc.lib().eoc_global_import_packing_key_blob(pks.ctypes.data, pks.size - 4)
        eoc.global_import_packing_key_blob(pks)
        np.save(%r, eoc.pack(cts))
        out['export'] = int(eoc.lib().eoc_global_packing_key_export(None, 0))
        out['dec'] = eoc.lib().eoc_global_decrypt_list_bits(lists.ctypes.data, 3, np.zeros(3, np.uint8).ctypes.data)
        eoc.Tfhe.resetGateKey()
    """ % (str(tmp_path / "cts.npy"), str(tmp_path / "pks.bin"), str(tmp_path / "got.npy")))
    assert server == {"mode": 2, "before": EOC_ERR_NO_KEY, "short": EOC_ERR_ARG, "export": 0, "dec": EOC_ERR_NO_KEY}
    assert np.array_equal(np.load(tmp_path / "got.npy"), ref)


def test_errors_the_missing_key_and_key_replacement(eoc):
    torch = torch_cuda()
    L = eoc.lib()
    p, sk, blob, kfft, _ = keys(eoc, 0)
    eng = eoc.Engine(p)
    x = to_dev(sk.encrypt_bits([1, 0, 1], 600))
    o = torch.full((1, 2, N), 7, dtype=torch.int32, device="cuda")
    assert L.eoc_pack_device(eng.h, x.data_ptr(), 3, o.data_ptr(), None) == EOC_ERR_NO_KEY
    assert L.eoc_pack_device(eng.h, x.data_ptr(), 0, o.data_ptr(), None) == EOC_ERR_NO_KEY
    pB = eoc.default_params(1)
    blobB = eoc.SecretKey(pB, 1, with_cloud_key=False).packing_key_bytes()
    bad_t = blob.copy()
    bad_t[44:48] = np.frombuffer(np.int32(2).tobytes(), np.uint8)
    for bad in (blobB, blob[:-4], bad_t, np.zeros(64, np.uint8)):
        assert L.eoc_engine_set_packing_key(eng.h, bad.ctypes.data, bad.size) == EOC_ERR_ARG
    assert L.eoc_engine_set_packing_key(eng.h, None, 0) == EOC_ERR_ARG
    assert L.eoc_pack_device(eng.h, x.data_ptr(), 3, o.data_ptr(), None) == EOC_ERR_NO_KEY      # refused blobs install nothing
    # another secret key's packing key, then this one's: the later image replaces the earlier
    other = eoc.SecretKey(p, 2, with_cloud_key=False).packing_key_bytes()
    eng.load_packing_key(other)
    eng.load_packing_key(blob)
    for bad in ((None, 3, o.data_ptr()), (x.data_ptr(), 3, None)):
        assert L.eoc_pack_device(eng.h, bad[0], bad[1], bad[2], None) == EOC_ERR_ARG
    assert L.eoc_pack_device(eng.h, x.data_ptr(), 0, o.data_ptr(), None) == 0
    sync()
    assert bool((o == 7).all()) and eng.stats()["pack_launches"] == 0          # count 0 touches nothing
    assert L.eoc_pack_device(eng.h, x.data_ptr(), 3, o.data_ptr(), None) == 0
    sync()
    assert np.array_equal(o.cpu().numpy(), po.pack(p.n, kfft, x.cpu().numpy()))
    assert eng.stats()["pack_launches"] == 1 and eng.stats()["packed_samples"] == 3
    eng.close()
