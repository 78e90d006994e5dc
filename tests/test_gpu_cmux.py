"""Leveled operations on the MI355X: eoc_tgsw_to_fft_device against orc_bk_to_fft, eoc_cmux_device against the reference
(tests/c/cmux_ref.c through tests/cmux_oracle.py) and against orc_blind_rotate_step itself, eoc_table_read_device against the
composed reference byte for byte with decryption, the workspace budget's slicing in a fresh process, read outputs as gate and
LUT inputs, the noise of a read against the model, the global context on one and two engines and in key mode 2, errors and
counters.  Host side: tests/test_cmux_cpu.py."""
import ctypes as C
import json
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import cmux_oracle as cx
import compact_oracle as co
import lut_oracle as lo
import oracle_lib as ol
from eoc_tfhe_amd import noise
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
    """params, secret key, public key, oracle (KSK only), engine with the cloud key"""
    if (pset, seed) not in _KEYS:
        p = eoc.default_params(pset)
        sk = eoc.SecretKey(p, seed)
        eng = eoc.Engine(p)
        eng.load_cloud_key(sk)
        _KEYS[(pset, seed)] = (p, sk, eoc.PublicKey(sk.public_key_bytes()), ol.Oracle(pset, seed, with_bk=False), eng)
    return _KEYS[(pset, seed)]


def wrap32(x):
    return ((np.asarray(x, np.int64) + 2**31) % 2**32) - 2**31


def tlwe_phase(tlwe, tlwe_key):
    """phase polynomials c1 - c0 s' of TLWE samples [count][2][N] (int64, wrapped)"""
    t = np.asarray(tlwe, np.int64).reshape(-1, 2, N)
    out = t[:, 1].copy()
    for m in np.flatnonzero(np.asarray(tlwe_key)):
        out -= np.concatenate((-t[:, 0, N - m:], t[:, 0, :N - m]), axis=1)
    return wrap32(out)


def convert(eng, sel):
    """selectors [...][2l][2][N] int32 -> device tensor of their converted form, [count][2l][2][512][2] float64"""
    torch = torch_cuda()
    sel = np.ascontiguousarray(sel, np.int32)
    kpl = sel.shape[-3]
    count = sel.size // (kpl * 2 * N)
    d_sel = to_dev(sel)
    d_fft = dev_empty((count, kpl, 2, N), torch.float64)
    assert d_fft.numel() * 8 == count * eng.tgsw_fft_bytes
    eng.tgsw_to_fft_device(d_sel.data_ptr(), count, d_fft.data_ptr())
    sync()
    return d_fft


def read_device(eng, table, d, lw, sel, n):
    """sel [queries][r + d][2l][2][N] torus form -> [queries][W][n+1]"""
    torch = torch_cuda()
    queries = len(sel)
    d_fft = convert(eng, sel) if np.asarray(sel).size else dev_empty((1,), torch.float64)
    d_tab = to_dev(np.ascontiguousarray(table, np.int32))
    d_out = dev_empty((queries, 1 << lw, n + 1), torch.int32)
    eng.table_read_device(d_tab.data_ptr(), d, lw, d_fft.data_ptr(), queries, d_out.data_ptr())
    sync()
    return d_out.cpu().numpy()


def index_selectors(sk, indices, depth, enc_seed):
    kpl = 2 * sk.params.l
    if depth == 0:
        return np.zeros((len(indices), 0, kpl, 2, N), np.int32)
    return np.stack([sk.encrypt_index(i, depth, enc_seed, first_idx=k * depth) for k, i in enumerate(indices)])


@pytest.mark.parametrize("pset", [0, 1])
def test_conversion_equals_the_oracle_transform(eoc, pset):
    p, sk, _, _, _ = keys(eoc, pset)
    eng = eoc.Engine(p)                                         # no key is required
    sel = sk.encrypt_selector_bits([1, 0, 1], enc_seed=3)
    got = convert(eng, sel).cpu().numpy()
    assert np.array_equal(got, cx.to_fft(sel) * 2.0**-9)        # the image carries 1/512 (exact scaling), as the key's does
    eng.close()


CMUX_SHAPES = [(0, None, None), (1, None, None), (0, 1, 10), (0, 4, 7)]


def shape_setup(eoc, shape):
    pset, l, Bgbit = shape
    p = eoc.default_params(pset)
    if l is not None:
        p.l, p.Bgbit = l, Bgbit
    return p, eoc.SecretKey(p, 21, with_cloud_key=False), eoc.Engine(p)


@pytest.mark.parametrize("shape", CMUX_SHAPES)
def test_cmux_equals_the_reference(eoc, shape):
    """random full-range inputs, an odd count (a partly filled workgroup), bits 0 and 1; gadget lengths 1 and 4 run the
    run-time-base instances.  No key is loaded."""
    torch = torch_cuda()
    p, sk, eng = shape_setup(eoc, shape)
    op = cx.orc_params(p)
    count, bits = 5, [0, 1, 1, 0, 1]
    rng = np.random.default_rng(400 + sum(x or 0 for x in shape))
    sel = sk.encrypt_selector_bits(bits, enc_seed=5)
    in0, in1 = (rng.integers(-2**31, 2**31, (count, 2, N)).astype(np.int32) for _ in range(2))
    d_fft, d0, d1 = convert(eng, sel), to_dev(in0), to_dev(in1)
    d_out = dev_empty((count, 2, N), torch.int32)
    before = eng.stats()["cmux_launches"]
    eng.cmux_device(d_fft.data_ptr(), d0.data_ptr(), d1.data_ptr(), d_out.data_ptr(), count)
    sync()
    got = d_out.cpu().numpy()
    fft = cx.to_fft(sel)
    for k in range(count):
        assert np.array_equal(got[k], cx.cmux(op, fft[k], in0[k], in1[k])), (shape, k)
    assert eng.stats()["cmux_launches"] - before == 1
    # the textbook CMux: the phase of in1 where the bit is 1, of in0 otherwise, up to the external product's noise and mean
    pick = np.where(np.array(bits)[:, None] == 1, tlwe_phase(in1, sk.tlwe_key), tlwe_phase(in0, sk.tlwe_key))
    q = 2.0 ** (-p.l * p.Bgbit)
    lim = (8 * np.sqrt(noise.cmux_var(p, sk.tlwe_key)) + (q / 2) * (1 + int(sk.tlwe_key.sum()))) * 2**32
    assert np.abs(wrap32(tlwe_phase(got, sk.tlwe_key) - pick)).max() < lim
    eng.close()


@pytest.mark.parametrize("pset", [0, 1])
def test_cmux_of_a_rotated_input_is_the_oracle_step(eoc, pset):
    """in1 = X^a in0 prepared in numpy: the item is one blind-rotation step, orc_blind_rotate_step(use_fft = 1) bit for bit"""
    torch = torch_cuda()
    p, sk, _, _, eng = keys(eoc, pset)
    op = cx.orc_params(p)
    amounts = [1, 1023, 1024, 2047, 700]
    rng = np.random.default_rng(410 + pset)
    sel = sk.encrypt_selector_bits([1, 0, 1, 1, 0], enc_seed=6)
    fft = cx.to_fft(sel)
    in0 = rng.integers(-2**31, 2**31, (5, 2, N)).astype(np.int32)
    in1 = np.stack([cx._u32(cx.rotate(in0[k], a)).view(np.int32) for k, a in enumerate(amounts)])
    d_fft, d0, d1 = convert(eng, sel), to_dev(in0), to_dev(in1)
    d_out = dev_empty((5, 2, N), torch.int32)
    eng.cmux_device(d_fft.data_ptr(), d0.data_ptr(), d1.data_ptr(), d_out.data_ptr(), 5)
    sync()
    got = d_out.cpu().numpy()
    for k, a in enumerate(amounts):
        want = in0[k].copy()
        ol.lib().orc_blind_rotate_step(C.byref(op), fft[k].ctypes.data, None, a, want, 1)
        assert np.array_equal(got[k], want), (pset, a)


READ_SHAPES = [(3, 0), (2, 3), (0, 0), (1, 10)]       # (d, log2 W): tree + rotations, rotations only, tree only


def make_table(eoc, pk, kind, d, rng, seed):
    """(table [2^d][2][N], values per slot, decoder)"""
    slots = N << d
    if kind == "bits":
        vals = rng.integers(0, 2, slots).astype(np.uint8)
        return pk.encrypt_bits(vals, enc_seed=seed), vals, None
    vals = rng.integers(0, 4, slots).astype(np.uint8)
    if kind == "trivial":
        return eoc.trivial_table(co.int_msgs(vals, 4)), vals, 4
    return pk.encrypt_ints(vals, 4, enc_seed=seed), vals, 4


@pytest.mark.parametrize("kind", ["trivial", "ints", "bits"])
@pytest.mark.parametrize("shape", READ_SHAPES)
@pytest.mark.parametrize("pset", [0, 1])
def test_table_read_equals_the_composed_reference_and_decrypts(eoc, pset, shape, kind):
    p, sk, pk, orc, eng = keys(eoc, pset)
    op = cx.orc_params(p)
    d, lw = shape
    W, depth = 1 << lw, d + 10 - lw
    rng = np.random.default_rng(500 + 10 * pset + d + lw)
    table, vals, q = make_table(eoc, pk, kind, d, rng, 600 + d)
    assert table.shape == (1 << d, 2, N)
    last = (1 << depth) - 1
    indices = [0, last, int(rng.integers(0, last + 1))]
    sel = index_selectors(sk, indices, depth, enc_seed=700 + pset)
    before = eng.stats()
    got = read_device(eng, table, d, lw, sel, p.n)
    after = eng.stats()
    assert after["keyswitches"] - before["keyswitches"] == 3 * W
    assert after["cmux_launches"] - before["cmux_launches"] == depth
    # decryption: entry idx is slots W idx .. W idx + W - 1 of the table
    for k, idx in enumerate(indices):
        want = vals[W * idx:W * idx + W]
        dec = sk.decrypt_bits(got[k]) if q is None else sk.decrypt_ints(got[k], q)
        assert np.array_equal(dec, want), (shape, kind, idx)
    # byte for byte against the composition (every slot; a sample of the 1 024 at full width)
    fft = [cx.to_fft(s) for s in sel]
    with cx.ThreadPoolExecutor(3) as ex:
        tl = np.stack(list(ex.map(lambda s: cx.table_read_tlwe(op, table, d, lw, s), fft)))
    ws = np.arange(W) if W <= 64 else np.r_[0:8, 500:508, W - 8:W]
    idx = (np.arange(3)[:, None] * N + ws[None, :]).ravel()
    want = co.expand(orc, tl, idx).reshape(3, len(ws), p.n + 1)
    assert np.array_equal(got[:, ws], want), (shape, kind)


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
    from test_gpu_cmux import read_device, index_selectors
    p = eoc.default_params(0)
    sk = eoc.SecretKey(p, 1)
    eng = eoc.Engine(p)
    eng.load_cloud_key(sk)
    rng = np.random.default_rng(800)
    vals = rng.integers(0, 4, 8 * 1024).astype(np.uint8)
    table = eoc.trivial_table((vals.astype(np.int64) << 32) // 8)
    sel = index_selectors(sk, [0, 8191, 4097, 77, 6000], 13, enc_seed=810)
    got = read_device(eng, table, 3, 0, sel, p.n)
    np.save(%r, got)
    out['launches'] = eng.stats()['cmux_launches']
    out['dec'] = sk.decrypt_ints(got.reshape(5, -1), 4).tolist()
    out['want'] = vals[[0, 8191, 4097, 77, 6000]].tolist()
"""


def test_workspace_budget_slices_the_queries(eoc, tmp_path):
    """EOC_TFHE_TABLE_WS_BYTES (read at engine creation) so that 5 queries at d = 3 -- (4 + 2) samples of 8 KiB each -- run as
    slices of 2, 2 and 1: three times the launches, the same words.  A budget below one query's need is refused."""
    a, b = str(tmp_path / "sliced.npy"), str(tmp_path / "whole.npy")
    sliced = child(SLICE_BODY % a, env={"EOC_TFHE_TABLE_WS_BYTES": str(2 * 6 * 8192 + 100)})
    whole = child(SLICE_BODY % b)
    assert sliced["launches"] == 3 * 13 and whole["launches"] == 13
    assert sliced["dec"] == sliced["want"] == whole["dec"]
    assert np.array_equal(np.load(a), np.load(b))
    small = child("""
        p = eoc.default_params(0)
        eng = eoc.Engine(p)
        eng.load_cloud_key(eoc.SecretKey(p, 1))
        x = torch.zeros(1 << 16, dtype=torch.int32, device='cuda')
        out['rc'] = eoc.lib().eoc_table_read_device(eng.h, x.data_ptr(), 3, 0, x.data_ptr(), 1, x.data_ptr(), None)
    """, env={"EOC_TFHE_TABLE_WS_BYTES": str(6 * 8192 - 1)})
    assert small["rc"] == EOC_ERR_ARG


def test_read_outputs_feed_gates_and_table_lookups(eoc):
    torch = torch_cuda()
    p, sk, pk, _, eng = keys(eoc, 0)
    orc = ol.Oracle(0, 1)                                   # with the bootstrapping key
    rng = np.random.default_rng(900)
    d, lw, depth = 1, 2, 9
    bits = rng.integers(0, 2, 2 * N).astype(np.uint8)
    tab_bits = pk.encrypt_bits(bits, enc_seed=910)
    ints = rng.integers(0, 4, 2 * N).astype(np.uint8)
    tab_ints = eoc.trivial_table(co.int_msgs(ints, 4))
    indices = [0, 511, 300]
    sel = index_selectors(sk, indices, depth, enc_seed=920)
    rb = read_device(eng, tab_bits, d, lw, sel, p.n)         # [3][4][n+1]
    ri = read_device(eng, tab_ints, d, lw, sel, p.n)
    a, b = np.ascontiguousarray(rb[:, 0]), np.ascontiguousarray(rb[:, 1])
    d_a, d_b = to_dev(a), to_dev(b)
    d_out = dev_empty((3, p.n + 1), torch.int32)
    eng.gate_batch_device(ol.OPS["NAND"], d_a.data_ptr(), d_b.data_ptr(), None, d_out.data_ptr(), 3)
    sync()
    got = d_out.cpu().numpy()
    want_bits = np.array([1 - (bits[4 * i] & bits[4 * i + 1]) for i in indices])
    assert np.array_equal(sk.decrypt_bits(got), want_bits)
    assert np.array_equal(got, orc.gate_batch(ol.OPS["NAND"], a, b))
    # a lookup of a read int: m -> 3 - m at p = 4
    tv = eoc.lut_test_polynomial(4, lo.int_table(lambda m: 3 - m, 4, 4))
    x = np.ascontiguousarray(ri[:, 2])
    d_tv, d_x = to_dev(tv), to_dev(x)
    d_o = dev_empty((1, 3, p.n + 1), torch.int32)
    eng.lut_batch_device(d_tv.data_ptr(), 1, d_x.data_ptr(), d_o.data_ptr(), 3)
    sync()
    got = d_o.cpu().numpy()
    assert np.array_equal(sk.decrypt_ints(got[0], 4), np.array([3 - ints[4 * i + 2] for i in indices]))
    assert np.array_equal(got, lo.lut_batch(orc, tv, x))


@pytest.mark.parametrize("pset", [0, 1])
def test_noise_of_a_read_matches_the_model(eoc, pset):
    """d = 3, W = 16 (depth 9), 1 024 queries: 16 384 samples.  The output variance is within 8 % of table_read_var.  The mean:
    a CMux whose bit is 1 leaves the truncating decomposition's -(q/2) J(1 - s') at the slot the entry occupies behind it
    (noise.cmux_mean; measured on the CPU reference in tests/test_cmux_cpu.py), a term that depends on the public index and the
    key only; with it removed sample by sample (noise.table_read_mean) the mean is within 4 standard errors of the key switch's
    ks_mean.  The raw figures are printed.  Measured (MI355X, key 1): variance 1.044 (Set A) / 1.020 (Set B) of the model, 1.004
    / 1.010 with the index term removed; mean -0.35 / -1.09 standard errors from ks_mean with it removed, -18.3 / -7.8 raw."""
    torch = torch_cuda()
    p, sk, _, _, eng = keys(eoc, pset)
    d, lw, depth, queries, W = 3, 4, 9, 1024, 16
    rng = np.random.default_rng(1000 + pset)
    vals = rng.integers(0, 2, 8 * N).astype(np.uint8)
    table = eoc.trivial_table(co.bit_msgs(vals))
    indices = rng.integers(0, 1 << depth, queries)
    bits = ((indices[:, None] >> np.arange(depth)[None, :]) & 1).astype(np.uint8)
    sel_ints = eoc.lib().eoc_tgsw_len(C.byref(p))
    d_fft = dev_empty((queries * depth, sel_ints), torch.float64)
    step = 64 * depth                                          # converted in blocks: the torus form never sits whole on the device
    for s0 in range(0, queries * depth, step):
        blk = sk.encrypt_selector_bits(bits.ravel()[s0:s0 + step], enc_seed=1100 + pset, first_idx=s0)
        d_blk = to_dev(blk)
        eng.tgsw_to_fft_device(d_blk.data_ptr(), len(blk), d_fft[s0:].data_ptr())
        sync()
    d_tab = to_dev(table)
    d_out = dev_empty((queries, W, p.n + 1), torch.int32)
    eng.table_read_device(d_tab.data_ptr(), d, lw, d_fft.data_ptr(), queries, d_out.data_ptr())
    sync()
    out = d_out.cpu().numpy().astype(np.int64).reshape(queries * W, p.n + 1)
    ph = wrap32(out[:, -1] - out[:, :-1] @ sk.lwe_key.astype(np.int64))
    slots = (indices[:, None] * W + np.arange(W)[None, :]).ravel()
    assert np.array_equal((ph > 0).astype(np.uint8), vals[slots])
    err = (ph - co.bit_msgs(vals[slots])) / 2.0**32
    cond = np.array([[noise.table_read_mean(p, sk.tlwe_key, i, d, lw, w) for w in range(W)] for i in indices]).ravel()
    pred = noise.predict(p, sk.lwe_key, sk.tlwe_key, sk.ksk)
    var = noise.table_read_var(p, sk.lwe_key, sk.tlwe_key, depth, 0.0, sk.ksk)
    res = err - cond
    z = (res.mean() - pred["ks_mean"]) / (res.std() / np.sqrt(len(res)))
    z_raw = (err.mean() - pred["ks_mean"]) / (err.std() / np.sqrt(len(err)))
    print(f"pset {pset}: var {err.var():.4e} model {var:.4e} ratio {err.var() / var:.4f} (index term removed: "
          f"{res.var() / var:.4f}); mean {err.mean():.3e}, index term {cond.mean():.3e}, ks_mean {pred['ks_mean']:.3e}: "
          f"z {z:.2f} (raw {z_raw:.2f})")
    assert abs(err.var() / var - 1) < 0.08
    assert abs(res.var() / var - 1) < 0.08
    assert abs(z) < 4


def test_global_context_one_and_two_engines_and_key_mode_2(eoc, tmp_path):
    p, sk, pk, _, eng = keys(eoc, 0)
    d, lw, depth = 2, 1, 11
    rng = np.random.default_rng(1200)
    vals = rng.integers(0, 4, 4 * N).astype(np.uint8)
    table = pk.encrypt_ints(vals, 4, enc_seed=1210)
    indices = [0, 2047, 1234]
    sel = index_selectors(sk, indices, depth, enc_seed=1220)
    ref = read_device(eng, table, d, lw, sel, p.n)
    try:
        eoc.gpu_shutdown()
        eoc.gpu_init(p, devices=[0])
        eoc.upload_cloud_key(sk)
        one = eoc.table_read(table, d, lw, sel)
        eoc.gpu_shutdown()
        eoc.gpu_init(p, devices=[0, 0])
        eoc.upload_cloud_key(sk)
        two = eoc.table_read(table, d, lw, sel)
        per = [e["keyswitches"] for e in eoc.stats_multi()["engines"]]
    finally:
        eoc.gpu_shutdown()
    assert np.array_equal(one, ref) and np.array_equal(two, ref)
    assert per == [4, 2]
    assert np.array_equal(sk.decrypt_ints(ref.reshape(-1, p.n + 1), 4).reshape(3, 2),
                          np.array([vals[2 * i:2 * i + 2] for i in indices]))
    # a server that holds the cloud key alone (key mode 2)
    np.save(tmp_path / "table.npy", table)
    np.save(tmp_path / "sel.npy", sel)
    server = child("""
        sk = eoc.SecretKey(eoc.default_params(0), 1)
        blob = sk.export_cloud_key()
        del sk
        eoc.global_import_cloud_key_blob(blob)
        out['mode'] = eoc.global_key_mode()
        np.save(%r, eoc.table_read(np.load(%r), 2, 1, np.load(%r)))
        bits = np.ones(1, np.uint8)
        o = np.zeros(eoc.lib().eoc_tgsw_len(eoc.global_params()), np.int32)
        out['enc'] = eoc.lib().eoc_global_tgsw_encrypt_bits(bits.ctypes.data, 1, o.ctypes.data)
        eoc.Tfhe.resetGateKey()
    """ % (str(tmp_path / "got.npy"), str(tmp_path / "table.npy"), str(tmp_path / "sel.npy")))
    assert server == {"mode": 2, "enc": EOC_ERR_NO_KEY}
    assert np.array_equal(np.load(tmp_path / "got.npy"), ref)


def test_errors_and_the_missing_key(eoc):
    torch = torch_cuda()
    L = eoc.lib()
    p = eoc.default_params(0)
    sk = eoc.SecretKey(p, 31, with_cloud_key=False)
    eng = eoc.Engine(p)
    sel = sk.encrypt_selector_bits([1], enc_seed=1)
    d_fft = convert(eng, sel)                                               # works without a key
    x = to_dev(np.random.default_rng(1).integers(-2**31, 2**31, (2, 2, N)).astype(np.int32))
    o = dev_empty((1, 2, N), torch.int32)
    assert L.eoc_cmux_device(eng.h, d_fft.data_ptr(), x[0].data_ptr(), x[1].data_ptr(), o.data_ptr(), 1, None) == 0
    sync()
    out = dev_empty((2, p.n + 1), torch.int32)
    args = (x.data_ptr(), 0, 9, d_fft.data_ptr(), 1, out.data_ptr(), None)
    assert L.eoc_table_read_device(eng.h, *args) == EOC_ERR_NO_KEY
    for bad in ((None,) + args[1:], args[:3] + (None,) + args[4:], args[:5] + (None, None),
                (args[0], 13) + args[2:], (args[0], -1) + args[2:], args[:2] + (11,) + args[3:], args[:2] + (-1,) + args[3:]):
        assert L.eoc_table_read_device(eng.h, *bad) == EOC_ERR_ARG, bad
    assert L.eoc_cmux_device(eng.h, None, x.data_ptr(), x.data_ptr(), o.data_ptr(), 1, None) == EOC_ERR_ARG
    assert L.eoc_cmux_device(eng.h, d_fft.data_ptr(), x.data_ptr(), x.data_ptr(), None, 1, None) == EOC_ERR_ARG
    assert L.eoc_cmux_device(eng.h, d_fft.data_ptr(), x.data_ptr(), x.data_ptr(), o.data_ptr(), 0, None) == 0
    assert L.eoc_tgsw_to_fft_device(eng.h, None, 1, d_fft.data_ptr(), None) == EOC_ERR_ARG
    assert eng.stats()["cmux_launches"] == 1 and eng.stats()["keyswitches"] == 0
    eng.close()
