"""Encrypted-index table updates on the MI355X: eoc_table_update_device against the composed reference
(tests/table_update_oracle.py) word for word on a random full-range table with guard words behind it, at the smallest shapes
that take different paths, on both sets and on two run-time-base gadget lengths; the workspace budget's slicing; the round trips
through eoc_table_read_device, the packing key switch and a gate; the global context on one and two engines and in key mode 2.
Host side: tests/test_table_update_cpu.py; the kernel instances one by one: tests/test_gpu_demux_instances.py."""
import numpy as np
import pytest

import cmux_oracle as cx
import compact_oracle as co
import lut_oracle as lo
import oracle_lib as ol
import table_update_oracle as tu
from gpu_util import dev_empty, sync, to_dev, torch_cuda
from test_gpu_cmux import child, convert, index_selectors, keys, read_device

pytestmark = pytest.mark.gpu
N = 1024
EOC_ERR_ARG = -1
GUARD = 0x6B6B6B6B
# (d, log2 W): pure add with NULL selectors | one rotation, no tree | the accumulating stage alone | a storing stage and the
# accumulating one | ten rotations, three stages, the ping-pong wrapping
SHAPES = [(0, 10), (0, 9), (1, 10), (2, 8), (3, 0)]


@pytest.fixture(scope="module")
def eoc(built_lib):
    torch_cuda()
    import eoc_tfhe_amd
    return eoc_tfhe_amd


def update_device(eng, table, d, lw, sel, values, offset_ints=0):
    """table [2^d][2][N], sel [queries][r + d][2l][2][N] torus form, values [queries][2][N] -> the updated table; one guard
    sample behind the table must keep its fill.  offset_ints shifts the values off their 16-byte alignment."""
    torch = torch_cuda()
    queries = len(values)
    d_fft = convert(eng, sel) if np.asarray(sel).size else None
    buf = torch.full(((1 << d) + 1, 2, N), GUARD, dtype=torch.int32, device="cuda")
    buf[:1 << d] = to_dev(np.ascontiguousarray(table, np.int32))
    flat = torch.zeros(values.size + offset_ints, dtype=torch.int32, device="cuda")
    flat[offset_ints:] = to_dev(np.ascontiguousarray(values, np.int32)).ravel()
    d_vals = flat[offset_ints:]
    eng.table_update_device(buf.data_ptr(), d, lw, d_fft.data_ptr() if d_fft is not None else None, d_vals.data_ptr(), queries)
    sync()
    out = buf.cpu().numpy()
    assert (out[1 << d] == GUARD).all()
    return out[:1 << d]


def run_shape(eoc, p, sk, eng, d, lw, seed, counts=(1, 3, 5)):
    """queries 1, 3 and 5 (prefixes of five, two of them on one index) against the reference; counters per call"""
    op = cx.orc_params(p)
    depth, r = d + 10 - lw, 10 - lw
    rng = np.random.default_rng(seed)
    table = rng.integers(-2**31, 2**31, (1 << d, 2, N)).astype(np.int32)
    last = (1 << depth) - 1
    indices = [last, 0, last, last // 2 + 1 if depth else 0, int(rng.integers(0, last + 1))]
    sel = index_selectors(sk, indices, depth, enc_seed=seed + 1)
    values = rng.integers(-2**31, 2**31, (5, 2, N)).astype(np.int32)
    fft = [cx.to_fft(s) if depth else None for s in sel]
    with cx.ThreadPoolExecutor(5) as ex:
        lv = np.stack(list(ex.map(lambda q: tu.leaves(op, d, lw, fft[q], values[q]), range(5)))).astype(np.int64)
    for count in counts:
        before = eng.stats()
        got = update_device(eng, table, d, lw, sel[:count], values[:count])
        after = eng.stats()
        want = tu.wrap_i32(table.astype(np.int64) + lv[:count].sum(0))
        assert np.array_equal(got, want), ((d, lw), count, np.argwhere(got != want)[:6].tolist())
        assert after["demux_launches"] - before["demux_launches"] == d
        assert after["cmux_launches"] - before["cmux_launches"] == r
        assert after["keyswitches"] == before["keyswitches"] and after["bootstraps"] == before["bootstraps"]
    return table, sel, values, want


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("pset", [0, 1])
def test_update_equals_the_composed_reference(eoc, pset, shape):
    p, sk, _, _, eng = keys(eoc, pset)
    d, lw = shape
    table, sel, values, want = run_shape(eoc, p, sk, eng, d, lw, 2000 + 100 * pset + 10 * d + lw)
    if shape == (0, 10):                                        # values off their 16-byte alignment: the word form of the add
        got = update_device(eng, table, d, lw, sel, values, offset_ints=1)
        assert np.array_equal(got, want)
        assert np.array_equal(want, tu.wrap_i32(table.astype(np.int64) + values.astype(np.int64).sum(0)))


@pytest.mark.parametrize("l,Bgbit", [(1, 10), (4, 7)])
def test_update_on_run_time_base_gadgets(eoc, l, Bgbit):
    """k_demux<1,0> and <4,0> behind the table call, at (1, 10): no key is loaded"""
    p = eoc.default_params(0)
    p.l, p.Bgbit = l, Bgbit
    sk = eoc.SecretKey(p, 21, with_cloud_key=False)
    eng = eoc.Engine(p)
    run_shape(eoc, p, sk, eng, 1, 10, 2500 + l, counts=(3,))
    eng.close()


def test_workspace_budget_slices_the_queries(eoc, monkeypatch):
    """EOC_TFHE_TABLE_WS_BYTES (read at engine creation) so that 5 queries at d = 3 -- (4 + 2) samples of 8 KiB each -- run as
    slices of 2, 2 and 1: three times the launches, the same words.  A budget below one query's need is refused."""
    torch = torch_cuda()
    p, sk, _, _, whole_eng = keys(eoc, 0)
    d, lw, r = 3, 8, 2
    rng = np.random.default_rng(2600)
    table = rng.integers(-2**31, 2**31, (1 << d, 2, N)).astype(np.int32)
    sel = index_selectors(sk, [31, 0, 31, 17, 6], d + r, enc_seed=2601)
    values = rng.integers(-2**31, 2**31, (5, 2, N)).astype(np.int32)
    whole = update_device(whole_eng, table, d, lw, sel, values)
    monkeypatch.setenv("EOC_TFHE_TABLE_WS_BYTES", str(2 * 6 * 8192 + 100))
    eng = eoc.Engine(p)
    sliced = update_device(eng, table, d, lw, sel, values)
    st = eng.stats()
    eng.close()
    assert st["demux_launches"] == 3 * d and st["cmux_launches"] == 3 * r
    assert np.array_equal(sliced, whole)
    monkeypatch.setenv("EOC_TFHE_TABLE_WS_BYTES", str(6 * 8192 - 1))
    eng = eoc.Engine(p)
    x = torch.zeros(1 << 16, dtype=torch.int32, device="cuda")
    rc = eoc.lib().eoc_table_update_device(eng.h, x.data_ptr(), 3, 0, x.data_ptr(), x.data_ptr(), 1, None)
    eng.close()
    assert rc == EOC_ERR_ARG


def test_errors_need_no_key(eoc):
    torch = torch_cuda()
    L = eoc.lib()
    p = eoc.default_params(0)
    eng = eoc.Engine(p)
    x = torch.zeros(1 << 16, dtype=torch.int32, device="cuda")
    args = (x.data_ptr(), 0, 9, x.data_ptr(), x.data_ptr(), 1, None)
    for bad in ((None,) + args[1:], args[:3] + (None,) + args[4:], args[:4] + (None,) + args[5:],
                (args[0], 13) + args[2:], (args[0], -1) + args[2:], args[:2] + (11,) + args[3:], args[:2] + (-1,) + args[3:]):
        assert L.eoc_table_update_device(eng.h, *bad) == EOC_ERR_ARG, bad
    assert L.eoc_table_update_device(eng.h, *args[:5], 0, None) == 0                       # no query: a no-op
    assert L.eoc_demux_device(eng.h, None, x.data_ptr(), x.data_ptr(), x.data_ptr(), 1, 0, None) == EOC_ERR_ARG
    assert L.eoc_demux_device(eng.h, x.data_ptr(), x.data_ptr(), x.data_ptr(), None, 1, 0, None) == EOC_ERR_ARG
    assert L.eoc_demux_device(eng.h, x.data_ptr(), x.data_ptr(), x.data_ptr(), x.data_ptr(), 0, 0, None) == 0
    sync()
    assert eng.stats()["demux_launches"] == 0 and eng.stats()["cmux_launches"] == 0 and not x.any().item()
    eng.close()


def test_update_then_read_decrypts_old_plus_value(eoc):
    """the same selectors serve the update and the read; values come as a trivial sample and as a public-key list"""
    p, sk, pk, _, eng = keys(eoc, 0)
    d, lw, depth, W = 1, 2, 9, 4
    rng = np.random.default_rng(2700)
    old = rng.integers(0, 4, 2 * N).astype(np.uint8)
    table = eoc.trivial_table(co.int_msgs(old, 8))
    indices = [0, 511, 300, 300]
    sel = index_selectors(sk, indices, depth, enc_seed=2710)
    add = rng.integers(0, 2, (len(indices), W)).astype(np.uint8)
    values = np.stack([eoc.trivial_table(co.int_msgs(add[0], 8))[0], eoc.trivial_table(co.int_msgs(add[1], 8))[0],
                       pk.encrypt_ints(add[2], 8, enc_seed=2720)[0], pk.encrypt_ints(add[3], 8, enc_seed=2721)[0]])
    new = update_device(eng, table, d, lw, sel, values)
    want = old.astype(np.int64).copy()
    for k, i in enumerate(indices):
        want[W * i:W * i + W] += add[k]
    assert np.array_equal(sk.decrypt_list_ints(new, 8), want)                # every slot of the table
    got = read_device(eng, new, d, lw, sel, p.n)
    dec = sk.decrypt_ints(got.reshape(-1, p.n + 1), 8).reshape(len(indices), W)
    assert np.array_equal(dec, np.stack([want[W * i:W * i + W] for i in indices]))


def test_lut_outputs_packed_into_an_update_and_a_read_into_a_gate(eoc):
    """p = 4 LUT outputs -> eoc_pack_device of W samples -> update -> read -> decrypt; then a bit table: the update sets a
    bit, and the read outputs feed a NAND bit for bit against the oracle"""
    torch = torch_cuda()
    p, sk, pk, _, eng = keys(eoc, 0)
    orc = ol.Oracle(0, 1)                                       # with the bootstrapping key
    eng.load_packing_key(sk.packing_key_bytes())
    d, lw, depth, W = 1, 2, 9, 4
    rng = np.random.default_rng(2800)
    old = rng.integers(0, 2, 2 * N).astype(np.uint8)            # old + f(m) <= 3 stays inside Z_4
    table = eoc.trivial_table(co.int_msgs(old, 4))
    m = rng.integers(0, 4, W).astype(np.uint8)
    tv = eoc.lut_test_polynomial(4, lo.int_table(lambda v: v % 3, 4, 4))
    d_tv, d_x = to_dev(tv), to_dev(sk.encrypt_ints(m, 4, enc_seed=2810))
    d_o = dev_empty((1, W, p.n + 1), torch.int32)
    eng.lut_batch_device(d_tv.data_ptr(), 1, d_x.data_ptr(), d_o.data_ptr(), W)
    d_list = dev_empty((1, 2, N), torch.int32)
    eng.pack_device(d_o.data_ptr(), W, d_list.data_ptr())
    sync()
    value = d_list.cpu().numpy()
    idx = 421
    sel = index_selectors(sk, [idx], depth, enc_seed=2820)
    new = update_device(eng, table, d, lw, sel, value)
    want = old.astype(np.int64).copy()
    want[W * idx:W * idx + W] += m % 3
    assert np.array_equal(sk.decrypt_list_ints(new, 4), want)
    got = read_device(eng, new, d, lw, sel, p.n)
    assert np.array_equal(sk.decrypt_ints(got[0], 4), want[W * idx:W * idx + W])
    # bits: -1/8 is 0 and +1/8 is 1, so adding 1/4 sets a bit that was 0
    bits = rng.integers(0, 2, 2 * N).astype(np.uint8)
    tab_bits = pk.encrypt_bits(bits, enc_seed=2830)
    indices = [0, 511, 300]
    bsel = index_selectors(sk, indices, depth, enc_seed=2840)
    quarter = np.zeros((len(indices), N), np.int64)
    quarter[:, 0] = [(1 - int(bits[W * i])) << 30 for i in indices]
    assert quarter[0, 0] == 1 << 30                             # entry 0 holds a 0 in its first slot: that bit is set
    bvals = np.stack([eoc.trivial_table(q)[0] for q in quarter])
    new_bits = update_device(eng, tab_bits, d, lw, bsel, bvals)
    rb = read_device(eng, new_bits, d, lw, bsel, p.n)            # [3][4][n+1]
    a, b = np.ascontiguousarray(rb[:, 0]), np.ascontiguousarray(rb[:, 1])
    assert np.array_equal(sk.decrypt_bits(a), np.ones(3, np.uint8))
    d_a, d_b = to_dev(a), to_dev(b)
    d_out = dev_empty((3, p.n + 1), torch.int32)
    eng.gate_batch_device(ol.OPS["NAND"], d_a.data_ptr(), d_b.data_ptr(), None, d_out.data_ptr(), 3)
    sync()
    out = d_out.cpu().numpy()
    assert np.array_equal(sk.decrypt_bits(out), np.array([1 - bits[W * i + 1] for i in indices]))
    assert np.array_equal(out, orc.gate_batch(ol.OPS["NAND"], a, b))


def test_global_context_one_and_two_engines_and_key_mode_2(eoc, tmp_path):
    p, sk, pk, _, eng = keys(eoc, 0)
    d, lw, depth = 2, 8, 4
    rng = np.random.default_rng(2900)
    table = rng.integers(-2**31, 2**31, (1 << d, 2, N)).astype(np.int32)
    sel = index_selectors(sk, [15, 0, 15], depth, enc_seed=2910)
    values = rng.integers(-2**31, 2**31, (3, 2, N)).astype(np.int32)
    ref = update_device(eng, table, d, lw, sel, values)
    before = table.copy()
    try:
        eoc.gpu_shutdown()
        eoc.gpu_init(p, devices=[0])
        eoc.upload_cloud_key(sk)
        one = eoc.table_update(table, d, lw, sel, values)
        eoc.gpu_shutdown()
        eoc.gpu_init(p, devices=[0, 0])
        eoc.upload_cloud_key(sk)
        two = eoc.table_update(table, d, lw, sel, values)
    finally:
        eoc.gpu_shutdown()
    assert np.array_equal(table, before)                        # the wrapper returns a new table
    assert np.array_equal(one, ref) and np.array_equal(two, ref)
    np.save(tmp_path / "table.npy", table)
    np.save(tmp_path / "sel.npy", sel)
    np.save(tmp_path / "values.npy", values)
    server = child("""
        sk = eoc.SecretKey(eoc.default_params(0), 1)
        blob = sk.export_cloud_key()
        del sk
        eoc.global_import_cloud_key_blob(blob)
        out['mode'] = eoc.global_key_mode()
        np.save(%r, eoc.table_update(np.load(%r), 2, 8, np.load(%r), np.load(%r)))
        eoc.Tfhe.resetGateKey()
    """ % (str(tmp_path / "got.npy"), str(tmp_path / "table.npy"), str(tmp_path / "sel.npy"), str(tmp_path / "values.npy")))
    assert server == {"mode": 2}
    assert np.array_equal(np.load(tmp_path / "got.npy"), ref)
