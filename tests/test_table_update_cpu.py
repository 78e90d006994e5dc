"""Encrypted-index table updates, host side (no GPU): the new symbols and their argument errors, the composed
reference (tests/table_update_oracle.py) decoded slot by slot, its order independence, the plain sum at d = r = 0, the
demultiplexer's external product against the exact schoolbook product, the noise model of one update against the reference,
and the updates-before-refresh helper.  Device side: tests/test_gpu_demux_instances.py, tests/test_gpu_table_update.py."""
import ctypes as C

import numpy as np
import pytest

import cmux_oracle as cx
import compact_oracle as co
import table_update_oracle as tu
from eoc_tfhe_amd import noise
from test_cmux_cpu import SHAPES, shape_params, tlwe_phase, wrap32

N = 1024
EOC_ERR_ARG = -1
NAMED = [0, 1, 255, 256, 512, 1022, 1023]


@pytest.fixture(scope="module")
def eoc(built_lib):
    import eoc_tfhe_amd
    return eoc_tfhe_amd


def test_symbols_and_argument_errors(eoc):
    L = eoc.lib()
    new = {"eoc_demux_device", "eoc_table_update_device", "eoc_engine_demux_launches", "eoc_table_update"}
    assert new <= set(eoc.abi_symbols()) and all(hasattr(L, s) for s in new)
    assert all(hasattr(eoc.Engine, m) for m in ("demux_device", "table_update_device")) and callable(eoc.table_update)
    # device entry points: a null engine / null pointers are refused before anything touches a device
    assert L.eoc_demux_device(None, 1, 1, 1, 1, 1, 0, None) == EOC_ERR_ARG
    assert L.eoc_table_update_device(None, 1, 0, 0, 1, 1, 1, None) == EOC_ERR_ARG
    assert L.eoc_engine_demux_launches(None) == 0
    # the global update checks its shape before it looks for a key or a device: the read's ranges, the read's code
    x = np.zeros(8, np.int32)
    for d, lw in ((13, 0), (-1, 0), (0, 11), (0, -1)):
        assert L.eoc_table_update(x.ctypes.data, d, lw, x.ctypes.data, x.ctypes.data, 1) == EOC_ERR_ARG, (d, lw)
    assert L.eoc_table_update(None, 0, 0, x.ctypes.data, x.ctypes.data, 1) == EOC_ERR_ARG
    assert L.eoc_table_update(x.ctypes.data, 0, 0, x.ctypes.data, None, 1) == EOC_ERR_ARG
    assert L.eoc_table_update(x.ctypes.data, 0, 0, None, x.ctypes.data, 1) == EOC_ERR_ARG      # selectors needed: depth 10
    assert L.eoc_table_update(x.ctypes.data, 0, 0, x.ctypes.data, x.ctypes.data, 0) == 0 and not x.any()   # no query: a no-op
    tab, val = np.zeros((2, 2, N), np.int32), np.zeros((1, 2, N), np.int32)
    with pytest.raises(eoc.EocError, match="table must be"):
        eoc.table_update(tab, 2, 0, np.zeros((1, 12, 4, 2, N), np.int32), val)
    with pytest.raises(eoc.EocError, match="log2_width"):
        eoc.table_update(tab, 1, 11, np.zeros((1, 0, 4, 2, N), np.int32), val)
    with pytest.raises(eoc.EocError, match="selectors must be"):
        eoc.table_update(tab, 1, 10, np.zeros((1, 2, 4, 2, N), np.int32), val)
    with pytest.raises(eoc.EocError, match="values must be"):
        eoc.table_update(tab, 1, 10, np.zeros((1, 1, 4, 2, N), np.int32), val[0])


def test_hot_path_fails_loudly_without_gpu(eoc):
    """no CPU fallback: without a device the update errors out as every other hot-path call does, and leaves the table alone"""
    if eoc.lib().eoc_device_count() > 0:
        return                                                               # tests/test_gpu_table_update.py runs it there
    p = eoc.default_params(0)
    with pytest.raises(eoc.EocError, match="no usable HIP device"):
        eoc.Engine(p)
    tab = np.arange(2 * N, dtype=np.int32).reshape(1, 2, N)
    x = tab.copy()
    rc = eoc.lib().eoc_table_update(x.ctypes.data, 0, 10, None, tab.ctypes.data, 1)
    assert rc != 0 and np.array_equal(x, tab)
    with pytest.raises(eoc.EocError):
        eoc.table_update(tab, 0, 10, None, tab)


def selectors_of(both, indices, depth):
    """both [depth][2][2l][2][N]: one converted selector per (bit position, bit value); index idx uses [k][idx >> k & 1]"""
    return [np.stack([both[k, (i >> k) & 1] for k in range(depth)]) for i in indices]


@pytest.mark.parametrize("pset", [0, 1])
def test_composed_update_on_the_cpu_decodes_every_slot_of_every_leaf(eoc, pset):
    """d = 2, W = 4, 64 indices (the ends of the slot range, of a list and of the table among them), trivial p = 8 values:
    the selected leaf carries the value at slots W (idx mod 2^r) .. + W - 1, every other slot of every leaf decodes to 0"""
    d, lw = 2, 2
    W, r, depth = 1 << lw, 10 - lw, d + 10 - lw
    p = eoc.default_params(pset)
    sk = eoc.SecretKey(p, 21 + pset, with_cloud_key=False)
    op = cx.orc_params(p)
    rng = np.random.default_rng(400 + pset)
    rest = rng.choice(np.setdiff1d(np.arange(1 << depth), NAMED), 64 - len(NAMED), replace=False)
    indices = NAMED + [int(i) for i in rest]
    both = cx.to_fft(sk.encrypt_selector_bits([0, 1] * depth, enc_seed=31 + pset)).reshape(depth, 2, 2 * p.l, 2, N)
    sels = selectors_of(both, indices, depth)
    vals = rng.integers(1, 8, (len(indices), W))
    sel_var, sel_max = [], 0.0
    for q, idx in enumerate(indices):
        value = eoc.trivial_table(co.int_msgs(vals[q], 8))[0]
        lv = tu.leaves(op, d, lw, sels[q], value)
        assert lv.shape == (1 << d, 2, N)
        want = np.zeros((1 << d, N), np.int64)
        s = W * (idx & ((1 << r) - 1))
        want[idx >> r, s:s + W] = vals[q]
        got = sk.decrypt_list_ints(lv, 8).reshape(1 << d, N)
        assert np.array_equal(got, want), (pset, idx, np.argwhere(got != want)[:6].tolist())
        err = wrap32(tlwe_phase(lv[idx >> r], sk.tlwe_key)[s:s + W] - co.int_msgs(vals[q], 8)) / 2.0**32
        sel_var.append(err)
        sel_max = max(sel_max, float(np.abs(err).max()))
    print(f"pset {pset}: selected entry over 64 indices: mean {np.mean(sel_var):.3e}, largest |error| {sel_max:.3e}")
    assert sel_max < 1.0 / 32                                                # half a step of the p = 8 grid


def test_updates_commute_and_collide_exactly(eoc):
    """three updates, two of them on one index: the batch in two orders and the three single updates give the same words"""
    d, lw = 1, 9
    depth = d + 10 - lw
    p = eoc.default_params(0)
    sk = eoc.SecretKey(p, 23, with_cloud_key=False)
    op = cx.orc_params(p)
    rng = np.random.default_rng(410)
    table = rng.integers(-2**31, 2**31, (1 << d, 2, N)).astype(np.int32)
    indices = [3, 0, 3]
    sel = np.stack([cx.to_fft(sk.encrypt_index(i, depth, 500, first_idx=k * depth)) for k, i in enumerate(indices)])
    values = rng.integers(-2**31, 2**31, (3, 2, N)).astype(np.int32)
    a = tu.table_update(op, table, d, lw, sel, values)
    order = [2, 0, 1]
    b = tu.table_update(op, table, d, lw, sel[order], values[order])
    c = table
    for q in range(3):
        c = tu.table_update(op, c, d, lw, sel[q:q + 1], values[q:q + 1])
    assert np.array_equal(a, b) and np.array_equal(a, c) and not np.array_equal(a, table)


def test_depth_zero_is_the_plain_wrapping_sum(eoc):
    op = cx.orc_params(eoc.default_params(0))
    rng = np.random.default_rng(411)
    table = rng.integers(-2**31, 2**31, (1, 2, N)).astype(np.int32)
    values = rng.integers(-2**31, 2**31, (3, 2, N)).astype(np.int32)
    got = tu.table_update(op, table, 0, 10, None, values)
    want = wrap32(table.astype(np.int64) + values.astype(np.int64).sum(0)).astype(np.int32)
    assert np.array_equal(got, want)
    assert np.array_equal(tu.table_update(op, table, 0, 10, None, values[:0]), table)


@pytest.mark.parametrize("shape", SHAPES)
def test_demux_product_is_within_8_lsb_of_the_exact_product(eoc, shape):
    """E of the demultiplexer is the CMux's external product on x itself; the two children add up to x exactly"""
    p = shape_params(eoc, shape)
    sk = eoc.SecretKey(p, 26, with_cloud_key=False)
    op = cx.orc_params(p)
    rng = np.random.default_rng(420 + sum(x or 0 for x in shape))
    sel = sk.encrypt_selector_bits([1, 0], enc_seed=12)
    fft = cx.to_fft(sel)
    for k in range(2):
        x = rng.integers(-2**31, 2**31, (2, N)).astype(np.int32)
        c0, c1 = tu.demux(op, fft[k], x)
        assert np.array_equal(c1, cx.cmux(op, fft[k], np.zeros((2, N), np.int32), x))      # in0 = 0, in1 = x, rot = 0
        exact = cx.extprod_exact(p, sel[k], x.astype(np.int64))
        assert np.abs(wrap32(c1.astype(np.int64) - exact)).max() <= 8, shape
        assert np.array_equal(wrap32(c0.astype(np.int64) + c1), x)


NOISE_D, NOISE_LW, NOISE_IDX = 2, 7, 13        # r = 3: rotation bits 1, 0, 1; tree bits 1 (stage 1), 0 (stage 0); list 1
PAIRS, NSLOT = 512, 16


@pytest.mark.parametrize("pset", [0, 1])
def test_update_noise_matches_the_model(eoc, pset):
    """512 independent (selectors, value) pairs of ONE index, random full-range values, 16 fixed slots per list class:
    S = 8 192 samples per class.  The error of a slot is phase(leaf) - phase(X^s value) on the selected list and
    phase(leaf) on the others (message 0).  The model mean (table_update_mean) is removed sample by sample; the variance of
    the residual over table_update_var must lie inside 1 +- 3.5 sqrt(2 / (S - 1)) (3.5 standard errors of a variance
    estimate) and the residual mean within 4 standard errors of 0.  Classes: the selected entry (list 1: x - E under bit 0,
    then E under bit 1, behind three rotations), list 3 (E under bit 0 starts afresh, E under bit 1 adds), list 2 (x - E
    under bit 1: the negated remainder alone) and list 0 (the same behind a stage that kept the value)."""
    d, lw, idx = NOISE_D, NOISE_LW, NOISE_IDX
    r, W, depth = 10 - lw, 1 << lw, NOISE_D + 10 - NOISE_LW
    p = eoc.default_params(pset)
    sk = eoc.SecretKey(p, 27 + pset, with_cloud_key=False)
    op = cx.orc_params(p)
    rng = np.random.default_rng(430 + pset)
    s = W * (idx & ((1 << r) - 1))
    sel_list = idx >> r
    slots = {lst: (s + 8 * np.arange(NSLOT) if lst == sel_list else 64 * np.arange(NSLOT)) for lst in range(1 << d)}
    assert sel_list == 1 and s + 8 * NSLOT <= s + W
    bits = np.array([(idx >> k) & 1 for k in range(depth)] * PAIRS, np.uint8)
    sel = sk.encrypt_selector_bits(bits, enc_seed=440 + pset).reshape(PAIRS, depth, 2 * p.l, 2, N)
    err = {lst: np.zeros((PAIRS, NSLOT)) for lst in slots}
    for k in range(PAIRS):
        value = rng.integers(-2**31, 2**31, (2, N)).astype(np.int32)
        lv = tu.leaves(op, d, lw, cx.to_fft(sel[k]), value)
        ph = tlwe_phase(lv, sk.tlwe_key)
        moved = tlwe_phase(wrap32(cx.rotate(value, s)), sk.tlwe_key)
        for lst, sl in slots.items():
            e = ph[lst, sl] - (moved[sl] if lst == sel_list else 0)
            err[lst][k] = wrap32(e) / 2.0**32
    S = PAIRS * NSLOT
    tol = 3.5 * np.sqrt(2.0 / (S - 1))
    report = []
    for lst, sl in slots.items():
        mean = np.array([noise.table_update_mean(p, sk.tlwe_key, idx, d, lw, slot=int(j), lst=lst) for j in sl])
        model = noise.table_update_var(p, sk.tlwe_key, idx, d, lw, lst=lst)
        res = (err[lst] - mean[None, :]).ravel()
        ratio = res.var(ddof=1) / model
        z = res.mean() / (res.std(ddof=1) / np.sqrt(S))
        report.append((lst, ratio, z))
        print(f"pset {pset} list {lst}{' (selected entry)' if lst == sel_list else ''}: var {res.var(ddof=1):.4e} model "
              f"{model:.4e} ratio {ratio:.4f} (1 +- {tol:.4f}); raw mean {err[lst].mean():.3e} model {mean.mean():.3e} "
              f"residual z {z:.2f}")
    for lst, ratio, z in report:
        assert abs(ratio - 1) < tol, (pset, lst, ratio, tol)
        assert abs(z) < 4, (pset, lst, z)


@pytest.mark.parametrize("pset", [0, 1])
def test_updates_before_refresh_is_monotone(eoc, pset):
    p = eoc.default_params(pset)
    sk = eoc.SecretKey(p, 29 + pset, with_cloud_key=False)
    budget = {(pp, d): noise.table_update_budget(p, sk.lwe_key, sk.tlwe_key, pp, d, 0) for pp in (2, 4, 8) for d in (0, 4, 8, 12)}
    print(pset, budget)
    for d in (0, 4, 8, 12):
        assert budget[2, d] >= budget[4, d] >= budget[8, d]
    for pp in (2, 4, 8):
        assert budget[pp, 0] >= budget[pp, 4] >= budget[pp, 8] >= budget[pp, 12]
    assert budget[2, 0] > 0
    # more standard deviations, a noisier value or a noisier table: never more updates
    base = noise.table_update_budget(p, sk.lwe_key, sk.tlwe_key, 4, 4, 0)
    assert noise.table_update_budget(p, sk.lwe_key, sk.tlwe_key, 4, 4, 0, sigmas=8.0) <= base
    assert noise.table_update_budget(p, sk.lwe_key, sk.tlwe_key, 4, 4, 0, value_var=1e-6) <= base
    assert noise.table_update_budget(p, sk.lwe_key, sk.tlwe_key, 4, 4, 0, table_var=1e-6) <= base
