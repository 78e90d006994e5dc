"""The edge inputs of tests/leveled_edge_inputs.py do what they claim (no GPU): the CMux differences sit on the gadget's cell
ends and end digits, the packing words on the rounding decomposition's, the crafted keys of the full-scale rows put the
references' conversions in the binade the tables name, and on all of these rows the references (tests/c/cmux_ref.c,
tests/c/pack_ref.c) stay within the project's 8-LSB rules of EXACT integer evaluation.  The device side is
tests/test_gpu_cmux_instances.py and tests/test_gpu_pack_edges.py."""
import ctypes as C

import numpy as np
import pytest

import cmux_oracle as cx
import leveled_edge_inputs as lei
import lut2_oracle as l2
import oracle_lib as ol
import pack_oracle as po

N = 1024
INSTANCES = list(lei.cmux_full_scale)
# measured max |reference - exact| in LSB of the Torus32 word (deterministic; x86-64, gcc -O2 -ffp-contract=off), printed
# by the tests below and recorded in DESIGN.md 12 / 13; the assertions are the project's bounds, not these
BOUND_EXTPROD_LSB = 8                      # per converted external product
BOUND_CHUNK_LSB = 8                        # per converted chunk


@pytest.fixture(scope="module")
def eoc(built_lib):
    import eoc_tfhe_amd
    return eoc_tfhe_amd


def wrap32(x):
    return ((np.asarray(x, np.int64) + 2**31) % 2**32) - 2**31


def params(eoc, l, Bgbit, n=16):
    p = eoc.default_params(0)
    p.n, p.l, p.Bgbit = n, l, Bgbit
    return p


# -- the CMux differences ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", INSTANCES)
def test_cmux_differences_sit_where_they_claim(name):
    cfg = lei.cmux_full_scale[name]
    l, Bgbit = cfg["l"], cfg["Bgbit"]
    Bg, off = 1 << Bgbit, lei.decomp_offset(l, Bgbit)
    D = lei.cmux_differences(l, Bgbit)
    assert set(D) == {"zero", "digits_min", "digits_max", "cells", "deltas", "alternating"}
    for v in D.values():
        assert v.dtype == np.uint32 and v.ndim == 3 and v.shape[1:] == (2, N)
    assert not D["zero"].any() and (lei.decomp_digits(D["zero"], l, Bgbit) == 0).all()
    assert (lei.decomp_digits(D["digits_min"], l, Bgbit) == -Bg // 2).all()
    assert (lei.decomp_digits(D["digits_max"], l, Bgbit) == Bg // 2 - 1).all()
    assert ((D["digits_max"].astype(np.int64) + off) & 0xFFFFFFFF == 0xFFFFFFFF).all()     # the truncated bits too
    # cells: [p][k][first, last of the cell below]
    words = lei.cell_end_words(l, Bgbit)
    assert words.shape == (2 * l * Bg,)                      # fewer distinct: k = 0's pair is the same word at every p, and
    assert np.unique(words).size >= 2 * l * Bg - 2 * l - Bg  # with l Bgbit = 32 the cells of position l are single words
    w = words.reshape(l, Bg, 2)
    d = lei.decomp_digits(w, l, Bgbit)                                                     # [l][l][Bg][2]
    for p in range(1, l + 1):
        first, last = d[:, p - 1, :, 0], d[:, p - 1, :, 1]                                 # [digit position][k]
        k = np.arange(Bg)
        assert np.array_equal(first[p - 1], k - Bg // 2)                                   # digit p takes every value ...
        assert np.array_equal(last[p - 1], (k - 1) % Bg - Bg // 2)                         # ... and one less, one word below
        assert (first[p:] == -Bg // 2).all() and (last[p:] == Bg // 2 - 1).all()           # below p: all clear / all set
        assert (first[:p - 1] == -Bg // 2).all()                                           # above p: untouched ...
        assert (last[:p - 1, 1:] == -Bg // 2).all() and (last[:p - 1, 0] == Bg // 2 - 1).all()   # ... but for k = 0's borrow
        x = (w[p - 1].astype(np.int64) + off) & 0xFFFFFFFF
        assert np.array_equal(x[:, 0], k << (32 - p * Bgbit)) and np.array_equal((x[:, 0] - x[:, 1]) % 2**32, np.ones(Bg))
    # every word lies in both polynomials of the samples, as many as needed and no more
    cells = D["cells"]
    assert cells.shape[0] == -(-words.size // N)
    for q in range(2):
        assert set(words.tolist()) == set(cells[:, q].ravel().tolist())
    # deltas: one non-zero word each, at the named places of polynomial 0, then of polynomial 1
    where = [tuple(np.argwhere(s)[0]) for s in D["deltas"]]
    assert all(np.count_nonzero(s) == 1 for s in D["deltas"])
    assert where == [(q, j) for q in range(2) for j in lei.DELTA_POSITIONS]
    assert {int(s[s != 0][0]) for s in D["deltas"]} == {int(D["digits_min"][0, 0, 0])}
    # inputs: in1 - in0 is the difference; the alternating pair is INT32_MIN / INT32_MAX in opposite phase
    ins = lei.cmux_inputs(l, Bgbit)
    for nm, (in0, in1) in ins.items():
        assert in0.dtype == in1.dtype == np.int32
        assert np.array_equal((in1.astype(np.int64) - in0) & 0xFFFFFFFF, D[nm]), nm
    a0, a1 = ins["alternating"]
    assert a0[0, 0, 0] == -2**31 and a0[0, 0, 1] == 2**31 - 1 and np.array_equal(a1[0, :, 1:], a0[0, :, :-1])
    assert set(np.unique(a0)) == set(np.unique(a1)) == {-2**31, 2**31 - 1}
    assert ins["zero"][0].min() < -2**30 and ins["zero"][0].max() > 2**30                  # in0: full-range words


@pytest.mark.parametrize("name", INSTANCES)
def test_cmux_full_scale_rows_lie_in_their_binade_and_fft_matches_exact(oracle_mod, name):
    """The condition on the inputs of tests/test_gpu_cmux_instances.py's full-scale part: with the constant-K selector of
    leveled_edge_inputs.cmux_full_scale the largest value the reference converts on digits_min and digits_max lies in the
    row's interval and below 2^51 -- [2^50, 2^51), the top binade of the conversion contract, for every instance but <3,7>,
    which reaches 1.5 x 2^49 with the largest int32 magnitude.  And the reference against the exact product there.
    Measured: max converted 2^50.585 on digits_min and 2^50.574 .. 2^50.584 on digits_max (2^49.585 / 2^49.562 for <3,7>);
    |reference - exact| = 1 LSB on every row."""
    cfg = lei.cmux_full_scale[name]
    l, Bgbit = cfg["l"], cfg["Bgbit"]
    op = ol.OrcParams()
    assert ol.lib().orc_default_params(0, C.byref(op)) == 0
    op.l, op.Bgbit = l, Bgbit
    sel = lei.constant_selector(l, cfg["K"])
    fft = cx.to_fft(sel)
    D = lei.cmux_differences(l, Bgbit)
    L = ol.lib()
    for nm in ("digits_min", "digits_max"):
        L.orc_dbg_max_conv(1)
        ref = cx.extprod(op, fft, D[nm][0])
        mx = L.orc_dbg_max_conv(0)
        worst = int(np.abs(wrap32(ref.astype(np.int64) - cx.extprod_exact(op, sel, D[nm][0]))).max())
        print(f"{name} {nm}: (l, Bgbit, K) = ({l}, {Bgbit}, {cfg['K']}): max converted 2^{np.log2(mx):.3f}, "
              f"reference vs exact max |diff| = {worst} LSB")
        assert cfg["lo"] <= mx < cfg["hi"] and mx < 2.0**51, (name, nm, np.log2(mx))
        assert worst <= BOUND_EXTPROD_LSB, (name, nm, worst)


@pytest.mark.parametrize("name", INSTANCES)
def test_cmux_reference_against_exact_on_the_edge_rows(eoc, name):
    """Real selectors of 0 and of 1 on every edge difference: the reference within 8 LSB of the exact schoolbook product
    (DESIGN.md 12), every conversion inside the contract; on `zero` the CMux returns in0 word for word.
    Measured max |reference - exact|: <2,10> 1, <3,7> 1, <1,0> 1, <2,0> 1, <3,0> 1, <4,0> 1 LSB."""
    cfg = lei.cmux_full_scale[name]
    l, Bgbit = cfg["l"], cfg["Bgbit"]
    p = params(eoc, l, Bgbit)
    op = cx.orc_params(p)
    sk = eoc.SecretKey(p, 21, with_cloud_key=False)
    sel = sk.encrypt_selector_bits([0, 1], enc_seed=5)
    fft = cx.to_fft(sel)
    L = ol.lib()
    L.orc_dbg_max_conv(1)
    worst = 0
    for nm, (in0, in1) in lei.cmux_inputs(l, Bgbit).items():
        D = lei.cmux_differences(l, Bgbit)[nm]
        for k in range(D.shape[0]):
            for b in range(2):
                ref = cx.extprod(op, fft[b], D[k])
                d = int(np.abs(wrap32(ref.astype(np.int64) - cx.extprod_exact(op, sel[b], D[k]))).max())
                worst = max(worst, d)
                assert d <= BOUND_EXTPROD_LSB, (name, nm, k, b, d)
                out = cx.cmux(op, fft[b], in0[k], in1[k])
                assert np.array_equal(out, cx._u32(in0[k].astype(np.int64) + ref).view(np.int32))
                if nm == "zero":
                    assert np.array_equal(out, in0[k])
    assert L.orc_dbg_max_conv(0) < 2.0**51
    print(f"{name}: edge rows, real selectors: reference vs exact max |diff| = {worst} LSB")


# -- the packing key switch --------------------------------------------------------------------------------------------------
def test_pack_mask_words_sit_on_the_rounding_cells_ends():
    w = lei.pack_mask_words()
    assert len(w) == 6 + 3 * 16 - 1 and len(set(w.values())) == len(w)      # top15_ripple is carry_out
    d = {k: po.digits(np.array([v]))[:, 0].tolist() for k, v in w.items()}
    assert d["digits_min"] == [-8] * 4 and d["digits_max"] == [7] * 4 and w["digits_max"] & 0xFFFF == 0x7FFF
    assert (w["digits_min"] + lei.PACK_OFFSET) % 2**32 == 0 and (w["digits_max"] + lei.PACK_OFFSET) % 2**32 == 2**32 - 1
    assert d["zero"] == [0] * 4 and d["carry_out"] == [0] * 4              # 0xFFFF8000 rounds up to 2^32 = 0
    assert w["carry_out"] + 0x8000 == 2**32
    assert d["int32_min"] == [-8, 0, 0, 0] and d["int32_max"] == [-8, 0, 0, 0]      # 0x7FFFFFFF rounds up to 2^31
    for t in range(16):
        top = (t + 8) % 16 - 8
        assert w[f"top{t}_down"] & 0xFFFF == 0x7FFF and w[f"top{t}_up"] & 0xFFFF == 0x8000
        assert d[f"top{t}_down"] == [top, 0, 0, 0]
        assert d[f"top{t}_up"] == [top, 0, 0, 1]                          # both ends of one cell differ in the last digit only
        if t < 15:
            assert d[f"top{t}_ripple"] == [(t + 9) % 16 - 8, 0, 0, 0]     # 0x_FFF8000 rounds up into the top digit
    # digits recompose to the word rounded to 16 bits
    for k, v in w.items():
        rec = sum(x << (32 - 4 * (j + 1)) for j, x in enumerate(d[k]))
        err = (v - rec + 2**31) % 2**32 - 2**31
        assert -2**15 <= err < 2**15, k
    assert lei.PACK_OFFSET == (1 << (31 - 16)) + sum(8 << (32 - 4 * p) for p in range(1, 5))


def test_pack_shapes_counts_and_samples():
    assert lei.pack_shapes == (1, 16, 17, 63, 64) and lei.pack_counts == (1, 63, 64, 65, N - 1, N + 1, 2 * N + 1)
    assert [po.n_chunks(n) for n in lei.pack_shapes] == [1, 1, 2, 4, 4]
    assert [n - 16 * (po.n_chunks(n) - 1) for n in lei.pack_shapes] == [1, 16, 1, 15, 16]      # indices of the last chunk
    assert [-(-(n + 1) // 64) for n in lei.pack_shapes] == [1, 1, 1, 1, 2]                     # column tiles of the gather
    assert (-(-(2 * N + 1) // N) * po.n_chunks(17)) % 4 == 2                                   # 6 items: half a workgroup
    words = set(lei.pack_mask_words().values())
    for n in lei.pack_shapes:
        s = lei.pack_samples(n, 65)
        assert s.shape == (65, n + 1) and s.dtype == np.int32
        for m in range(n):
            assert set(s[:, m].view(np.uint32).tolist()) == words, (n, m)                      # each word meets each column
        for m in range(1, min(n, 53)):
            assert not (s[:, m] == s[:, 0]).any()
        if n > 1:                                                                              # ... at several slots
            slots = {int(np.flatnonzero(s[:53, m].view(np.uint32) == 0xFFFF8000)[0]) for m in range(n)}
            assert len(slots) >= min(n, 8)


@pytest.mark.parametrize("n", lei.pack_shapes)
def test_pack_reference_against_exact_on_the_edge_words(eoc, n):
    """A real packing key of the shape's n, one full list of pack_samples: the reference within 8 LSB per converted chunk
    of exact wrapping-integer arithmetic, every conversion inside the contract.
    Measured max |reference - exact| over the whole list (chunks): n = 1: 1 (1), 16: 1 (1), 17: 2 (2), 63: 4 (4),
    64: 4 (4) LSB."""
    p = params(eoc, 2, 10, n)
    sk = eoc.SecretKey(p, 5, with_cloud_key=False)
    rows = po.blob_rows(sk.packing_key_bytes(), n)
    kfft = po.key_fft(rows)
    cts = lei.pack_samples(n, N)
    nch = po.n_chunks(n)
    L = ol.lib()
    L.orc_dbg_max_conv(1)
    ref = po.pack_list(n, kfft, cts)
    assert L.orc_dbg_max_conv(0) < 2.0**51
    d = int(np.abs(wrap32(ref.astype(np.int64) - po.pack_list_exact(n, rows, cts, 0, nch))).max())
    print(f"n = {n}: {nch} chunks: reference vs exact max |diff| = {d} LSB")
    assert d <= BOUND_CHUNK_LSB * nch, (n, d)
    for c in range(nch):                                                  # and chunk by chunk
        one = po.pack_list(n, kfft, cts, c, c + 1)
        dc = int(np.abs(wrap32(one.astype(np.int64) - po.pack_list_exact(n, rows, cts, c, c + 1))).max())
        assert dc <= BOUND_CHUNK_LSB, (n, c, dc)


def test_pack_full_scale_lies_in_its_binade_and_fft_matches_exact(eoc):
    """The crafted key of PACK_FULL_SCALE (every word K = -3 x 2^29, n = 16) on the all-digits -8 batch: the reference's
    largest converted value lies in [2^49, 2^50), the highest binade below the documented bound 2^50 (K = -2^31 gives 2^50
    itself, the closed end: asserted too, and still inside the contract).  Measured: 2^49.585 and 2^50.000;
    |reference - exact| 1 LSB on both."""
    fs = lei.PACK_FULL_SCALE
    n = fs["n"]
    p = params(eoc, 2, 10, n)
    blob = eoc.SecretKey(p, 5, with_cloud_key=False).packing_key_bytes()
    cts = lei.pack_full_scale_samples()
    assert (po.digits(cts[:, :n]) == -8).all() and not cts[:, n].any()
    L = ol.lib()
    for K, lo, hi in ((fs["K"], fs["lo"], fs["hi"]), (-2**31, 2.0**50, 2.0**50 + 1)):
        crafted = lei.constant_packing_blob(blob, K)
        assert bytes(crafted[:52]) == bytes(blob[:52]) and crafted.size == blob.size
        rows = po.blob_rows(crafted, n)
        assert (rows == K).all()
        L.orc_dbg_max_conv(1)
        ref = po.pack_list(n, po.key_fft(rows), cts)
        mx = L.orc_dbg_max_conv(0)
        d = int(np.abs(wrap32(ref.astype(np.int64) - po.pack_list_exact(n, rows, cts, 0, 1))).max())
        print(f"pack full scale K = {K}: max converted 2^{np.log2(mx):.3f}, reference vs exact max |diff| = {d} LSB")
        assert lo <= mx < hi and mx < 2.0**51, (K, np.log2(mx))
        assert d <= BOUND_CHUNK_LSB, (K, d)
    q = eoc.Params()
    assert eoc.lib().eoc_packing_key_blob_params(crafted.ctypes.data, crafted.size, C.byref(q)) == 0 and q.n == n


# -- the test-polynomial pack ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [2, 4, 8])
def test_tv_values_put_the_extreme_words_under_the_negated_window(p):
    for n in lei.TV_SHAPES:
        seen_b = set()
        for rows in lei.TV_ROWS:
            v = lei.tv_values(n, p, rows)
            assert v.shape == (2, p, rows, n + 1) and v.dtype == np.int32
            for f in range(2):
                for s in range(rows):
                    zero = v[f, 0, s]                                     # the sample the last window negates
                    assert zero[:4].tolist() == list(lei.TV_WORDS)
                    assert set(zero[n - 4:n].tolist()) == set(lei.TV_WORDS)
                    seen_b.add(int(zero[n]))
                    batch = l2.tv_batch(v[f, :, s], p)
                    neg = np.arange(N) >= N - N // (2 * p)
                    assert np.array_equal(batch[neg][:, :4], np.tile([-2**31, -2**31 + 1, 0, 1], (neg.sum(), 1)))
                    assert np.array_equal(batch[~neg][:64], np.tile(zero, (64, 1)))
            assert all(set(lei.TV_WORDS) <= set(v[f, j, s].tolist()) for f in range(2) for j in range(p) for s in range(rows))
        assert seen_b == set(lei.TV_WORDS)
