"""The exact test-polynomial pack on the MI355X: eoc_tv_pack_exact_device -- k_pks_limbs at key install,
k_tvpack_mm, k_tv_spread<p> -- word for word against the integer reference (tests/tv_pack_exact_oracle.py):
  real keys        Set A and Set B, p in {2, 4, 8}, n_funcs in {1, 2}, rows in {1, 3}
  custom n         1, 7, 8, 9, 63, 64 with a real packing key of that n: K = 4 n below, at and just past a multiple of 32 (one K
                   step with 4, 28 and 32 live digits, a second step of 4), and 8 full steps with and without a ragged last one;
                   every mask column cycles through leveled_edge_inputs.pack_mask_words(); list counts that use the 256-row
                   tile once (5 rows), leave it one row short (255) and run one tile past it (260); the list behind the output
                   keeps its fill
  full scale       a key whose four limbs are all -128 under mask words whose digits are all -8, at n = 500
  slices           EOC_TFHE_PACK_WS_BYTES at one list's need: 3 lists as 1 + 1 + 1, the unsliced words
  the parent's path  eoc_tv_pack_device on the same inputs: within 8 LSB per chunk of 16 key indices, the same test polynomial
  errors           EOC_ERR_NO_KEY, EOC_ERR_ARG, count == 0
Host side: tests/test_lut_tree_cpu.py."""
import numpy as np
import pytest

import leveled_edge_inputs as lei
import lut2_oracle as l2
import pack_oracle as po
import tv_pack_exact_oracle as tpe
from gpu_util import dev_empty, sync, to_dev, torch_cuda

pytestmark = pytest.mark.gpu
N = 1024
FILL = 0x5A5A5A5A
EOC_OK, EOC_ERR_ARG, EOC_ERR_NO_KEY = 0, -1, -4
ALL_LIMBS_MIN = 0x7F7F7F80                                       # -128 (1 + 2^8 + 2^16 + 2^24) mod 2^32: four limbs of -128


@pytest.fixture(scope="module")
def eoc(built_lib):
    torch_cuda()
    import eoc_tfhe_amd
    return eoc_tfhe_amd


def pack_exact(eng, p, vals, parent=False):
    """lists [F][rows][2][N] of vals [F][p][rows][n+1]; the output buffer is pre-filled and holds one list more, which must
    keep its fill; the counters move as eoc_tv_pack_device's do"""
    F, _, rows, _ = vals.shape
    d_vals = to_dev(vals)
    d_out = torch_cuda().full((F * rows + 1, 2, N), FILL, dtype=torch_cuda().int32, device="cuda")
    before = eng.stats()
    (eng.tv_pack_device if parent else eng.tv_pack_exact_device)(p, d_vals.data_ptr(), F, rows, d_out.data_ptr())
    sync()
    after = eng.stats()
    assert after["packed_samples"] - before["packed_samples"] == F * rows * p
    assert after["keyswitches"] == before["keyswitches"] and after["bootstraps"] == before["bootstraps"]
    out = d_out.cpu().numpy()
    assert (out[F * rows] == FILL).all()
    return out[:F * rows].reshape(F, rows, 2, N), after["pack_launches"] - before["pack_launches"]


def differ(got, want):
    bad = np.argwhere(got != want)
    return len(bad), bad[:6].tolist()


def real_vals(eoc, pset, p, count):
    """fresh encryptions [2][p][count][n+1] under the shared key"""
    params, sk = l2.keys(eoc, pset)[:2]
    return sk.encrypt_ints(np.random.default_rng(p + count).integers(0, p, 2 * p * count).astype(np.uint8), p,
                           5000 + 100 * pset + 10 * p + count).reshape(2, p, count, params.n + 1)


_ENG = {}


def real_engine(eoc, pset):
    if pset not in _ENG:
        params, _, blob = l2.keys(eoc, pset)[:3]
        _ENG[pset] = eoc.Engine(params)
        _ENG[pset].load_packing_key(blob)
    return _ENG[pset]


# -- real keys -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pset", [0, 1], ids=["setA", "setB"])
@pytest.mark.parametrize("p", [2, 4, 8])
def test_real_keys_word_for_word(eoc, pset, p):
    """n = 500: 63 K steps, the last with 4 key indices; n = 630: 79 steps, the last with 6"""
    params, _, blob = l2.keys(eoc, pset)[:3]
    rows_key = po.blob_rows(blob, params.n)
    eng = real_engine(eoc, pset)
    for count in (1, 3):
        vals = real_vals(eoc, pset, p, count)
        for F in (1, 2):
            got, launches = pack_exact(eng, p, vals[:F])
            assert launches == 1
            n_bad, first = differ(got, tpe.tv_pack_exact(params.n, rows_key, vals[:F], p))
            assert n_bad == 0, (pset, p, count, F, n_bad, first)


@pytest.mark.parametrize("pset", [0, 1], ids=["setA", "setB"])
def test_against_the_fft_pack_of_the_same_inputs(eoc, pset):
    """eoc_tv_pack_device evaluates the same rule through transforms: every word within 8 LSB per converted chunk of 16 key
    indices (the project's asserted bound between the FFT reference and exact evaluation), wrapping; and both lists decrypt,
    coefficient by coefficient, to the test polynomial of the row's values"""
    params, sk = l2.keys(eoc, pset)[:2]
    eng = real_engine(eoc, pset)
    for p in (2, 4, 8):
        vals = real_vals(eoc, pset, p, 3)
        exact, _ = pack_exact(eng, p, vals)
        fft, _ = pack_exact(eng, p, vals, parent=True)
        diff = (exact.astype(np.int64) - fft.astype(np.int64) + 2**31) % 2**32 - 2**31
        bound = 8 * po.n_chunks(params.n)
        print(f"pset {pset} p {p}: max |exact - fft| = {np.abs(diff).max()} LSB (bound {bound})")
        assert np.abs(diff).max() <= bound, (p, np.abs(diff).max())
        msgs = sk.decrypt_ints(vals.reshape(-1, params.n + 1), p).reshape(2, p, 3).astype(np.int64)
        j, neg = l2.tv_slots(p)
        want = np.where(neg[None, None, :], (2 * p - msgs[:, 0, :, None]) % (2 * p), msgs.transpose(0, 2, 1)[:, :, j])   # [2][3][N]
        for lists in (exact, fft):
            ph = sk.list_phases(lists.reshape(-1, 2, N)).astype(np.int64).reshape(2, 3, N)
            assert np.array_equal(((ph * 2 * p + (1 << 31)) >> 32) % (2 * p), want), p


# -- every shape ---------------------------------------------------------------------------------------------------------------
SHAPES = (1, 7, 8, 9, 63, 64)
# (p, n_funcs, rows): samples = n_funcs rows (p + 1).  No count fills the 256-row tile exactly: p + 1 is odd.
LISTS = ((4, 1, 1), (4, 3, 17), (4, 2, 26), (2, 2, 26), (8, 2, 26))     # 5, 255, 260, 156 and 468 rows of S
_KEYS = {}


def small_keys(eoc, n):
    if n not in _KEYS:
        p = eoc.default_params(0)
        p.n = n
        blob = eoc.SecretKey(p, 5, with_cloud_key=False).packing_key_bytes()
        eng = eoc.Engine(p)
        eng.load_packing_key(blob)
        _KEYS[n] = (p, blob, eng)
    return _KEYS[n]


@pytest.mark.parametrize("n", SHAPES)
def test_edge_words_and_shapes_word_for_word(eoc, n):
    _, blob, eng = small_keys(eoc, n)
    rows_key = po.blob_rows(blob, n)
    for p, F, rows in LISTS:
        vals = lei.pack_samples(n, F * p * rows, seed=p).reshape(F, p, rows, n + 1)
        got, launches = pack_exact(eng, p, vals)
        assert launches == 1
        n_bad, first = differ(got, tpe.tv_pack_exact(n, rows_key, vals, p))
        assert n_bad == 0, (n, p, F, rows, n_bad, first)


def test_full_scale_accumulators(eoc):
    """every key word 0x7F7F7F80 (all four limbs -128), every mask word of the p values at all digits -8: each limb accumulator
    of their rows reaches 4 n 8 128 = 2 048 000 (n = 500), the bound the kernel's comment states for Set A"""
    params, _, blob = l2.keys(eoc, 0)[:3]
    crafted = lei.constant_packing_blob(blob, np.int64(ALL_LIMBS_MIN).astype(np.int32))
    n, p = params.n, 4
    vals = np.full((1, p, 2, n + 1), lei.pack_mask_words()["digits_min"], np.int64)
    vals[..., n] = np.random.default_rng(3).integers(-2**31, 2**31, (1, p, 2))
    vals = (vals & 0xFFFFFFFF).astype(np.uint32).view(np.int32)
    assert (po.digits(vals[..., :n]) == -8).all()
    eng = eoc.Engine(params)                                     # an engine of its own: the shared one keeps its real key
    eng.load_packing_key(crafted)
    got, _ = pack_exact(eng, p, vals)
    eng.close()
    n_bad, first = differ(got, tpe.tv_pack_exact(n, po.blob_rows(crafted, n), vals, p))
    assert n_bad == 0, (n_bad, first)


def test_workspace_budget_slices_the_lists_without_changing_a_word(eoc, monkeypatch):
    """EOC_TFHE_PACK_WS_BYTES (read at engine creation) at one list's constant-slot samples and a little: 3 lists as 1 + 1 + 1"""
    params, _, blob = l2.keys(eoc, 0)[:3]
    p = 4
    vals = real_vals(eoc, 0, p, 3)[:1]
    monkeypatch.setenv("EOC_TFHE_PACK_WS_BYTES", str((p + 1) * 2 * N * 4 + 100))
    eng = eoc.Engine(params)
    monkeypatch.delenv("EOC_TFHE_PACK_WS_BYTES")
    eng.load_packing_key(blob)
    got, launches = pack_exact(eng, p, vals)
    eng.close()
    assert launches == 3
    whole, one = pack_exact(real_engine(eoc, 0), p, vals)
    assert one == 1 and np.array_equal(got, whole)
    assert np.array_equal(got, tpe.tv_pack_exact(params.n, po.blob_rows(blob, params.n), vals, p))


def test_errors_missing_key_and_empty_call(eoc):
    torch = torch_cuda()
    L = eoc.lib()
    params = l2.keys(eoc, 0)[0]
    eng = real_engine(eoc, 0)
    buf = torch.full((1 << 16,), 7, dtype=torch.int32, device="cuda")
    a = buf.data_ptr()
    before = eng.stats()
    for p in (0, 1, 3, 16):
        assert L.eoc_tv_pack_exact_device(eng.h, p, a, 1, 1, a, None) == EOC_ERR_ARG
    assert L.eoc_tv_pack_exact_device(eng.h, 4, a, 0, 1, a, None) == EOC_ERR_ARG
    assert L.eoc_tv_pack_exact_device(eng.h, 4, None, 1, 1, a, None) == EOC_ERR_ARG
    assert L.eoc_tv_pack_exact_device(eng.h, 4, a, 1, 1, None, None) == EOC_ERR_ARG
    assert L.eoc_tv_pack_exact_device(eng.h, 4, a, 1, 0, a, None) == EOC_OK       # count 0 touches nothing
    no_key = eoc.Engine(params)
    assert L.eoc_tv_pack_exact_device(no_key.h, 4, a, 1, 1, a, None) == EOC_ERR_NO_KEY
    no_key.close()
    sync()
    assert bool((buf == 7).all()) and eng.stats() == before
    # below one list's need the budget refuses
    import os
    os.environ["EOC_TFHE_PACK_WS_BYTES"] = "1000"
    try:
        tiny = eoc.Engine(params)
    finally:
        del os.environ["EOC_TFHE_PACK_WS_BYTES"]
    tiny.load_packing_key(l2.keys(eoc, 0)[2])
    assert L.eoc_tv_pack_exact_device(tiny.h, 4, a, 1, 1, a, None) == EOC_ERR_ARG
    tiny.close()
