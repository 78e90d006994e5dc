"""The packing kernels -- k_pack_gather, k_pack_rows, k_tvpack_cols<p> -- on the MI355X at the shapes and words where they take
another path (tests/leveled_edge_inputs.py), through eoc_engine_set_packing_key, eoc_pack_device and eoc_tv_pack_device:
  n in {1, 16, 17, 63, 64}   a short chunk only (the peeled first index alone), exactly one full chunk, a chunk of one index
                             behind a full one, n + 1 = 64 and 65 (the gather's column tile: b last in the only tile, b alone
                             in a second one), with a real packing key of that n
  mask words                 both ends of the rounding decomposition's cells (low half 0x7FFF / 0x8000), carries that ripple
                             into the top digit and out of bit 31, all digits -8 and 7, INT32_MIN / INT32_MAX, in every column
  counts                     1, 63, 64, 65, N - 1, N + 1, 2N + 1: ragged sample tiles, ragged last lists, and item counts that
                             are no multiple of the four waves of a k_pack_rows workgroup
  full scale                 a packing key of one constant word: the chunk's converted sum at 1.5 x 2^49, in the highest
                             binade below the documented bound of 2^50
  test-polynomial lists      p in {2, 4, 8} at n = 63 and 64, rows 1 and 3, INT32_MIN / INT32_MAX / 0 / -1 under the negated
                             last window
and compared with the references (tests/pack_oracle.py, tests/lut2_oracle.py) word for word, each computed under
test_gpu_br_instances.reference: every conversion stayed inside the contract (include/eoc_tfhe_gpu.h).
Host side of the inputs: tests/test_leveled_edge_inputs_cpu.py."""
import numpy as np
import pytest

import leveled_edge_inputs as lei
import lut2_oracle as l2
import oracle_lib as ol
import pack_oracle as po
from gpu_util import sync, to_dev, torch_cuda
from test_gpu_br_instances import reference

pytestmark = pytest.mark.gpu
N = 1024
FILL = 0x5A5A5A5A


@pytest.fixture(scope="module")
def eoc(built_lib):
    torch_cuda()
    import eoc_tfhe_amd
    return eoc_tfhe_amd


_KEYS = {}


def keys(eoc, n):
    """params, packing-key blob of a real secret key at this n, its reference spectra, engine with the key"""
    if n not in _KEYS:
        p = eoc.default_params(0)
        p.n = n
        blob = eoc.SecretKey(p, 5, with_cloud_key=False).packing_key_bytes()
        eng = eoc.Engine(p)
        eng.load_packing_key(blob)
        _KEYS[n] = (p, blob, po.key_fft(po.blob_rows(blob, n)), eng)
    return _KEYS[n]


def filled(shape):
    torch = torch_cuda()
    return torch.full(shape, FILL, dtype=torch.int32, device="cuda")


def pack_device(eng, cts):
    """lists of `cts`; the output buffer is pre-filled and holds one list more, which must keep its fill"""
    lists = -(-cts.shape[0] // N)
    d_in, d_out = to_dev(cts), filled((lists + 1, 2, N))
    before = eng.stats()
    eng.pack_device(d_in.data_ptr(), cts.shape[0], d_out.data_ptr())
    sync()
    after = eng.stats()
    assert after["pack_launches"] - before["pack_launches"] == 1
    assert after["packed_samples"] - before["packed_samples"] == cts.shape[0]
    out = d_out.cpu().numpy()
    assert (out[lists] == FILL).all()
    return out[:lists]


def differ(got, want):
    bad = np.argwhere(got != want)
    return len(bad), bad[:6].tolist()


@pytest.mark.parametrize("n", lei.pack_shapes)
def test_pack_bit_exact_on_edge_words_and_shapes(eoc, n):
    p, _, kfft, eng = keys(eoc, n)
    cts = lei.pack_samples(n, max(lei.pack_counts))
    for count in lei.pack_counts:
        got = pack_device(eng, cts[:count])
        want = reference(("pack", n, count), lambda: po.pack(n, kfft, cts[:count]))
        assert got.shape == want.shape == (-(-count // N), 2, N)
        n_bad, first = differ(got, want)
        # a differing word (list, polynomial, slot): slot i of polynomial 1 starts as b_i; mask word of column m there:
        # pack_mask_words()[(i + 7 m) mod 53]
        assert n_bad == 0, (n, count, n_bad, first)


def test_pack_full_scale_chunk(eoc):
    fs = lei.PACK_FULL_SCALE
    n = fs["n"]
    p, blob, _, _ = keys(eoc, n)
    crafted = lei.constant_packing_blob(blob, fs["K"])
    kfft = po.key_fft(po.blob_rows(crafted, n))
    cts = lei.pack_full_scale_samples()

    def compute():
        out = po.pack(n, kfft, cts, threads=1)
        mx = ol.lib().orc_dbg_max_conv(0)                        # reference() reset it and asserts the contract behind this
        assert fs["lo"] <= mx < fs["hi"], np.log2(mx)
        return out
    want = reference(("pack", "full scale"), compute)
    eng = eoc.Engine(p)                                          # an engine of its own: the shared one keeps its real key
    eng.load_packing_key(crafted)
    got = pack_device(eng, cts)
    eng.close()
    n_bad, first = differ(got, want)
    assert n_bad == 0, (n_bad, first)


@pytest.mark.parametrize("n", lei.TV_SHAPES)
@pytest.mark.parametrize("p", [2, 4, 8])
def test_tv_pack_bit_exact_on_extreme_words(eoc, p, n):
    _, _, kfft, eng = keys(eoc, n)
    for rows in lei.TV_ROWS:
        vals = lei.tv_values(n, p, rows)
        F = vals.shape[0]
        d_vals, d_out = to_dev(vals), filled((F * rows + 1, 2, N))
        before = eng.stats()
        eng.tv_pack_device(p, d_vals.data_ptr(), F, rows, d_out.data_ptr())
        sync()
        after = eng.stats()
        assert after["pack_launches"] - before["pack_launches"] == 1
        assert after["packed_samples"] - before["packed_samples"] == F * rows * p
        out = d_out.cpu().numpy()
        assert (out[F * rows] == FILL).all()
        want = reference(("tv pack", n, p, rows), lambda: l2.tv_pack(n, kfft, vals, p))
        n_bad, first = differ(out[:F * rows].reshape(F, rows, 2, N), want)
        assert n_bad == 0, (p, n, rows, n_bad, first)
