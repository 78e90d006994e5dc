"""Every instance of the encrypted-seed blind rotation (k_br_enc / k_br_enc_wide) that blind_rotate_kernel()
(engine.hip) can dispatch, on the MI355X, with the edge inputs of tests/br_edge_inputs.py: six pair shapes and two wide shapes,
each with the rotation amounts read back by vector loads (vabar) or by scalar loads (sabar): 16 instances, one test id each,
named after the kernel.  The scheme is tests/test_gpu_br_instances.py's, through its helpers: a real key at n = 1 -- every
rotation amount in [0, 2N) as abar and as barb, from the smallest and the largest word of its rounding cell -- and at n = 2 --
br_edge_inputs.two_step_rows() --, compared word for word with the composed reference (tests/lut2_oracle.py).  Nothing is
decrypted.

The seed lists have BOTH polynomials non-zero: pairs of br_edge_inputs.extreme_polys(l, Bgbit) and random words.  Each runs
with one list per group (per_row = 0) and with one list per job (per_row = 1: job (g, s) uses list (g + s) mod G of the same
lists, so the per-group reference serves both).  The conversion contract (include/eoc_tfhe_gpu.h): every (l, Bgbit) here but
Set A's (2, 10) keeps any input below 2^51; the oracle's recorded maximum is asserted below 2^51 for every reference
(test_gpu_br_instances.reference), Set A's shape included.

The family has no earlier-form twin: the two gadget-length-2 pair shapes run once more with EOC_TFHE_BR_TABLES_LDS=1, where
blind_rotate_kernel() must still pick k_br_enc."""
import numpy as np
import pytest

import br_edge_inputs as bei
import lut2_oracle as l2
from gpu_util import dev_empty, sync, to_dev, torch_cuda
from test_gpu_br_instances import SHAPES, engine, keys, reference

pytestmark = pytest.mark.gpu
N = 1024
ENC_SHAPES = [s for s in SHAPES if not s.startswith("lds")]           # the family has no earlier-form twin
INSTANCES = [(shape, readback) for shape in ENC_SHAPES for readback in ("vabar", "sabar")]


def kernel_name(shape, readback):
    return f"{'k_br_enc_wide' if shape.startswith('wide') else 'k_br_enc'}<{SHAPES[shape][0]},{readback}>"


@pytest.fixture(scope="module")
def eoc(built_lib):
    torch_cuda()
    import eoc_tfhe_amd
    return eoc_tfhe_amd


def seed_lists(l, Bgbit, n):
    """[G][2][N]: n = 1: (alternating, random), (random, random); n = 2: three pairs of extreme polynomials and a random one"""
    ext = bei.extreme_polys(l, Bgbit)
    rnd = np.random.default_rng(100 * l + Bgbit).integers(-2**31, 2**31, (3, N)).astype(np.int32)
    if n == 1:
        pairs = [(ext["alternating"], rnd[0]), (rnd[1], rnd[2])]
    else:
        pairs = [(ext["digits_min"], ext["alternating"]), (ext["alternating"], ext["digits_max"]),
                 (ext["digits_max"], ext["digits_min"]), (rnd[1], rnd[2])]
    lists = np.ascontiguousarray(np.stack([np.stack(pr) for pr in pairs]).astype(np.int32))
    assert all(lists[g, q].any() for g in range(len(pairs)) for q in range(2))
    return lists


def rows_of(n):
    """(device rows, indices of the rows compared with the reference): the _tv instances' choice"""
    if n == 2:
        rows = bei.two_step_rows(1)[0]
        return rows, np.arange(rows.shape[0])
    return bei.sweep(1)[0], bei.sweep_subset(1)


def run_enc(eng, lists, n_groups, per_row, rows):
    d_lists, d_in = to_dev(lists), to_dev(rows)
    d_out = dev_empty((n_groups, rows.shape[0], rows.shape[1]), torch_cuda().int32)
    eng.lut_enc_batch_device(d_lists.data_ptr(), n_groups, per_row, d_in.data_ptr(), d_out.data_ptr(), rows.shape[0])
    sync()
    return d_out.cpu().numpy()


@pytest.mark.parametrize("shape,readback", INSTANCES, ids=[kernel_name(*i) for i in INSTANCES])
def test_instance_bit_exact_on_edge_inputs(eoc, monkeypatch, shape, readback):
    check_instance(eoc, monkeypatch, shape, readback)


LDS_SHAPES = [s for s in SHAPES if s.startswith("lds")]


@pytest.mark.parametrize("shape", LDS_SHAPES, ids=[f"k_br_enc<{SHAPES[s][0]},vabar>+tables_lds" for s in LDS_SHAPES])
def test_family_runs_its_shipped_form_under_the_earlier_form_knob(eoc, monkeypatch, shape):
    """EOC_TFHE_BR_TABLES_LDS=1 sends the other three families of gadget length 2 to their k_br_lds* twins; this family has
    none, and blind_rotate_kernel() keeps it on k_br_enc: the same inputs, the same reference, the same words"""
    check_instance(eoc, monkeypatch, shape, "vabar")


def check_instance(eoc, monkeypatch, shape, readback):
    _, (l, Bgbit), env = SHAPES[shape]
    wide = shape.startswith("wide")
    for n in (1, 2):
        p, sk, orc = keys(eoc, l, Bgbit, n)
        assert np.array_equal(sk.bk, orc.bk) and np.array_equal(sk.ksk, orc.ksk)
        lists = seed_lists(l, Bgbit, n)
        G = lists.shape[0]
        rows, pick = rows_of(n)
        want = reference((l, Bgbit, n, "enc"), lambda: l2.lut_enc_rows(orc, lists, rows[pick]))
        eng = engine(eoc, monkeypatch, p, env, readback)
        eng.load_cloud_key(sk)
        before = eng.stats()
        got0 = run_enc(eng, lists, G, False, rows)[:, pick]
        # one list per job: job (g, s) of 2 groups over the compared rows starts from list (g + s) mod G
        sub = np.ascontiguousarray(rows[pick])
        which = (np.arange(2)[:, None] + np.arange(sub.shape[0])[None, :]) % G
        got1 = run_enc(eng, lists[which], 2, True, sub)
        st = eng.stats()
        eng.close()
        assert st["br_launches"] > before["br_launches"]
        moved = st["br_wide_launches"] - before["br_wide_launches"]
        assert (moved == st["br_launches"] - before["br_launches"]) if wide else (moved == 0), (shape, st, before)
        assert st["bootstraps"] - before["bootstraps"] == G * rows.shape[0] + 2 * sub.shape[0]
        assert got0.shape == want.shape
        bad = np.argwhere((got0 != want).any(axis=-1))
        assert bad.size == 0, (kernel_name(shape, readback), n, "per_row=0", len(bad), bad[:8].tolist())
        want1 = want[which, np.arange(sub.shape[0])[None, :]]
        bad = np.argwhere((got1 != want1).any(axis=-1))
        assert bad.size == 0, (kernel_name(shape, readback), n, "per_row=1", len(bad), bad[:8].tolist())
