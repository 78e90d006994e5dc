"""The rounding mode of the leveled calls, host side (no GPU): the reference tests/leveled_round_oracle.py against
the identity that defines the mode and against the exact schoolbook product with rounded digits, on edge words; the noise of one
rounding CMux against the model (same variance, the mean gone); the budgets the model gives with and without the mode; a long
automaton run on the reference inside the rounding model's bound; the new symbols and their argument errors.  Device side:
tests/test_gpu_leveled_round.py."""
import json
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import automaton_oracle as ao
import cmux_oracle as cx
import compact_oracle as co
import leveled_edge_inputs as le
import leveled_round_oracle as lr
import oracle_lib as ol
from eoc_tfhe_amd import noise
from test_cmux_cpu import SLOTS, custom, tlwe_phase, wrap32

N = 1024
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROTS = (0, 1, 1023, 1024, 2047)
# (parameter set, l, Bgbit): both default sets, gadget lengths 1 and 4 at a run-time base
SHAPES = [(0, None, None), (1, None, None), (0, 1, 10), (0, 4, 7)]


@pytest.fixture(scope="module")
def eoc(built_lib):
    import eoc_tfhe_amd
    return eoc_tfhe_amd


def shape_params(eoc, shape):
    pset, l, Bgbit = shape
    return eoc.default_params(pset) if l is None else custom(eoc, l, Bgbit, pset)


def low_part_words(l, Bgbit, seed=0):
    """uint32 [2][N]: random decomposed bits over a dropped part that cycles through 0, q/2 - 1, q/2 and q - 1 (q = 2^(32 - l Bgbit)
    in words): the two ends of the rounding cell and the two words on either side of its middle, where + h carries or does not"""
    q = 1 << (32 - l * Bgbit)
    rng = np.random.default_rng(40 + 100 * l + Bgbit + seed)
    hi = rng.integers(0, 1 << (l * Bgbit), (2, N)).astype(np.int64) << (32 - l * Bgbit)
    low = np.array([0, q // 2 - 1, q // 2, q - 1], np.int64)[(np.arange(2 * N).reshape(2, N) + seed) % 4]
    return ((hi + low) & 0xFFFFFFFF).astype(np.uint32)


def edge_differences(l, Bgbit):
    """name -> uint32 [2][N] differences D: the rows of leveled_edge_inputs (cell ends of every digit, all digits at an end, a
    lone word per polynomial, +-1), the dropped-part rows above, and every word 0xFFFFFFFF, where + h carries through every digit
    and wraps"""
    out = {}
    for name, rows in le.cmux_differences(l, Bgbit).items():
        for k in ((0, len(rows) - 1) if len(rows) > 1 else (0,)):
            out[f"{name}[{k}]"] = rows[k]
    if l * Bgbit < 32:
        out["low_parts"] = low_part_words(l, Bgbit)
        out["low_parts_shifted"] = low_part_words(l, Bgbit, seed=1)
    out["all_ones"] = np.full((2, N), 0xFFFFFFFF, np.uint32)
    return out


def inputs_for(D, rot, rng):
    """(A, B) int32 [2][N] with X^rot B - A = D: A random full-range words"""
    A = rng.integers(-2**31, 2**31, (2, N))
    B = cx.rotate(A + np.asarray(D, np.int64), (2 * N - rot) % (2 * N))
    return le._i32(A), le._i32(B)


# ---- reference identity and edge inputs ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_reference_is_the_truncating_product_of_D_plus_h_and_within_8_lsb_of_rounded_digits(eoc, shape):
    p = shape_params(eoc, shape)
    sk = eoc.SecretKey(p, 6, with_cloud_key=False)
    op = cx.orc_params(p)
    h = lr.half(p)
    assert h == 1 << (31 - p.l * p.Bgbit)
    rng = np.random.default_rng(300 + sum(x or 0 for x in shape))
    sel = sk.encrypt_selector_bits([1, 0], enc_seed=10)
    fft = cx.to_fft(sel)
    differs = 0
    for j, (name, D) in enumerate(edge_differences(p.l, p.Bgbit).items()):
        for rot in ROTS:
            k = (j + rot) & 1
            A, B = inputs_for(D, rot, rng)
            assert np.array_equal(le._i32(cx.rotate(B, rot) - A.astype(np.int64)).view(np.uint32), D), (name, rot)
            got = lr.cmux(op, fft[k], A, B, rot)
            ext = cx.extprod(op, fft[k], D.astype(np.int64) + h)
            assert np.array_equal(got, le._i32(A.astype(np.int64) + ext)), (shape, name, rot)
            exact = cx.extprod_exact(p, sel[k], D.astype(np.int64) + h)
            assert np.array_equal(exact, lr.extprod_exact(p, sel[k], D))
            assert np.abs(wrap32(ext.astype(np.int64) - exact)).max() <= 8, (shape, name, rot)
            differs += not np.array_equal(got, cx.cmux(op, fft[k], A, B, rot))
    assert differs                                                           # the mode is not the truncating one


def test_rounded_digits_are_the_nearest_multiple_of_q(eoc):
    """the digits cmux_oracle.extprod_exact takes from D + h are those of D rounded to the nearest multiple of q (ties up): with a
    selector whose rows are the noiseless gadget of 1 the exact product IS that multiple"""
    for l, Bgbit in ((2, 10), (3, 7), (1, 10), (4, 7)):
        p = custom(eoc, l, Bgbit)
        q = 1 << (32 - l * Bgbit)
        gadget = np.zeros((2 * l, 2, N), np.int32)
        for row in range(2 * l):
            gadget[row, row // l, 0] = le._i32(1 << (32 - (row % l + 1) * Bgbit))
        for D in (low_part_words(l, Bgbit), np.full((2, N), 0xFFFFFFFF, np.uint32)):
            want = ((D.astype(np.int64) + q // 2) // q * q) & 0xFFFFFFFF
            assert np.array_equal(lr.extprod_exact(p, gadget, D).view(np.uint32), want.astype(np.uint32)), (l, Bgbit)


def test_the_mode_changes_no_word_where_the_gadget_drops_nothing(eoc):
    p = custom(eoc, 4, 8)
    sk = eoc.SecretKey(p, 6, with_cloud_key=False)
    op = cx.orc_params(p)
    assert lr.half(p) == 0
    fft = cx.to_fft(sk.encrypt_selector_bits([1], enc_seed=12))[0]
    rng = np.random.default_rng(17)
    for name, D in edge_differences(4, 8).items():
        A, B = inputs_for(D, 1023, rng)
        assert np.array_equal(lr.cmux(op, fft, A, B, 1023), cx.cmux(op, fft, A, B, 1023)), name
    x = rng.integers(-2**31, 2**31, (2, N)).astype(np.int32)
    import table_update_oracle as tu
    assert all(np.array_equal(a, b) for a, b in zip(lr.demux(op, fft, x), tu.demux(op, fft, x)))


# ---- noise --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pset", [0, 1])
def test_rounding_cmux_noise_matches_the_model(eoc, pset):
    """the sample plan of tests/test_cmux_cpu.py's truncating measurement: 16 slots x 1 024 independent (selector, input) pairs,
    bit 1, the same key and seeds.  Variance over cmux_var within that test's 8 %; every slot's mean within 4 standard errors of
    cmux_mean(rounding=True); slot 0's mean more than 10 standard errors away from the truncating cmux_mean (the model: about
    47)."""
    p = eoc.default_params(pset)
    sk = eoc.SecretKey(p, 11, with_cloud_key=False)
    op = cx.orc_params(p)
    pairs = 1024
    rng = np.random.default_rng(200 + pset)
    sel = sk.encrypt_selector_bits(np.ones(pairs, np.uint8), enc_seed=300 + pset)
    err = np.zeros((pairs, len(SLOTS)))
    for k in range(pairs):
        A, B = (rng.integers(-2**31, 2**31, (2, N)).astype(np.int32) for _ in range(2))
        out = lr.cmux(op, cx.to_fft(sel[k]), A, B)
        err[k] = wrap32(tlwe_phase(out, sk.tlwe_key)[SLOTS] - tlwe_phase(B, sk.tlwe_key)[SLOTS]) / 2.0**32
    var = float(err.var(axis=0, ddof=1).mean())
    model = noise.cmux_var(p, sk.tlwe_key)
    se = err.std(0) / np.sqrt(pairs)
    z = (err.mean(0) - noise.cmux_mean(p, sk.tlwe_key, SLOTS, rounding=True)) / se
    z_trunc = (err[:, 0].mean() - float(noise.cmux_mean(p, sk.tlwe_key, 0))) / se[0]
    print(f"pset {pset}: var {var:.4e} model {model:.4e} ratio {var / model:.4f}; slot means z in [{z.min():.2f}, {z.max():.2f}]; "
          f"mean at slot 0 {err[:, 0].mean():.3e}, rounding model {float(noise.cmux_mean(p, sk.tlwe_key, 0, rounding=True)):.3e}, "
          f"truncating model {float(noise.cmux_mean(p, sk.tlwe_key, 0)):.3e}: {z_trunc:.1f} standard errors away; "
          f"mean over slots / truncating model at slot 0 {err.mean() / float(noise.cmux_mean(p, sk.tlwe_key, 0)):.4f}")
    assert abs(var / model - 1) < 0.08
    assert np.abs(z).max() < 4
    assert abs(z_trunc) > 10


def test_model_of_the_residual_mean(eoc):
    for pset in (0, 1):
        p = eoc.default_params(pset)
        sk = eoc.SecretKey(p, 11, with_cloud_key=False)
        trunc = noise.cmux_mean(p, sk.tlwe_key, SLOTS)
        rnd = noise.cmux_mean(p, sk.tlwe_key, SLOTS, rounding=True)
        q = 2.0 ** (-p.l * p.Bgbit)
        assert np.allclose(rnd * (q / 2), -trunc * 2.0**-33, rtol=1e-12, atol=0)    # the same polynomial, half an LSB of it
        assert not noise.cmux_mean(p, sk.tlwe_key, 0, bit=0, rounding=True)
        idx, d, lw = 0b1011011, 2, 5
        assert noise.table_read_mean(p, sk.tlwe_key, idx, d, lw, rounding=True) * (q / 2) == pytest.approx(
            -noise.table_read_mean(p, sk.tlwe_key, idx, d, lw) * 2.0**-33, rel=1e-9)
        assert noise.table_update_mean(p, sk.tlwe_key, idx, d, lw, rounding=True) * (q / 2) == pytest.approx(
            -noise.table_update_mean(p, sk.tlwe_key, idx, d, lw) * 2.0**-33, rel=1e-9)
        assert noise.automaton_mean_bound(p, sk.tlwe_key, 7, rounding=True) == pytest.approx(
            7 * 2.0**-33 * (1 + int(sk.tlwe_key.sum())))
    full = custom(eoc, 4, 8)                                                 # l Bgbit = 32: the mode is the default one
    sk = eoc.SecretKey(full, 11, with_cloud_key=False)
    assert np.array_equal(noise.cmux_mean(full, sk.tlwe_key, SLOTS, rounding=True), noise.cmux_mean(full, sk.tlwe_key, SLOTS))


# ---- budgets ------------------------------------------------------------------------------------------------------------------
def test_budgets_rise_with_the_mode(eoc):
    """from the model alone (nothing fitted, no factor asserted): key seed 1; table updates at W = 1, trivial table and value"""
    for pset in (0, 1):
        p = eoc.default_params(pset)
        sk = eoc.SecretKey(p, 1, with_cloud_key=False)
        for m in (2, 8):
            a0 = noise.automaton_budget(p, sk.lwe_key, sk.tlwe_key, m)
            a1 = noise.automaton_budget(p, sk.lwe_key, sk.tlwe_key, m, rounding=True)
            print(f"pset {pset} p = {m}: automaton_budget {a0} -> {a1} with rounding")
            assert a1 > a0
            for d in (0, 4, 12):
                u0 = noise.table_update_budget(p, sk.lwe_key, sk.tlwe_key, m, d, 0)
                u1 = noise.table_update_budget(p, sk.lwe_key, sk.tlwe_key, m, d, 0, rounding=True)
                print(f"pset {pset} p = {m} d = {d}: table_update_budget {u0} -> {u1} with rounding")
                assert u1 > u0
        # the definition, at the edge
        pr = noise.predict(p, sk.lwe_key, sk.tlwe_key)
        s = noise.automaton_budget(p, sk.lwe_key, sk.tlwe_key, 2, rounding=True)
        for steps, ok in ((s, True), (s + 1, False)):
            total = (noise.automaton_mean_bound(p, sk.tlwe_key, steps, rounding=True) + abs(pr["ks_mean"])
                     + 6.0 * np.sqrt(noise.automaton_var(p, sk.tlwe_key, [1] * steps) + pr["ks_var"]))
            assert (total <= 1.0 / 8) == ok


# ---- a composed run on the reference --------------------------------------------------------------------------------------------
LONG_SEED, LONG_LW = 1, 2


def long_run_steps(eoc):
    """S = min(2 automaton_budget(), 1 024) on Set A, a boolean at 6 sigma: twice what the truncating mode is good for"""
    p = eoc.default_params(0)
    sk = eoc.SecretKey(p, LONG_SEED, with_cloud_key=False)
    return min(2 * noise.automaton_budget(p, sk.lwe_key, sk.tlwe_key, 2), 1024)


def popcount_case(eoc, steps, enc_seed):
    """Automaton.popcount() -- one state, weight 0 under bit 0 and 1 under bit 1: both rotations of a step -- over an all-ones
    string, the worst case of the mean bound, on the parity table: slot j of the trivial final vector holds j mod 2 (of 2)"""
    p = eoc.default_params(0)
    sk = eoc.SecretKey(p, LONG_SEED, with_cloud_key=False)
    aut = eoc.Automaton.popcount()
    table = np.arange(N) % 2
    final = eoc.trivial_table(co.int_msgs(table, 2))
    bits = [1] * steps
    sel = sk.encrypt_selector_bits(bits, enc_seed=enc_seed)
    return p, sk, aut, table, final, bits, sel


def check_run(eoc, sk, p, aut, table, bits, tl, out, rounding):
    """every read slot's phase error before the key switch inside mean bound + 6 sigma of the mode's model; the key-switched
    output decodes to evaluate_plain"""
    W = 1 << LONG_LW
    want = [aut.evaluate_plain(bits, final=[np.roll(table, -w)]) for w in range(W)]
    assert want == [(len(bits) + w) % 2 for w in range(W)]
    err = wrap32(tlwe_phase(tl, sk.tlwe_key)[:W] - co.int_msgs(want, 2)) / 2.0**32
    bound = (noise.automaton_mean_bound(p, sk.tlwe_key, len(bits), rounding=rounding)
             + 6 * np.sqrt(noise.automaton_var(p, sk.tlwe_key, bits)))
    print(f"{len(bits)} steps, rounding {rounding}: |phase error| max {np.abs(err).max():.4e}, bound {bound:.4e} "
          f"(mean part {noise.automaton_mean_bound(p, sk.tlwe_key, len(bits), rounding=rounding):.4e})")
    assert np.abs(err).max() <= bound
    assert sk.decrypt_ints(out.reshape(-1, p.n + 1), 2).tolist() == want


_LONG = {}


def long_run_reference(eoc):
    """the long run on the rounding reference, computed once (tests/test_gpu_leveled_round.py compares the device's words with
    it): the case and `out` [1][1][W][n+1], `tl` [2][N]"""
    if not _LONG:
        p, sk, aut, table, final, bits, sel = popcount_case(eoc, long_run_steps(eoc), enc_seed=95)
        orc, op = ol.Oracle(0, LONG_SEED, with_bk=False), cx.orc_params(p)
        out, tl = lr.run(orc, op, aut, final, [cx.to_fft(sel)], [aut.start], LONG_LW)
        out.setflags(write=False)
        tl.setflags(write=False)
        _LONG.update(p=p, sk=sk, aut=aut, table=table, final=final, bits=bits, sel=sel, out=out, tl=tl[0, 0])
    return _LONG


def test_long_run_on_the_reference_stays_inside_the_rounding_model(eoc):
    c = long_run_reference(eoc)
    assert len(c["bits"]) == min(2 * noise.automaton_budget(c["p"], c["sk"].lwe_key, c["sk"].tlwe_key, 2), 1024) > 16
    check_run(eoc, c["sk"], c["p"], c["aut"], c["table"], c["bits"], c["tl"], c["out"], True)


def test_short_truncating_run_stays_inside_the_truncating_model(eoc):
    """the same check at 16 steps on the default mode's reference and model: it is not vacuous"""
    p, sk, aut, table, final, bits, sel = popcount_case(eoc, 16, enc_seed=96)
    orc, op = ol.Oracle(0, LONG_SEED, with_bk=False), cx.orc_params(p)
    out, tl = ao.run(orc, op, aut, final, [cx.to_fft(sel)], [aut.start], LONG_LW)
    check_run(eoc, sk, p, aut, table, bits, tl[0, 0], out, False)


# ---- the references of the twins' instance tests, ahead of the device ------------------------------------------------------------
INSTANCE_SHAPES = [(name, cfg["l"], cfg["Bgbit"]) for name, cfg in le.cmux_full_scale.items()] + [("k_cmux<4,0>", 4, 7)]


@pytest.mark.parametrize("name,l,Bgbit", INSTANCE_SHAPES, ids=[f"{n}@({l},{b})" for n, l, b in INSTANCE_SHAPES])
def test_instance_references_keep_the_contract_and_the_shifted_row_identities(eoc, name, l, Bgbit):
    """what tests/test_gpu_leveled_round_instances.py sends to the MI355X at this shape, on the reference alone: every
    computation under test_gpu_br_instances.reference (recorded maximum below 2^51, asserted there), the full-scale ones in the
    instance's [lo, hi) (asserted in tests/leveled_round_cases.py), and the rounding reference of a row less h equal to the
    TRUNCATING reference of the row: the identity the device test uses as its second route"""
    import leveled_round_cases as lrc
    from test_gpu_br_instances import custom_params, reference
    from test_gpu_cmux_instances import pool_map
    p = custom_params(eoc, l, Bgbit, 16)
    op = cx.orc_params(p)
    h = lr.half(p)
    assert h == lrc.half(l, Bgbit) == ((1 << (31 - l * Bgbit)) if l * Bgbit < 32 else 0)
    tag = lrc.tag_of(name, l, Bgbit)
    sk = eoc.SecretKey(p, 83, with_cloud_key=False)
    fft = cx.to_fft(sk.encrypt_selector_bits([0, 1], enc_seed=5))

    # the CMux: in1 - h
    names, in0, in1, items_t = lrc.cmux_rows(l, Bgbit)
    assert len(in0) == 2 * len(names) and items_t == 2 * sum(len(a) for a, _ in le.cmux_inputs(l, Bgbit).values())
    want_t = lrc.cmux_truncating(tag, op, fft, in0, in1, items_t)
    want_r = lrc.cmux_rounding(tag, op, fft, in0, in1)
    assert (not np.array_equal(want_r[:items_t], want_t)) == (h != 0)
    shifted = lrc.minus(in1[:items_t], h)
    got = reference(("rcmux", tag, "shifted"),
                    lambda: np.stack(pool_map(lambda k: lr.cmux(op, fft[k % 2], in0[k], shifted[k]), items_t)))
    assert np.array_equal(got, want_t)

    # the demultiplexer: x - h
    names, x, items_t = lrc.demux_rows(l, Bgbit)
    want_t = lrc.demux_truncating(tag, op, fft, x, items_t)
    want_r = lrc.demux_rounding(tag, op, fft, x)
    assert (not np.array_equal(want_r[:items_t], want_t)) == (h != 0)
    shifted = lrc.minus(x[:items_t], h)
    got = reference(("rdemux", tag, "shifted"),
                    lambda: np.stack(pool_map(lambda k: np.stack(lr.demux(op, fft[k % 2], shifted[k])), items_t)))
    assert np.array_equal(got[:, 1], want_t[:, 1]) and np.array_equal(got[:, 0], lrc.minus(want_t[:, 0], h))

    # the step: its rows and, at the instance's own shape, the three full-scale references
    vectors = lrc.step_vectors(l, Bgbit)
    cut, want_of = lrc.step_edges(tag, op, fft, vectors)
    states = len(vectors[0][2])
    assert want_of(2, 1, states).shape == (states, 2, N)
    if tag == name:
        kfft = cx.to_fft(le.constant_selector(l, le.cmux_full_scale[name]["K"])[None])[0]
        assert lrc.cmux_full_scale(name, op, kfft, l, Bgbit)[2].shape == (2, 2, N)
        assert lrc.demux_full_scale(name, op, kfft, l, Bgbit)[1].shape == (2, 2, 2, N)
        assert lrc.step_full_scale(name, op, kfft, l, Bgbit)[3].shape == (4, 2, N)


# ---- API ----------------------------------------------------------------------------------------------------------------------
def test_symbols_and_wrappers(eoc):
    L = eoc.lib()
    new = {"eoc_engine_set_leveled_rounding", "eoc_engine_leveled_rounding", "eoc_global_set_leveled_rounding"}
    assert new <= set(eoc.abi_symbols()) and all(hasattr(L, s) for s in new)
    assert isinstance(eoc.Engine.leveled_rounding, property) and eoc.Engine.leveled_rounding.fset is not None
    assert callable(eoc.set_leveled_rounding)


# The ladder of tests/test_host_entry_ladder_cpu.py for the new entries: one fresh child process with no key and no engine; which
# code each call gets, in this order, and the text eoc_last_error holds behind a failure.
CHILD = textwrap.dedent("""
    import json, sys
    sys.path.insert(0, %r)
    import numpy as np
    import eoc_tfhe_amd as eoc
    L = eoc.lib()
    x = np.zeros(8, np.int32)
    t = x.ctypes.data                               # never followed: `on` is checked before the engine is touched
    calls = [("eoc_engine_leveled_rounding", (None,)),
             ("eoc_engine_set_leveled_rounding", (None, 1)),
             ("eoc_engine_set_leveled_rounding", (t, 2)),
             ("eoc_engine_set_leveled_rounding", (t, -1)),
             ("eoc_global_set_leveled_rounding", (2,)),
             ("eoc_global_set_leveled_rounding", (-1,)),
             ("eoc_global_set_leveled_rounding", (1,)),     # no engine yet: remembered for the engines to come
             ("eoc_table_read", (t, 0, 10, t, 1, t)),       # ... and the leveled entries still ask for one
             ("eoc_global_set_leveled_rounding", (0,))]
    out = []
    for name, args in calls:
        rc = getattr(L, name)(*args)
        out.append([name, rc, L.eoc_last_error().decode() if rc else None])
    print("RESULT" + json.dumps(out))
""") % ROOT

OK, ERR_ARG, ERR_NO_DEVICE = 0, -1, -2
EXPECTED = [
    ("eoc_engine_leveled_rounding", 0, None),
    ("eoc_engine_set_leveled_rounding", ERR_ARG, "eoc_engine_set_leveled_rounding: null engine"),
    ("eoc_engine_set_leveled_rounding", ERR_ARG, "eoc_engine_set_leveled_rounding: on = 2 is neither 0 nor 1"),
    ("eoc_engine_set_leveled_rounding", ERR_ARG, "eoc_engine_set_leveled_rounding: on = -1 is neither 0 nor 1"),
    ("eoc_global_set_leveled_rounding", ERR_ARG, "eoc_global_set_leveled_rounding: on = 2 is neither 0 nor 1"),
    ("eoc_global_set_leveled_rounding", ERR_ARG, "eoc_global_set_leveled_rounding: on = -1 is neither 0 nor 1"),
    ("eoc_global_set_leveled_rounding", OK, None),
    ("eoc_table_read", ERR_NO_DEVICE, "eoc_table_read: no GPU engine (eoc_gpu_init not called or failed); there is no CPU fallback"),
    ("eoc_global_set_leveled_rounding", OK, None),
]


@pytest.fixture(scope="module")
def ladder(built_lib):
    r = subprocess.run([sys.executable, "-c", CHILD], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT")][-1]
    return [tuple(x) for x in json.loads(line[len("RESULT"):])]


@pytest.mark.parametrize("k", range(len(EXPECTED)))
def test_entry_ladder(ladder, k):
    print(ladder[k])
    assert ladder[k] == EXPECTED[k]
