"""Every blind-rotation kernel instance blind_rotate_kernel() (engine.hip) can dispatch, on the MI355X, with the edge inputs
of tests/br_edge_inputs.py: six pair shapes, the two gadget-length-2 pair shapes in their earlier form (k_br_lds*) and two
wide shapes, each as gate / _tv / many-LUT kernel, each with the rotation amounts read back by vector loads (vabar) or by
scalar loads (sabar, EOC_TFHE_SCALAR_ABAR=1): 60 instances, one test id each, named after the kernel.

An instance runs on a real key at n = 1 -- the rotation sweep: every amount in [0, 2N) as abar and as barb, from both ends
of its rounding cell -- and at n = 2 -- 256 two-step rows over the borrow edges and switch cases, so that the second step
decomposes a full accumulator in both polynomials -- and is compared with the composed CPU oracle word for word.  Nothing is
decrypted: exotic shapes are noisy, and parity does not depend on the noise.

The conversion contract (include/eoc_tfhe_gpu.h): the kernels convert like Torus32(int64(v)) for |v| < 2^51.  Every
(l, Bgbit) below except Set A's (2, 10) has l Bg < 1024, where the exact bound l Bg 2^41 keeps ANY input inside the contract
(tests/test_gpu_parity.py::test_conversion_contract_pinned_around_2_pow_51), so the extreme test polynomials are fair inputs
there; on (2, 10) the bound is 2^52 and the contract holds with overwhelming probability on real keys -- the
oracle's recorded maximum is asserted below 2^51 for every reference computed here.  The contract's top binade INSIDE the
step loop is the full-scale case at the end of this file (crafted keys).

The oracle side is Python around ctypes calls, shared between the instances of one (l, Bgbit) and family and run through 16
threads.  The gate family compares all 8 192 sweep rows.  The _tv and many-LUT (T = 2) families run all sweep rows on the
device and compare the fixed half br_edge_inputs.sweep_subset picks -- every abar and every barb of the grid once, even
amounts by their smallest word and odd ones by their largest (4 096 and 2 048 rows per polynomial); T = 8 compares its whole
sweep (1 024 rows).  Host side of the inputs: tests/test_br_edge_inputs_cpu.py."""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import br_edge_inputs as bei
import lut_many_oracle as lmo
import lut_oracle as lo
import oracle_lib as ol
from gpu_util import dev_empty, sync, to_dev, torch_cuda

pytestmark = pytest.mark.gpu
N = 1024
ENV_KNOBS = ("EOC_TFHE_BR_WIDE", "EOC_TFHE_BR_TABLES_LDS", "EOC_TFHE_SCALAR_ABAR", "EOC_TFHE_BR_SLICE", "EOC_TFHE_BR_PARTS",
             "EOC_TFHE_SLICE_SAMPLES")

# shape -> (template arguments in the kernel's name, (l, Bgbit), environment at engine creation)
SHAPES = {
    "pair<2,10>": ("2,10", (2, 10), {"EOC_TFHE_BR_WIDE": "0"}),
    "pair<2,0>": ("2,0", (2, 8), {"EOC_TFHE_BR_WIDE": "0"}),
    "pair<3,7>": ("3,7", (3, 7), {}),
    "pair<3,0>": ("3,0", (3, 6), {}),
    "pair<1,0>": ("1,0", (1, 9), {}),
    "pair<4,0>": ("4,0", (4, 6), {}),
    "lds<2,10>": ("2,10", (2, 10), {"EOC_TFHE_BR_TABLES_LDS": "1", "EOC_TFHE_BR_WIDE": "0"}),
    "lds<2,0>": ("2,0", (2, 8), {"EOC_TFHE_BR_TABLES_LDS": "1", "EOC_TFHE_BR_WIDE": "0"}),
    "wide<10>": ("10", (2, 10), {"EOC_TFHE_BR_WIDE": "1"}),
    "wide<0>": ("0", (2, 8), {"EOC_TFHE_BR_WIDE": "1"}),
}
STEMS = {
    "pair": dict(gate="k_blind_rotate", tv="k_blind_rotate_tv", many="k_lut_many"),
    "lds": dict(gate="k_br_lds", tv="k_br_lds_tv", many="k_br_lds_many"),
    "wide": dict(gate="k_blind_rotate_wide", tv="k_blind_rotate_wide_tv", many="k_lut_many_wide"),
}
INSTANCES = [(shape, family, readback) for shape in SHAPES for family in ("gate", "tv", "many") for readback in ("vabar", "sabar")]


def kernel_name(shape, family, readback):
    return f"{STEMS[shape.split('<')[0]][family]}<{SHAPES[shape][0]},{readback}>"


@pytest.fixture(scope="module")
def eoc(built_lib):
    torch_cuda()
    import eoc_tfhe_amd
    return eoc_tfhe_amd


def custom_oracle(l, Bgbit, n, seed):
    orc = ol.Oracle(0, seed, n_override=n, with_bk=False)
    orc.p.l, orc.p.Bgbit = l, Bgbit
    orc.l, orc.kpl = l, 2 * l
    orc.gen_cloud()
    return orc


def custom_params(eoc, l, Bgbit, n):
    p = eoc.default_params(0)
    p.n, p.l, p.Bgbit = n, l, Bgbit
    return p


_KEYS, _REF = {}, {}


def keys(eoc, l, Bgbit, n):
    """a real key of SecretKey(p, seed) and the oracle with the same overrides, shared by the instances of (l, Bgbit)"""
    k = (l, Bgbit, n)
    if k not in _KEYS:
        p = custom_params(eoc, l, Bgbit, n)
        _KEYS[k] = (p, eoc.SecretKey(p, 83), custom_oracle(l, Bgbit, n, 83))
    return _KEYS[k]


def pool_chunks(fn, count, threads=16):
    """fn(r0, r1) over `threads` consecutive ranges of [0, count), concatenated (ctypes drops the GIL inside the oracle)"""
    cuts = np.linspace(0, count, threads + 1).astype(int)
    with ThreadPoolExecutor(threads) as ex:
        return np.concatenate(list(ex.map(lambda k: fn(cuts[k], cuts[k + 1]), [k for k in range(threads) if cuts[k] < cuts[k + 1]])))


def reference(key, compute):
    """computed once per (l, Bgbit, n, family ...), shared by the instances that need it, never written to; every
    conversion of the computation stayed inside the contract"""
    if key not in _REF:
        L = ol.lib()
        L.orc_dbg_max_conv(1)
        want = compute()
        assert L.orc_dbg_max_conv(0) < 2.0**51, key
        want.setflags(write=False)
        _REF[key] = want
    return _REF[key]


def engine(eoc, monkeypatch, p, env, readback):
    for k in ENV_KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)                              # read at engine creation
    if readback == "sabar":
        monkeypatch.setenv("EOC_TFHE_SCALAR_ABAR", "1")
    return eoc.Engine(p)


def gate_rows(n):
    return bei.sweep(1)[0] if n == 1 else bei.two_step_rows(1)[0]


def lut_polys(eoc, l, Bgbit, n, T):
    """the test polynomials of an instance: one real table (packed for T > 1) and the extreme ones -- at n = 1 the
    alternating INT32_MIN / INT32_MAX polynomial (the sign wrap of X^(2N - barb) on words that are their own negation or
    one off it), at n = 2 all four"""
    p = 16 // max(T, 2)
    if T == 1:
        real = eoc.lut_test_polynomial(p, lo.int_table(lambda m: (3 * m + 1) % p, p, p))
    else:
        real = eoc.lut_many_test_polynomial(p, [lo.int_table(lambda m, j=j: ((2 * j + 1) * m + j) % p, p, p) for j in range(T)])
    ext = bei.extreme_polys(l, Bgbit)
    names = ("alternating",) if n == 1 else ("zero", "alternating", "digits_min", "digits_max")
    return np.ascontiguousarray(np.stack([real] + [ext[k] for k in names]).astype(np.int32))


def lut_rows(n, T):
    """(device rows, indices of the rows compared with the oracle)"""
    if n == 2:
        rows = bei.two_step_rows(T)[0]
        return rows, np.arange(rows.shape[0])
    rows = bei.sweep(T)[0]
    return rows, (bei.sweep_subset(T) if T < 8 else np.arange(rows.shape[0]))


def run_gate(eng, rows):
    d_t = to_dev(rows)
    d_u = dev_empty((rows.shape[0], N + 1), torch_cuda().int32)
    eng.blind_rotate_device(d_t.data_ptr(), d_u.data_ptr(), rows.shape[0])
    sync()
    return d_u.cpu().numpy()


def run_lut(eng, T, tvs, rows):
    torch = torch_cuda()
    d_tv, d_in = to_dev(tvs), to_dev(rows)
    if T == 1:
        d_out = dev_empty((tvs.shape[0], rows.shape[0], rows.shape[1]), torch.int32)
        eng.lut_batch_device(d_tv.data_ptr(), tvs.shape[0], d_in.data_ptr(), d_out.data_ptr(), rows.shape[0])
    else:
        d_out = dev_empty((tvs.shape[0], T, rows.shape[0], rows.shape[1]), torch.int32)
        eng.lut_many_batch_device(T, d_tv.data_ptr(), tvs.shape[0], d_in.data_ptr(), d_out.data_ptr(), rows.shape[0])
    sync()
    return d_out.cpu().numpy()


def oracle_gate(orc, rows):
    return pool_chunks(lambda r0, r1: np.stack([orc.blind_rotate_extract(r) for r in rows[r0:r1]]), rows.shape[0])


def oracle_lut(orc, T, tvs, rows):
    """lut_oracle.lut_batch (T = 1: [tv][rows][n+1]) / lut_many_oracle.lut_many_batch ([tv][T][rows][n+1]) for thousands of
    rows: the same composition -- mod switch on the grid of T, ACC = (0, X^(2N - barb) tv), orc_blind_rotate_step per
    non-zero amount, extraction at 0 .. T - 1, orc_keyswitch -- with the numpy parts done for all rows at once, so that a
    thread's loop is ctypes calls only.  The first and last rows are checked against those two functions themselves."""
    L, p, n = orc.L, orc.p, orc.n
    R, G = rows.shape[0], tvs.shape[0]
    bar = lmo.modswitch_coarse(rows, T)
    rot = (2 * N - bar[:, n].astype(np.int64)) & (2 * N - 1)
    idx = (np.arange(N)[None, :] - rot[:, None]) & (2 * N - 1)
    step = orc.kpl * 2 * N * 8
    base = orc.bkfft.ctypes.data
    out = np.zeros((G, T, R, n + 1), np.int32)

    def chunk(g, r0, r1):
        tv = tvs[g].astype(np.int64)
        acc = np.zeros((r1 - r0, 2 * N), np.int32)
        acc[:, N:] = (np.concatenate([tv, -tv])[idx[r0:r1]] & 0xFFFFFFFF).astype(np.uint32).view(np.int32)
        for k, r in enumerate(range(r0, r1)):
            for i in range(n):
                if bar[r, i]:
                    L.orc_blind_rotate_step(C.byref(p), C.c_void_p(base + i * step), None, int(bar[r, i]), acc[k], 1)
        a = acc[:, :N].astype(np.int64)
        ext = np.concatenate([a, -a], axis=1)
        u = np.zeros((r1 - r0, N + 1), np.int32)
        for j in range(T):
            u[:, :N] = (ext[:, (2 * N + j - np.arange(N)) & (2 * N - 1)] & 0xFFFFFFFF).astype(np.uint32).view(np.int32)
            u[:, N] = acc[:, N + j]
            for k in range(r1 - r0):
                out[g, j, r0 + k] = orc.keyswitch(u[k])
        return np.zeros(1)

    for g in range(G):
        pool_chunks(lambda r0, r1, g=g: chunk(g, r0, r1), R)
    few = np.r_[0:2, R - 1]
    if T == 1:
        assert np.array_equal(out[:, 0][:, few], lo.lut_batch(orc, tvs, rows[few]))
        return np.ascontiguousarray(out[:, 0])
    assert np.array_equal(out[:, :, few], lmo.lut_many_batch(orc, tvs, rows[few], T))
    return out


@pytest.mark.parametrize("shape,family,readback", INSTANCES, ids=[kernel_name(*i) for i in INSTANCES])
def test_instance_bit_exact_on_edge_inputs(eoc, monkeypatch, shape, family, readback):
    _, (l, Bgbit), env = SHAPES[shape]
    wide = shape.startswith("wide")
    for n in (1, 2):
        p, sk, orc = keys(eoc, l, Bgbit, n)
        assert np.array_equal(sk.bk, orc.bk) and np.array_equal(sk.ksk, orc.ksk)
        eng = engine(eoc, monkeypatch, p, env, readback)
        eng.load_cloud_key(sk)
        checks = []                                           # (what, device words, oracle words)
        before = eng.stats()
        if family == "gate":
            rows = gate_rows(n)
            got = run_gate(eng, rows)
            want = reference((l, Bgbit, n, "gate"), lambda: oracle_gate(orc, rows))
            checks.append(("gate", got, want))
        else:
            for T in ((1,) if family == "tv" else (2, 8)):
                tvs = lut_polys(eoc, l, Bgbit, n, T)
                rows, pick = lut_rows(n, T)
                got = run_lut(eng, T, tvs, rows)
                want = reference((l, Bgbit, n, family, T), lambda: oracle_lut(orc, T, tvs, rows[pick]))
                checks.append((f"T={T}", got[..., pick, :], want))
        st = eng.stats()
        eng.close()
        assert st["br_launches"] > before["br_launches"]
        moved = st["br_wide_launches"] - before["br_wide_launches"]
        assert (moved == st["br_launches"] - before["br_launches"]) if wide else (moved == 0), (shape, st, before)
        for what, got, want in checks:
            assert got.shape == want.shape
            bad = np.argwhere((got != want).any(axis=-1))
            assert bad.size == 0, (kernel_name(shape, family, readback), n, what, len(bad), bad[:8].tolist())


# -- full-scale operands inside the step loop ----------------------------------------------------------------------------
FULL_SCALE_ENV = {"pair<3,7>": {}, "pair<4,0>": {}, "pair<1,0>": {},
                  "lds<2,0>": SHAPES["lds<2,0>"][2], "wide<0>": SHAPES["wide<0>"][2]}


@pytest.mark.parametrize("shape", list(bei.FULL_SCALE), ids=[kernel_name(s, "tv", "vabar") for s in bei.FULL_SCALE])
def test_full_scale_operands_in_the_step_loop(eoc, monkeypatch, shape):
    """The conversion contract |v| < 2^51 inside a step loop, not only on the debug kernel k_fft_inv_polys: a crafted
    bootstrapping key (every word one constant K; a real key-switch key) and the all-digits -Bg/2 and all-digits Bg/2 - 1
    test polynomials at n = 2, abar in {1024, 1, 2047}, put the external products of both steps at the top of what the shape
    can reach -- [2^50, 2^51) for the run-time-base shapes, 1.5 x 2^48 for <3,7> and 1.5 x 2^49 for <4,0>, which cannot get
    further (br_edge_inputs.FULL_SCALE; the interval is asserted on the oracle's recorded maximum here and in
    tests/test_br_edge_inputs_cpu.py).  At 2^50 one ulp is half an output LSB: any difference in operation order or FMA
    contraction between a kernel instance and the oracle changes output words.  GPU == oracle, word for word."""
    cfg = bei.FULL_SCALE[shape]
    l, Bgbit = cfg["l"], cfg["Bgbit"]
    orc = custom_oracle(l, Bgbit, 2, 61)
    orc.bk[:] = cfg["K"]
    orc.L.orc_bk_to_fft(C.byref(orc.p), orc.bk, orc.bkfft)
    ext = bei.extreme_polys(l, Bgbit)
    tvs = np.ascontiguousarray(np.stack([ext["digits_min"], ext["digits_max"]]))
    rows = bei.full_scale_rows()
    orc.L.orc_dbg_max_conv(1)
    want = lo.lut_batch(orc, tvs, rows)
    mx = orc.L.orc_dbg_max_conv(0)
    assert cfg["lo"] <= mx < cfg["hi"] and mx < 2.0**51, (shape, np.log2(mx))
    eng = engine(eoc, monkeypatch, custom_params(eoc, l, Bgbit, 2), FULL_SCALE_ENV[shape], "vabar")
    eng.load_cloud_key(orc.bk, orc.ksk)
    before = eng.stats()
    got = run_lut(eng, 1, tvs, rows)
    st = eng.stats()
    eng.close()
    moved = st["br_wide_launches"] - before["br_wide_launches"]
    assert st["br_launches"] > before["br_launches"] and (moved > 0) == shape.startswith("wide")
    bad = np.argwhere((got != want).any(axis=-1))
    assert bad.size == 0, (shape, len(bad), bad[:8].tolist())
