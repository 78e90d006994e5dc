"""GPU parity tests: the HIP path, called through the C ABI, against the CPU oracle on the same
seeded inputs.  Bit-exact (integer / Torus32) everywhere; spectra compare as exact binary64 values.

Run on the GPU box:  python -m pytest tests -m gpu -x -q
"""
import numpy as np
import pytest

import oracle_lib as ol
from gpu_util import br_segments, dev_empty, sync, to_dev, torch_cuda

pytestmark = pytest.mark.gpu
N = 1024


@pytest.fixture(scope="module")
def eoc(built_lib):
    torch_cuda()
    import eoc_tfhe_amd
    return eoc_tfhe_amd


class Rig:
    """Oracle keys + product keys + engine for one parameter set (optionally reduced n)."""

    def __init__(self, eoc, pset, seed, n_override=None):
        self.eoc = eoc
        self.orc = ol.Oracle(pset, seed, n_override=n_override)
        p = eoc.default_params(pset)
        if n_override is not None:
            p.n = n_override
        self.p = p
        self.sk = eoc.SecretKey(p, seed)
        self.eng = eoc.Engine(p)
        self.eng.load_cloud_key(self.sk)
        self.n = p.n

    def gate(self, op, c0, c1=None, c2=None, ops=None):
        torch = torch_cuda()
        d0 = to_dev(c0)
        d1 = None if c1 is None else to_dev(c1)
        d2 = None if c2 is None else to_dev(c2)
        out = torch.empty_like(d0)
        self.eng.gate_batch_device(op, d0.data_ptr(), None if d1 is None else d1.data_ptr(),
                                   None if d2 is None else d2.data_ptr(), out.data_ptr(), d0.shape[0], ops=ops)
        sync()
        return out.cpu().numpy()


@pytest.fixture(scope="module")
def rig_small(eoc):
    return Rig(eoc, 0, 7, n_override=24)


@pytest.fixture(scope="module")
def rig_small_b(eoc):
    return Rig(eoc, 1, 9, n_override=20)


@pytest.fixture(scope="module")
def rig_a(eoc):
    return Rig(eoc, 0, 1)


# ---------------------------------------------------------------------------------------------
def test_native_library_loaded(eoc):
    """the HIP extension is the thing under test, not a fallback"""
    import ctypes
    assert eoc.lib().eoc_device_count() >= 1
    assert isinstance(eoc.lib(), ctypes.CDLL)


def test_fft_forward_inverse_bit_exact(eoc, rig_small):
    rng = np.random.default_rng(11)
    polys = np.concatenate([
        rng.integers(-512, 512, (5, N)),
        rng.integers(-2**31, 2**31, (5, N)),
        np.zeros((1, N)), np.full((1, N), -2**31), np.full((1, N), 2**31 - 1),
    ]).astype(np.int32)
    d_p = to_dev(polys)
    d_s = dev_empty((polys.shape[0], N), torch_cuda().float64)
    rig_small.eng.fft_fwd_device(d_p.data_ptr(), d_s.data_ptr(), polys.shape[0])
    sync()
    got = d_s.cpu().numpy()
    want = np.stack([ol.fft_fwd(p) for p in polys])
    assert np.array_equal(got, want), f"max |diff| = {np.abs(got - want).max()}"
    # inverse on products of spectra (full-magnitude values)
    specs = want.view(np.complex128)
    prod = np.stack([specs[i] * specs[5 + i] for i in range(5)]).view(np.float64)
    d_in = to_dev(prod)
    d_out = dev_empty((5, N), torch_cuda().int32)
    rig_small.eng.fft_inv_device(d_in.data_ptr(), d_out.data_ptr(), 5)
    sync()
    got_i = d_out.cpu().numpy()
    want_i = np.stack([ol.fft_inv(s) for s in prod])
    assert np.array_equal(got_i, want_i)


def test_conversion_contract_pinned_around_2_pow_51(eoc, rig_small):
    """Torus32(int64(x)).  The kernel converts with two exact operations, t = trunc(x) and
    t + 1.5 * 2^52 (low dword), which IS Torus32(int64(x)) for |x| < 2^51 and is NOT beyond (the sum leaves the binade
    whose unit is 1).  This test pins both halves of that contract on the device:
      * |x| < 2^51, including values within 2^31 of the limit and non-integers of both signs: device == oracle;
      * 2^51 <= |x| < 2^52: the device returns exactly what the two-operation form computes (emulated here in numpy
        on the oracle's pre-conversion doubles) -- a defined, documented divergence from the oracle, not noise.
    Why no reachable accumulator is up there: DESIGN.md 2.1 (Set B and every shape with l * Bg < 1024: impossible by
    the exact bound 2 l N (Bg/2) 2^31 < 2^51; Set A: the exact bound is 2^52 and the probability bound is 2 e^-512)."""
    rng = np.random.default_rng(51)
    rows = []
    for scale_bits, hi in ((31, (1 << 20) - 1), (31, (1 << 21) - 1), (30.5, (1 << 20) - 1), (31.7, (1 << 19))):
        c = rng.integers(-hi, hi + 1, N).astype(np.int32)
        c[:8] = [hi, -hi, hi - 1, -(hi - 1), 1, -1, 0, hi // 2]
        rows.append(ol.fft_fwd(c) * (2.0 ** scale_bits))         # inverse transform returns ~ c * 2^scale_bits
    specs = np.stack(rows)
    raw = np.stack([ol.fft_inv_raw(s) for s in specs])           # the values the conversion is applied to
    want = np.stack([ol.fft_inv(s) for s in specs])
    d_in = to_dev(specs)
    d_out = dev_empty((specs.shape[0], N), torch_cuda().int32)
    rig_small.eng.fft_inv_device(d_in.data_ptr(), d_out.data_ptr(), specs.shape[0])
    sync()
    got = d_out.cpu().numpy()
    mag = np.abs(raw)
    low, high = mag < 2.0 ** 51, (mag >= 2.0 ** 51) & (mag < 2.0 ** 52)
    assert low.sum() > 2000 and high.sum() > 400                  # both ranges are populated ...
    assert (mag[low] > 2.0 ** 51 - 2.0 ** 32).sum() >= 4          # ... also right below the limit
    assert (raw != np.trunc(raw)).sum() > 1000                    # ... with fractional parts to truncate
    assert np.array_equal(got[low], want[low])                    # the contract
    emu = ((np.trunc(raw) + 6755399441055744.0).view(np.uint64) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)
    assert np.array_equal(got, emu)                               # the device is the two-operation form, everywhere
    assert (got[high] != want[high]).mean() > 0.5                 # and that form is not int64 conversion up there


def test_keygen_and_bkfft_parity(eoc, rig_small):
    r = rig_small
    assert np.array_equal(r.sk.lwe_key, r.orc.lwe_key)
    assert np.array_equal(r.sk.tlwe_key, r.orc.tlwe_key)
    assert np.array_equal(r.sk.bk, r.orc.bk)
    assert np.array_equal(r.sk.ksk, r.orc.ksk)
    d_bk, d_ksk = r.eng.cloud_key_device()
    got = r.eng.download(d_bk, r.eng.bkfft_bytes, np.float64).reshape(r.orc.bkfft.shape)
    assert np.array_equal(got, r.orc.bkfft * 2.0**-9)  # the image carries 1/512 (exact scaling)
    # KSK device image: [N*t][base-1][n1p], padding zero
    p = r.p
    base, n1p = 1 << p.ks_basebit, (p.n + 1 + 255) // 256 * 256
    img = r.eng.download(d_ksk, r.eng.ksk_dev_bytes, np.int32).reshape(N * p.ks_t * (base - 1), n1p)
    assert not img[:, p.n + 1:].any()
    assert np.array_equal(img[:, : p.n + 1], r.orc.ksk)


def _rand_cts(rig, count, enc_seed, first=0):
    bits = np.random.default_rng(enc_seed).integers(0, 2, count)
    return bits, rig.sk.encrypt_bits(bits, enc_seed, first)


@pytest.mark.parametrize("which", ["A", "B"])
def test_blind_rotate_and_keyswitch_small(eoc, rig_small, rig_small_b, which):
    r = rig_small if which == "A" else rig_small_b
    torch = torch_cuda()
    rng = np.random.default_rng(5)
    cnt = 7  # odd: exercises the idle wave pair
    t = rng.integers(-2**31, 2**31, (cnt, r.n + 1)).astype(np.int32)
    t[0, :] = 0          # all bara = 0 (every step skipped upstream)
    t[1, : r.n] = 0      # only barb
    d_t = to_dev(t)
    d_u = dev_empty((cnt, N + 1), torch.int32)
    r.eng.blind_rotate_device(d_t.data_ptr(), d_u.data_ptr(), cnt)
    sync()
    got = d_u.cpu().numpy()
    want = np.stack([r.orc.blind_rotate_extract(x) for x in t])
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    d_o = dev_empty((cnt, r.n + 1), torch.int32)
    r.eng.keyswitch_device(d_u.data_ptr(), d_o.data_ptr(), cnt)
    sync()
    want_ks = np.stack([r.orc.keyswitch(x) for x in want])
    assert np.array_equal(d_o.cpu().numpy(), want_ks)


@pytest.mark.parametrize("name", ["NAND", "AND", "OR", "NOR", "XOR", "XNOR", "ANDNY", "ANDYN", "ORNY", "ORYN"])
def test_gates_small_bit_exact(eoc, rig_small, name):
    r = rig_small
    b0, c0 = _rand_cts(r, 9, 21)
    b1, c1 = _rand_cts(r, 9, 22, 100)
    got = r.gate(eoc.OPS[name], c0, c1)
    want = r.orc.gate_batch(ol.OPS[name], c0, c1)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("pset,n,widths", [(0, 24, (1, 9, 130)), (1, 20, (7,)), (0, 500, (5, 1030, 2300)), (1, 630, (5, 1030))],
                         ids=["setA-small", "setB-small", "setA-full-pair-and-wide", "setB-full-two-part"])
def test_extension_gates_maj_and_xor3_bit_exact(eoc, pset, n, widths):
    """round 6: the extension gates -- EOC_MAJ (t = a + b + c: a full adder's carry) and EOC_XOR3 (t = -2 (a + b + c): its sum),
    one bootstrap each behind a three-operand linear stage (k_prepare; the folded key-switch set-up stays).  Bit for bit against
    the oracle on both kernels (1 030 rows = a full pair launch + remainder, 2 300 = a wide launch + a pair remainder), both
    parameter sets, and through the truth table on all eight input combinations; inputs that are themselves gate outputs;
    a mixed batch and a netlist that contain them.  Full Set B: 1 030 rows are two segments x two parts (accumulators
    parked in between), the second segment starting at job0 > 0; the rows on both sides of the cut are in the sample."""
    r = Rig(eoc, pset, 13, n_override=None if n in (500, 630) else n)
    full_b = pset == 1 and r.n == 630
    for cnt in widths:
        bits, cts = zip(*[_rand_cts(r, cnt, 300 + k, 40 * k) for k in range(3)])
        sample = slice(None) if r.n < 100 else np.random.default_rng(cnt).choice(cnt, min(cnt, 24), replace=False)
        if full_b:
            segs = br_segments(cnt, r.eng.resident_jobs())
            assert cnt != 1030 or len(segs) == 2, segs                     # 515 + 515 at 4 x 256 CUs
            sample = np.union1d(sample, np.concatenate([np.r_[max(0, s0 - 8):min(cnt, s0 + 8)] for s0 in segs[1:]] + [[cnt - 1]]))
        for name, truth in (("MAJ", (bits[0].astype(int) + bits[1] + bits[2]) >= 2), ("XOR3", bits[0] ^ bits[1] ^ bits[2])):
            br0 = r.eng.stats()["br_launches"]
            got = r.gate(eoc.OPS[name], cts[0], cts[1], cts[2])
            if full_b:
                assert r.eng.stats()["br_launches"] - br0 == 2 * len(segs), (name, cnt, segs)
            assert np.array_equal(r.sk.decrypt_bits(got), truth.astype(np.uint8)), (name, cnt)
            assert np.array_equal(got[sample], r.orc.gate_batch(ol.OPS[name], cts[0][sample], cts[1][sample], cts[2][sample])), (name, cnt)
    b8 = [np.array([(k >> j) & 1 for k in range(8)], np.uint8) for j in range(3)]
    c8 = [r.sk.encrypt_bits(b8[j], 900 + j, 0) for j in range(3)]
    maj, x3 = r.gate(eoc.OPS["MAJ"], *c8), r.gate(eoc.OPS["XOR3"], *c8)
    assert np.array_equal(r.sk.decrypt_bits(maj), (b8[0] + b8[1] + b8[2] >= 2)) and np.array_equal(r.sk.decrypt_bits(x3), b8[0] ^ b8[1] ^ b8[2])
    # outputs of bootstrapped gates as inputs (a carry chain step): MAJ(XOR3(a, b, c), MAJ(a, b, c), c)
    got = r.gate(eoc.OPS["MAJ"], x3, maj, c8[2])
    assert np.array_equal(got, r.orc.gate_batch(ol.OPS["MAJ"], x3, maj, c8[2]))
    ops = np.array([15, 0, 16, 10, 16, 15, 11, 4], np.uint8)
    assert np.array_equal(r.gate(0, *c8, ops=ops), r.orc.gate_batch(0, *c8, ops=ops))
    r.eng.close()


def test_mux_not_copy_small(eoc, rig_small):
    r = rig_small
    _, a = _rand_cts(r, 5, 31)
    _, b = _rand_cts(r, 5, 32, 50)
    _, c = _rand_cts(r, 5, 33, 90)
    assert np.array_equal(r.gate(eoc.OPS["MUX"], a, b, c), r.orc.gate_batch(ol.OPS["MUX"], a, b, c))
    assert np.array_equal(r.gate(eoc.OPS["NOT"], a), r.orc.gate_batch(ol.OPS["NOT"], a))
    assert np.array_equal(r.gate(eoc.OPS["COPY"], a), a)
    # bootsCONSTANT: no input (NULL), noiseless trivial sample; mixed into a batch it needs no operand either
    torch = torch_cuda()
    for name, bit in (("CONST0", 0), ("CONST1", 1)):
        out = torch.empty((5, r.p.n + 1), dtype=torch.int32, device="cuda")
        r.eng.gate_batch_device(eoc.OPS[name], None, None, None, out.data_ptr(), 5)
        sync()
        got = out.cpu().numpy()
        assert np.array_equal(got, r.orc.gate_batch(ol.OPS[name], np.zeros_like(a)))
        assert not got[:, :-1].any() and np.all(got[:, -1] == (1 << 29) * (2 * bit - 1))
        assert np.array_equal(r.sk.decrypt_bits(got), np.full(5, bit, np.uint8))
    ops = np.array([eoc.OPS["CONST1"], eoc.OPS["AND"], eoc.OPS["CONST0"], eoc.OPS["NOT"], eoc.OPS["XOR"]], np.uint8)
    assert np.array_equal(r.gate(0, a, b, None, ops=ops), r.orc.gate_batch(0, a, b, None, ops=ops))


def test_mixed_ops_small(eoc, rig_small):
    r = rig_small
    cnt = 12
    _, a = _rand_cts(r, cnt, 41)
    _, b = _rand_cts(r, cnt, 42, 50)
    _, c = _rand_cts(r, cnt, 43, 90)
    ops = np.array([0, 0, 4, 4, 4, 10, 10, 0, 11, 2, 10, 4], np.uint8)
    got = r.gate(0, a, b, c, ops=ops)
    want = r.orc.gate_batch(0, a, b, c, ops=ops)
    assert np.array_equal(got, want)


def test_full_size_set_a_truth_tables_and_parity(eoc, rig_a):
    """Set A (n=500): all four input combinations of every 2-input gate decrypt to the truth table,
    and the ciphertexts equal the oracle's bit for bit."""
    r = rig_a
    bits0 = np.array([0, 0, 1, 1]); bits1 = np.array([0, 1, 0, 1])
    c0 = r.sk.encrypt_bits(bits0, 2, 0)
    c1 = r.sk.encrypt_bits(bits1, 2, 100)
    assert np.array_equal(c0, r.orc.encrypt_bits(bits0, 2, 0))
    tt = dict(NAND=1 - (bits0 & bits1), AND=bits0 & bits1, OR=bits0 | bits1, NOR=1 - (bits0 | bits1),
              XOR=bits0 ^ bits1, XNOR=1 - (bits0 ^ bits1), ANDNY=(1 - bits0) & bits1, ANDYN=bits0 & (1 - bits1),
              ORNY=(1 - bits0) | bits1, ORYN=bits0 | (1 - bits1))
    for name, want_bits in tt.items():
        got = r.gate(eoc.OPS[name], c0, c1)
        assert np.array_equal(r.sk.decrypt_bits(got), want_bits), name
        assert np.array_equal(got, r.orc.gate_batch(ol.OPS[name], c0, c1)), name


def test_full_size_batch_parity_set_a(eoc, rig_a):
    """BASELINE config 2 at its full size: 1024 NAND gates, decrypt-checked AND compared with the oracle bit for bit
    (all 1024; the oracle runs OpenMP over the gates, about a second on the GPU box's host cores)."""
    r = rig_a
    cnt = 1024
    b0, c0 = _rand_cts(r, cnt, 2, 0)
    b1, c1 = _rand_cts(r, cnt, 3, 0)
    got = r.gate(eoc.OPS["NAND"], c0, c1)
    assert np.array_equal(r.sk.decrypt_bits(got), 1 - (b0 & b1))
    assert np.array_equal(got, r.orc.gate_batch(ol.OPS["NAND"], c0, c1))
    # determinism: same inputs, same bits
    assert np.array_equal(got, r.gate(eoc.OPS["NAND"], c0, c1))


def test_full_size_set_b_parity(eoc):
    """Set B (n=630, l=3, Bgbit=7 -- what the reference's minimum_lambda=128 selects) at the width the bench measures:
    ALL 1024 NAND gates of a batch bit-exact vs the oracle -- this is the two-part blind-rotate launch with the
    accumulators parked in d_acc_state between the parts -- plus 64 XOR and 64 MUX (two blind rotations each)."""
    r = Rig(eoc, 1, 1)
    cnt = 1024
    b0, c0 = _rand_cts(r, cnt, 52, 0)
    b1, c1 = _rand_cts(r, cnt, 53, 0)
    b2, c2 = _rand_cts(r, cnt, 54, 0)
    got = r.gate(eoc.OPS["NAND"], c0, c1)
    assert np.array_equal(r.sk.decrypt_bits(got), 1 - (b0 & b1))
    want = r.orc.gate_batch(ol.OPS["NAND"], c0, c1)
    assert np.array_equal(got, want), np.argwhere((got != want).any(axis=1))[:8]
    sl = slice(0, 64)
    assert np.array_equal(r.gate(eoc.OPS["XOR"], c0[sl], c1[sl]), r.orc.gate_batch(ol.OPS["XOR"], c0[sl], c1[sl]))
    gm = r.gate(eoc.OPS["MUX"], c0, c1, c2)
    assert np.array_equal(r.sk.decrypt_bits(gm), np.where(b0 == 1, b1, b2))
    assert np.array_equal(gm[sl], r.orc.gate_batch(ol.OPS["MUX"], c0[sl], c1[sl], c2[sl]))


def test_edge_cases_and_errors(eoc, rig_small):
    r = rig_small
    torch = torch_cuda()
    _, a = _rand_cts(r, 3, 61)
    _, b = _rand_cts(r, 3, 62)
    da, db = to_dev(a), to_dev(b)
    out = torch.zeros_like(da)
    # empty batch is a no-op
    r.eng.gate_batch_device(0, da.data_ptr(), db.data_ptr(), None, out.data_ptr(), 0)
    sync()
    assert not out.cpu().numpy().any()
    # bad opcode, missing operand
    with pytest.raises(eoc.EocError):
        r.eng.gate_batch_device(99, da.data_ptr(), db.data_ptr(), None, out.data_ptr(), 3)
    with pytest.raises(eoc.EocError):
        r.eng.gate_batch_device(eoc.OPS["MUX"], da.data_ptr(), db.data_ptr(), None, out.data_ptr(), 3)
    with pytest.raises(eoc.EocError):
        r.eng.gate_batch_device(0, da.data_ptr(), db.data_ptr(), None, out.data_ptr(), 3, ops=np.array([0, 77, 0], np.uint8))
    # an engine without a cloud key refuses to run gates
    e2 = eoc.Engine(r.p)
    with pytest.raises(eoc.EocError, match="no cloud key"):
        e2.gate_batch_device(0, da.data_ptr(), db.data_ptr(), None, out.data_ptr(), 3)
    # adopting another engine's images works (the multi-GPU hand-off path)
    kb, kk = r.eng.cloud_key_device()
    e2.set_cloud_key_device(kb, kk)
    e2.gate_batch_device(0, da.data_ptr(), db.data_ptr(), None, out.data_ptr(), 3)
    sync()
    assert np.array_equal(out.cpu().numpy(), r.orc.gate_batch(0, a, b))
    e2.close()
    # single gate, and a batch that is not a multiple of any tile size
    for cnt in (1, 67):
        _, x = _rand_cts(r, cnt, 63)
        _, y = _rand_cts(r, cnt, 64)
        assert np.array_equal(r.gate(eoc.OPS["XNOR"], x, y), r.orc.gate_batch(ol.OPS["XNOR"], x, y))


def test_properties_at_bench_size(eoc, rig_a):
    """BASELINE config 2 size (1024 gates, Set A): size-independent properties -- double negation through
    bootstrapped gates, De Morgan, XOR self-inverse -- checked by decryption on the full batch."""
    r = rig_a
    cnt = 1024
    b0, c0 = _rand_cts(r, cnt, 71)
    b1, c1 = _rand_cts(r, cnt, 72)
    nand = r.gate(eoc.OPS["NAND"], c0, c1)
    and_ = r.gate(eoc.OPS["AND"], c0, c1)
    assert np.array_equal(r.sk.decrypt_bits(r.gate(eoc.OPS["NOT"], nand)), r.sk.decrypt_bits(and_))
    nor_of_not = r.gate(eoc.OPS["NOR"], r.gate(eoc.OPS["NOT"], c0), r.gate(eoc.OPS["NOT"], c1))
    assert np.array_equal(r.sk.decrypt_bits(nor_of_not), b0 & b1)            # De Morgan
    x = r.gate(eoc.OPS["XOR"], c0, c1)
    assert np.array_equal(r.sk.decrypt_bits(r.gate(eoc.OPS["XOR"], x, c1)), b0)  # (a^b)^b = a
    # outputs of bootstrapped gates are fresh: noise stays small after three levels
    ph = np.array([r.sk.phase(v) for v in r.gate(eoc.OPS["XOR"], x, c1)[:64]]) / 2**32
    assert np.abs(np.abs(ph) - 0.125).max() < 1 / 16


def test_truth_tables_16k_random_encryptions_per_gate(eoc, rig_a):
    """every gate decrypts to its truth table over >= 10^4 random encryptions with zero
    failures; the output noise of bootstrap + key switch has the variance eoc_tfhe_amd/noise.py predicts for this key
    (the full before / after key switch anchor, means included: tests/test_gpu_noise.py)."""
    from eoc_tfhe_amd import noise
    pred = noise.predict(rig_a.p, rig_a.sk.lwe_key, rig_a.sk.tlwe_key, rig_a.sk.ksk)
    r = rig_a
    cnt = 16384
    b0, c0 = _rand_cts(r, cnt, 81)
    b1, c1 = _rand_cts(r, cnt, 82)
    b2, c2 = _rand_cts(r, cnt, 83)
    tt = dict(NAND=1 - (b0 & b1), AND=b0 & b1, OR=b0 | b1, NOR=1 - (b0 | b1), XOR=b0 ^ b1, XNOR=1 - (b0 ^ b1),
              ANDNY=(1 - b0) & b1, ANDYN=b0 & (1 - b1), ORNY=(1 - b0) | b1, ORYN=b0 | (1 - b1))
    lwe = r.sk.lwe_key.astype(np.int64)
    for name, want in tt.items():
        got = r.gate(eoc.OPS[name], c0, c1)
        assert np.array_equal(r.sk.decrypt_bits(got), want), name
        if name in ("NAND", "XOR"):
            g = got.astype(np.int64)
            phase = ((g[:, -1] - g[:, :-1] @ lwe) + 2**31) % 2**32 - 2**31
            err = (phase - np.sign(phase) * 2**29) / 2**32
            assert np.abs(err).max() < 1 / 16 and 0.8 < err.var() / pred["total_var"] < 1.25, (name, err.var(), pred)
            assert abs(err.mean() - pred["total_mean"]) < 5 * err.std() / np.sqrt(cnt), (name, err.mean(), pred)
    got = r.gate(eoc.OPS["MUX"], c0, c1, c2)
    assert np.array_equal(r.sk.decrypt_bits(got), np.where(b0 == 1, b1, b2))


@pytest.mark.parametrize("n,l,bgbit", [(1, 2, 10), (5, 1, 12), (6, 4, 6), (9, 4, 8), (300, 2, 10), (1023, 3, 7)])
def test_custom_parameter_shapes_bit_exact(eoc, n, l, bgbit):
    """every kernel instantiation (gadget lengths 1..4, run-time gadget base, key-switch widths for n up to the
    maximum 1023, the degenerate n = 1): GPU == oracle bit for bit.  Parity does not depend on the noise level,
    so exotic shapes are compared as ciphertexts, not by decryption."""
    torch = torch_cuda()
    p = eoc.default_params(0)
    p.n, p.l, p.Bgbit = n, l, bgbit
    sk = eoc.SecretKey(p, 77)
    eng = eoc.Engine(p)
    eng.load_cloud_key(sk)
    orc = ol.Oracle(0, 77, n_override=n, with_bk=False)
    orc.p.l, orc.p.Bgbit = l, bgbit
    orc.l, orc.kpl = l, 2 * l
    orc.gen_cloud()
    assert np.array_equal(sk.bk, orc.bk) and np.array_equal(sk.ksk, orc.ksk)
    cnt = 5
    rng = np.random.default_rng(n)
    c = [sk.encrypt_bits(rng.integers(0, 2, cnt), 90 + k, 0) for k in range(3)]
    d = [to_dev(x) for x in c]
    out = torch.empty_like(d[0])
    for name in ("NAND", "XOR", "MUX"):
        eng.gate_batch_device(eoc.OPS[name], d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), out.data_ptr(), cnt)
        sync()
        want = orc.gate_batch(ol.OPS[name], c[0], c[1], c[2] if name == "MUX" else None)
        assert np.array_equal(out.cpu().numpy(), want), (name, n, l, bgbit)
    eng.close()


@pytest.mark.parametrize("ks_t,ks_basebit,n", [(4, 3, 8), (5, 1, 11), (3, 4, 300), (10, 3, 17)])
def test_other_keyswitch_shapes(eoc, ks_t, ks_basebit, n):
    """the tiled key-switch kernels exist for basebit = 2, t = 8 (both reference sets); every other (basebit <= 4, t)
    takes the plain one-thread-per-word kernel (round 2 refused them) -- NAND, MUX and the stand-alone key switch
    against the oracle"""
    torch = torch_cuda()
    p = eoc.default_params(0)
    p.n, p.ks_t, p.ks_basebit = n, ks_t, ks_basebit
    sk = eoc.SecretKey(p, 3)
    orc = ol.Oracle(0, 3, n_override=n)
    orc.p.ks_t, orc.p.ks_basebit = ks_t, ks_basebit
    orc.gen_cloud()
    assert np.array_equal(sk.ksk, orc.ksk)
    eng = eoc.Engine(p)
    eng.load_cloud_key(sk)
    cnt = 9
    rng = np.random.default_rng(5)
    c = [sk.encrypt_bits(rng.integers(0, 2, cnt), 70 + k, 0) for k in range(3)]
    d = [to_dev(x) for x in c]
    out = torch.empty_like(d[0])
    for name in ("NAND", "MUX"):
        eng.gate_batch_device(eoc.OPS[name], d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), out.data_ptr(), cnt)
        sync()
        assert np.array_equal(out.cpu().numpy(), orc.gate_batch(ol.OPS[name], c[0], c[1], c[2] if name == "MUX" else None)), name
    u = rng.integers(-2**31, 2**31, (cnt, N + 1)).astype(np.int32)
    d_o = dev_empty((cnt, n + 1), torch.int32)
    eng.keyswitch_device(to_dev(u).data_ptr(), d_o.data_ptr(), cnt)
    sync()
    assert np.array_equal(d_o.cpu().numpy(), np.stack([orc.keyswitch(x) for x in u]))
    eng.close()


def test_mixed_ops_arbitrary_order_large(eoc, rig_small):
    """BASELINE config 4's op stream is uniform over {NAND, XOR, MUX} in ARBITRARY order: the engine sorts by
    opcode on the device (gather, per-opcode runs, scatter); results equal the oracle gate by gate"""
    r = rig_small
    cnt = 300
    rng = np.random.default_rng(44)
    ops = rng.choice(np.array([eoc.OPS[k] for k in ("NAND", "XOR", "MUX", "NOT", "ORYN", "COPY")], np.uint8), cnt)
    _, a = _rand_cts(r, cnt, 45)
    _, b = _rand_cts(r, cnt, 46)
    _, c = _rand_cts(r, cnt, 47)
    got = r.gate(0, a, b, c, ops=ops)
    want = r.orc.gate_batch(0, a, b, c, ops=ops)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("no_fold", [False, True], ids=["folded", "unfolded"])
def test_mixed_all_opcodes_run_as_one_level(eoc, no_fold, monkeypatch):
    """A mixed batch over ALL seventeen opcodes (the extension gates MAJ and XOR3 are groups of their own) in arbitrary order: the ten two-input opcodes differ only in their linear
    stage and form ONE group (one descriptor, the row's opcode read per job: OP_MULTI) instead of one partly filled
    launch per opcode; the MUX run is a second group; both share ONE blind rotation over the concatenated jobs (round 6:
    one pool per call -- one partly filled last launch instead of two); NOT / COPY / CONSTANT take no bootstrap.  Row for
    row against the oracle, with the separate k_prepare / k_ks_init launches too (EOC_TFHE_NO_FOLD), by the engine's
    level counter and by its blind-rotate spans (HIP-event pairs, one per launch_blind_rotate call)."""
    if no_fold:
        monkeypatch.setenv("EOC_TFHE_NO_FOLD", "1")
    r = Rig(eoc, 0, 7, n_override=31)
    cnt = 700
    rng = np.random.default_rng(144)
    ops = rng.integers(0, 17, cnt).astype(np.uint8)
    assert len(set(ops.tolist())) == 17
    _, a = _rand_cts(r, cnt, 145)
    _, b = _rand_cts(r, cnt, 146)
    _, c = _rand_cts(r, cnt, 147)
    want = r.orc.gate_batch(0, a, b, c, ops=ops)
    r.gate(0, a, b, c, ops=ops)                                        # workspace growth outside the counted call
    r.eng.set_profiling(True)
    r.eng.kernel_times(reset=True)
    before = r.eng.stats()
    got = r.gate(0, a, b, c, ops=ops)
    after = r.eng.stats()
    kt = r.eng.kernel_times(reset=True)
    r.eng.set_profiling(False)
    assert np.array_equal(got, want)
    assert after["batches"] - before["batches"] == 1                  # the two-input block and the MUX run: one pool
    assert kt["blind_rotate"]["launches"] == 1, kt                    # ONE blind-rotate span for the whole mixed call
    assert kt["keyswitch"]["launches"] == 4, kt                       # a key switch per group: two-input, MUX, MAJ, XOR3
    n_mux = int((ops == eoc.OPS["MUX"]).sum())
    assert after["bootstraps"] - before["bootstraps"] == int((ops < 10).sum()) + 2 * n_mux + int((ops >= 15).sum())
    # few runs (no gather): every bootstrapped run is a group of the same pool -- NAND run, MUX run, XOR run, free run
    ops3 = np.concatenate([np.full(200, 0), np.full(150, 10), np.full(250, 4), np.full(100, 11)]).astype(np.uint8)
    r.eng.set_profiling(True)
    r.eng.kernel_times(reset=True)
    got3 = r.gate(0, a, b, c, ops=ops3)
    kt3 = r.eng.kernel_times(reset=True)
    r.eng.set_profiling(False)
    assert np.array_equal(got3, r.orc.gate_batch(0, a, b, c, ops=ops3))
    assert kt3["blind_rotate"]["launches"] == 1 and kt3["keyswitch"]["launches"] == 3, kt3
    # a batch with a single two-input opcode among free gates keeps its plain descriptor (and the folded single-level path)
    ops2 = np.where(ops < 10, 4, np.where((ops == 10) | (ops >= 15), 11, ops)).astype(np.uint8)
    assert np.array_equal(r.gate(0, a, b, c, ops=ops2), r.orc.gate_batch(0, a, b, c, ops=ops2))
    # in place (out = in0) through the pool: rows are independent, every group reads its rows before any group writes
    da, db, dc = to_dev(a), to_dev(b), to_dev(c)
    r.eng.gate_batch_device(0, da.data_ptr(), db.data_ptr(), dc.data_ptr(), da.data_ptr(), cnt, ops=ops3)
    sync()
    assert np.array_equal(da.cpu().numpy(), r.orc.gate_batch(0, a, b, c, ops=ops3))
    r.eng.close()


def _truth(ops, x, y, z):
    """plaintext of every opcode (OPS numbering) on bits x, y, z"""
    tt = [1 - (x & y), x & y, x | y, 1 - (x | y), x ^ y, 1 - (x ^ y), (1 - x) & y, x & (1 - y), (1 - x) | y, x | (1 - y),
          np.where(x == 1, y, z), 1 - x, x, 0 * x, 0 * x + 1, (x + y + z >= 2).astype(x.dtype), x ^ y ^ z]
    return np.choose(ops, tt).astype(np.uint8)


def _pool_job_rows(ops, gather):
    """the caller's row behind every job of a mixed batch's pooled blind rotation, in job order: with the gather (opcode-
    sorted, stable) the two-input block (OP_MULTI), then the MUX, MAJ and XOR3 runs; without it the bootstrapped runs in
    the caller's order.  A MUX row owns two jobs: its run's k-th row is job k and job m + k of that run."""
    order = np.argsort(ops, kind="stable") if gather else np.arange(len(ops))
    o = ops[order]
    cut = np.flatnonzero(np.diff(o)) + 1
    groups = [g for g in np.split(order, cut) if ops[g[0]] == 10 or ops[g[0]] < 10 or ops[g[0]] >= 15]
    if gather:
        two = [g for g in groups if ops[g[0]] < 10]
        groups = [np.concatenate(two)] + [g for g in groups if ops[g[0]] >= 10]
    return np.concatenate([np.concatenate([g, g]) if ops[g[0]] == 10 else g for g in groups])


def _gate_on(eng, a, b, c, ops, out_alias=False):
    """a mixed batch on engine `eng`; out_alias: in place (out = in0)"""
    torch = torch_cuda()
    da, db, dc = to_dev(a), to_dev(b), to_dev(c)
    out = da if out_alias else torch.empty_like(da)
    eng.gate_batch_device(0, da.data_ptr(), db.data_ptr(), dc.data_ptr(), out.data_ptr(), len(ops), ops=ops)
    sync()
    return out.cpu().numpy()


def test_mixed_all_opcodes_set_b_full(eoc, monkeypatch):
    """Set B at n = 630: a 4 096-row mixed batch over all seventeen opcodes in random order takes the gather path
    (k_gather_rows at stride 631, the opcode in the permutation's top four bits) and ONE pool (run_pool: OP_MULTI, MUX, MAJ and
    XOR3 groups, a k_prepare and a key switch per group) whose blind rotation is cut into several segments of two launches
    each; every row decrypts, a slice -- every segment boundary on both sides included -- equals the oracle, and the same
    inputs with every group as a level of its own (EOC_TFHE_NO_POOL) give the same bytes on all 4 096 rows.  Then a few-runs
    batch (no gather) of 1 500 rows, out of place and in place."""
    r = Rig(eoc, 1, 21)
    assert (r.n, r.p.l) == (630, 3)
    R = r.eng.resident_jobs()
    cnt = 4096
    rng = np.random.default_rng(1630)
    ops = rng.integers(0, 17, cnt).astype(np.uint8)
    assert len(set(ops.tolist())) == 17
    x, a = _rand_cts(r, cnt, 161)
    y, b = _rand_cts(r, cnt, 162)
    z, c = _rand_cts(r, cnt, 163)
    _gate_on(r.eng, a, b, c, ops)                                       # workspace growth outside the counted call
    r.eng.set_profiling(True)
    r.eng.kernel_times(reset=True)
    before = r.eng.stats()
    got = _gate_on(r.eng, a, b, c, ops)
    after = r.eng.stats()
    kt = r.eng.kernel_times(reset=True)
    r.eng.set_profiling(False)
    n_two, n_mux, n_lin3 = int((ops < 10).sum()), int((ops == 10).sum()), int((ops >= 15).sum())
    jobs = n_two + 2 * n_mux + n_lin3
    job_rows = _pool_job_rows(ops, gather=True)
    assert len(job_rows) == jobs
    segs = br_segments(jobs, R)
    assert len(segs) >= 2, segs
    assert after["batches"] - before["batches"] == 1                   # one pool
    assert kt["blind_rotate"]["launches"] == 1, kt                     # one blind-rotate span ...
    assert kt["keyswitch"]["launches"] == 4, kt                        # ... and a key switch per group
    assert after["bootstraps"] - before["bootstraps"] == jobs
    assert after["br_launches"] - before["br_launches"] == 2 * len(segs), (before, after, segs)
    assert after["br_wide_launches"] == before["br_wide_launches"]
    assert np.array_equal(r.sk.decrypt_bits(got), _truth(ops, x, y, z))
    per_op = [np.flatnonzero(ops == o)[:8] for o in range(17)]
    edges = [job_rows[max(0, s0 - 16):s0 + 16] for s0 in segs[1:]]
    check = np.unique(np.concatenate([np.arange(64)] + per_op + edges))
    want = r.orc.gate_batch(0, a[check], b[check], c[check], ops=ops[check])
    bad = np.flatnonzero((got[check] != want).any(axis=1))
    assert bad.size == 0, (check[bad][:8], ops[check[bad][:8]])
    # every opcode group as a level of its own: a fresh engine (the variable is read at creation), the same bytes
    monkeypatch.setenv("EOC_TFHE_NO_POOL", "1")
    e2 = eoc.Engine(r.p)
    monkeypatch.delenv("EOC_TFHE_NO_POOL")
    e2.load_cloud_key(r.sk)
    s0 = e2.stats()
    got_np = _gate_on(e2, a, b, c, ops)
    assert e2.stats()["batches"] - s0["batches"] == 4                  # two-input, MUX, MAJ, XOR3: four levels
    assert np.array_equal(got_np, got)
    e2.close()
    # few runs (no gather): NAND, MUX, XOR3 and NOT runs, the bootstrapped ones one pool of 1 500 jobs
    m = 1500
    ops3 = np.concatenate([np.full(500, 0), np.full(300, 10), np.full(400, 16), np.full(300, 11)]).astype(np.uint8)
    segs3 = br_segments(500 + 2 * 300 + 400, R)
    r.eng.set_profiling(True)
    r.eng.kernel_times(reset=True)
    before = r.eng.stats()
    got3 = _gate_on(r.eng, a[:m], b[:m], c[:m], ops3)
    after = r.eng.stats()
    kt3 = r.eng.kernel_times(reset=True)
    r.eng.set_profiling(False)
    assert kt3["blind_rotate"]["launches"] == 1 and kt3["keyswitch"]["launches"] == 3, kt3
    assert after["br_launches"] - before["br_launches"] == 2 * len(segs3), (before, after, segs3)
    assert np.array_equal(r.sk.decrypt_bits(got3), _truth(ops3, x[:m], y[:m], z[:m]))
    jr3 = _pool_job_rows(ops3, gather=False)
    check3 = np.unique(np.concatenate([np.r_[0:8, 496:504, 796:804, 1196:1204, 1492:1500]] +
                                      [jr3[max(0, s0 - 16):s0 + 16] for s0 in segs3[1:]]))
    assert np.array_equal(got3[check3], r.orc.gate_batch(0, a[check3], b[check3], c[check3], ops=ops3[check3]))
    assert np.array_equal(_gate_on(r.eng, a[:m], b[:m], c[:m], ops3, out_alias=True), got3)
    r.eng.close()


def test_deep_chain_bit_exact_set_a(eoc, rig_a):
    """24 dependent levels x 96 gates on Set A (outputs of one level feed the next, alternating opcodes): GPU and
    oracle stay bit-identical through the whole depth (2304 bootstraps, ~1.1 M CMux steps, so the rare
    abar = 0 steps -- one in 2048 -- occur hundreds of times) and every level decrypts correctly."""
    r = rig_a
    width, depth = 96, 24
    bits, cur = _rand_cts(r, width, 91)
    ref = cur.copy()
    names = ["NAND", "XOR", "ORNY", "XNOR", "AND", "NOR"]
    for lv in range(depth):
        op = names[lv % len(names)]
        a, b = cur, np.roll(cur, lv + 1, axis=0)
        cur = r.gate(eoc.OPS[op], a, b)
        ref = r.orc.gate_batch(ol.OPS[op], ref, np.roll(ref, lv + 1, axis=0))
        assert np.array_equal(cur, ref), f"diverged at level {lv} ({op})"
        x, y = bits, np.roll(bits, lv + 1)
        bits = {"NAND": 1 - (x & y), "XOR": x ^ y, "ORNY": (1 - x) | y, "XNOR": 1 - (x ^ y), "AND": x & y,
                "NOR": 1 - (x | y)}[op]
        assert np.array_equal(r.sk.decrypt_bits(cur), bits), f"wrong plaintext at level {lv}"


@pytest.mark.parametrize("env", [{"EOC_TFHE_BR_PARTS": "3"}, {"EOC_TFHE_BR_PARTS": "1", "EOC_TFHE_BR_SLICE": "5"},
                                 {"EOC_TFHE_NO_FOLD": "1"}, {"EOC_TFHE_PRIO_DUTY": "-1", "EOC_TFHE_BR_SLICE": "-1"},
                                 {"EOC_TFHE_BR_WIDE": "1"}, {"EOC_TFHE_BR_WIDE": "1", "EOC_TFHE_BR_PARTS": "3", "EOC_TFHE_NO_FOLD": "1"},
                                 {"EOC_TFHE_BR_WIDE": "1", "EOC_TFHE_BR_SLICE": "5"}, {"EOC_TFHE_BR_WIDE": "0"},
                                 {"EOC_TFHE_SCALAR_ABAR": "1"}, {"EOC_TFHE_SCALAR_ABAR": "1", "EOC_TFHE_BR_WIDE": "1"},
                                 {"EOC_TFHE_SCALAR_ABAR": "1", "EOC_TFHE_NO_FOLD": "1", "EOC_TFHE_BR_PARTS": "2"},
                                 {"EOC_TFHE_NO_POOL": "1"}, {"EOC_TFHE_NO_POOL": "1", "EOC_TFHE_NO_FOLD": "1"}])
def test_launch_shapes_do_not_change_results(eoc, monkeypatch, env):
    """the launch-shape knobs of the engine -- a blind rotation cut into consecutive launches (accumulators parked in
    between), job slices, the separate k_ks_init launch, wave priorities off, the one-wave-per-ciphertext kernel forced
    on narrow launches (gadget length 2; odd job counts leave an idle wave) or off, the rotation amounts read back by
    scalar loads instead of through LDS (round 6: the shipped form stays inside the memory model), the opcode runs of a
    mixed batch as levels of their own instead of one pooled blind rotation -- give the oracle's bits, all of them"""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    for pset in (0, 1):
        r = Rig(eoc, pset, 11, n_override=33)
        b0, c0 = _rand_cts(r, 13, 61, 0)
        b1, c1 = _rand_cts(r, 13, 62, 0)
        b2, c2 = _rand_cts(r, 13, 63, 0)
        assert np.array_equal(r.gate(eoc.OPS["NAND"], c0, c1), r.orc.gate_batch(ol.OPS["NAND"], c0, c1))
        assert np.array_equal(r.gate(eoc.OPS["MUX"], c0, c1, c2), r.orc.gate_batch(ol.OPS["MUX"], c0, c1, c2))
        ops = np.array([0, 4, 10, 11, 10, 0, 2, 13, 4, 12, 10, 14, 0], np.uint8)
        assert np.array_equal(r.gate(0, c0, c1, c2, ops=ops), r.orc.gate_batch(0, c0, c1, c2, ops=ops))
        r.eng.close()


def test_wide_kernel_full_width_bit_exact(eoc, rig_a):
    """k_blind_rotate_wide (one wave per ciphertext; levels wider than the pair kernel's resident set, gadget length 2)
    against the oracle and against the pair kernel.  3 400 NAND gates = one full wide launch (2 048) + a 1 352-job wide
    remainder; 2 304 = a full wide launch + a 256-job remainder on the pair kernel; both compared row for row with the pair
    kernel's output for the same operands (narrow calls) and on a seeded sample with the oracle; plus a 1 100-gate MUX
    level (2 200 blind rotations, unfolded key-switch set-up)."""
    r = rig_a
    cnt = 3400
    b0, c0 = _rand_cts(r, cnt, 91)
    b1, c1 = _rand_cts(r, cnt, 92)
    st0 = r.eng.stats()
    got = r.gate(eoc.OPS["NAND"], c0, c1)
    st1 = r.eng.stats()
    assert st1["br_wide_launches"] - st0["br_wide_launches"] == 2 and st1["br_launches"] - st0["br_launches"] == 2, (st0, st1)
    assert np.array_equal(r.sk.decrypt_bits(got), 1 - (b0 & b1))
    pick = np.random.default_rng(3).choice(cnt, 96, replace=False)
    assert np.array_equal(got[pick], r.orc.gate_batch(ol.OPS["NAND"], c0[pick], c1[pick]))
    narrow = np.concatenate([r.gate(eoc.OPS["NAND"], c0[a:a + 1000], c1[a:a + 1000]) for a in range(0, cnt, 1000)])
    st2 = r.eng.stats()
    assert st2["br_wide_launches"] == st1["br_wide_launches"]                     # the pair kernel ran those
    assert np.array_equal(got, narrow)
    got2 = r.gate(eoc.OPS["NAND"], c0[:2304], c1[:2304])
    st3 = r.eng.stats()
    assert st3["br_wide_launches"] - st2["br_wide_launches"] == 1 and st3["br_launches"] - st2["br_launches"] == 2
    assert np.array_equal(got2, narrow[:2304])
    m = 1100
    b2, c2 = _rand_cts(r, m, 93)
    gm = r.gate(eoc.OPS["MUX"], c0[:m], c1[:m], c2)
    assert r.eng.stats()["br_wide_launches"] == st3["br_wide_launches"] + 1
    assert np.array_equal(r.sk.decrypt_bits(gm), np.where(b0[:m] == 1, b1[:m], b2))
    pm = pick[pick < m][:24]
    assert np.array_equal(gm[pm], r.orc.gate_batch(ol.OPS["MUX"], c0[pm], c1[pm], c2[pm]))


def test_descriptor_ring_wraps_without_a_device_synchronise(eoc, rig_small):
    """1 300 back-to-back asynchronous MUX calls on one stream push 1 300 descriptors through the 1 024-slot ring (a MUX level
    keeps the separate k_prepare / k_ks_init launches and therefore the ring; a single two-input gate travels as a kernel
    argument and never touches it): the wrap waits for the engine's own earlier kernels (an event), results
    before and after it are the oracle's"""
    torch = torch_cuda()
    r = rig_small
    c = [_rand_cts(r, 4, 71 + k)[1] for k in range(3)]
    d = [to_dev(x) for x in c]
    outs = dev_empty((1300, 4, r.n + 1), torch.int32)
    perms = [(0, 1, 2), (1, 2, 0), (2, 0, 1)]
    for k in range(1300):
        i0, i1, i2 = perms[k % 3]
        r.eng.gate_batch_device(eoc.OPS["MUX"], d[i0].data_ptr(), d[i1].data_ptr(), d[i2].data_ptr(), outs[k].data_ptr(), 4)
    sync()
    got = outs.cpu().numpy()
    want = [r.orc.gate_batch(ol.OPS["MUX"], c[i0], c[i1], c[i2]) for i0, i1, i2 in perms]
    for k in list(range(0, 1300, 97)) + list(range(1015, 1035)) + [1299]:
        assert np.array_equal(got[k], want[k % 3]), k


def test_ring_wrap_inside_a_level_behind_an_earlier_push(eoc):
    """the wrap event is recorded at the END of a level; a level whose free-gate push fits behind the mark but
    whose boot push wraps waits for that mark AND, because a push was queued behind it, drains its own stream before
    rewriting slots.  A fresh engine (ring of 1 024 slots): call 1 = one level of 900 NAND gates (ring position 900, mark
    recorded); call 2 = 60 COPY gates (fit: position 960) + 900 XOR gates (wrap inside the level); call 3 repeats call 2
    (the wrap is now its first push).  Every output against the oracle."""
    torch = torch_cuda()
    r = Rig(eoc, 0, 7, n_override=16)
    _, base = _rand_cts(r, 8, 201)
    n_in, nb, nf = 8, 900, 60
    g1 = [eoc.Gate(eoc.OPS["NAND"], k % n_in, (3 * k + 1) % n_in, -1, n_in + k) for k in range(nb)]
    g2 = [eoc.Gate(eoc.OPS["COPY"], k % n_in, -1, -1, n_in + nb + k) for k in range(nf)] + \
         [eoc.Gate(eoc.OPS["XOR"], (5 * k) % n_in, (k + 2) % n_in, -1, n_in + k) for k in range(nb)]
    n_wires = n_in + nb + nf
    wires = dev_empty((n_wires, 1, r.n + 1), torch.int32)
    wires.zero_()
    wires[:n_in, 0] = to_dev(base)
    ref = np.zeros((n_wires, 1, r.n + 1), np.int32)
    ref[:n_in, 0] = base
    for gates in (g1, g2, g2):
        r.eng.circuit_run_device(gates, wires.data_ptr(), n_wires, 1)
        for g in gates:
            ref[g.out] = ref[g.in0] if g.op == eoc.OPS["COPY"] else r.orc.gate_batch(g.op, ref[g.in0], ref[g.in1])
    sync()
    assert np.array_equal(wires.cpu().numpy(), ref)
    r.eng.close()


@pytest.mark.parametrize("cnt", [700, 1500, 2300])
def test_in_place_batches_with_the_folded_prologue(eoc, rig_a, cnt):
    """out aliases an operand (d_out == d_in0, then d_out == d_in1).  Since round 5 the blind rotation's own prologue reads
    the operand rows (k_prepare folded away) while other workgroups' epilogues already write output rows: a job reads only
    ITS rows, before its own epilogue writes them, so exact aliasing stays safe -- on the pair kernel (700), the wide kernel
    (1 500) and a level cut into a wide launch plus a pair-kernel remainder (2 300)."""
    torch = torch_cuda()
    r = rig_a
    b0, c0 = _rand_cts(r, cnt, 31)
    b1, c1 = _rand_cts(r, cnt, 32)
    want = r.gate(eoc.OPS["XOR"], c0, c1)                        # out of place
    pick = np.random.default_rng(cnt).choice(cnt, 40, replace=False)
    assert np.array_equal(want[pick], r.orc.gate_batch(ol.OPS["XOR"], c0[pick], c1[pick]))
    for alias in (0, 1):
        d0, d1 = to_dev(c0), to_dev(c1)
        out = d0 if alias == 0 else d1
        r.eng.gate_batch_device(eoc.OPS["XOR"], d0.data_ptr(), d1.data_ptr(), None, out.data_ptr(), cnt)
        sync()
        assert np.array_equal(out.cpu().numpy(), want), alias
    assert np.array_equal(r.sk.decrypt_bits(want), b0 ^ b1)


@pytest.mark.parametrize("n,bgbit,cnt", [(12, 8, 9), (7, 12, 6), (5, 11, 3), (9, 10, 2051)])
def test_wide_kernel_custom_gadget_bases_bit_exact(eoc, monkeypatch, n, bgbit, cnt):
    """k_blind_rotate_wide's run-time-base instance (gadget length 2 with Bgbit != 10) and the compile-time one on a
    custom n, forced onto narrow batches (odd counts leave an idle wave) and taken by width (2 051 rows: a full wide
    launch + a 3-row remainder on the pair kernel): GPU == oracle bit for bit, NAND / XOR / MUX.  (Bases beyond 2^12 at
    gadget length 2 leave the conversion contract |v| < 2^51 -- include/eoc_tfhe_gpu.h -- and are not claimed.)"""
    torch = torch_cuda()
    if cnt < 1024:
        monkeypatch.setenv("EOC_TFHE_BR_WIDE", "1")
    p = eoc.default_params(0)
    p.n, p.l, p.Bgbit = n, 2, bgbit
    sk = eoc.SecretKey(p, 78)
    eng = eoc.Engine(p)
    eng.load_cloud_key(sk)
    orc = ol.Oracle(0, 78, n_override=n, with_bk=False)
    orc.p.l, orc.p.Bgbit = 2, bgbit
    orc.l, orc.kpl = 2, 4
    orc.gen_cloud()
    assert np.array_equal(sk.bk, orc.bk)
    rng = np.random.default_rng(n)
    c = [sk.encrypt_bits(rng.integers(0, 2, cnt), 95 + k, 0) for k in range(3)]
    d = [to_dev(x) for x in c]
    out = torch.empty_like(d[0])
    w0 = eng.stats()["br_wide_launches"]
    for name in ("NAND", "XOR", "MUX"):
        eng.gate_batch_device(eoc.OPS[name], d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), out.data_ptr(), cnt)
        sync()
        want = orc.gate_batch(ol.OPS[name], c[0], c[1], c[2] if name == "MUX" else None)
        assert np.array_equal(out.cpu().numpy(), want), (name, n, bgbit)
    assert eng.stats()["br_wide_launches"] >= w0 + 3
    eng.close()
