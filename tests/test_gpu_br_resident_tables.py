"""Gadget length 2 on the pair kernels: the form that keeps every loop-invariant table value in registers and streams the
key rows through the chains (shipped) against the earlier form (EOC_TFHE_BR_TABLES_LDS=1, read when an engine is created:
k_br_lds*) and against the oracle: the same words, row for row.  Integers: equal, never close.  The loop's instruction mix
is guarded on the CPU side (tests/test_isa_br_resident.py).

Run on the GPU box:  python -m pytest tests/test_gpu_br_resident_tables.py -m gpu -x -q
"""
import numpy as np
import pytest

import lut_many_oracle as lmo
import lut_oracle as lo
import oracle_lib as ol
from gpu_util import dev_empty, sync, to_dev, torch_cuda

pytestmark = pytest.mark.gpu
N = 1024


@pytest.fixture(scope="module")
def eoc(built_lib):
    torch_cuda()
    import eoc_tfhe_amd
    return eoc_tfhe_amd


_KEYS = {}


def keys(eoc, seed=1):
    if seed not in _KEYS:
        p = eoc.default_params(0)                              # Set A: gadget length 2, base 2^10
        _KEYS[seed] = (p, eoc.SecretKey(p, seed), ol.Oracle(0, seed))
    return _KEYS[seed]


class Pair:
    """two engines on one key: `new` = the shipped form, `old` = the tables read from LDS in every step"""

    def __init__(self, eoc, monkeypatch, env=None):
        self.p, self.sk, self.orc = keys(eoc)
        for k, v in (env or {}).items():
            monkeypatch.setenv(k, v)
        monkeypatch.delenv("EOC_TFHE_BR_TABLES_LDS", raising=False)
        self.new = eoc.Engine(self.p)
        monkeypatch.setenv("EOC_TFHE_BR_TABLES_LDS", "1")
        self.old = eoc.Engine(self.p)
        monkeypatch.delenv("EOC_TFHE_BR_TABLES_LDS", raising=False)
        self.new.load_cloud_key(self.sk)
        self.old.load_cloud_key(self.sk)

    def cts(self, count, enc_seed, first=0):
        bits = np.random.default_rng(enc_seed).integers(0, 2, count)
        return bits, self.sk.encrypt_bits(bits, enc_seed, first)

    @staticmethod
    def gate(eng, op, c0, c1=None, c2=None):
        torch = torch_cuda()
        d = [None if c is None else to_dev(c) for c in (c0, c1, c2)]
        out = torch.empty_like(d[0])
        eng.gate_batch_device(op, d[0].data_ptr(), None if d[1] is None else d[1].data_ptr(),
                              None if d[2] is None else d[2].data_ptr(), out.data_ptr(), d[0].shape[0])
        sync()
        return out.cpu().numpy()

    def close(self):
        self.new.close()
        self.old.close()


def sample(count, k=12):
    return np.arange(count) if count <= k else np.unique(np.r_[0:k // 3, count // 2:count // 2 + k // 3, count - k // 3:count])


@pytest.mark.parametrize("width", [1, 255, 1024, 1100])
def test_gate_batches_new_equals_old_equals_oracle(eoc, monkeypatch, width):
    """1, 255, 1024: one pair-kernel launch (1024 = every workgroup resident, the benchmark's shape); 1100 is wider than the
    pair kernel's resident set: with the wide kernel off it is two pair-kernel launches of 550 (several rounds' priorities)"""
    r = Pair(eoc, monkeypatch, {"EOC_TFHE_BR_WIDE": "0"})
    (b0, c0), (b1, c1) = r.cts(width, 100 + width), r.cts(width, 200 + width, 5000)
    st0 = r.new.stats()
    got = r.gate(r.new, eoc.OPS["NAND"], c0, c1)
    st1 = r.new.stats()
    assert st1["br_wide_launches"] == st0["br_wide_launches"]
    assert st1["br_launches"] - st0["br_launches"] == (2 if width > r.new.resident_jobs() else 1)
    old = r.gate(r.old, eoc.OPS["NAND"], c0, c1)
    assert np.array_equal(got, old), np.argwhere(got != old)[:5]
    pick = sample(width)
    assert np.array_equal(got[pick], r.orc.gate_batch(ol.OPS["NAND"], c0[pick], c1[pick]))
    assert np.array_equal(r.sk.decrypt_bits(got), 1 - (b0 & b1))
    r.close()


def test_mux_level_new_equals_old_equals_oracle(eoc, monkeypatch):
    """two blind rotations per gate, key-switch set-up not folded into the kernel's epilogue"""
    r = Pair(eoc, monkeypatch)
    S = 70
    (ba, a), (bb, b), (bc, c) = r.cts(S, 51), r.cts(S, 52, 200), r.cts(S, 53, 400)
    got = r.gate(r.new, eoc.OPS["MUX"], a, b, c)
    assert np.array_equal(got, r.gate(r.old, eoc.OPS["MUX"], a, b, c))
    pick = sample(S)
    assert np.array_equal(got[pick], r.orc.gate_batch(ol.OPS["MUX"], a[pick], b[pick], c[pick]))
    assert np.array_equal(r.sk.decrypt_bits(got), np.where(ba, bb, bc))
    r.close()


def lut_inputs(eoc, sk, p, rows, enc_seed):
    m = np.arange(rows) % (2 * p)
    m[np.arange(rows) % 4 != 3] %= p
    cts = np.empty((rows, sk.n + 1), np.int32)
    for i in range(rows):
        mu = np.int64((int(m[i]) << 32) // (2 * p)).astype(np.uint32).view(np.int32)
        assert eoc.lib().eoc_lwe_encrypt(sk.h, enc_seed, i, int(mu), sk.params.ks_stdev, cts[i].ctypes.data) == 0
    return m, cts


def test_table_lookup_new_equals_old_equals_oracle(eoc, monkeypatch):
    """k_blind_rotate_tv: 3 tables x 32 rows on the pair kernel"""
    r = Pair(eoc, monkeypatch)
    torch = torch_cuda()
    p, rows = 4, 32
    tabs = [lo.int_table(f, p, p) for f in (lambda m: m, lambda m: (3 * m + 1) % p, lambda m: (m * m) % p)]
    tvs = np.ascontiguousarray(np.stack([eoc.lut_test_polynomial(p, t) for t in tabs]).astype(np.int32).reshape(-1, N))
    _, cts = lut_inputs(eoc, r.sk, p, rows, 7100)
    res = []
    for eng in (r.new, r.old):
        d_tv, d_in = to_dev(tvs), to_dev(cts)
        d_out = dev_empty((tvs.shape[0], rows, cts.shape[1]), torch.int32)
        before = eng.stats()
        eng.lut_batch_device(d_tv.data_ptr(), tvs.shape[0], d_in.data_ptr(), d_out.data_ptr(), rows)
        sync()
        assert eng.stats()["br_wide_launches"] == before["br_wide_launches"]
        res.append(d_out.cpu().numpy())
    assert np.array_equal(res[0], res[1])
    pick = sample(rows)
    assert np.array_equal(res[0][:, pick], lo.lut_batch(r.orc, tvs, cts[pick]))
    r.close()


def test_many_lut_step_new_equals_old_equals_oracle(eoc, monkeypatch):
    """k_lut_many: 2 polynomials of T = 4 tables x 32 rows on the pair kernel"""
    r = Pair(eoc, monkeypatch)
    torch = torch_cuda()
    T, p, rows = 4, 4, 32
    tabs = [[lo.int_table(lambda m, a=2 * (g * T + j) + 1, c=g + j: (a * m + c) % p, p, p) for j in range(T)] for g in range(2)]
    tvs = np.ascontiguousarray(np.stack([eoc.lut_many_test_polynomial(p, row) for row in tabs]).astype(np.int32).reshape(-1, N))
    _, cts = lut_inputs(eoc, r.sk, p, rows, 9100)
    res = []
    for eng in (r.new, r.old):
        d_tv, d_in = to_dev(tvs), to_dev(cts)
        d_out = dev_empty((tvs.shape[0], T, rows, cts.shape[1]), torch.int32)
        before = eng.stats()
        eng.lut_many_batch_device(T, d_tv.data_ptr(), tvs.shape[0], d_in.data_ptr(), d_out.data_ptr(), rows)
        sync()
        assert eng.stats()["br_wide_launches"] == before["br_wide_launches"]
        res.append(d_out.cpu().numpy())
    assert np.array_equal(res[0], res[1])
    pick = sample(rows)
    assert np.array_equal(res[0][:, :, pick], lmo.lut_many_batch(r.orc, tvs, cts[pick], T))
    r.close()


def test_blind_rotation_cut_into_parts_new_equals_old_equals_oracle(eoc, monkeypatch):
    """three consecutive launches per blind rotation: the accumulator is parked and picked up again between them"""
    r = Pair(eoc, monkeypatch, {"EOC_TFHE_BR_PARTS": "3"})
    S = 37
    (b0, c0), (b1, c1) = r.cts(S, 61), r.cts(S, 62, 900)
    st0 = r.new.stats()
    got = r.gate(r.new, eoc.OPS["XOR"], c0, c1)
    assert r.new.stats()["br_launches"] - st0["br_launches"] == 3
    assert np.array_equal(got, r.gate(r.old, eoc.OPS["XOR"], c0, c1))
    pick = sample(S)
    assert np.array_equal(got[pick], r.orc.gate_batch(ol.OPS["XOR"], c0[pick], c1[pick]))
    assert np.array_equal(r.sk.decrypt_bits(got), b0 ^ b1)
    # and one whole rotation against the cut one, on engines without the knob
    monkeypatch.delenv("EOC_TFHE_BR_PARTS")
    whole = Pair(eoc, monkeypatch)
    assert np.array_equal(got, whole.gate(whole.new, eoc.OPS["XOR"], c0, c1))
    whole.close()
    r.close()
