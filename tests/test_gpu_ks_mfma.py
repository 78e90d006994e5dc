"""The matrix-core key switch (k_keyswitch_mfma) against the look-up kernel (k_keyswitch_waves) and the oracle: the same
words, bit for bit.  Integers: equal, never close.  EOC_TFHE_KS_MFMA=1 / 0 (read when an engine is created) forces either
form, and eoc_engine_keyswitch_mfma_launches says which one ran.  The arithmetic alone: tests/test_ks_limbs_cpu.py.

Run on the GPU box:  python -m pytest tests/test_gpu_ks_mfma.py -m gpu -x -q
"""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import oracle_lib as ol
from gpu_util import dev_empty, sync, to_dev, torch_cuda

pytestmark = pytest.mark.gpu
N = 1024
WIDTHS = (1, 31, 32, 33, 1000, 1024, 3400)


@pytest.fixture(scope="module")
def eoc(built_lib):
    torch_cuda()
    import eoc_tfhe_amd
    return eoc_tfhe_amd


def engine(eoc, monkeypatch, p, mfma):
    """an engine that takes the matrix-core form (mfma = 1), the look-up form (0) or the shipped policy (None)"""
    if mfma is None:
        monkeypatch.delenv("EOC_TFHE_KS_MFMA", raising=False)
    else:
        monkeypatch.setenv("EOC_TFHE_KS_MFMA", str(int(mfma)))
    return eoc.Engine(p)


def params(eoc, pset, n):
    p = eoc.default_params(pset)
    if n is not None:
        p.n = n
    return p


def oracle_rows(orc, u):
    with ThreadPoolExecutor(16) as ex:                        # ctypes drops the GIL inside the oracle
        return np.stack(list(ex.map(orc.keyswitch, u)))


def operands(rng, rows):
    """uniform random operand words; rows of all-zero digits (nothing subtracted) and of all-3 digits (the accumulator bound)
    at both ends of the first 32-row tile and of the batch"""
    u = rng.integers(-2**31, 2**31, (rows, N + 1)).astype(np.int32)
    for r in (0, 31, 32, rows - 1):
        u[r % rows, :N] = -65536         # ubar = u + 2^15 = 0xFFFF8000: every digit 3
    for r in (1, 30, 33, rows - 2):
        u[r % rows, :N] = 0              # every digit 0
    return u


def keyswitch(eng, d_u, rows, n):
    torch = torch_cuda()
    d_o = dev_empty((rows, n + 1), torch.int32)
    d_o.fill_(0x5A5A5A5)                                      # whatever was there must not matter
    eng.keyswitch_device(d_u.data_ptr(), d_o.data_ptr(), rows)
    sync()
    return d_o.cpu().numpy()


@pytest.mark.parametrize("pset,n", [(0, None), (1, None), (0, 200), (0, 255), (0, 800)],
                         ids=["setA-n500", "setB-n630", "n200-n1p256", "n255-n1p256", "n800-n1p1024"])
def test_stand_alone_key_switch_new_equals_old_equals_oracle(eoc, monkeypatch, pset, n):
    p = params(eoc, pset, n)
    orc = ol.Oracle(pset, 17, n_override=n, with_bk=False)
    orc.ksk = np.zeros((N * p.ks_t * 3, p.n + 1), np.int32)
    orc.L.orc_keygen_ksk(C.byref(orc.p), orc.seed, orc.lwe_key, orc.tlwe_key, orc.ksk)
    bk = np.zeros((p.n, 2 * p.l, 2, N), np.int32)             # the key switch does not read it
    new, old = engine(eoc, monkeypatch, p, 1), engine(eoc, monkeypatch, p, 0)
    new.load_cloud_key(bk, orc.ksk)
    old.load_cloud_key(bk, orc.ksk)
    u = operands(np.random.default_rng(100 + p.n), max(WIDTHS))
    want = oracle_rows(orc, u)
    assert not want[1, :p.n].any() and want[1, p.n] == u[1, N]
    d_u = to_dev(u)
    for rows in WIDTHS:
        k0 = new.stats()["ks_mfma_launches"]
        got_new = keyswitch(new, d_u, rows, p.n)
        assert new.stats()["ks_mfma_launches"] == k0 + 1, rows
        got_old = keyswitch(old, d_u, rows, p.n)
        assert np.array_equal(got_new, got_old), (rows, np.argwhere(got_new != got_old)[:5])
        assert np.array_equal(got_new, want[:rows]), (rows, np.argwhere(got_new != want[:rows])[:5])
    assert old.stats()["ks_mfma_launches"] == 0
    # the last rows of a batch whose width is no multiple of a tile, with the all-3 / all-0 rows at ITS end
    for rows in (33, 1000):
        v = operands(np.random.default_rng(rows), rows)
        assert np.array_equal(keyswitch(new, to_dev(v), rows, p.n), oracle_rows(orc, v)), rows
    new.close()
    old.close()


class Rig:
    def __init__(self, eoc, monkeypatch, pset, seed, n=None):
        self.p = params(eoc, pset, n)
        self.n = self.p.n
        self.orc = ol.Oracle(pset, seed, n_override=n)
        self.sk = eoc.SecretKey(self.p, seed)
        self.new, self.old = engine(eoc, monkeypatch, self.p, 1), engine(eoc, monkeypatch, self.p, 0)
        self.new.load_cloud_key(self.sk)
        self.old.load_cloud_key(self.sk)

    def cts(self, count, enc_seed, first=0):
        bits = np.random.default_rng(enc_seed).integers(0, 2, count)
        return bits, self.sk.encrypt_bits(bits, enc_seed, first)

    @staticmethod
    def gate(eng, op, c0, c1=None, c2=None, ops=None):
        torch = torch_cuda()
        d = [None if c is None else to_dev(c) for c in (c0, c1, c2)]
        out = torch.empty_like(d[0])
        eng.gate_batch_device(op, d[0].data_ptr(), None if d[1] is None else d[1].data_ptr(),
                              None if d[2] is None else d[2].data_ptr(), out.data_ptr(), d[0].shape[0], ops=ops)
        sync()
        return out.cpu().numpy()

    def close(self):
        self.new.close()
        self.old.close()


@pytest.mark.parametrize("pset", [0, 1], ids=["setA", "setB"])
def test_one_1024_gate_batch_per_set_against_the_oracle(eoc, monkeypatch, pset):
    r = Rig(eoc, monkeypatch, pset, 31)
    (b0, c0), (b1, c1) = r.cts(1024, 41), r.cts(1024, 42, 5000)
    r.new.set_profiling(True)
    k0 = r.new.stats()["ks_mfma_launches"]
    got = r.gate(r.new, eoc.OPS["NAND"], c0, c1)
    assert r.new.stats()["ks_mfma_launches"] == k0 + 1
    assert r.new.kernel_times()["keyswitch"]["launches"] == 1           # one key-switch span per call, as before
    assert np.array_equal(got, r.gate(r.old, eoc.OPS["NAND"], c0, c1))
    assert np.array_equal(got, r.orc.gate_batch(ol.OPS["NAND"], c0, c1))
    assert np.array_equal(r.sk.decrypt_bits(got), 1 - (b0 & b1))
    r.close()


def test_mux_level_and_several_gate_groups_in_one_launch(eoc, monkeypatch):
    """a MUX level (two blind rotations per gate, k_ks_init sums them first), a mixed batch and a netlist whose levels hold
    several gates (several gate groups = grid.y of ONE key-switch launch), at a width with a partly filled tile"""
    from eoc_tfhe_amd import circuits
    r = Rig(eoc, monkeypatch, 0, 33, n=40)
    S = 70
    (ba, a), (bb, b), (bc, c) = r.cts(S, 51), r.cts(S, 52, 200), r.cts(S, 53, 400)
    k0 = r.new.stats()["ks_mfma_launches"]
    got = r.gate(r.new, eoc.OPS["MUX"], a, b, c)
    assert r.new.stats()["ks_mfma_launches"] > k0
    assert np.array_equal(got, r.gate(r.old, eoc.OPS["MUX"], a, b, c))
    assert np.array_equal(got, r.orc.gate_batch(ol.OPS["MUX"], a, b, c))
    assert np.array_equal(r.sk.decrypt_bits(got), np.where(ba, bb, bc))
    ops = np.resize(np.array([0, 10, 4, 15, 16, 11, 1, 10, 13, 5], np.uint8), S)
    got = r.gate(r.new, 0, a, b, c, ops=ops)
    assert np.array_equal(got, r.gate(r.old, 0, a, b, c, ops=ops))
    assert np.array_equal(got, r.orc.gate_batch(0, a, b, c, ops=ops))
    gates, n_wires, aw, bw, sw = circuits.ripple_carry_adder(4)
    rng = np.random.default_rng(6)
    A, B = rng.integers(0, 16, S), rng.integers(0, 16, S)
    wires = np.zeros((n_wires, S, r.n + 1), np.int32)
    for i in range(4):
        wires[aw[0] + i] = r.sk.encrypt_bits(((A >> i) & 1).astype(np.uint8), 600 + i, 0)
        wires[bw[0] + i] = r.sk.encrypt_bits(((B >> i) & 1).astype(np.uint8), 700 + i, 0)
    res = []
    for eng in (r.new, r.old):
        d_w = to_dev(wires)
        eng.circuit_run_device(gates, d_w.data_ptr(), n_wires, S)
        sync()
        res.append(d_w.cpu().numpy())
    assert np.array_equal(res[0], res[1])
    tot = sum(r.sk.decrypt_bits(res[0][sw[0] + i]).astype(np.int64) << i for i in range(5))
    assert np.array_equal(tot, A + B)
    r.close()


def test_captured_call_replays_bit_identically_after_reserve(eoc, monkeypatch):
    """the benchmark's graph leg: one gate batch of 1024 captured after eoc_engine_reserve (nothing allocated on the launch
    path: the limb image exists since the key was installed) and replayed on new operand values"""
    torch = torch_cuda()
    r = Rig(eoc, monkeypatch, 0, 35)
    L, S, eng = eoc.lib(), 1024, r.new
    assert L.eoc_engine_reserve(eng.h, 2 * S, 64, 0) == 0
    (_, c0), (_, c1) = r.cts(S, 61), r.cts(S, 62, 3000)
    d0, d1 = to_dev(c0), to_dev(c1)
    out = torch.empty_like(d0)
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        eng.gate_batch_device(eoc.OPS["NAND"], d0.data_ptr(), d1.data_ptr(), None, out.data_ptr(), S, stream=st.cuda_stream)
    st.synchronize()
    eager = out.cpu().numpy()
    grows = L.eoc_engine_workspace_grows(eng.h)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=st):
        eng.gate_batch_device(eoc.OPS["NAND"], d0.data_ptr(), d1.data_ptr(), None, out.data_ptr(), S, stream=st.cuda_stream)
    assert L.eoc_engine_workspace_grows(eng.h) == grows
    out.zero_()
    g.replay()
    sync()
    assert np.array_equal(out.cpu().numpy(), eager)
    (_, e0), (_, e1) = r.cts(S, 63), r.cts(S, 64, 7000)
    d0.copy_(to_dev(e0))
    d1.copy_(to_dev(e1))
    g.replay()
    sync()
    got = out.cpu().numpy()
    assert np.array_equal(got, r.gate(r.old, eoc.OPS["NAND"], e0, e1))
    sample = np.r_[0:8, 500:508, 1016:1024]
    assert np.array_equal(got[sample], r.orc.gate_batch(ol.OPS["NAND"], e0[sample], e1[sample]))
    del g
    r.close()


def test_borrowed_and_adopted_key_images(eoc, monkeypatch):
    """an engine that borrows another engine's images (eoc_engine_set_cloud_key_device) and one that adopts copies made with
    its own allocator (eoc_engine_adopt_cloud_key_device, the replica path) derive their own limb image at install"""
    torch = torch_cuda()
    r = Rig(eoc, monkeypatch, 0, 37)
    L, p = eoc.lib(), r.p
    S = 300
    (_, c0), (_, c1) = r.cts(S, 71), r.cts(S, 72, 900)
    want = r.gate(r.old, eoc.OPS["XOR"], c0, c1)
    assert np.array_equal(want[:16], r.orc.gate_batch(ol.OPS["XOR"], c0[:16], c1[:16]))
    kb, kk = r.new.cloud_key_device()
    borrowed = engine(eoc, monkeypatch, p, 1)
    borrowed.set_cloud_key_device(kb, kk)
    assert np.array_equal(r.gate(borrowed, eoc.OPS["XOR"], c0, c1), want)
    assert borrowed.stats()["ks_mfma_launches"] == 1
    adopted = engine(eoc, monkeypatch, p, 1)
    ptrs = []
    for src, nbytes in ((kb, adopted.bkfft_bytes), (kk, adopted.ksk_dev_bytes)):
        d = C.c_void_p()
        assert L.eoc_device_alloc(adopted.h, nbytes, C.byref(d)) == 0
        host = r.new.download(src, nbytes)
        assert L.eoc_host_to_device(adopted.h, d, host.ctypes.data, nbytes) == 0
        ptrs.append(d.value)
    sync()
    assert L.eoc_engine_adopt_cloud_key_device(adopted.h, C.c_void_p(ptrs[0]), C.c_void_p(ptrs[1])) == 0
    assert np.array_equal(r.gate(adopted, eoc.OPS["XOR"], c0, c1), want)
    assert adopted.stats()["ks_mfma_launches"] == 1
    # installing a key again re-derives the image: a second key on the same engines
    sk2 = eoc.SecretKey(p, 38)
    borrowed.load_cloud_key(sk2)
    r.old.load_cloud_key(sk2)
    f0 = sk2.encrypt_bits(np.ones(S, np.uint8), 81, 0)
    assert np.array_equal(r.gate(borrowed, eoc.OPS["NAND"], f0, f0), r.gate(r.old, eoc.OPS["NAND"], f0, f0))
    borrowed.close()
    adopted.close()
    r.close()


def test_shipped_policy_takes_the_matrix_cores_on_default_shapes_only(eoc, monkeypatch):
    p = params(eoc, 0, 48)
    sk = eoc.SecretKey(p, 3)
    eng = engine(eoc, monkeypatch, p, None)
    eng.load_cloud_key(sk)
    c = sk.encrypt_bits(np.ones(256, np.uint8), 5, 0)
    Rig.gate(eng, eoc.OPS["AND"], c, c)
    assert eng.stats()["ks_mfma_launches"] == 1
    eng.close()
    q = params(eoc, 0, 48)
    q.ks_t, q.ks_basebit = 5, 3                               # not a shape of the kernel: k_keyswitch_generic, also when forced
    sk = eoc.SecretKey(q, 3)
    orc_u = np.random.default_rng(2).integers(-2**31, 2**31, (9, N + 1)).astype(np.int32)
    res = []
    for force in (1, 0):
        eng = engine(eoc, monkeypatch, q, force)
        eng.load_cloud_key(sk)
        res.append(keyswitch(eng, to_dev(orc_u), 9, q.n))
        assert eng.stats()["ks_mfma_launches"] == 0
        eng.close()
    assert np.array_equal(res[0], res[1])
