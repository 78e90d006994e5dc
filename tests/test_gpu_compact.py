"""Compact public-key encryption on the MI355X: eoc_compact_expand_device against the oracle composition (numpy extraction +
orc_keyswitch, tests/compact_oracle.py) byte for byte on both sets, decryption of bits and ints, the noise after the key
switch against compact_var + ks_var, expanded inputs in gates, a circuit and a many-LUT step, the client / encryptor /
server split across processes, the global context on one and two engines, a call across the 2^20-sample slice boundary
under a reserved workspace, and the missing-key error.  Host side: tests/test_compact_cpu.py."""
import json
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import compact_oracle as co
import lut_oracle as lo
import oracle_lib as ol
from eoc_tfhe_amd import noise
from gpu_util import dev_empty, sync, to_dev, torch_cuda

pytestmark = pytest.mark.gpu
N = 1024
EOC_ERR_NO_KEY = -4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def eoc(built_lib):
    torch_cuda()
    import eoc_tfhe_amd
    return eoc_tfhe_amd


_KEYS = {}


def keys(eoc, pset, seed=1):
    """params, secret key, public key, oracle (KSK only), engine with the cloud key"""
    if (pset, seed) not in _KEYS:
        p = eoc.default_params(pset)
        sk = eoc.SecretKey(p, seed)
        eng = eoc.Engine(p)
        eng.load_cloud_key(sk)
        _KEYS[(pset, seed)] = (p, sk, eoc.PublicKey(sk.public_key_bytes()), ol.Oracle(pset, seed, with_bk=False), eng)
    return _KEYS[(pset, seed)]


def expand_device(eng, lists, count, n):
    torch = torch_cuda()
    d_lists = to_dev(lists)
    d_out = dev_empty((count, n + 1), torch.int32)
    eng.compact_expand_device(d_lists.data_ptr(), count, d_out.data_ptr())
    sync()
    return d_out.cpu().numpy()


@pytest.mark.parametrize("pset", [0, 1])
def test_expansion_equals_the_oracle_composition(eoc, pset):
    p, sk, pk, orc, eng = keys(eoc, pset)
    rng = np.random.default_rng(30 + pset)
    bits = rng.integers(0, 2, 5000).astype(np.uint8)
    lists = pk.encrypt_bits(bits, enc_seed=300 + pset)
    edges = [b + d for b in range(N, 5000, N) for d in (-2, -1, 0, 1)] + [4998, 4999]
    check = np.unique(np.r_[np.arange(1025), edges])
    want = dict(zip(check.tolist(), co.expand(orc, lists, check)))
    before = eng.stats()["keyswitches"]
    for count in (1, 1023, 1024, 1025, 5000):
        got = expand_device(eng, lists[: -(-count // N)], count, p.n)
        rows = np.arange(count) if count <= 1025 else np.array(edges)
        for r in rows:
            assert np.array_equal(got[r], want[int(r)]), (count, int(r))
        assert np.array_equal(sk.decrypt_bits(got), bits[:count]), count
    assert eng.stats()["keyswitches"] - before == 1 + 1023 + 1024 + 1025 + 5000


@pytest.mark.parametrize("pset", [0, 1])
def test_expanded_bits_and_ints_decrypt(eoc, pset):
    p, sk, pk, _, eng = keys(eoc, pset)
    rng = np.random.default_rng(40 + pset)
    bits = rng.integers(0, 2, 3000).astype(np.uint8)
    assert np.array_equal(sk.decrypt_bits(expand_device(eng, pk.encrypt_bits(bits), 3000, p.n)), bits)
    for q in (2, 4, 8):
        vals = rng.integers(0, q, 3000).astype(np.uint8)
        got = expand_device(eng, pk.encrypt_ints(vals, q), 3000, p.n)
        assert np.array_equal(sk.decrypt_ints(got, q), vals), q


@pytest.mark.parametrize("pset", [0, 1])
def test_noise_after_the_key_switch_matches_the_model(eoc, pset):
    p, sk, pk, _, eng = keys(eoc, pset)
    count = 16384
    rng = np.random.default_rng(50 + pset)
    bits = rng.integers(0, 2, count).astype(np.uint8)
    got = expand_device(eng, pk.encrypt_bits(bits, enc_seed=500 + pset), count, p.n).astype(np.int64)
    ph = ((got[:, -1] - got[:, :-1] @ sk.lwe_key.astype(np.int64)) + 2**31) % 2**32 - 2**31
    err = (ph - co.bit_msgs(bits)) / 2.0**32
    pred = noise.predict(p, sk.lwe_key, sk.tlwe_key, sk.ksk)
    var = noise.compact_var(p, sk.tlwe_key, pk) + pred["ks_var"]
    mean = pred["ks_mean"] + float(noise.compact_offset(sk.tlwe_key, pk)[np.arange(count) % N].mean())
    z = (err.mean() - mean) / (err.std() / np.sqrt(count))
    print(f"pset {pset}: var {err.var():.4e} predicted {var:.4e} ratio {err.var() / var:.4f}; mean {err.mean():.3e} "
          f"predicted {mean:.3e} (z = {z:.2f}); sigma {err.std():.5f}")
    assert abs(err.var() / var - 1) < 0.05
    assert abs(z) < 4


def test_expanded_inputs_in_gates_a_circuit_and_a_many_lut_step(eoc):
    torch = torch_cuda()
    from eoc_tfhe_amd import circuits
    p, sk, pk, _, eng = keys(eoc, 0)
    orc = ol.Oracle(0, 1)                                   # with the bootstrapping key: gates and circuits
    rng = np.random.default_rng(60)
    rows = 700
    bits = rng.integers(0, 2, (3, rows)).astype(np.uint8)
    ins = [expand_device(eng, pk.encrypt_bits(bits[k]), rows, p.n) for k in range(3)]
    ops = rng.choice(np.array([ol.OPS["NAND"], ol.OPS["XOR"], ol.OPS["MUX"]], np.uint8), rows)
    d = [to_dev(x) for x in ins]
    d_out = dev_empty((rows, p.n + 1), torch.int32)
    eng.gate_batch_device(0, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d_out.data_ptr(), rows, ops=ops)
    sync()
    got = d_out.cpu().numpy()
    b0, b1, b2 = bits.astype(np.int64)
    want = np.where(ops == ol.OPS["NAND"], 1 - (b0 & b1), np.where(ops == ol.OPS["XOR"], b0 ^ b1, np.where(b0 == 1, b1, b2)))
    assert np.array_equal(sk.decrypt_bits(got), want)
    assert np.array_equal(got, orc.gate_batch(0, ins[0], ins[1], ins[2], ops=ops))
    # the 8-bit ripple-carry adder on expanded inputs, one circuit call, against the oracle gate by gate
    gates, n_wires, aw, bw, sw = circuits.ripple_carry_adder(8)
    S = 16
    A, B = rng.integers(0, 256, S), rng.integers(0, 256, S)
    planes = np.stack([(A >> i) & 1 for i in range(8)] + [(B >> i) & 1 for i in range(8)]).astype(np.uint8)   # [16][S]
    flat = expand_device(eng, pk.encrypt_bits(planes.ravel()), 16 * S, p.n).reshape(16, S, p.n + 1)
    wires = np.zeros((n_wires, S, p.n + 1), np.int32)
    wires[aw[0]:aw[0] + 8], wires[bw[0]:bw[0] + 8] = flat[:8], flat[8:]
    want_w = wires.copy()
    d_w = to_dev(wires)
    eng.circuit_run_device(gates, d_w.data_ptr(), n_wires, S)
    sync()
    got_w = d_w.cpu().numpy()
    for g in gates:
        want_w[g.out] = orc.gate_batch(g.op, want_w[g.in0], None if g.in1 < 0 else want_w[g.in1],
                                       None if g.in2 < 0 else want_w[g.in2])
        assert np.array_equal(got_w[g.out], want_w[g.out]), g.out
    sums = sum(sk.decrypt_bits(got_w[sw[0] + i]).astype(np.int64) << i for i in range(9))
    assert np.array_equal(sums, A + B)
    # a many-LUT ripple step on expanded ints (p = 4): s = a + b + c, one call gives s mod 2 and s >= 2
    q, T, pairs = 4, 2, 1500
    abc = rng.integers(0, 2, (3, pairs)).astype(np.uint8)
    x = [to_dev(expand_device(eng, pk.encrypt_ints(abc[k], q), pairs, p.n)) for k in range(3)]
    s = x[0] + x[1] + x[2]
    tv = to_dev(eoc.lut_many_test_polynomial(q, [lo.int_table(lambda v: v % 2, q, q), lo.int_table(lambda v: v >= 2, q, q)]))
    out = dev_empty((T, pairs, p.n + 1), torch.int32)
    eng.lut_many_batch_device(T, tv.data_ptr(), 1, s.data_ptr(), out.data_ptr(), pairs)
    sync()
    tot = abc.astype(np.int64).sum(0)
    assert np.array_equal(sk.decrypt_ints(out[0].cpu().numpy(), q), tot % 2)
    assert np.array_equal(sk.decrypt_ints(out[1].cpu().numpy(), q), (tot >= 2).astype(np.int64))


def child(body, cwd, timeout=900):
    code = textwrap.dedent("""
        import json, sys, os
        import numpy as np
        sys.path.insert(0, %r)
        import eoc_tfhe_amd as eoc
        from eoc_tfhe_amd import Tfhe
        out = {}
    """ % ROOT) + textwrap.dedent(body) + "\nprint('RESULT' + json.dumps(out))\n"
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=timeout, cwd=cwd)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT")][-1][len("RESULT"):])


def test_client_encryptor_server_split(eoc, tmp_path):
    """client: secret key, EOCCK1 and EOCPK1 -> a second party encrypts compact lists from EOCPK1 alone -> a fresh server in
    key mode 2 expands them and runs a gate batch -> the client decrypts"""
    wire, vault = tmp_path / "wire", tmp_path / "vault"
    wire.mkdir()
    vault.mkdir()
    rows = 1500
    rng = np.random.default_rng(70)
    bits = rng.integers(0, 2, (2, rows)).astype(np.uint8)
    np.save(tmp_path / "bits.npy", bits)
    client = child("""
        import base64
        blob = eoc.SecretKey(eoc.default_params(0), None, with_cloud_key=False).export_bytes()
        open(%r, 'wb').write(blob)
        assert Tfhe.importSecretKey(base64.b64encode(blob).decode()) == 0
        assert Tfhe.exportCloudKeyToFile('cloud.key') == 0
        open('public.key', 'wb').write(eoc.global_public_key_export())
        out['mode'], out['engines'] = Tfhe.keyMode(), eoc.gpu_engine_count()
    """ % str(vault / "secret.key"), cwd=str(wire))
    assert client == {"mode": 1, "engines": 0}
    enc = child("""
        pk = eoc.PublicKey(open('public.key', 'rb').read())
        bits = np.load(%r)
        for k in range(2):
            np.save('lists%%d.npy' %% k, pk.encrypt_bits(bits[k]))
        out['mode'], out['engines'] = Tfhe.keyMode(), eoc.gpu_engine_count()
    """ % str(tmp_path / "bits.npy"), cwd=str(wire))
    assert enc == {"mode": 0, "engines": 0}
    assert os.path.getsize(wire / "lists0.npy") < 2 * 2 * N * 4 + 200          # two lists carry 1 500 bits
    for f in os.listdir(wire):
        assert b"EOCSK" not in open(wire / f, "rb").read(), f
    server = child("""
        assert Tfhe.importCloudKeyFromFile('cloud.key') == 0
        out['mode'] = Tfhe.keyMode()
        x = [eoc.compact_expand(np.load('lists%%d.npy' %% k), %d) for k in range(2)]
        np.save('xor.npy', eoc.global_gate_batch(eoc.OPS['XOR'], x[0], x[1]))
        out['pk'] = eoc.lib().eoc_global_public_key_export(None, 0)
        out['keyswitches'] = int(eoc.stats()['keyswitches'])
        Tfhe.resetGateKey()
    """ % rows, cwd=str(wire))
    assert server == {"mode": 2, "pk": 0, "keyswitches": 3 * rows}
    back = child("""
        import base64
        assert Tfhe.importSecretKey(base64.b64encode(open(%r, 'rb').read()).decode()) == 0
        out['xor'] = eoc.global_decrypt_bits(np.load('xor.npy')).tolist()
    """ % str(vault / "secret.key"), cwd=str(wire))
    assert back["xor"] == (bits[0] ^ bits[1]).tolist()


def test_global_context_one_and_two_engines(eoc):
    p, sk, pk, _, eng = keys(eoc, 0)
    count = 3001                                           # two blocks of 1 501 / 1 500: the second starts at slot 477
    lists = pk.encrypt_bits(np.random.default_rng(80).integers(0, 2, count).astype(np.uint8), enc_seed=800)
    ref = expand_device(eng, lists, count, p.n)
    try:
        eoc.gpu_shutdown()
        eoc.gpu_init(p, devices=[0])
        eoc.upload_cloud_key(sk)
        one = eoc.compact_expand(lists, count)
        eoc.gpu_shutdown()
        eoc.gpu_init(p, devices=[0, 0])
        eoc.upload_cloud_key(sk)
        two = eoc.compact_expand(lists, count)
        per = [e["keyswitches"] for e in eoc.stats_multi()["engines"]]
    finally:
        eoc.gpu_shutdown()
    assert np.array_equal(one, ref) and np.array_equal(two, ref)
    assert per == [1501, 1500]


def test_call_across_the_slice_boundary_under_a_reserved_workspace(eoc):
    torch = torch_cuda()
    p, sk, pk, orc, _ = keys(eoc, 0)
    count = (1 << 20) + 1500
    bits = np.random.default_rng(90).integers(0, 2, count).astype(np.uint8)
    lists = pk.encrypt_bits(bits, enc_seed=900)
    eng = eoc.Engine(p)
    eng.load_cloud_key(sk)
    L = eoc.lib()
    assert L.eoc_engine_reserve(eng.h, 1 << 20, 0, 0) == 0
    d_lists = to_dev(lists)
    d_out = dev_empty((count, p.n + 1), torch.int32)
    eng.compact_expand_device(d_lists.data_ptr(), count, d_out.data_ptr())
    sync()
    assert L.eoc_engine_workspace_grows(eng.h) == 0
    idx = np.r_[0, (1 << 20) - 3:(1 << 20) + 3, count - 2, count - 1]
    got = d_out[torch.from_numpy(idx).cuda()].cpu().numpy()
    assert np.array_equal(got, co.expand(orc, lists, idx))
    step = 4099
    assert np.array_equal(sk.decrypt_bits(d_out[::step].cpu().numpy()), bits[::step])
    del d_out, d_lists
    eng.close()


def test_engine_without_a_cloud_key(eoc):
    torch = torch_cuda()
    p = eoc.default_params(0)
    eng = eoc.Engine(p)
    d = dev_empty((2, 2, N), torch.int32)
    o = dev_empty((2, p.n + 1), torch.int32)
    assert eoc.lib().eoc_compact_expand_device(eng.h, d.data_ptr(), 2, o.data_ptr(), None) == EOC_ERR_NO_KEY
    eng.close()
