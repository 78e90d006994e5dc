"""An n-digit addition three ways on one engine (device-pointer API).
Usage (GPU box): python tools/int_circuit_sweep.py [--json OUT]
For Set A and Set B (PSETS=0,1) and 4 096 and 8 instances (INSTANCES=4096,8), DIGITS = 8 binary digits at p = 4, alternated
leg by leg after a second of warm-up, REPS alternations, host time per addition (device synchronise):
  circuit   radix_add as ONE eoc_int_circuit_run_device call (per digit: k_lin_modswitch, one T = 2 blind rotation, key switch)
  host      what tools/lut_many_sweep.py does: per digit torch adds of the operand rows, then one eoc_lut_many_batch_device call
  maj       circuits.maj_adder (XOR3 + MAJ gates, 2 bootstraps per digit) through eoc_circuit_run_device, same operands
Every result of every leg is decrypt-checked.  Per leg the mean, and min / max over the alternations: max - min of the host
leg is the run-to-run spread the circuit leg is judged against.  Kernel times by name (k_lin_modswitch against
k_modswitch_coarse at equal rows) come from a separate run under `rocprofv3 --kernel-trace --stats` with INSTANCES=4096."""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import eoc_tfhe_amd as eoc  # noqa: E402
from eoc_tfhe_amd import circuits  # noqa: E402

PSETS = [int(x) for x in os.environ.get("PSETS", "0,1").split(",")]
INSTANCES = [int(x) for x in os.environ.get("INSTANCES", "4096,8").split(",")]
DIGITS = int(os.environ.get("DIGITS", "8"))
REPS = int(os.environ.get("REPS", "5"))


def alternate(legs):
    """the legs alternated call by call (the device clock drifts over a run): per leg the list of host ms"""
    for _ in range(2):
        for f in legs:
            f()
    times = [[] for _ in legs]
    for _ in range(REPS):
        for k, f in enumerate(legs):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) * 1e3)
    return times


def warm(eng, sk):
    c0 = torch.from_numpy(sk.encrypt_bits(np.zeros(1024, np.uint8), 2)).cuda()
    out = torch.empty_like(c0)
    t_end = time.perf_counter() + 1.0                        # a second of work first: the clock ramps up after an idle gap
    while time.perf_counter() < t_end:
        eng.gate_batch_device(0, c0.data_ptr(), c0.data_ptr(), None, out.data_ptr(), 1024)
        torch.cuda.synchronize()


def addition(pset, params, sk, eng, pairs):
    n1, nd = params.n + 1, DIGITS
    rng = np.random.default_rng(3)
    A, B = rng.integers(0, 1 << nd, pairs), rng.integers(0, 1 << nd, pairs)
    bit = lambda x, i: ((x >> i) & 1).astype(np.uint8)
    ea = [sk.encrypt_ints(bit(A, i), 4, 100 + i) for i in range(nd)]
    eb = [sk.encrypt_ints(bit(B, i), 4, 200 + i) for i in range(nd)]
    # circuit leg
    c = eoc.IntCircuit()
    aw = [c.input(4, 1, fresh=True) for _ in range(nd)]
    bw = [c.input(4, 1, fresh=True) for _ in range(nd)]
    S, carry = eoc.radix_add(c, aw, bw)
    margin = c.check(params, sk.lwe_key, sk.tlwe_key)["worst_sigma"]
    nodes = c.nodes()
    d_tv = torch.from_numpy(c.test_polynomials()).cuda()
    d_w = torch.zeros((c.n_wires, pairs, n1), dtype=torch.int32, device="cuda")
    for i in range(nd):
        d_w[aw[i]] = torch.from_numpy(ea[i]).cuda()
        d_w[bw[i]] = torch.from_numpy(eb[i]).cuda()

    def circuit_leg():
        eng.int_circuit_run_device(nodes, d_tv.data_ptr(), d_tv.shape[0], d_w.data_ptr(), c.n_wires, pairs)

    # host-driven leg
    da, db = [torch.from_numpy(x).cuda() for x in ea], [torch.from_numpy(x).cuda() for x in eb]
    tv = d_tv[:1]                                            # every digit uses the same two tables
    outs = torch.empty((nd, 2, pairs, n1), dtype=torch.int32, device="cuda")
    s = torch.empty((pairs, n1), dtype=torch.int32, device="cuda")

    def host_leg():
        for i in range(nd):
            torch.add(da[i], db[i], out=s)
            if i:
                s.add_(outs[i - 1, 1])
            eng.lut_many_batch_device(2, tv.data_ptr(), 1, s.data_ptr(), outs[i].data_ptr(), pairs)

    # gate-circuit leg
    gates, n_wires, gaw, gbw, gsw = circuits.maj_adder(nd)
    wires = torch.zeros((n_wires, pairs, n1), dtype=torch.int32, device="cuda")
    for w0, X in ((gaw[0], A), (gbw[0], B)):
        for i in range(nd):
            wires[w0 + i] = torch.from_numpy(sk.encrypt_bits(bit(X, i), 300 + w0 + i, 0)).cuda()

    def maj_leg():
        eng.circuit_run_device(gates, wires.data_ptr(), n_wires, pairs)

    t_c, t_h, t_m = alternate([circuit_leg, host_leg, maj_leg])
    w = d_w.cpu().numpy()
    got_c = sum(sk.decrypt_ints(w[x], 4).astype(np.int64) << i for i, x in enumerate(S + [carry]))
    o = outs.cpu().numpy()
    got_h = sum(sk.decrypt_ints(o[i, 0], 4).astype(np.int64) << i for i in range(nd))
    got_h += sk.decrypt_ints(o[nd - 1, 1], 4).astype(np.int64) << nd
    gw = wires[gsw[0]: gsw[0] + nd + 1].cpu().numpy()
    got_m = sum(sk.decrypt_bits(gw[i]).astype(np.int64) << i for i in range(nd + 1))
    same = all(np.array_equal(w[S[i]], o[i, 0]) for i in range(nd)) and np.array_equal(w[carry], o[nd - 1, 1])
    stat = lambda t: dict(mean_ms=round(float(np.mean(t)), 4), min_ms=round(min(t), 4), max_ms=round(max(t), 4))
    r = dict(pset=pset, instances=pairs, digits=nd, reps=REPS, checked_margin_sigma=round(margin, 2),
             circuit=stat(t_c), host=stat(t_h), maj=stat(t_m),
             host_spread_ms=round(max(t_h) - min(t_h), 4), circuit_minus_host_ms=round(float(np.mean(t_c) - np.mean(t_h)), 4),
             circuit_over_host=round(float(np.mean(t_c) / np.mean(t_h)), 4), maj_over_circuit=round(float(np.mean(t_m) / np.mean(t_c)), 4),
             circuit_ok=bool(np.array_equal(got_c, A + B)), host_ok=bool(np.array_equal(got_h, A + B)),
             maj_ok=bool(np.array_equal(got_m, A + B)), circuit_equals_host_bytes=bool(same))
    print(json.dumps(r), flush=True)
    return r


if __name__ == "__main__":
    out = dict(reps=REPS, runs=[])
    for pset in PSETS:
        params = eoc.default_params(pset)
        sk = eoc.SecretKey(params, 1)
        eng = eoc.Engine(params)
        eng.load_cloud_key(sk)
        warm(eng, sk)
        for pairs in INSTANCES:
            out["runs"].append(addition(pset, params, sk, eng, pairs))
        eng.close()
    if "--json" in sys.argv:
        with open(sys.argv[sys.argv.index("--json") + 1], "w") as fh:
            json.dump(out, fh, indent=1)
