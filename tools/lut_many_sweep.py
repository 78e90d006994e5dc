"""Many-LUT lookups against single-table lookups of the same T tables (device-pointer API).
Usage (GPU box): python tools/lut_many_sweep.py [--json OUT] [--no-ripple]
For Set A and Set B (PSETS=0,1), 1 024, 4 096 and 16 384 rows and T = 2, 4, 8 tables at p = 2 (p T <= 16), times
eoc_lut_many_batch_device (ONE packed polynomial: rows blind rotations, T x rows key switches) and eoc_lut_batch_device on
the same T tables (T x rows blind rotations), call by call in alternation after a second of warm-up: host time per call
(device synchronise).  Every result of both calls is decrypt-checked.  Then (Set A) an 8-bit ripple addition over 4 096
pairs in the integer encoding (p = 4; per bit one many-LUT call with T = 2: s mod 2 and s >= 2 of s = a + b + carry)
against the XOR3 + MAJ circuit (circuits.maj_adder: 16 bootstraps on 8 levels), alternated in the same way, both checked.
Kernel times by name (k_lut_many* against the k_blind_rotate*_tv twins at the same job count) come from a separate run of
this script under `rocprofv3 --kernel-trace --stats`."""
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
ROWS = [int(x) for x in os.environ.get("ROWS", "1024,4096,16384").split(",")]
TS = [int(x) for x in os.environ.get("TS", "2,4,8").split(",")]
REPS = int(os.environ.get("REPS", "5"))
P = 2


def int_table(f, p):
    return np.array([((int(f(m)) % p) << 32) // (2 * p) for m in range(p)], np.uint64).astype(np.uint32).view(np.int32)


def timed_pair(fa, fb):
    """fa and fb alternated call by call (the device clock drifts over a run): mean host ms of each"""
    for _ in range(3):
        fa()
        fb()
    tot = [0.0, 0.0]
    for _ in range(REPS):
        for k, f in enumerate((fa, fb)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            tot[k] += time.perf_counter() - t0
    return [t / REPS * 1e3 for t in tot]


def warm(eng, sk, n):
    bits = np.zeros(1024, np.uint8)
    c0 = torch.from_numpy(sk.encrypt_bits(bits, 2)).cuda()
    out = torch.empty_like(c0)
    t_end = time.perf_counter() + 1.0                        # a second of work first: the clock ramps up after an idle gap
    while time.perf_counter() < t_end:
        eng.gate_batch_device(0, c0.data_ptr(), c0.data_ptr(), None, out.data_ptr(), 1024)
        torch.cuda.synchronize()


def sweep(pset):
    params = eoc.default_params(pset)
    sk = eoc.SecretKey(params, 1)
    eng = eoc.Engine(params)
    eng.load_cloud_key(sk)
    warm(eng, sk, params.n)
    vals = np.random.default_rng(0).integers(0, P, max(ROWS)).astype(np.uint8)
    d_in = torch.from_numpy(sk.encrypt_ints(vals, P, 1)).cuda()
    res = []
    for T in TS:
        fs = [lambda m, k=k: (m + k) % P if k % 2 == 0 else (m * (k // 2 + 1) + 1) % P for k in range(T)]
        tabs = [int_table(f, P) for f in fs]
        d_many = torch.from_numpy(eoc.lut_many_test_polynomial(P, tabs)[None]).cuda()
        d_single = torch.from_numpy(np.stack([eoc.lut_test_polynomial(P, t) for t in tabs])).cuda()
        for rows in ROWS:
            d_o1 = torch.empty((T, rows, params.n + 1), dtype=torch.int32, device="cuda")
            d_o2 = torch.empty_like(d_o1)
            many = lambda: eng.lut_many_batch_device(T, d_many.data_ptr(), 1, d_in.data_ptr(), d_o1.data_ptr(), rows)
            single = lambda: eng.lut_batch_device(d_single.data_ptr(), T, d_in.data_ptr(), d_o2.data_ptr(), rows)
            t_many, t_single = timed_pair(many, single)
            o1, o2 = d_o1.cpu().numpy(), d_o2.cpu().numpy()
            ok = all(np.array_equal(sk.decrypt_ints(o[j], P), [fs[j](v) for v in vals[:rows]]) for o in (o1, o2)
                     for j in range(T))
            r = dict(pset=pset, T=T, p=P, rows=rows, many_ms=round(t_many, 4), single_ms=round(t_single, 4),
                     speedup=round(t_single / t_many, 4), decrypt_ok=bool(ok))
            res.append(r)
            print(json.dumps(r), flush=True)
    return res, (params, sk, eng)


def ripple(params, sk, eng, pairs=4096):
    """8-bit a + b: many-LUT levels (T = 2, p = 4) against the XOR3 + MAJ circuit, alternated"""
    n1 = params.n + 1
    rng = np.random.default_rng(3)
    A, B = rng.integers(0, 256, pairs), rng.integers(0, 256, pairs)
    bit = lambda x, i: ((x >> i) & 1).astype(np.uint8)
    da = [torch.from_numpy(sk.encrypt_ints(bit(A, i), 4, 100 + i)).cuda() for i in range(8)]
    db = [torch.from_numpy(sk.encrypt_ints(bit(B, i), 4, 200 + i)).cuda() for i in range(8)]
    tv = torch.from_numpy(eoc.lut_many_test_polynomial(4, [int_table(lambda s: s % 2, 4), int_table(lambda s: s >= 2, 4)])).cuda()
    outs = torch.empty((8, 2, pairs, n1), dtype=torch.int32, device="cuda")
    s = torch.empty((pairs, n1), dtype=torch.int32, device="cuda")

    def lut_add():
        for i in range(8):
            torch.add(da[i], db[i], out=s)
            if i:
                s.add_(outs[i - 1, 1])
            eng.lut_many_batch_device(2, tv.data_ptr(), 1, s.data_ptr(), outs[i].data_ptr(), pairs)

    gates, n_wires, aw, bw, sw = circuits.maj_adder(8)
    wires = torch.zeros((n_wires, pairs, n1), dtype=torch.int32, device="cuda")
    for w0, X in ((aw[0], A), (bw[0], B)):
        for i in range(8):
            wires[w0 + i] = torch.from_numpy(sk.encrypt_bits(bit(X, i), 300 + w0 + i, 0)).cuda()

    def circ_add():
        eng.circuit_run_device(gates, wires.data_ptr(), n_wires, pairs)

    t_lut, t_circ = timed_pair(lut_add, circ_add)
    o = outs.cpu().numpy()
    got = sum(sk.decrypt_ints(o[i, 0], 4).astype(np.int64) << i for i in range(8))
    got += sk.decrypt_ints(o[7, 1], 4).astype(np.int64) << 8
    w = wires[sw[0]: sw[0] + 9].cpu().numpy()
    got_c = sum(sk.decrypt_bits(w[i]).astype(np.int64) << i for i in range(9))
    r = dict(pairs=pairs, lut_many_ms=round(t_lut, 4), maj_circuit_ms=round(t_circ, 4), speedup=round(t_circ / t_lut, 4),
             lut_bootstraps_per_pair=8, circuit_bootstraps_per_pair=int(eoc.circuit_bootstraps(gates)),
             lut_ok=bool(np.array_equal(got, A + B)), circuit_ok=bool(np.array_equal(got_c, A + B)))
    print(json.dumps(r), flush=True)
    return r


if __name__ == "__main__":
    out = dict(reps=REPS, sweep=[], ripple=None)
    for pset in PSETS:
        res, ctx = sweep(pset)
        out["sweep"] += res
        if pset == 0 and "--no-ripple" not in sys.argv:
            out["ripple"] = ripple(*ctx)
        ctx[2].close()
    if "--json" in sys.argv:
        with open(sys.argv[sys.argv.index("--json") + 1], "w") as fh:
            json.dump(out, fh, indent=1)
