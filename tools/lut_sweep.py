"""Table lookups against NAND batches of the same job count (device-pointer API, Set A; PSET=1 for Set B).
Usage (GPU box): python tools/lut_sweep.py [--json OUT]
For 1 024, 4 096 and 16 384 rows and 1 and 4 tables, times eoc_lut_batch_device (n_luts x rows jobs) and
eoc_gate_batch_device(NAND) over n_luts x rows gates, call by call in alternation after a second of warm-up: host time per
call (device synchronise), and the engine's per-kernel event times (prepare / blind rotation / key switch; these are
averaged over BOTH calls of a pair, so they do not separate the two -- the rocprofv3 run does).  Every LUT result is decrypt-checked.  Kernel times by name come from
a separate run of this script under `rocprofv3 --kernel-trace --stats`."""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import eoc_tfhe_amd as eoc  # noqa: E402

PSET = int(os.environ.get("PSET", "0"))
ROWS = [int(x) for x in os.environ.get("ROWS", "1024,4096,16384").split(",")]
LUTS = [1, 4]
REPS = int(os.environ.get("REPS", "5"))
P = 4

params = eoc.default_params(PSET)
sk = eoc.SecretKey(params, 1)
eng = eoc.Engine(params)
eng.load_cloud_key(sk)
eng.set_profiling(True)
maxj = max(ROWS) * max(LUTS)
vals = np.random.default_rng(0).integers(0, P, max(ROWS)).astype(np.uint8)
d_in = torch.from_numpy(sk.encrypt_ints(vals, P, 1)).cuda()
bits = np.random.default_rng(1).integers(0, 2, maxj).astype(np.uint8)
c0 = torch.from_numpy(sk.encrypt_bits(bits, 2)).cuda()
c1 = torch.from_numpy(sk.encrypt_bits(bits, 3)).cuda()
d_out = torch.empty((maxj, params.n + 1), dtype=torch.int32, device="cuda")
fs = [lambda m, k=k: (m + k) % P for k in range(max(LUTS))]
tabs = [[((f(m) % P) << 32) // (2 * P) for m in range(P)] for f in fs]
tvs = np.stack([eoc.lut_test_polynomial(P, np.array(t, np.int64).astype(np.uint32).view(np.int32)) for t in tabs])
d_tv = torch.from_numpy(tvs).cuda()


def timed_pair(fa, fb):
    """fa and fb alternated call by call (the device clock drifts over a run): (host ms, kernel ms by kind) for each"""
    for _ in range(3):
        fa()
        fb()
    out = []
    for f in (fa, fb):
        torch.cuda.synchronize()
        eng.kernel_times(reset=True)
        tot = 0.0
        kt_sum = {}
        for _ in range(REPS):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            tot += time.perf_counter() - t0
            (fb if f is fa else fa)()                                   # the other one runs between two timed calls
            torch.cuda.synchronize()
        kt = eng.kernel_times(reset=True)
        out.append((tot / REPS * 1e3, {k: v["ms"] / (2 * REPS) for k, v in kt.items()}))
    return out


# a second of work first: the clock ramps up after an idle gap
t_end = time.perf_counter() + 1.0
while time.perf_counter() < t_end:
    eng.gate_batch_device(0, c0.data_ptr(), c1.data_ptr(), None, d_out.data_ptr(), 1024)
    torch.cuda.synchronize()


res = []
for rows in ROWS:
    for nl in LUTS:
        jobs = rows * nl
        lut = lambda: eng.lut_batch_device(d_tv.data_ptr(), nl, d_in.data_ptr(), d_out.data_ptr(), rows)
        nand = lambda: eng.gate_batch_device(0, c0.data_ptr(), c1.data_ptr(), None, d_out.data_ptr(), jobs)
        lut()
        torch.cuda.synchronize()
        out = d_out[:jobs].cpu().numpy().reshape(nl, rows, -1)
        ok = all(np.array_equal(sk.decrypt_ints(out[t], P), (vals[:rows] + t) % P) for t in range(nl))
        (t_lut, k_lut), (t_nand, k_nand) = timed_pair(lut, nand)
        r = dict(rows=rows, n_luts=nl, jobs=jobs, lut_ms=round(t_lut, 4), nand_ms=round(t_nand, 4),
                 lut_over_nand=round(t_lut / t_nand, 4), lut_kernel_ms={k: round(v, 4) for k, v in k_lut.items()},
                 nand_kernel_ms={k: round(v, 4) for k, v in k_nand.items()}, lut_decrypt_ok=bool(ok))
        res.append(r)
        print(json.dumps(r), flush=True)
if "--json" in sys.argv:
    with open(sys.argv[sys.argv.index("--json") + 1], "w") as fh:
        json.dump(dict(pset=PSET, p=P, reps=REPS, results=res), fh, indent=1)
