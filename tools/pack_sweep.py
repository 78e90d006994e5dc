"""The packing key switch against the only other way to move the same samples (device-pointer API).
Usage (GPU box): python tools/pack_sweep.py [--json OUT]
For Set A and Set B (PSETS=0,1) and 1, 16 and 256 lists (LISTS=...; a list is 1 024 samples), times eoc_pack_device
(k_pack_gather + k_pack_rows) and eoc_keyswitch_device on the same sample count (what the parent had for samples on their way
out: a device-to-device copy of [count][N+1] + the LWE key switch; its input here is random words), call by call in
alternation after a second of warm-up: host time per call ending in a device synchronise, and the engine's own event times of
the two packing kernels (eoc_engine_kernel_times, booked under the key switch) from one more profiled call.  For scale, one
level of 1 024 NAND gates (eoc_gate_batch_device) is timed the same way.  Packed lists are decrypt-checked.  Kernel times by
name come from a separate run of this script under `rocprofv3 --kernel-trace --stats`."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N = 1024
PSETS = [int(x) for x in os.environ.get("PSETS", "0,1").split(",")]
LISTS = [int(x) for x in os.environ.get("LISTS", "1,16,256").split(",")]
REPS = int(os.environ.get("REPS", "5"))


def timed(torch, fns):
    """ms per call of each of `fns`, alternated REPS times after two untimed rounds"""
    for _ in range(2):
        for f in fns:
            f()
    tot = [0.0] * len(fns)
    for _ in range(REPS):
        for k, f in enumerate(fns):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            tot[k] += time.perf_counter() - t0
    return [t / REPS * 1e3 for t in tot]


def warm(torch, f, seconds=1.0):
    t_end = time.perf_counter() + seconds                   # the clock ramps up after an idle gap
    while time.perf_counter() < t_end:
        f()
        torch.cuda.synchronize()


def sweep(eoc, torch, pset):
    p = eoc.default_params(pset)
    sk = eoc.SecretKey(p, 1)
    eng = eoc.Engine(p)
    eng.load_cloud_key(sk)
    eng.load_packing_key(sk.packing_key_bytes())
    rows = []
    # scale: one bootstrap level of 1 024 gates
    bits = np.random.default_rng(1).integers(0, 2, 2 * N).astype(np.uint8)
    d_a = torch.from_numpy(sk.encrypt_bits(bits[:N], 1)).cuda()
    d_b = torch.from_numpy(sk.encrypt_bits(bits[N:], 2)).cuda()
    d_g = torch.empty_like(d_a)
    gate = lambda: eng.gate_batch_device(eoc.OPS["NAND"], d_a.data_ptr(), d_b.data_ptr(), None, d_g.data_ptr(), N)
    warm(torch, gate)
    gate_ms = timed(torch, [gate])[0]
    for lists in LISTS:
        count = lists * N
        bits = np.random.default_rng(count).integers(0, 2, count).astype(np.uint8)
        d_in = torch.from_numpy(sk.encrypt_bits(bits, count)).cuda()
        d_lists = torch.empty((lists, 2, N), dtype=torch.int32, device="cuda")
        d_u = torch.randint(-2**31, 2**31 - 1, (count, N + 1), dtype=torch.int32, device="cuda")
        d_ks = torch.empty((count, p.n + 1), dtype=torch.int32, device="cuda")
        fa = lambda: eng.pack_device(d_in.data_ptr(), count, d_lists.data_ptr())
        fb = lambda: eng.keyswitch_device(d_u.data_ptr(), d_ks.data_ptr(), count)
        warm(torch, fa)
        ta, tb = timed(torch, [fa, fb])
        eng.set_profiling(True)
        eng.kernel_times()
        fa()
        kt = eng.kernel_times()["keyswitch"]
        eng.set_profiling(False)
        ok = bool(np.array_equal(sk.decrypt_list_bits(d_lists.cpu().numpy(), count), bits))
        row = dict(pset=pset, lists=lists, samples=count, pack_ms=ta, pack_us_per_list=ta * 1e3 / lists,
                   pack_kernels_ms=kt["ms"], pack_kernel_launches=int(kt["launches"]), keyswitch_ms=tb, ratio=ta / tb,
                   gate_level_1024_ms=gate_ms, list_share_of_gate_level=ta / lists / gate_ms, decrypt_ok=ok)
        print(json.dumps(row), flush=True)
        rows.append(row)
        del d_in, d_lists, d_u, d_ks
    eng.close()
    return rows


def main():
    import torch
    import eoc_tfhe_amd as eoc
    out = dict(sweep=[])
    for pset in PSETS:
        out["sweep"] += sweep(eoc, torch, pset)
    if "--json" in sys.argv:
        with open(sys.argv[sys.argv.index("--json") + 1], "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
