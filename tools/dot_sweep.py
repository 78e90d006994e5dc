"""The linear stage of a dense layer against the bootstrap level that consumes it, and against the only other route to the
same sums (device-pointer API).
Usage (GPU box): python tools/dot_sweep.py [--json OUT]
Set A, (rows, cols) = (1 024, 1 024), batch 1, 16 and 256 (BATCHES=...): times eoc_linear_device (k_fft_fwd_polys of the lists,
k_dot_init, k_dot_mask, the key switch) and the level of rows x batch sign bootstraps that reads its outputs
(eoc_lut_batch_device), call by call in alternation after a second of warm-up: host time per call ending in a device
synchronise, and the engine's own event times of the linear stage's kernels (eoc_engine_kernel_times, all booked under the
key switch) from one more profiled call.  At batch 1 the other route is timed too: eoc_compact_expand_device of the 1 024
inputs (one key switch per INPUT) and the weighted sums of the [1 024][n+1] rows in numpy on the host.  One output row is
decrypt-checked against the plain sum."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N = 1024
BATCHES = [int(x) for x in os.environ.get("BATCHES", "1,16,256").split(",")]
REPS = int(os.environ.get("REPS", "3"))
ROWS = COLS = 1024


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


def main():
    import torch
    import eoc_tfhe_amd as eoc
    from eoc_tfhe_amd import dinn
    p = eoc.default_params(0)
    sk = eoc.SecretKey(p, 1)
    pk = eoc.PublicKey(sk.public_key_bytes())
    eng = eoc.Engine(p)
    eng.load_cloud_key(sk)
    rng = np.random.default_rng(1)
    w = rng.integers(-3, 4, (ROWS, COLS)).astype(np.int8)
    img = torch.empty(eng.weights_image_bytes(ROWS, COLS), dtype=torch.uint8, device="cuda")
    t0 = time.perf_counter()
    eng.weights_to_device(w, img.data_ptr())
    load_ms = (time.perf_counter() - t0) * 1e3
    d_tv = torch.from_numpy(dinn.sign_test_polynomial(1 << 29)).cuda()
    delta = 1 << 19                                         # |sum w x| is near 64 here: pre-activations near 2^-7, far inside 1/4
    rows = []
    for batch in BATCHES:
        x = rng.choice([-1, 1], (batch, COLS))
        lists = np.stack([pk.encrypt_torus(v * delta, 100 + k) for k, v in enumerate(x[:4])])
        lists = np.resize(lists, (batch, 1, 2, N))          # the first four vectors, repeated: the timing does not read them
        d_lists = torch.from_numpy(lists).cuda()
        d_lin = torch.empty((batch, ROWS, p.n + 1), dtype=torch.int32, device="cuda")
        d_act = torch.empty_like(d_lin)
        fa = lambda: eng.linear_device(img.data_ptr(), ROWS, COLS, d_lists.data_ptr(), batch, None, d_lin.data_ptr())
        fb = lambda: eng.lut_batch_device(d_tv.data_ptr(), 1, d_lin.data_ptr(), d_act.data_ptr(), batch * ROWS)
        warm(torch, fa)
        ta, tb = timed(torch, [fa, fb])
        eng.set_profiling(True)
        eng.kernel_times()
        fa()
        kt = eng.kernel_times()["keyswitch"]
        eng.set_profiling(False)
        out = d_lin[0].cpu().numpy().astype(np.int64)
        ph = ((out[:, -1] - out[:, :-1] @ np.asarray(sk.lwe_key, np.int64)) + 2**31) % 2**32 - 2**31
        err = (ph - (w.astype(np.int64) @ x[0]) * delta) / 2.0**32
        row = dict(rows=ROWS, cols=COLS, batch=batch, linear_ms=ta, linear_kernels_ms=kt["ms"], linear_kernel_launches=int(kt["launches"]),
                   bootstrap_level_ms=tb, linear_share_of_level=ta / tb, max_abs_err=float(np.abs(err).max()), model_load_ms=load_ms)
        if batch == 1:
            d_exp = torch.empty((COLS, p.n + 1), dtype=torch.int32, device="cuda")

            def other():
                eng.compact_expand_device(d_lists.data_ptr(), COLS, d_exp.data_ptr())
                torch.cuda.synchronize()
                rows_ = d_exp.cpu().numpy().astype(np.int64)
                return (w.astype(np.int64) @ rows_).astype(np.uint32)            # wrapping sums, [rows][n+1]
            tc = timed(torch, [other])[0]
            row.update(expand_and_host_sum_ms=tc, ratio_other_route=tc / ta)
        print(json.dumps(row), flush=True)
        rows.append(row)
        del d_lists, d_lin, d_act
    eng.close()
    if "--json" in sys.argv:
        with open(sys.argv[sys.argv.index("--json") + 1], "w") as f:
            json.dump(dict(sweep=rows), f, indent=1)


if __name__ == "__main__":
    main()
