"""A convolution layer on compact lists against the bootstrap level that consumes it, and against the only other route to the
same outputs: a dense layer whose rows are the shifted copies of the filters (device-pointer API).
Usage (GPU box): python tools/conv_sweep.py [--json OUT]
Set A, a 28 x 28 image in one list, 1 -> 8 channels, 3 x 3 filters, the 676 valid positions of every channel (5 408 outputs per
image), batch 1, 16 and 256 (BATCHES=...).  Every batch runs in a child process of its own under a time limit (STEP_TIMEOUT
seconds), one after the other; the first child that fails or runs out of time ends the sweep.  A child times, call by call in
alternation after a second of warm-up (host time per call ending in a device synchronise):
  eoc_conv_linear_device   k_fft_fwd_polys of the lists, k_conv_lists, k_conv_extract, the key switch
  eoc_lut_batch_device     the level of 5 408 x batch sign bootstraps that reads its outputs
  eoc_linear_device        on the 5 408 x 784 matrix of shifted rows: the same outputs by the inner-product route
and, from one more profiled call each, the engine's own event times of the two linear stages' kernels
(eoc_engine_kernel_times, all booked under the key switch), with the two models' image bytes.  Both routes' outputs of the
first image are decrypt-checked against the plain correlation."""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N = 1024
BATCHES = [int(x) for x in os.environ.get("BATCHES", "1,16,256").split(",")]
REPS = int(os.environ.get("REPS", "3"))
STEP_TIMEOUT = int(os.environ.get("STEP_TIMEOUT", "240"))
HEIGHT = WIDTH = 28
COUT, KH, KW = 8, 3, 3


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


def profiled(eng, f):
    eng.set_profiling(True)
    eng.kernel_times()
    f()
    kt = eng.kernel_times()["keyswitch"]
    eng.set_profiling(False)
    return kt


def one_batch(batch):
    import torch
    import eoc_tfhe_amd as eoc
    from eoc_tfhe_amd import dinn
    p = eoc.default_params(0)
    sk = eoc.SecretKey(p, 1)
    pk = eoc.PublicKey(sk.public_key_bytes())
    eng = eoc.Engine(p)
    eng.load_cloud_key(sk)
    rng = np.random.default_rng(1)
    taps = rng.choice([-1, 1], (COUT, 1, KH, KW))
    slots = dinn.conv_slots(HEIGHT, WIDTH, KH, KW)
    conv = dinn.ConvLayer(dinn.conv2d_weights(taps, WIDTH), slots)
    n_out, pixels = conv.n_out, HEIGHT * WIDTH
    img = torch.empty(eng.weights_image_bytes(COUT, N), dtype=torch.uint8, device="cuda")
    eng.weights_to_device(conv.weights, img.data_ptr())
    d_slots = torch.empty(n_out, dtype=torch.int32, device="cuda")
    eng.conv_slots_to_device(conv.slot_table(), COUT, d_slots.data_ptr())
    # the other route: one dense row per (channel, position), the filter shifted to the position
    dense = np.zeros((COUT, slots.size, pixels), np.int8)
    at = (np.arange(KH)[:, None] * WIDTH + np.arange(KW)[None, :]).reshape(-1)
    for i, t in enumerate(slots):
        dense[:, i, t + at] = taps.reshape(COUT, KH * KW)
    dense = dense.reshape(n_out, pixels)
    dimg = torch.empty(eng.weights_image_bytes(n_out, pixels), dtype=torch.uint8, device="cuda")
    t0 = time.perf_counter()
    eng.weights_to_device(dense, dimg.data_ptr())
    dense_load_ms = (time.perf_counter() - t0) * 1e3
    d_tv = torch.from_numpy(dinn.sign_test_polynomial(1 << 29)).cuda()
    delta = 3 << 25
    x = rng.choice([-1, 1], (min(batch, 4), pixels))
    lists = np.stack([pk.encrypt_torus(v * delta, 100 + k) for k, v in enumerate(x)])
    d_lists = torch.from_numpy(np.resize(lists, (batch, 1, 2, N))).cuda()   # the first four images, repeated
    d_lin = torch.empty((batch, n_out, p.n + 1), dtype=torch.int32, device="cuda")
    d_act = torch.empty_like(d_lin)
    d_den = torch.empty_like(d_lin)
    fa = lambda: eng.conv_linear_device(img.data_ptr(), COUT, N, d_lists.data_ptr(), batch, None, d_slots.data_ptr(), n_out,
                                        d_lin.data_ptr())
    fb = lambda: eng.lut_batch_device(d_tv.data_ptr(), 1, d_lin.data_ptr(), d_act.data_ptr(), batch * n_out)
    fc = lambda: eng.linear_device(dimg.data_ptr(), n_out, pixels, d_lists.data_ptr(), batch, None, d_den.data_ptr())
    warm(torch, fa)
    ta, tb, tc = timed(torch, [fa, fb, fc])
    ka, kc = profiled(eng, fa), profiled(eng, fc)
    plain = conv.pre_activation(conv.pad_input(x[:1, None, :]) * delta)[0]
    s = np.asarray(sk.lwe_key, np.int64)
    errs = []
    for d in (d_lin, d_den):
        o = d[0].cpu().numpy().astype(np.int64)
        ph = ((o[:, -1] - o[:, :-1] @ s) + 2**31) % 2**32 - 2**31
        errs.append(float(np.abs((ph - plain + 2**31) % 2**32 - 2**31).max() / 2.0**32))
    row = dict(batch=batch, outputs_per_image=n_out, conv_linear_ms=ta, conv_kernels_ms=ka["ms"], conv_kernel_launches=int(ka["launches"]),
               bootstrap_level_ms=tb, conv_share_of_level=ta / tb, dense_linear_ms=tc, dense_kernels_ms=kc["ms"],
               dense_kernel_launches=int(kc["launches"]), dense_over_conv=tc / ta, conv_image_bytes=int(img.numel()),
               dense_image_bytes=int(dimg.numel()), dense_model_load_ms=dense_load_ms, conv_max_abs_err=errs[0], dense_max_abs_err=errs[1])
    print(json.dumps(row), flush=True)
    eng.close()


def main():
    if "--batch" in sys.argv:
        return one_batch(int(sys.argv[sys.argv.index("--batch") + 1]))
    rows = []
    for batch in BATCHES:                                    # one child per batch, each under its own time limit, chained
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--batch", str(batch)], capture_output=True, text=True,
                               timeout=STEP_TIMEOUT)
        except subprocess.TimeoutExpired:
            print(f"batch {batch}: no result within {STEP_TIMEOUT} s; the sweep ends here", flush=True)
            return 1
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-4000:])
            print(f"batch {batch}: exit status {r.returncode}; the sweep ends here", flush=True)
            return 1
        rows.append(json.loads(r.stdout.strip().splitlines()[-1]))
    if "--json" in sys.argv:
        with open(sys.argv[sys.argv.index("--json") + 1], "w") as f:
            json.dump(dict(sweep=rows), f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
