"""Dense layers on LWE samples against the list route (device-pointer API).
Usage (GPU box): python tools/lwe_matmul_sweep.py [--out FILE]
Set A.  Every shape times two legs with HIP events on one stream, alternated call by call in one process after a second of
warm-up, REPS (default 20) timed rounds:
  layer 0      rows = cols = 1 024, width n + 1, batch 8
                 leg 1  lwe_matmul_device on [8][1024][n+1] samples
                 leg 2  linear_device on one list per vector (the transform, k_dot_init, k_dot_mask, the key switch)
  hidden link  8 -> 2 and 256 -> 64, batch 64
                 leg 1  lwe_matmul_device on the [64][cols][n+1] LUT outputs
                 leg 2  64 pack_device calls (one per vector) + linear_device
Per shape: ms per call of each leg, the ratio, each leg's (max - min) / mean, the kernel's share of the int8 datasheet rate
(useful operations 2 x 4 limbs x rows x cols x width x batch per second against 5.0e15, the dense int8 figure: twice bf16),
leg 1's share of the bootstrap level that consumes the outputs (lut_batch_device on batch x rows samples, timed the same way),
and the shader clock the box reports while leg 1 runs.  The inputs are random words: neither leg's time depends on them.  The
first vector's words are checked against numpy."""
import glob
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N = 1024
REPS = int(os.environ.get("REPS", "20"))
INT8_DATASHEET = 5.0e15
SHAPES = [("layer 0", 1024, 1024, 8), ("hidden link", 2, 8, 64), ("hidden link", 64, 256, 64)]


def timed(torch, legs):
    """per leg, the ms of REPS calls between two events, the legs alternated"""
    ms = [[] for _ in legs]
    for _ in range(REPS):
        for k, f in enumerate(legs):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b))
    return [np.array(m) for m in ms]


def box_clock_mhz():
    """the highest shader clock any GPU of the host reports right now (hwmon freq1_input, read only): this process's GPU is
    the busy one; 0 where the files are not readable"""
    best = 0
    for f in glob.glob("/sys/class/drm/card*/device/hwmon/hwmon*/freq1_input"):
        try:
            best = max(best, int(open(f).read()) // 1000000)
        except (OSError, ValueError):
            pass
    return best


def warm(torch, legs, seconds=1.0):
    t_end = time.perf_counter() + seconds                   # the clock ramps up after an idle gap
    while time.perf_counter() < t_end:
        for f in legs:
            f()
        torch.cuda.synchronize()


def main():
    import torch
    import eoc_tfhe_amd as eoc
    from eoc_tfhe_amd import dinn
    p = eoc.default_params(0)
    sk = eoc.SecretKey(p, 1)
    eng = eoc.Engine(p)
    eng.load_cloud_key(sk)
    eng.load_packing_key(sk.packing_key_bytes())
    width = p.n + 1
    rng = np.random.default_rng(1)
    d_tv = torch.from_numpy(dinn.sign_test_polynomial(1 << 29)).cuda()
    lines = [f"# tools/lwe_matmul_sweep.py, Set A, width {width}, REPS {REPS}, {torch.cuda.get_device_name(0)}",
             "# what rows cols batch | lwe_ms (spread) | list_ms (spread) | lwe/list | int8 share | level_ms lwe/level | clock"]
    for what, rows, cols, batch in SHAPES:
        w = rng.integers(-3, 4, (rows, cols)).astype(np.int8)
        limg = torch.empty(eng.lwe_weights_image_bytes(rows, cols), dtype=torch.uint8, device="cuda")
        eng.lwe_weights_to_device(w, limg.data_ptr())
        img = torch.empty(eng.weights_image_bytes(rows, cols), dtype=torch.uint8, device="cuda")
        eng.weights_to_device(w, img.data_ptr())
        cts = rng.integers(-2**31, 2**31, (batch, cols, width)).astype(np.int32)
        d_cts = torch.from_numpy(cts).cuda()
        L = -(-cols // N)
        d_lists = torch.from_numpy(rng.integers(-2**31, 2**31, (batch, L, 2, N)).astype(np.int32)).cuda()
        d_a = torch.empty((batch, rows, width), dtype=torch.int32, device="cuda")
        d_b = torch.empty_like(d_a)
        d_act = torch.empty_like(d_a)

        def lwe():
            eng.lwe_matmul_device(limg.data_ptr(), rows, cols, d_cts.data_ptr(), width, batch, None, d_a.data_ptr())

        def lists_leg():
            if what != "layer 0":                               # the hidden link's pack: one call per vector, as Network.run_device
                for b in range(batch):
                    eng.pack_device(d_cts[b].data_ptr(), cols, d_lists[b].data_ptr())
            eng.linear_device(img.data_ptr(), rows, cols, d_lists.data_ptr(), batch, None, d_b.data_ptr())

        def level():
            eng.lut_batch_device(d_tv.data_ptr(), 1, d_a.data_ptr(), d_act.data_ptr(), batch * rows)

        legs = [lwe, lists_leg, level]
        warm(torch, legs)
        t_lwe, t_list, t_level = timed(torch, legs)
        for _ in range(50):                                      # the clock the box holds under leg 1, read while it runs
            lwe()
        mhz = box_clock_mhz()
        torch.cuda.synchronize()
        want = (w.astype(np.int64) @ cts[0].view(np.uint32).astype(np.int64)) & 0xFFFFFFFF
        assert np.array_equal(d_a[0].cpu().numpy().view(np.uint32), want.astype(np.uint32)), "leg 1 differs from numpy"
        spread = lambda t: (t.max() - t.min()) / t.mean()
        share = 2.0 * 4 * rows * cols * width * batch / (t_lwe.mean() * 1e-3) / INT8_DATASHEET
        lines.append(f"{what} {rows} {cols} {batch} | {t_lwe.mean():.4f} ({spread(t_lwe):.2f}) | {t_list.mean():.4f} "
                     f"({spread(t_list):.2f}) | {t_lwe.mean() / t_list.mean():.4f} | {share:.5f} | {t_level.mean():.3f} "
                     f"{t_lwe.mean() / t_level.mean():.5f} | {mhz} MHz")
        print(lines[-1], flush=True)
    eng.close()
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
