"""Seeded inputs and the seeded cloud key (device-pointer API): what the expansion on the device costs beside
the upload it replaces.
Usage (GPU box): python tools/seeded_sweep.py [--out FILE]
Inputs, Set A, COUNTS (1 024, 16 384, 262 144) samples: host time per call ending in a device synchronise, REPS calls each,
two alternated rounds, of
  expand   eoc_seeded_expand_device on bodies already on the device (their own upload, 4 bytes per sample, is timed apart as
           bodies_h2d), with the kernel's own time from the engine's events (eoc_engine_kernel_times, booked under prepare);
  h2d      a pinned-memory H2D copy of the same [count][n + 1] samples: the only way to put unseeded samples on the device.
The expansion is checked once per point against the host twin on 64 samples spread over the batch.
Global context, Set A, the same COUNTS on one engine and on three engines of device 0 (GLOBAL_DEVICES): eoc_seeded_expand on
pageable host buffers, the whole synchronous call (bodies up, expansion, samples down), REPS calls, two rounds; the result is
checked once per point against the host twin on the same 64 samples.
Key install, PSETS (0, 1): eoc_engine_load_seeded_cloud_key (EOCCKS1 blob) alternated with eoc_engine_load_cloud_key (the
torus-form arrays of the same key material, host-expanded), KEY_REPS calls each; both are synchronous."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COUNTS = [int(x) for x in os.environ.get("COUNTS", "1024,16384,262144").split(",")]
PSETS = [int(x) for x in os.environ.get("PSETS", "0,1").split(",")]
REPS = int(os.environ.get("REPS", "10"))
KEY_REPS = int(os.environ.get("KEY_REPS", "3"))
GLOBAL_DEVICES = [[0], [0, 0, 0]]
SEED = bytes(range(32))


def host_ms(torch, f, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def input_point(eoc, torch, eng, p, count):
    rng = np.random.default_rng(count)
    bodies = rng.integers(-2**31, 2**31, count).astype(np.int32)
    h_bodies = torch.from_numpy(bodies).pin_memory()
    h_full = torch.empty((count, p.n + 1), dtype=torch.int32).pin_memory()
    d_bodies = torch.empty(count, dtype=torch.int32, device="cuda")
    d_out = torch.empty((count, p.n + 1), dtype=torch.int32, device="cuda")
    d_bodies.copy_(h_bodies)
    expand = lambda: eng.seeded_expand_device(SEED, d_bodies.data_ptr(), count, d_out.data_ptr())
    h2d = lambda: d_out.copy_(h_full, non_blocking=True)
    bod = lambda: d_bodies.copy_(h_bodies, non_blocking=True)
    expand()
    torch.cuda.synchronize()
    idx = np.unique(np.r_[0, count - 1, rng.integers(0, count, 62)])
    got = d_out[torch.from_numpy(idx).cuda()].cpu().numpy()
    ok = all(np.array_equal(got[k], eoc.seeded_expand_host(p, SEED, bodies[i:i + 1], int(i))[0]) for k, i in enumerate(idx))
    e_host = e_kernel = c_host = b_host = 0.0
    for _ in range(2):                                                       # alternated: expand, copy, expand, copy
        eng.set_profiling(True)
        eng.kernel_times(reset=True)
        e_host += host_ms(torch, expand, REPS) / 2
        e_kernel += eng.kernel_times(reset=True)["prepare"]["ms"] / REPS / 2
        eng.set_profiling(False)
        c_host += host_ms(torch, h2d, REPS) / 2
        b_host += host_ms(torch, bod, REPS) / 2
    full_bytes = count * (p.n + 1) * 4
    return dict(samples=count, expand_host_ms=e_host, expand_kernel_ms=e_kernel, bodies_h2d_host_ms=b_host,
                full_h2d_host_ms=c_host, full_bytes=full_bytes, seeded_bytes=count * 4 + 32,
                full_h2d_GBps=full_bytes / c_host / 1e6, expand_out_GBps=full_bytes / max(e_kernel, 1e-9) / 1e6,
                kernel_ns_per_sample=e_kernel * 1e6 / count, h2d_over_expand_plus_bodies=c_host / (e_host + b_host),
                expansion_equals_host=bool(ok))


def global_point(eoc, p, count, devices):
    rng = np.random.default_rng(count)
    bodies = rng.integers(-2**31, 2**31, count).astype(np.int32)
    seed = np.frombuffer(SEED, np.uint8)
    out = np.zeros((count, p.n + 1), np.int32)
    call = lambda: eoc.lib().eoc_seeded_expand(seed.ctypes.data, 0, bodies.ctypes.data, count, out.ctypes.data)
    eoc.gpu_shutdown()
    eoc.gpu_init(p, devices=devices)
    try:
        assert call() == 0, eoc.lib().eoc_last_error()
        idx = np.unique(np.r_[0, count - 1, rng.integers(0, count, 62)])
        ok = all(np.array_equal(out[i], eoc.seeded_expand_host(p, SEED, bodies[i:i + 1], int(i))[0]) for i in idx)
        grows = eoc.stats_multi()["host_buffer_grows"]
        ms = []
        for _ in range(2):
            t0 = time.perf_counter()
            for _ in range(REPS):
                call()
            ms.append((time.perf_counter() - t0) / REPS * 1e3)
        grows = eoc.stats_multi()["host_buffer_grows"] - grows
        return dict(samples=count, engines=len(devices), global_expand_host_ms=sum(ms) / 2, rounds_ms=ms,
                    us_per_sample=sum(ms) / 2 * 1e3 / count, host_buffer_grows_in_timed_calls=grows,
                    expansion_equals_host=bool(ok))
    finally:
        eoc.gpu_shutdown()


def key_point(eoc, torch, pset):
    p = eoc.default_params(pset)
    sk = eoc.SecretKey(p, 1, with_cloud_key=False)
    blob = sk.seeded_cloud_key_bytes()
    bk, ksk = eoc.seeded_cloud_key_expand(blob)
    eng = eoc.Engine(p)
    seeded = lambda: eng.load_seeded_cloud_key(blob)
    plain = lambda: eng.load_cloud_key(bk, ksk)
    seeded()
    plain()
    s_ms = p_ms = 0.0
    for _ in range(2):
        s_ms += host_ms(torch, seeded, KEY_REPS) / 2
        p_ms += host_ms(torch, plain, KEY_REPS) / 2
    eng.close()
    return dict(pset=pset, load_seeded_ms=s_ms, load_torus_ms=p_ms, seeded_blob_bytes=int(blob.size),
                torus_bytes=int(bk.nbytes + ksk.nbytes), torus_over_seeded=p_ms / s_ms)


def main():
    import torch
    import eoc_tfhe_amd as eoc
    lines = []
    p = eoc.default_params(0)
    eng = eoc.Engine(p)
    for count in COUNTS:
        lines.append(json.dumps(dict(pset=0, **input_point(eoc, torch, eng, p, count))))
        print(lines[-1], flush=True)
    eng.close()
    for devices in GLOBAL_DEVICES:
        for count in COUNTS:
            lines.append(json.dumps(dict(pset=0, **global_point(eoc, p, count, devices))))
            print(lines[-1], flush=True)
    for pset in PSETS:
        lines.append(json.dumps(key_point(eoc, torch, pset)))
        print(lines[-1], flush=True)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
