"""Compact-list expansion against the key switch alone (device-pointer API), and client encryption speed.
Usage (GPU box): python tools/compact_sweep.py [--json OUT]
For Set A and Set B (PSETS=0,1) and 1 024, 16 384 and 262 144 samples (COUNTS=...), times eoc_compact_expand_device
(k_compact_expand + the key switch) and eoc_keyswitch_device on the same count (a device-to-device copy of [count][N+1]
extracted samples + the same key switch), call by call in alternation after a second of warm-up: host time per call (device
synchronise).  Expanded samples are decrypt-checked.  Then client encryption (eoc_pk_encrypt_bits_keyed) per 1 024 bits over
LISTS lists on eoc_host_threads() threads and, in a child process with EOC_TFHE_THREADS=1, on one thread.  Kernel times by
name come from a separate run of this script under `rocprofv3 --kernel-trace --stats` (ENCRYPT=0 skips the client part)."""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N = 1024
PSETS = [int(x) for x in os.environ.get("PSETS", "0,1").split(",")]
COUNTS = [int(x) for x in os.environ.get("COUNTS", "1024,16384,262144").split(",")]
REPS = int(os.environ.get("REPS", "5"))
LISTS = int(os.environ.get("LISTS", "64"))


def encrypt_rate(eoc, lists):
    """ms per 1 024 bits (one list) of secure compact encryption on this process's thread count"""
    sk = eoc.SecretKey(eoc.default_params(0), None, with_cloud_key=False)
    pk = eoc.PublicKey(sk.public_key_bytes())
    bits = np.random.default_rng(1).integers(0, 2, lists * N).astype(np.uint8)
    pk.encrypt_bits(bits[:N])
    t0 = time.perf_counter()
    pk.encrypt_bits(bits)
    return (time.perf_counter() - t0) * 1e3 / lists


def timed_pair(torch, fa, fb):
    for _ in range(2):
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


def sweep(eoc, torch, pset):
    p = eoc.default_params(pset)
    sk = eoc.SecretKey(p, 1)
    pk = eoc.PublicKey(sk.public_key_bytes())
    eng = eoc.Engine(p)
    eng.load_cloud_key(sk)
    rows = []
    for count in COUNTS:
        bits = np.random.default_rng(count).integers(0, 2, count).astype(np.uint8)
        d_lists = torch.from_numpy(pk.encrypt_bits(bits, enc_seed=count)).cuda()
        d_out = torch.empty((count, p.n + 1), dtype=torch.int32, device="cuda")
        d_u = torch.randint(-2**31, 2**31 - 1, (count, N + 1), dtype=torch.int32, device="cuda")
        d_ks = torch.empty_like(d_out)
        fa = lambda: eng.compact_expand_device(d_lists.data_ptr(), count, d_out.data_ptr())
        fb = lambda: eng.keyswitch_device(d_u.data_ptr(), d_ks.data_ptr(), count)
        t_end = time.perf_counter() + 1.0                   # the clock ramps up after an idle gap
        while time.perf_counter() < t_end:
            fa()
            torch.cuda.synchronize()
        ta, tb = timed_pair(torch, fa, fb)
        ok = bool(np.array_equal(sk.decrypt_bits(d_out.cpu().numpy()), bits))
        row = dict(pset=pset, count=count, expand_ms=ta, keyswitch_ms=tb, ratio=ta / tb,
                   samples_per_s=count / (ta * 1e-3), decrypt_ok=ok)
        print(json.dumps(row), flush=True)
        rows.append(row)
        del d_lists, d_out, d_u, d_ks
    eng.close()
    return rows


def main():
    if "--encrypt-child" in sys.argv:
        import eoc_tfhe_amd as eoc
        print(json.dumps(dict(ms_per_1024=encrypt_rate(eoc, LISTS), threads=eoc.lib().eoc_host_threads())))
        return
    import torch
    import eoc_tfhe_amd as eoc
    out = dict(sweep=[], encrypt=[])
    for pset in PSETS:
        out["sweep"] += sweep(eoc, torch, pset)
    if os.environ.get("ENCRYPT", "1") != "0":
        out["encrypt"].append(dict(threads=eoc.lib().eoc_host_threads(), ms_per_1024=encrypt_rate(eoc, LISTS)))
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--encrypt-child"], capture_output=True, text=True,
                           env=dict(os.environ, EOC_TFHE_THREADS="1"), timeout=600, check=True)
        out["encrypt"].append(json.loads(r.stdout.strip().splitlines()[-1]))
        for e in out["encrypt"]:
            print(json.dumps(e), flush=True)
    if "--json" in sys.argv:
        with open(sys.argv[sys.argv.index("--json") + 1], "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
