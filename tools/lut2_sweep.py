"""Two-input lookups: what the encrypted seed and the composed call cost (device-pointer API).
Usage (GPU box): python tools/lut2_sweep.py [--json OUT] [--level2-only]
One process, calls alternated after a second of warm-up, host time per call (device synchronise), every result
decrypt-checked.

  level 2 alone   eoc_lut_enc_batch_device (per_row = 1: 8 KiB of seed per job) against eoc_lut_batch_device (a shared 4 KiB
                  polynomial) at equal job counts -- 1 024, 4 096 and 16 384 jobs (JOBS), Set A and Set B (PSETS) -- REPS
                  alternated calls each: mean ms per call, the ratio, and the _tv leg's own max - min over its calls (the spread
                  the ratio is read against).  Per launch by kernel name: run this script once more with --level2-only under
                  `rocprofv3 --kernel-trace --stats`.
  composed call   eoc_lut2_batch_device per row and function at p = 4, T in {1, 2, 4} (Set B at T = 4 is timed but not decoded:
                  its level-1 margin is below 6 sigma), ROWS2 rows, split into level 1, pack and
                  level 2 by eoc_engine_kernel_times around each of the three calls the composed call consists of
                  (lut_batch / lut_many_batch, tv_pack, lut_enc_batch), beside the cost model
                  (p / T + 1) t_job + (p + 1) t_ks + t_list with the per-job, per-key-switch and per-list times of the same run."""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import eoc_tfhe_amd as eoc  # noqa: E402

PSETS = [int(x) for x in os.environ.get("PSETS", "0,1").split(",")]
JOBS = [int(x) for x in os.environ.get("JOBS", "1024,4096,16384").split(",")]
ROWS2 = int(os.environ.get("ROWS2", "4096"))
REPS = int(os.environ.get("REPS", "5"))
P = 4
N = 1024


def int_table(f, p):
    return np.array([((int(f(m)) % p) << 32) // (2 * p) for m in range(p)], np.uint64).astype(np.uint32).view(np.int32)


def table2(F, p):
    return np.array([[((int(F(x, y)) % p) << 32) // (2 * p) for y in range(p)] for x in range(p)], np.uint64).astype(np.uint32).view(np.int32)


def timed_pair(fa, fb):
    """fa and fb alternated call by call (the device clock drifts over a run): per-call host ms of each, REPS values"""
    for _ in range(3):
        fa()
        fb()
    ms = [[], []]
    for _ in range(REPS):
        for k, f in enumerate((fa, fb)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) * 1e3)
    return ms


def warm(eng, sk):
    c0 = torch.from_numpy(sk.encrypt_bits(np.zeros(1024, np.uint8), 2)).cuda()
    out = torch.empty_like(c0)
    t_end = time.perf_counter() + 1.0                        # a second of work first: the clock ramps up after an idle gap
    while time.perf_counter() < t_end:
        eng.gate_batch_device(0, c0.data_ptr(), c0.data_ptr(), None, out.data_ptr(), 1024)
        torch.cuda.synchronize()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def level2(pset, params, sk, eng):
    """the encrypted-seed kernel against its _tv twin at equal job counts"""
    res = []
    n1 = params.n + 1
    f = lambda m: (3 * m + 1) % P                             # noqa: E731
    tv = eoc.lut_test_polynomial(P, int_table(f, P))
    rows = max(JOBS)
    yv = np.random.default_rng(1).integers(0, P, rows).astype(np.uint8)
    d_y = dev(sk.encrypt_ints(yv, P, 11))
    d_tv = dev(tv)
    # one list per job: 64 distinct packed lists of f, repeated (the seed traffic is per job whatever the lists hold)
    vals = sk.encrypt_ints(np.tile(np.array([f(m) for m in range(P)], np.uint8), 64), P, 12).reshape(64, P, n1).transpose(1, 0, 2)
    d_vals = dev(vals[None])
    d_l64 = torch.empty((64, 2, N), dtype=torch.int32, device="cuda")
    eng.tv_pack_device(P, d_vals.data_ptr(), 1, 64, d_l64.data_ptr())
    d_lists = d_l64.repeat(rows // 64, 1, 1).contiguous()
    for jobs in JOBS:
        d_o1 = torch.empty((1, jobs, n1), dtype=torch.int32, device="cuda")
        d_o2 = torch.empty_like(d_o1)
        enc = lambda: eng.lut_enc_batch_device(d_lists.data_ptr(), 1, True, d_y.data_ptr(), d_o1.data_ptr(), jobs)   # noqa: E731
        pub = lambda: eng.lut_batch_device(d_tv.data_ptr(), 1, d_y.data_ptr(), d_o2.data_ptr(), jobs)              # noqa: E731
        ms_enc, ms_tv = timed_pair(enc, pub)
        want = np.array([f(v) for v in yv[:jobs]])
        ok = all(np.array_equal(sk.decrypt_ints(o.cpu().numpy()[0], P), want) for o in (d_o1, d_o2))
        m_enc, m_tv = float(np.mean(ms_enc)), float(np.mean(ms_tv))
        r = dict(what="level2", pset=pset, jobs=jobs, enc_ms=round(m_enc, 4), tv_ms=round(m_tv, 4), ratio=round(m_enc / m_tv, 4),
                 tv_spread=round((max(ms_tv) - min(ms_tv)) / m_tv, 4), enc_spread=round((max(ms_enc) - min(ms_enc)) / m_enc, 4),
                 enc_us_per_job=round(m_enc / jobs * 1e3, 3), tv_us_per_job=round(m_tv / jobs * 1e3, 3), decrypt_ok=bool(ok))
        res.append(r)
        print(json.dumps(r), flush=True)
    return res


def kernel_ms(eng, fn):
    """(prepare, blind rotation, key switch + pack kernels) device ms of one call, by the engine's event spans"""
    torch.cuda.synchronize()
    eng.kernel_times()
    fn()
    torch.cuda.synchronize()
    t = eng.kernel_times()
    return {k: t[k]["ms"] for k in ("prepare", "blind_rotate", "keyswitch")}


def composed(pset, params, sk, eng):
    res = []
    n1, S = params.n + 1, ROWS2
    F = lambda x, y: (x + y) % P                              # noqa: E731
    rng = np.random.default_rng(2)
    xv, yv = rng.integers(0, P, S).astype(np.uint8), rng.integers(0, P, S).astype(np.uint8)
    d_x, d_y = dev(sk.encrypt_ints(xv, P, 21)), dev(sk.encrypt_ints(yv, P, 22))
    want = np.array([F(int(a), int(b)) for a, b in zip(xv, yv)])
    d_vals = torch.empty((P, S, n1), dtype=torch.int32, device="cuda")
    d_lists = torch.empty((S, 2, N), dtype=torch.int32, device="cuda")
    d_out = torch.empty((1, S, n1), dtype=torch.int32, device="cuda")
    d_out3 = torch.empty_like(d_out)
    eng.set_profiling(True)
    for T in (1, 2, 4):
        d_tv0 = dev(eoc.lut2_test_polynomials(P, table2(F, P), T))

        def l1():
            if T == 1:
                eng.lut_batch_device(d_tv0.data_ptr(), P, d_x.data_ptr(), d_vals.data_ptr(), S)
            else:
                eng.lut_many_batch_device(T, d_tv0.data_ptr(), P // T, d_x.data_ptr(), d_vals.data_ptr(), S)
        pk = lambda: eng.tv_pack_device(P, d_vals.data_ptr(), 1, S, d_lists.data_ptr())                              # noqa: E731
        l2 = lambda: eng.lut_enc_batch_device(d_lists.data_ptr(), 1, True, d_y.data_ptr(), d_out3.data_ptr(), S)     # noqa: E731
        whole = lambda: eng.lut2_batch_device(P, T, d_tv0.data_ptr(), 1, d_x.data_ptr(), d_y.data_ptr(), d_out.data_ptr(), S)   # noqa: E731
        for _ in range(2):
            whole()
        parts = []
        for _ in range(REPS):                                 # the three stages and the composed call, alternated
            a, b, c, w = kernel_ms(eng, l1), kernel_ms(eng, pk), kernel_ms(eng, l2), kernel_ms(eng, whole)
            parts.append((sum(a.values()), b["keyswitch"], sum(c.values()), sum(w.values()), a["blind_rotate"], a["keyswitch"],
                          c["blind_rotate"], c["keyswitch"]))
        m = np.mean(np.array(parts), axis=0)
        same = bool(torch.equal(d_out, d_out3))               # the three calls ARE the composed call
        got = sk.decrypt_ints(d_out.cpu().numpy()[0], P)
        ok = bool(np.array_equal(got, want)) if not (pset == 1 and T == 4) else None
        t_job = m[6] / S                                      # per blind-rotation job: level 2's, this run
        t_ks = m[7] / S                                       # per key switch
        t_list = m[1] / S                                     # per list: gather + k_pack_rows
        model = (P // T + 1) * t_job + (P + 1) * t_ks + t_list
        r = dict(what="composed", pset=pset, p=P, T=T, rows=S, level1_us=round(m[0] / S * 1e3, 3), pack_us=round(m[1] / S * 1e3, 3),
                 level2_us=round(m[2] / S * 1e3, 3), sum_us=round((m[0] + m[1] + m[2]) / S * 1e3, 3),
                 composed_us=round(m[3] / S * 1e3, 3), model_us=round(model * 1e3, 3), job_us=round(t_job * 1e3, 3),
                 ks_us=round(t_ks * 1e3, 3), list_us=round(t_list * 1e3, 3), l1_br_us=round(m[4] / S * 1e3, 3),
                 l1_ks_us=round(m[5] / S * 1e3, 3), stages_equal_composed=same, decrypt_ok=ok)
        res.append(r)
        print(json.dumps(r), flush=True)
    eng.set_profiling(False)
    return res


if __name__ == "__main__":
    out = dict(reps=REPS, level2=[], composed=[])
    for pset in PSETS:
        params = eoc.default_params(pset)
        sk = eoc.SecretKey(params, 1)
        eng = eoc.Engine(params)
        eng.load_cloud_key(sk)
        eng.load_packing_key(sk.packing_key_bytes())
        warm(eng, sk)
        out["level2"] += level2(pset, params, sk, eng)
        if "--level2-only" not in sys.argv:
            out["composed"] += composed(pset, params, sk, eng)
        eng.close()
    if "--json" in sys.argv:
        with open(sys.argv[sys.argv.index("--json") + 1], "w") as fh:
            json.dump(out, fh, indent=1)
