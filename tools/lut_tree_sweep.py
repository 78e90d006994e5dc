"""Multi-digit lookups: what the exact matrix-core pack and the deeper trees cost (device-pointer API).
Usage (GPU box): python tools/lut_tree_sweep.py [--json OUT] [--pack-only]
One process, legs alternated call by call after a second of warm-up, host time per call (device synchronise), every result
decrypt-checked.

  the pack        eoc_tv_pack_exact_device against eoc_tv_pack_device on the same inputs at p = 4, LISTS lists (256 and
                  4 096), Set A and Set B (PSETS), REPS alternated calls each: mean ms per call, us per list, the ratio, each
                  leg's own max - min over its calls, and the device time of each leg's kernels from eoc_engine_kernel_times
                  (k_tvpack_mm + k_tv_spread together; by kernel name: run once more with --pack-only under
                  `rocprofv3 --kernel-trace --stats`).
  d = 2           eoc_lut_tree_batch_device against eoc_lut2_batch_device at ROWS2 rows, p = 4, T in {1, 4}, alternated.
  d = 3, 4        device time per row and function (engine events) beside the cost model rotations x t_job + key switches x
                  t_ks + lists x t_list, with t_job and t_ks from an eoc_lut_enc_batch_device call and t_list from the exact
                  pack of the same run (SHAPES: (p, d, T), ROWS3 rows)."""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import eoc_tfhe_amd as eoc  # noqa: E402

PSETS = [int(x) for x in os.environ.get("PSETS", "0,1").split(",")]
LISTS = [int(x) for x in os.environ.get("LISTS", "256,4096").split(",")]
ROWS2 = int(os.environ.get("ROWS2", "4096"))
ROWS3 = int(os.environ.get("ROWS3", "1024"))
REPS = int(os.environ.get("REPS", "5"))
SHAPES = [(4, 3, 1), (4, 3, 4), (4, 4, 4), (2, 4, 2)]
P = 4
N = 1024


def torus_table(F, p, d):
    t = np.zeros((p,) * d, np.uint64)
    for idx in np.ndindex(*t.shape):
        t[idx] = ((int(F(*idx)) % p) << 32) // (2 * p)
    return t.astype(np.uint32).view(np.int32)


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


def kernel_ms(eng, fn):
    """(prepare, blind rotation, key switch + pack kernels) device ms of one call, by the engine's event spans"""
    torch.cuda.synchronize()
    eng.kernel_times()
    fn()
    torch.cuda.synchronize()
    t = eng.kernel_times()
    return {k: t[k]["ms"] for k in ("prepare", "blind_rotate", "keyswitch")}


def spread(ms):
    return round((max(ms) - min(ms)) / float(np.mean(ms)), 4)


def pack(pset, params, sk, eng):
    res = []
    n1 = params.n + 1
    for lists in LISTS:
        msgs = np.random.default_rng(lists).integers(0, P, P * lists).astype(np.uint8)
        vals = sk.encrypt_ints(msgs, P, 31).reshape(1, P, lists, n1)
        d_vals = dev(vals)
        d_a = torch.empty((lists, 2, N), dtype=torch.int32, device="cuda")
        d_b = torch.empty_like(d_a)
        new = lambda: eng.tv_pack_exact_device(P, d_vals.data_ptr(), 1, lists, d_a.data_ptr())      # noqa: E731
        old = lambda: eng.tv_pack_device(P, d_vals.data_ptr(), 1, lists, d_b.data_ptr())            # noqa: E731
        ms_new, ms_old = timed_pair(new, old)
        eng.set_profiling(True)
        k_new = float(np.mean([kernel_ms(eng, new)["keyswitch"] for _ in range(REPS)]))
        k_old = float(np.mean([kernel_ms(eng, old)["keyswitch"] for _ in range(REPS)]))
        eng.set_profiling(False)
        a, b = d_a.cpu().numpy(), d_b.cpu().numpy()
        diff = int(np.abs((a.astype(np.int64) - b.astype(np.int64) + 2**31) % 2**32 - 2**31).max())
        few = slice(0, min(lists, 64))
        ok = True
        for got in (a[few], b[few]):                          # the middle of window j decrypts as sample j does
            ph = sk.list_phases(got).astype(np.int64)
            for j in range(P):
                ok &= bool(np.array_equal(((ph[:, j * (N // P)] * 2 * P + (1 << 31)) >> 32) % P, msgs.reshape(P, lists)[j, few]))
        m_new, m_old = float(np.mean(ms_new)), float(np.mean(ms_old))
        r = dict(what="pack", pset=pset, p=P, lists=lists, exact_ms=round(m_new, 4), fft_ms=round(m_old, 4),
                 ratio=round(m_new / m_old, 4), exact_us_per_list=round(m_new / lists * 1e3, 3),
                 fft_us_per_list=round(m_old / lists * 1e3, 3), exact_max_minus_min_ms=round(max(ms_new) - min(ms_new), 4),
                 fft_max_minus_min_ms=round(max(ms_old) - min(ms_old), 4), exact_kernels_ms=round(k_new, 4),
                 fft_kernels_ms=round(k_old, 4), max_abs_diff_lsb=diff, decrypt_ok=ok)
        res.append(r)
        print(json.dumps(r), flush=True)
    return res


def trees(pset, params, sk, eng):
    res = []
    n1 = params.n + 1
    rng = np.random.default_rng(4)
    # d = 2 against lut2
    S = ROWS2
    F2 = lambda x, y: (x + y) % P                             # noqa: E731
    xs = rng.integers(0, P, (2, S)).astype(np.uint8)
    d_dig = dev(np.stack([sk.encrypt_ints(xs[k], P, 41 + k) for k in range(2)]))
    want = (xs[0] + xs[1]) % P
    d_o1 = torch.empty((1, S, n1), dtype=torch.int32, device="cuda")
    d_o2 = torch.empty_like(d_o1)
    row = S * n1 * 4
    for T in (1, 4):
        d_tv = dev(eoc.lut_tree_test_polynomials(P, 2, torus_table(F2, P, 2), T))
        tree = lambda: eng.lut_tree_batch_device(P, 2, T, d_tv.data_ptr(), 1, d_dig.data_ptr(), d_o1.data_ptr(), S)   # noqa: E731
        lut2 = lambda: eng.lut2_batch_device(P, T, d_tv.data_ptr(), 1, d_dig.data_ptr(), d_dig.data_ptr() + row, d_o2.data_ptr(), S)   # noqa: E731
        ms_t, ms_2 = timed_pair(tree, lut2)
        ok = None if (pset == 1 and T == 4) else bool(all(np.array_equal(sk.decrypt_ints(o.cpu().numpy()[0], P), want) for o in (d_o1, d_o2)))
        m_t, m_2 = float(np.mean(ms_t)), float(np.mean(ms_2))
        r = dict(what="d2", pset=pset, p=P, T=T, rows=S, tree_ms=round(m_t, 4), lut2_ms=round(m_2, 4), ratio=round(m_t / m_2, 4),
                 tree_us_per_row=round(m_t / S * 1e3, 3), lut2_us_per_row=round(m_2 / S * 1e3, 3), tree_spread=spread(ms_t),
                 lut2_spread=spread(ms_2), decrypt_ok=ok)
        res.append(r)
        print(json.dumps(r), flush=True)
    # the unit costs of this run: one encrypted-seed level and one exact pack at ROWS3 jobs / lists
    S = ROWS3
    eng.set_profiling(True)
    vals = dev(sk.encrypt_ints(rng.integers(0, P, P * S).astype(np.uint8), P, 51).reshape(1, P, S, n1))
    d_lists = torch.empty((S, 2, N), dtype=torch.int32, device="cuda")
    d_out = torch.empty((1, S, n1), dtype=torch.int32, device="cuda")
    pk = lambda: eng.tv_pack_exact_device(P, vals.data_ptr(), 1, S, d_lists.data_ptr())                     # noqa: E731
    l2 = lambda: eng.lut_enc_batch_device(d_lists.data_ptr(), 1, True, d_dig.data_ptr(), d_out.data_ptr(), S)   # noqa: E731
    pk(), l2()
    t_list = float(np.mean([kernel_ms(eng, pk)["keyswitch"] for _ in range(REPS)])) / S
    lv = [kernel_ms(eng, l2) for _ in range(REPS)]
    t_job = float(np.mean([x["blind_rotate"] + x["prepare"] for x in lv])) / S
    t_ks = float(np.mean([x["keyswitch"] for x in lv])) / S
    for p, d, T in SHAPES:
        F = lambda *x: sum((k + 1) * v for k, v in enumerate(x)) % p     # noqa: E731
        xs = rng.integers(0, p, (d, S)).astype(np.uint8)
        d_x = dev(np.stack([sk.encrypt_ints(xs[k], p, 61 + k) for k in range(d)]))
        d_tv = dev(eoc.lut_tree_test_polynomials(p, d, torus_table(F, p, d), T))
        call = lambda: eng.lut_tree_batch_device(p, d, T, d_tv.data_ptr(), 1, d_x.data_ptr(), d_out.data_ptr(), S)   # noqa: E731
        call()
        dev_ms = float(np.mean([sum(kernel_ms(eng, call).values()) for _ in range(REPS)]))
        rot = p ** (d - 1) // T + sum(p ** (d - k) for k in range(2, d + 1))
        kss = sum(p ** (d - k) for k in range(1, d + 1))
        nlists = sum(p ** (d - k) for k in range(2, d + 1))
        model = rot * t_job + kss * t_ks + nlists * t_list
        want = np.array([F(*(int(v) for v in col)) % p for col in xs.T], np.uint8)
        margin_ok = not (T == 4 and pset == 1)                # level 1 at T = 4 on Set B is below 6 sigma: timed, not decoded
        ok = bool(np.array_equal(sk.decrypt_ints(d_out.cpu().numpy()[0], p), want)) if margin_ok else None
        r = dict(what="tree", pset=pset, p=p, d=d, T=T, rows=S, rotations=rot, keyswitches=kss, lists=nlists,
                 device_us_per_row=round(dev_ms / S * 1e3, 3), model_us_per_row=round(model * 1e3, 3), job_us=round(t_job * 1e3, 3),
                 ks_us=round(t_ks * 1e3, 4), list_us=round(t_list * 1e3, 4), decrypt_ok=ok)
        res.append(r)
        print(json.dumps(r), flush=True)
    eng.set_profiling(False)
    return res


if __name__ == "__main__":
    out = dict(reps=REPS, pack=[], trees=[])
    for pset in PSETS:
        params = eoc.default_params(pset)
        sk = eoc.SecretKey(params, 1)
        eng = eoc.Engine(params)
        eng.load_cloud_key(sk)
        eng.load_packing_key(sk.packing_key_bytes())
        warm(eng, sk)
        out["pack"] += pack(pset, params, sk, eng)
        if "--pack-only" not in sys.argv:
            out["trees"] += trees(pset, params, sk, eng)
        eng.close()
    if "--json" in sys.argv:
        with open(sys.argv[sys.argv.index("--json") + 1], "w") as fh:
            json.dump(out, fh, indent=1)
