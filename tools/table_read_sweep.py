"""Encrypted-index table reads (device-pointer API): time per call and per CMux over table size, entry width
and query count, beside the blind rotation's cost per job-step and the MUX-tree alternative.
Usage (GPU box): python tools/table_read_sweep.py [--out FILE]
For PSETS (default 0) x d in DS (0,4,8,12) x W in WS (1,8) x queries in (1, 64, the most the workspace budget holds, capped at
QMAX = 1024): every read is decrypt-checked, then timed over REPS calls with the engine's event timers
(eoc_engine_kernel_times: the CMux launches are booked under the blind rotation, k_tlwe_extract under prepare), host time per
call beside them.  Yardsticks taken in the same run: a 1 024-NAND batch's blind-rotation time / (n x 1 024) = the cost of one
external product inside the blind rotation; a 1 024-MUX batch's time per MUX x (2^(d + r) - 1) = the gate alternative (priced,
not run); bytes moved per CMux (24 KiB of samples) over the time per CMux = the bandwidth the launches reach."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N = 1024
PSETS = [int(x) for x in os.environ.get("PSETS", "0").split(",")]
DS = [int(x) for x in os.environ.get("DS", "0,4,8,12").split(",")]
WS = [int(x) for x in os.environ.get("WS", "1,8").split(",")]
REPS = int(os.environ.get("REPS", "3"))
QMAX = int(os.environ.get("QMAX", "1024"))
BUDGET = 256 << 20


def gate_yardsticks(eoc, torch, eng, sk, p):
    rows = 1024
    rng = np.random.default_rng(1)
    cts = [torch.from_numpy(sk.encrypt_bits(rng.integers(0, 2, rows).astype(np.uint8), 10 + k)).cuda() for k in range(3)]
    out = torch.empty_like(cts[0])
    res = {}
    for name in ("NAND", "MUX"):
        f = lambda: eng.gate_batch_device(eoc.OPS[name], cts[0].data_ptr(), cts[1].data_ptr(), cts[2].data_ptr(), out.data_ptr(), rows)
        for _ in range(3):
            f()
        torch.cuda.synchronize()
        eng.set_profiling(True)
        eng.kernel_times(reset=True)
        t0 = time.perf_counter()
        for _ in range(REPS):
            f()
        torch.cuda.synchronize()
        host = (time.perf_counter() - t0) / REPS * 1e3
        kt = eng.kernel_times(reset=True)
        eng.set_profiling(False)
        res[name] = dict(host_ms=host, br_ms=kt["blind_rotate"]["ms"] / REPS, ks_ms=kt["keyswitch"]["ms"] / REPS)
    res["ns_per_job_step"] = res["NAND"]["br_ms"] * 1e6 / (p.n * rows)
    res["ms_per_mux"] = res["MUX"]["host_ms"] / rows
    return res


def point(eoc, torch, eng, sk, p, d, lw, queries, table, vals):
    W, depth = 1 << lw, d + 10 - lw
    rng = np.random.default_rng(d * 100 + lw * 10 + queries)
    idx = rng.integers(0, 1 << depth, queries)
    idx[0], idx[-1] = 0, (1 << depth) - 1
    bits = ((idx[:, None] >> np.arange(depth)[None, :]) & 1).astype(np.uint8).ravel()
    sel_ints = eoc.lib().eoc_tgsw_len(p)
    d_fft = torch.empty((queries * depth, sel_ints), dtype=torch.float64, device="cuda")
    step = 512
    for s0 in range(0, len(bits), step):
        blk = torch.from_numpy(sk.encrypt_selector_bits(bits[s0:s0 + step], enc_seed=7, first_idx=s0)).cuda()
        eng.tgsw_to_fft_device(blk.data_ptr(), blk.shape[0], d_fft[s0:].data_ptr())
        torch.cuda.synchronize()
    d_out = torch.empty((queries, W, p.n + 1), dtype=torch.int32, device="cuda")
    f = lambda: eng.table_read_device(table.data_ptr(), d, lw, d_fft.data_ptr(), queries, d_out.data_ptr())
    f()
    torch.cuda.synchronize()
    got = sk.decrypt_ints(d_out.cpu().numpy().reshape(-1, p.n + 1), 4).reshape(queries, W)
    ok = bool(np.array_equal(got, vals[(idx[:, None] * W + np.arange(W)[None, :])]))
    eng.set_profiling(True)
    eng.kernel_times(reset=True)
    t0 = time.perf_counter()
    for _ in range(REPS):
        f()
    torch.cuda.synchronize()
    host = (time.perf_counter() - t0) / REPS * 1e3
    kt = eng.kernel_times(reset=True)
    eng.set_profiling(False)
    n_cmux = queries * ((1 << d) - 1 + (10 - lw))
    cm = kt["blind_rotate"]["ms"] / REPS
    return dict(d=d, W=W, queries=queries, depth=depth, cmux_per_call=n_cmux, host_ms=host, cmux_ms=cm,
                extract_ms=kt["prepare"]["ms"] / REPS, keyswitch_ms=kt["keyswitch"]["ms"] / REPS,
                ns_per_cmux=cm * 1e6 / max(n_cmux, 1), GBps_24KiB=24576 * n_cmux / max(cm * 1e6, 1e-9), decrypt_ok=ok)


def main():
    import torch
    import eoc_tfhe_amd as eoc
    lines = []
    for pset in PSETS:
        p = eoc.default_params(pset)
        sk = eoc.SecretKey(p, 1)
        eng = eoc.Engine(p)
        eng.load_cloud_key(sk)
        y = gate_yardsticks(eoc, torch, eng, sk, p)
        lines.append(json.dumps(dict(pset=pset, yardsticks=y)))
        print(lines[-1], flush=True)
        for d in DS:
            vals = np.random.default_rng(d).integers(0, 4, N << d).astype(np.uint8)
            table = torch.from_numpy(eoc.trivial_table((vals.astype(np.int64) << 32) // 8)).cuda()
            for W in WS:
                lw = W.bit_length() - 1
                s0, s1 = (1 << (d - 1) if d >= 1 else 1), (1 << (d - 2) if d >= 2 else 1)
                qmax = max(1, min(QMAX, BUDGET // ((s0 + s1) * 8192)))
                for q in sorted({1, min(64, qmax), qmax}):
                    row = point(eoc, torch, eng, sk, p, d, lw, q, table, vals)
                    row.update(pset=pset, x_job_step=row["ns_per_cmux"] / y["ns_per_job_step"],
                               mux_tree_ms=y["ms_per_mux"] * ((1 << row["depth"]) - 1) * q)
                    lines.append(json.dumps(row))
                    print(lines[-1], flush=True)
        eng.close()
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
