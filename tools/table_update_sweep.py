"""Encrypted-index table updates (device-pointer API): time per call and per external product, alternated with
the read of the same shape on the same engine, beside the blind rotation's cost per job-step from the same run.
Usage (GPU box): python tools/table_update_sweep.py [--out FILE]
For PSETS (default 0) x d in DS (4, 8, 10) at W = 1 x queries in QS (1, 16, 256): the first update of every point is
decrypt-checked slot by slot (a trivial p = 4 table of 0 / 1 plus 1 per query at its entry; the number of wrong slots is
reported next to noise.table_update_budget for the shape -- every update reaches every list, so a batch beyond the budget
is expected to lose slots to the accumulated mean of the truncating decomposition), then update and read are timed
alternately, REPS calls each, with the engine's event timers (eoc_engine_kernel_times: k_cmux, k_demux and k_sample_add are
booked under the blind rotation) and the host clock.  An update runs queries x (r + 2^d - 1) external products, as a read does.
A last line times eoc_demux_device alone on ITEMS items in store mode and in accumulate mode (distinct destinations): the
accumulating stage's 16 KiB of integer atomics per item against the storing stages' plain stores."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from eoc_tfhe_amd import noise  # noqa: E402

N = 1024
PSETS = [int(x) for x in os.environ.get("PSETS", "0").split(",")]
DS = [int(x) for x in os.environ.get("DS", "4,8,10").split(",")]
QS = [int(x) for x in os.environ.get("QS", "1,16,256").split(",")]
REPS = int(os.environ.get("REPS", "3"))
ITEMS = int(os.environ.get("ITEMS", "1024"))
LW = 0


def timed(torch, eng, f):
    eng.set_profiling(True)
    eng.kernel_times(reset=True)
    t0 = time.perf_counter()
    for _ in range(REPS):
        f()
    torch.cuda.synchronize()
    host = (time.perf_counter() - t0) / REPS * 1e3
    kt = eng.kernel_times(reset=True)
    eng.set_profiling(False)
    return host, kt


def job_step_ns(eoc, torch, eng, sk, p):
    rows = 1024
    rng = np.random.default_rng(1)
    cts = [torch.from_numpy(sk.encrypt_bits(rng.integers(0, 2, rows).astype(np.uint8), 10 + k)).cuda() for k in range(2)]
    out = torch.empty_like(cts[0])
    f = lambda: eng.gate_batch_device(eoc.OPS["NAND"], cts[0].data_ptr(), cts[1].data_ptr(), None, out.data_ptr(), rows)
    for _ in range(3):
        f()
    torch.cuda.synchronize()
    _, kt = timed(torch, eng, f)
    return kt["blind_rotate"]["ms"] / REPS * 1e6 / (p.n * rows)


def selectors(eoc, torch, eng, sk, p, bits):
    d_fft = torch.empty((len(bits), eoc.lib().eoc_tgsw_len(p)), dtype=torch.float64, device="cuda")
    for s0 in range(0, len(bits), 512):
        blk = torch.from_numpy(sk.encrypt_selector_bits(bits[s0:s0 + 512], enc_seed=7, first_idx=s0)).cuda()
        eng.tgsw_to_fft_device(blk.data_ptr(), blk.shape[0], d_fft[s0:].data_ptr())
        torch.cuda.synchronize()
    return d_fft


def point(eoc, torch, eng, sk, p, d, queries, y):
    depth, r = d + 10 - LW, 10 - LW
    rng = np.random.default_rng(d * 1000 + queries)
    old = rng.integers(0, 2, N << d).astype(np.uint8)
    table = torch.from_numpy(eoc.trivial_table((old.astype(np.int64) << 32) // 8)).cuda()
    idx = rng.choice(1 << depth, queries, replace=False)                      # distinct: old + 1 stays inside Z_4
    idx[0] = 0
    if queries > 1:
        idx[-1] = (1 << depth) - 1
    bits = ((idx[:, None] >> np.arange(depth)[None, :]) & 1).astype(np.uint8).ravel()
    d_fft = selectors(eoc, torch, eng, sk, p, bits)
    one = eoc.trivial_table(np.array([1 << 29], np.int64))[0]                 # the value 1 at p = 4, slot 0
    d_vals = torch.from_numpy(np.repeat(one[None], queries, axis=0)).cuda()
    d_out = torch.empty((queries, 1, p.n + 1), dtype=torch.int32, device="cuda")
    work = table.clone()
    upd = lambda: eng.table_update_device(work.data_ptr(), d, LW, d_fft.data_ptr(), d_vals.data_ptr(), queries)
    rd = lambda: eng.table_read_device(table.data_ptr(), d, LW, d_fft.data_ptr(), queries, d_out.data_ptr())
    upd()
    torch.cuda.synchronize()
    want = old.astype(np.int64)
    want[idx] += 1
    wrong = int((sk.decrypt_list_ints(work.cpu().numpy(), 4) != want).sum())
    budget = noise.table_update_budget(p, sk.lwe_key, sk.tlwe_key, 4, d, LW)
    rd()
    torch.cuda.synchronize()
    ok_read = bool(np.array_equal(sk.decrypt_ints(d_out.cpu().numpy().reshape(-1, p.n + 1), 4), old[idx]))
    u_host = u_ms = r_host = r_ms = r_ks = 0.0
    for _ in range(2):                                                       # alternated: update, read, update, read
        work.copy_(table)
        h, kt = timed(torch, eng, upd)
        u_host, u_ms = u_host + h / 2, u_ms + kt["blind_rotate"]["ms"] / REPS / 2
        h, kt = timed(torch, eng, rd)
        r_host, r_ms, r_ks = r_host + h / 2, r_ms + kt["blind_rotate"]["ms"] / REPS / 2, r_ks + kt["keyswitch"]["ms"] / REPS / 2
    prods = queries * (r + (1 << d) - 1)
    return dict(d=d, W=1 << LW, queries=queries, products_per_call=prods, update_host_ms=u_host, update_kernels_ms=u_ms,
                read_host_ms=r_host, read_cmux_ms=r_ms, read_keyswitch_ms=r_ks, update_ns_per_product=u_ms * 1e6 / prods,
                read_ns_per_product=r_ms * 1e6 / prods, update_x_job_step=u_ms * 1e6 / prods / y,
                update_over_read_cmux=u_ms / max(r_ms, 1e-12), update_decrypt_ok=wrong == 0, update_wrong_slots=wrong,
                slots=N << d, budget_updates_p4_6sigma=budget, read_decrypt_ok=ok_read)


def stage_rates(eoc, torch, eng, sk, p):
    rng = np.random.default_rng(5)
    d_fft = selectors(eoc, torch, eng, sk, p, rng.integers(0, 2, ITEMS).astype(np.uint8))
    x = torch.from_numpy(rng.integers(-2**31, 2**31, (ITEMS, 2, N)).astype(np.int32)).cuda()
    o0, o1 = torch.zeros_like(x), torch.zeros_like(x)
    res = {}
    for name, acc in (("store", False), ("accumulate", True), ("store_again", False), ("accumulate_again", True)):
        f = lambda: eng.demux_device(d_fft.data_ptr(), x.data_ptr(), o0.data_ptr(), o1.data_ptr(), ITEMS, accumulate=acc)
        f()
        torch.cuda.synchronize()
        _, kt = timed(torch, eng, f)
        res[name + "_ns_per_item"] = kt["blind_rotate"]["ms"] / REPS * 1e6 / ITEMS
    res["accumulate_over_store"] = (res["accumulate_ns_per_item"] + res["accumulate_again_ns_per_item"]) / \
        (res["store_ns_per_item"] + res["store_again_ns_per_item"])
    return dict(demux_alone=dict(items=ITEMS, **res))


def main():
    import torch
    import eoc_tfhe_amd as eoc
    lines = []
    for pset in PSETS:
        p = eoc.default_params(pset)
        sk = eoc.SecretKey(p, 1)
        eng = eoc.Engine(p)
        eng.load_cloud_key(sk)
        y = job_step_ns(eoc, torch, eng, sk, p)
        lines.append(json.dumps(dict(pset=pset, ns_per_job_step=y)))
        print(lines[-1], flush=True)
        for d in DS:
            for q in QS:
                row = point(eoc, torch, eng, sk, p, d, q, y)
                row.update(pset=pset)
                lines.append(json.dumps(row))
                print(lines[-1], flush=True)
        lines.append(json.dumps(dict(pset=pset, **stage_rates(eoc, torch, eng, sk, p))))
        print(lines[-1], flush=True)
        eng.close()
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
