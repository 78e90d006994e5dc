"""Finite automata on encrypted bit strings (device-pointer API): k_automaton_step against k_cmux per item, and a
whole run against the gate circuit it replaces.
Usage (GPU box): python tools/automaton_sweep.py [--out FILE]
Part 1, Set A, ITEMS (64, 1 024, 16 384) items per launch, one process, one call: eoc_cmux_device (one selector per item) and
eoc_automaton_step_device alternate ROUNDS (3) times, REPS launches each, timed with the engine's event timers (both kernels
are booked under the blind rotation).  Two automaton shapes at equal item counts: `own` -- 1 state per query, so one selector per
item as the CMux has, both operands the query's sample under two different rotations -- and `shared` -- 64 states per query
that read two other states' samples, the shape a run launches, where 64 items share a selector; `own_w0` and `own_w64` are
`own` with weights (0, N) and (64, N + 64): gathers that start on a cache line; `pair` has 2 states per query, the smallest
shape whose workgroups carry no dead pair (grid x = ceil(states / 2): with 1 state every workgroup computes its item twice).  Reported: ns per item per round, the ratio of the means, and k_cmux's own (max - min) / mean over its rounds beside it.
Part 2: divisible_by(3) on BITS-bit (32) inputs over QUERIES (64) queries through eoc_automaton_run_device against the same
predicate as a netlist (per bit NOR + two MUX on a two-bit state, one NOR at the end) through eoc_circuit_run_device; both are
decrypt-checked, then timed alternately on the host clock (synchronised).  Reported: the ratio."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N = 1024
ITEMS = [int(x) for x in os.environ.get("ITEMS", "64,1024,16384").split(",")]
ROUNDS = int(os.environ.get("ROUNDS", "3"))
REPS = int(os.environ.get("REPS", "5"))
BITS = int(os.environ.get("BITS", "32"))
QUERIES = int(os.environ.get("QUERIES", "64"))


def kernel_ns(torch, eng, f, items):
    f()
    torch.cuda.synchronize()
    eng.set_profiling(True)
    eng.kernel_times(reset=True)
    for _ in range(REPS):
        f()
    torch.cuda.synchronize()
    kt = eng.kernel_times(reset=True)
    eng.set_profiling(False)
    return kt["blind_rotate"]["ms"] / REPS * 1e6 / items


def step_against_cmux(eoc, torch, eng, sk, items):
    rng = np.random.default_rng(items)
    base = torch.from_numpy(sk.encrypt_selector_bits(rng.integers(0, 2, 64).astype(np.uint8), enc_seed=3)).cuda()
    fft64 = torch.empty(base.shape, dtype=torch.float64, device="cuda")
    eng.tgsw_to_fft_device(base.data_ptr(), 64, fft64.data_ptr())
    torch.cuda.synchronize()
    d_fft = fft64.repeat((items // 64, 1, 1, 1))                               # one selector per item
    a, b = (torch.from_numpy(rng.integers(-2**31, 2**31, (items, 2, N)).astype(np.int32)).cuda() for _ in range(2))
    out = torch.empty_like(a)
    own = np.array([[0, 5, 0, N + 5]], np.int32)
    own0 = np.array([[0, 0, 0, N]], np.int32)                                 # no shift: every load starts a cache line
    own64 = np.array([[0, 64, 0, N + 64]], np.int32)                          # a shift of 256 bytes: aligned, wrapping
    pair = np.array([[1, 5, 0, N + 5], [0, 3, 1, N + 7]], np.int32)           # 2 states per query: no dead pair, a selector per workgroup
    q = np.arange(64)
    shared = np.stack([(q + 1) % 64, (7 * q) % (2 * N), (q + 33) % 64, (N + 11 * q) % (2 * N)], axis=1).astype(np.int32)
    runs = dict(cmux=lambda: eng.cmux_device(d_fft.data_ptr(), a.data_ptr(), b.data_ptr(), out.data_ptr(), items),
                own=lambda: eng.automaton_step_device(own, a.data_ptr(), 1, d_fft.data_ptr(), 1, out.data_ptr(), items),
                own_w0=lambda: eng.automaton_step_device(own0, a.data_ptr(), 1, d_fft.data_ptr(), 1, out.data_ptr(), items),
                pair=lambda: eng.automaton_step_device(pair, a.data_ptr(), 2, d_fft.data_ptr(), 1, out.data_ptr(), items // 2),
                own_w64=lambda: eng.automaton_step_device(own64, a.data_ptr(), 1, d_fft.data_ptr(), 1, out.data_ptr(), items),
                shared=lambda: eng.automaton_step_device(shared, a.data_ptr(), 64, d_fft.data_ptr(), 1, out.data_ptr(), items // 64))
    ns = {k: [] for k in runs}
    for _ in range(ROUNDS):
        for k, f in runs.items():
            ns[k].append(kernel_ns(torch, eng, f, items))
    c = np.array(ns["cmux"])
    return dict(items=items, ns_per_item=ns, cmux_spread=float((c.max() - c.min()) / c.mean()),
                **{k + "_over_cmux": float(np.mean(v) / c.mean()) for k, v in ns.items() if k != "cmux"})


def div3_netlist(eoc, bits):
    """wires 0 .. bits-1: the input, MSB first; then the state bits; returns (gates, n_wires, output wire)"""
    G, OPS = eoc.Gate, eoc.OPS
    gates, nxt = [], bits
    s1, s0 = nxt, nxt + 1
    gates += [G(OPS["CONST0"], 0, 0, 0, s1), G(OPS["CONST0"], 0, 0, 0, s0)]
    nxt += 2
    for t in range(bits):
        z, n0, n1 = nxt, nxt + 1, nxt + 2
        gates += [G(OPS["NOR"], s1, s0, 0, z),                               # remainder 0
                  G(OPS["MUX"], t, z, s1, n0),                                # remainder 1 next: 0 under bit 1, 2 under bit 0
                  G(OPS["MUX"], t, s1, s0, n1)]                               # remainder 2 next: 2 under bit 1, 1 under bit 0
        s1, s0, nxt = n1, n0, nxt + 3
    gates.append(G(OPS["NOR"], s1, s0, 0, nxt))
    return gates, nxt + 1, nxt


def run_against_circuit(eoc, torch, eng, sk, p):
    from eoc_tfhe_amd import circuits
    rng = np.random.default_rng(9)
    values = rng.integers(0, 1 << BITS, QUERIES, dtype=np.uint64)
    values[:2] = [0, 3]
    bits = ((values[:, None] >> np.arange(BITS - 1, -1, -1, dtype=np.uint64)[None, :]) & 1).astype(np.uint8)   # MSB first
    want = (values % 3 == 0).astype(np.uint8)
    aut = eoc.Automaton.divisible_by(3)
    assert [aut.evaluate_plain(b) for b in bits] == want.tolist()
    msgs = np.zeros((aut.states, N), np.int64)
    msgs[0, 0] = 1 << 30                                                      # 1 of p = 2
    d_final = torch.from_numpy(eoc.trivial_table(msgs.ravel())).cuda()
    sel = torch.from_numpy(sk.encrypt_selector_bits(bits.ravel(), enc_seed=11)).cuda()
    d_fft = torch.empty(sel.shape, dtype=torch.float64, device="cuda")
    eng.tgsw_to_fft_device(sel.data_ptr(), sel.shape[0], d_fft.data_ptr())
    d_out = torch.empty((QUERIES, p.n + 1), dtype=torch.int32, device="cuda")
    auto = lambda: eng.automaton_run_device(aut, d_final.data_ptr(), d_fft.data_ptr(), BITS, [0], 0, d_out.data_ptr(), QUERIES)
    gates, n_wires, out_wire = div3_netlist(eoc, BITS)
    plain = np.zeros((n_wires, QUERIES), np.uint8)
    plain[:BITS] = bits.T
    assert circuits.evaluate_plain(gates, plain)[out_wire].tolist() == want.tolist()
    host = np.zeros((n_wires, QUERIES, p.n + 1), np.int32)
    host[:BITS] = sk.encrypt_bits(bits.T.ravel(), 12).reshape(BITS, QUERIES, p.n + 1)
    d_wires = torch.from_numpy(host).cuda()
    circ = lambda: eng.circuit_run_device(gates, d_wires.data_ptr(), n_wires, QUERIES)
    auto()
    circ()
    torch.cuda.synchronize()
    ok_auto = bool(np.array_equal(sk.decrypt_ints(d_out.cpu().numpy(), 2), want))
    ok_circ = bool(np.array_equal(sk.decrypt_bits(d_wires[out_wire].cpu().numpy()), want))
    ms = dict(automaton=[], circuit=[])
    for _ in range(ROUNDS):
        for k, f in (("automaton", auto), ("circuit", circ)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) * 1e3)
    return dict(bits=BITS, queries=QUERIES, automaton_decrypt_ok=ok_auto, circuit_decrypt_ok=ok_circ,
                circuit_bootstraps_per_query=int(eoc.circuit_bootstraps(gates)), ms=ms,
                circuit_over_automaton=float(np.mean(ms["circuit"]) / np.mean(ms["automaton"])))


def main():
    import torch
    import eoc_tfhe_amd as eoc
    p = eoc.default_params(0)
    sk = eoc.SecretKey(p, 1)
    eng = eoc.Engine(p)
    eng.load_cloud_key(sk)
    lines = []
    for items in ITEMS:
        lines.append(json.dumps(dict(step_against_cmux=step_against_cmux(eoc, torch, eng, sk, items))))
        print(lines[-1], flush=True)
    if os.environ.get("PART2", "1") != "0":
        lines.append(json.dumps(dict(run_against_circuit=run_against_circuit(eoc, torch, eng, sk, p))))
        print(lines[-1], flush=True)
    eng.close()
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
