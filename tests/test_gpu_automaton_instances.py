"""Every k_automaton_step instance launch_leveled() (engine.hip) can dispatch, on the MI355X, with the edge inputs of
tests/automaton_edge_inputs.py: one test id per instance, named after the kernel.

An instance runs on a real key at n = 16 (only the key switch behind a run uses n) through the public calls:
  edge states   eoc_automaton_step_device on edge_automaton -- through both rotations the step decomposes the cell ends of
                every digit position, all digits -Bg/2 and Bg/2 - 1, single coefficients at the lane / register borders and
                the wrapping alternating pair, each with its negation, under every weight of W_ALL on either branch -- cut
                to 1, 2, 3, 33 and all states (two items per workgroup: a dead pair in the only workgroup, a full workgroup,
                a dead pair in the last one, a longer odd grid), as one query on a shared vector (stride 0) under the
                selector of 0 and of 1, and as three queries on vectors of their own, a poisoned sample between them
                (prev_query_stride = states + 1), their selectors interleaved with unused ones of the other bit
                (sel_query_stride = 2)
  full scale    a selector of one constant word (full_scale) through eoc_tgsw_to_fft_device, bit-identical to the oracle's
                transform, on the digits_min and digits_max states, D and -D: the top binade of the conversion contract
  weight sweep  2 048 states, every weight in [0, 2N) once on either branch, under the selector of 0 and of 1
  run           eoc_automaton_run_device with steps = 1 (the first launch is the last: it reads the shared final vector
                through the start records) and 3, five start states against three states, with repeats
and is compared with the reference (tests/automaton_oracle.py) word for word.  Nothing is decrypted: exotic shapes are
noisy, and parity does not depend on the noise.  Every reference is computed under test_gpu_br_instances.reference: the
oracle's recorded maximum is reset first and asserted below 2^51 (include/eoc_tfhe_gpu.h) before anything goes to the
device.  Host side of the inputs: tests/test_automaton_edge_inputs_cpu.py."""
import numpy as np
import pytest

import automaton_edge_inputs as aei
import automaton_oracle as ao
import cmux_oracle as cx
import oracle_lib as ol
from gpu_util import sync, to_dev, torch_cuda
from test_gpu_automaton import RUN_TRANS, run_device
from test_gpu_br_instances import custom_oracle, custom_params, reference
from test_gpu_cmux_instances import convert, differ, pool_map

pytestmark = pytest.mark.gpu
N = 1024
N_LWE = 16
FILL, POISON = 0x5A5A5A5A, 0x7E7E7E7E
QUERIES = 3
RUN_STARTS = [2, 0, 2, 1, 0]               # against RUN_TRANS' three states (one weight past N): more starts than states, repeats
RUN_QUERIES, RUN_LW = 2, 1


@pytest.fixture(scope="module")
def eoc(built_lib):
    torch_cuda()
    import eoc_tfhe_amd
    return eoc_tfhe_amd


def step_device(eng, trans, prev, prev_stride, d_fft, sel_stride, queries):
    """next [queries][states][2][N]; the buffer holds one sample more, which must keep its fill"""
    torch = torch_cuda()
    Q = len(trans)
    d_prev = to_dev(prev)
    d_next = torch.full((queries * Q + 1, 2, N), FILL, dtype=torch.int32, device="cuda")
    before = eng.stats()
    eng.automaton_step_device(trans, d_prev.data_ptr(), prev_stride, d_fft.data_ptr(), sel_stride, d_next.data_ptr(), queries)
    sync()
    after = eng.stats()
    assert after["automaton_launches"] - before["automaton_launches"] == 1 == eng.automaton_launches() - before["automaton_launches"]
    assert after["cmux_launches"] == before["cmux_launches"]
    out = d_next.cpu().numpy()
    assert (out[-1] == FILL).all()
    return out[:-1].reshape(queries, Q, 2, N)


@pytest.mark.parametrize("name", list(aei.full_scale))
def test_instance_bit_exact_on_edge_inputs(eoc, name):
    torch = torch_cuda()
    cfg = aei.full_scale[name]
    l, Bgbit = cfg["l"], cfg["Bgbit"]
    p = custom_params(eoc, l, Bgbit, N_LWE)
    op = cx.orc_params(p)
    sk = eoc.SecretKey(p, 83, with_cloud_key=False)
    eng = eoc.Engine(p)                                         # no key is loaded: a step needs none

    sel = sk.encrypt_selector_bits([0, 1], enc_seed=5)
    fft = cx.to_fft(sel)
    d_two = convert(eng, sel)
    assert np.array_equal(d_two.cpu().numpy(), fft * 2.0**-9)

    # -- edge states: vector s holds other random words and the same differences ---------------------------------------------
    vectors = [aei.edge_automaton(l, Bgbit, seed=s) for s in range(QUERIES)]
    trans, _, names = vectors[0]
    states = len(names)
    assert states > max(aei.COUNTS) and states % 2 == 0
    counts = aei.COUNTS + (states,)
    cut = {(s, c): aei.truncated(trans, vectors[s][1], c) for s in range(QUERIES) for c in counts}
    jobs = [(s, b, c, q) for s in range(QUERIES) for b in range(2) for c in counts for q in range(c)]
    at = {(s, b, c): i for i, (s, b, c, q) in enumerate(jobs) if q == 0}
    edges = reference(("automaton", name, "edges"), lambda: np.stack(pool_map(
        lambda i: ao.step(op, *cut[jobs[i][0], jobs[i][2]], fft[jobs[i][1]], [jobs[i][3]])[0], len(jobs))))

    def want_of(s, b, c):
        return edges[at[s, b, c]:at[s, b, c] + c]

    def row_of(c, q):
        return names[q] if q < c - (c & 1) else f"self-loop at {names[q]}"

    for c in counts:
        t, prev = cut[0, c]
        for b in range(2):                                      # one query, the shared vector
            got = step_device(eng, t, prev, 0, d_two[b:b + 1].contiguous(), 1, 1)[0]
            n_bad, first = differ(got, want_of(0, b, c))
            assert n_bad == 0, (name, "shared", c, b, n_bad, [row_of(c, q) for q, _, _ in first], first)
            zero = [q for q in range(c - (c & 1)) if names[q].startswith("zero")]
            assert len(zero) == (2 if c > 1 else 0)
            for q in zero:                                      # D = 0: the turned successor itself
                assert np.array_equal(got[q], ao.successor(prev, t[q, 0], t[q, 1])), (name, names[q], c, b)
        own = np.full((QUERIES, c + 1, 2, N), POISON, np.int32)  # three queries, a poisoned sample behind each vector
        for s in range(QUERIES):
            own[s, :c] = cut[s, c][1]
        for flip in range(2):
            bits = [(s + flip) & 1 for s in range(QUERIES)]      # 0, 1, 0, then flipped
            pick = torch.tensor([x for bit in bits for x in (bit, 1 - bit)], device="cuda")
            got = step_device(eng, t, own, c + 1, d_two[pick].contiguous(), 2, QUERIES)
            for s in range(QUERIES):
                n_bad, first = differ(got[s], want_of(s, bits[s], c))
                assert n_bad == 0, (name, "own vectors", c, bits, s, n_bad, [row_of(c, q) for q, _, _ in first], first)

    # -- full scale: the contract's top binade, D and -D ----------------------------------------------------------------------
    ksel = aei.constant_selector(l, cfg["K"])[None]
    kfft = cx.to_fft(ksel)
    d_k = convert(eng, ksel)
    assert np.array_equal(d_k.cpu().numpy(), kfft * 2.0**-9)
    ft, fprev, fnames = aei.full_scale_states(l, Bgbit)

    def full_scale():
        L = ol.lib()
        out = []
        for q in range(len(fnames)):                            # reference() reset the maximum; read and reset per state:
            out.append(ao.step(op, ft, fprev, kfft[0], [q])[0])  # each direction reaches the binade, none leaves the
            mx = L.orc_dbg_max_conv(1)                          # contract (hi <= 2^51)
            assert cfg["lo"] <= mx < cfg["hi"] <= 2.0**51, (name, fnames[q], np.log2(mx))
        return np.stack(out)
    want = reference(("automaton", name, "full scale"), full_scale)
    got = step_device(eng, ft, fprev, 0, d_k, 1, 1)[0]
    n_bad, first = differ(got, want)
    assert n_bad == 0, (name, "full scale", n_bad, [fnames[q] for q, _, _ in first], first)

    # -- weight sweep: every weight in [0, 2N) on either branch ---------------------------------------------------------------
    wt, wprev = aei.weight_sweep()
    nw = len(wt)
    want = reference(("automaton", name, "sweep"), lambda: np.stack(pool_map(
        lambda i: ao.step(op, wt, wprev, fft[i // nw], [i % nw])[0], 2 * nw)).reshape(2, nw, 2, N))
    for b in range(2):
        got = step_device(eng, wt, wprev, 0, d_two[b:b + 1].contiguous(), 1, 1)[0]
        bad = np.unique(np.argwhere(got != want[b])[:, 0])
        assert len(bad) == 0, (name, "sweep", b, len(bad), [dict(state=int(q), w0=(int(wt[q, 1]) & 63, int(wt[q, 1]) >> 6),
                                                                 w1=(int(wt[q, 3]) & 63, int(wt[q, 3]) >> 6)) for q in bad[:8]])
    eng.close()

    # -- run: the cloud key for this part only --------------------------------------------------------------------------------
    sk = eoc.SecretKey(p, 83)
    orc = custom_oracle(l, Bgbit, N_LWE, 83)
    assert np.array_equal(sk.ksk, orc.ksk) and np.array_equal(sk.tlwe_key, orc.tlwe_key)
    eng = eoc.Engine(p)
    eng.load_cloud_key(sk)
    rng = np.random.default_rng(1900 + 10 * l + Bgbit)
    final = eoc.trivial_table(rng.integers(-2**31, 2**31, N * len(RUN_TRANS)))
    assert final.shape == (len(RUN_TRANS), 2, N)
    for steps in (1, 3):
        bits = rng.integers(0, 2, RUN_QUERIES * steps)
        rsel = sk.encrypt_selector_bits(bits, enc_seed=1910 + steps)
        rfft = cx.to_fft(rsel).reshape(RUN_QUERIES, steps, 2 * l, 2, N)
        want = reference(("automaton", name, "run", steps), lambda: ao.run(orc, op, RUN_TRANS, final, rfft, RUN_STARTS, RUN_LW)[0])
        before = eng.stats()["keyswitches"]
        got, launches = run_device(eng, RUN_TRANS, final, convert(eng, rsel), steps, RUN_STARTS, RUN_LW, RUN_QUERIES, N_LWE)
        assert launches == steps and eng.stats()["keyswitches"] - before == RUN_QUERIES * 5 * 2
        assert got.shape == want.shape
        assert np.array_equal(got, want), (name, "run", steps, bits.tolist(), np.argwhere((got != want).any(axis=-1)).tolist())
    eng.close()
