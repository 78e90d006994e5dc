"""Finite automata on encrypted bit strings, host side (no GPU): the plain-Python Automaton and its builders, the
composed reference (tests/automaton_oracle.py) decrypted for every 5-bit input, the new symbols and their argument errors, and
the noise rule of a long chain against the reference's phase errors.  Device side: tests/test_gpu_automaton.py."""
import ctypes as C
import itertools

import numpy as np
import pytest

import automaton_oracle as ao
import cmux_oracle as cx
import compact_oracle as co
import oracle_lib as ol
from eoc_tfhe_amd import noise
from test_cmux_cpu import tlwe_phase, wrap32

N = 1024
EOC_ERR_ARG = -1
CHAIN_STEPS = 24          # the chain length of the noise test and of the long GPU decrypt case: within automaton_budget below


@pytest.fixture(scope="module")
def eoc(built_lib):
    import eoc_tfhe_amd
    return eoc_tfhe_amd


def acceptor_final(eoc, aut, p=2):
    """[states][2][N] trivial: the accepting states hold 1 (of p) on slot 0, every other slot and state 0"""
    msgs = np.zeros((aut.states, N), np.int64)
    msgs[list(aut.accepting), 0] = co.int_msgs(1, p)
    return eoc.trivial_table(msgs.ravel())


def table_final(eoc, table, p):
    """[1][2][N] trivial: slot j holds table[j] (of p)"""
    msgs = np.zeros(N, np.int64)
    msgs[:len(table)] = co.int_msgs(table, p)
    return eoc.trivial_table(msgs)


def test_plain_automata(eoc):
    A = eoc.Automaton
    div3, has101, pop = A.divisible_by(3), A.contains([1, 0, 1]), A.popcount()
    assert (div3.states, has101.states, pop.states) == (3, 4, 1)
    for bits in itertools.product((0, 1), repeat=7):
        value = int("".join(map(str, bits)), 2)
        assert div3.evaluate_plain(bits) == (value % 3 == 0)
        assert has101.evaluate_plain(bits) == ("101" in "".join(map(str, bits)))
        assert pop.run_plain(bits) == (0, sum(bits))
        assert pop.evaluate_plain(bits, final=[np.arange(8) % 4]) == sum(bits) % 4
    assert A.contains([1, 1]).evaluate_plain([1, 0, 1, 1]) == 1 and A.contains([0]).evaluate_plain([1, 1]) == 0
    # weights add up modulo 2N, and a table entry read past N comes back negated
    w = A([[0, 0, 0, N - 1]])
    assert w.run_plain([1, 1, 1]) == (0, (3 * N - 3) % (2 * N))
    assert w.evaluate_plain([1, 1], final=[np.arange(N)]) == -(N - 2)
    for bad in ([[1, 0, 0, 0]], [[0, 2 * N, 0, 0]], [[0, 0, -1, 0]], [[0, -1, 0, 0]], np.zeros((0, 4))):
        with pytest.raises(eoc.EocError):
            A(bad)
    with pytest.raises(eoc.EocError):
        A([[0, 0, 0, 0]], start=1)


def test_symbols_and_argument_errors(eoc):
    L = eoc.lib()
    new = {"eoc_automaton_step_device", "eoc_automaton_run_device", "eoc_engine_automaton_launches", "eoc_automaton_run"}
    assert new <= set(eoc.abi_symbols()) and all(hasattr(L, s) for s in new)
    assert all(hasattr(eoc.Engine, m) for m in ("automaton_step_device", "automaton_run_device", "automaton_launches"))
    assert callable(eoc.automaton_run) and L.eoc_engine_automaton_launches(None) == 0

    def err():
        return L.eoc_last_error().decode()

    good = np.array([[1, 0, 0, 5], [1, 2047, 1, 0]], np.int32)
    starts = np.array([0, 1], np.int32)
    x = np.zeros(8, np.int32)
    ptr = x.ctypes.data                                                      # never followed: every call below is refused first

    def run(trans, states, st=starts, n_starts=2, lw=0, e=None):
        t = None if trans is None else np.ascontiguousarray(trans, np.int32)
        return L.eoc_automaton_run_device(e, None if t is None else t.ctypes.data, states, ptr, ptr, 3,
                                          None if st is None else st.ctypes.data, n_starts, lw, ptr, 1, None)

    def step(trans, states, stride=0):
        t = np.ascontiguousarray(trans, np.int32)
        return L.eoc_automaton_step_device(None, t.ctypes.data, states, ptr, stride, ptr, 1, ptr, 1, None)

    # a well-formed automaton reaches the pointer check: without an engine that is the refusal, and nothing else happens
    assert run(good, 2) == EOC_ERR_ARG and "null argument" in err()
    assert step(good, 2) == EOC_ERR_ARG and "null argument" in err()
    malformed = {"successor under bit 0 past the states": [[2, 0, 0, 0], [0, 0, 0, 0]],
                 "successor under bit 1 negative": [[0, 0, -1, 0], [0, 0, 0, 0]],
                 "weight under bit 0 of 2N": [[0, 2 * N, 0, 0], [0, 0, 0, 0]],
                 "weight under bit 1 negative": [[0, 0, 0, 0], [0, 0, 1, -1]]}
    for what, trans in malformed.items():
        assert run(trans, 2) == EOC_ERR_ARG and "successors must lie" in err(), what
        assert step(trans, 2) == EOC_ERR_ARG and "successors must lie" in err(), what
    for states in (0, 4097):
        assert run(np.zeros((4097, 4)), states) == EOC_ERR_ARG and "states outside" in err()
        assert step(np.zeros((4097, 4)), states) == EOC_ERR_ARG and "states outside" in err()
    assert run(None, 2) == EOC_ERR_ARG and "no transition table" in err()
    for st in (np.array([0, 2], np.int32), np.array([-1, 0], np.int32)):
        assert run(good, 2, st=st) == EOC_ERR_ARG and "start state" in err()
    assert run(good, 2, st=None) == EOC_ERR_ARG and run(good, 2, n_starts=0) == EOC_ERR_ARG
    assert run(good, 2, st=np.zeros(4097, np.int32), n_starts=4097) == EOC_ERR_ARG
    for lw in (-1, 11):
        assert run(good, 2, lw=lw) == EOC_ERR_ARG and "log2_width" in err()
    # the global form checks the automaton before it looks for a key or a device
    g = np.ascontiguousarray(good)
    bad = np.array(malformed["weight under bit 0 of 2N"], np.int32)
    args = (ptr, ptr, 3, starts.ctypes.data, 2, 0, ptr, 1)
    assert L.eoc_automaton_run(bad.ctypes.data, 2, *args) == EOC_ERR_ARG and "successors must lie" in err()
    assert L.eoc_automaton_run(g.ctypes.data, 2, None, ptr, 3, starts.ctypes.data, 2, 0, ptr, 1) == EOC_ERR_ARG
    assert L.eoc_automaton_run(g.ctypes.data, 2, ptr, None, 3, starts.ctypes.data, 2, 0, ptr, 1) == EOC_ERR_ARG
    assert L.eoc_automaton_run(g.ctypes.data, 2, ptr, ptr, 3, starts.ctypes.data, 2, 0, ptr, 0) == 0      # no query: a no-op
    with pytest.raises(eoc.EocError, match="final must be"):
        eoc.automaton_run(good, np.zeros((3, 2, N), np.int32), np.zeros((1, 3, 4, 2, N), np.int32), [0])
    with pytest.raises(eoc.EocError, match="selectors must be"):
        eoc.automaton_run(good, np.zeros((2, 2, N), np.int32), np.zeros((3, 4, 2, N), np.int32), [0])
    with pytest.raises(eoc.EocError, match="transitions must be"):
        eoc.automaton_run(np.zeros((2, 3)), np.zeros((2, 2, N), np.int32), np.zeros((1, 3, 4, 2, N), np.int32), [0])


def test_hot_path_fails_loudly_without_gpu(eoc):
    """no CPU fallback: without a device the run errors out as every other hot-path call does"""
    if eoc.lib().eoc_device_count() > 0:
        return                                                               # tests/test_gpu_automaton.py runs it there
    aut = eoc.Automaton.divisible_by(3)
    with pytest.raises(eoc.EocError):
        eoc.automaton_run(aut, acceptor_final(eoc, aut), np.zeros((1, 2, 4, 2, N), np.int32), [0])


def test_composed_run_on_the_cpu_decrypts_every_5_bit_input(eoc):
    """Set A, a reproducible key: divisible_by(3) (MSB first), contains([1, 0, 1]) and popcount() with the table count mod 4 at
    p = 4, all 2^5 inputs each, through the steps, the extraction and the key switch of the reference"""
    p = eoc.default_params(0)
    sk = eoc.SecretKey(p, 1, with_cloud_key=False)
    orc = ol.Oracle(0, 1, with_bk=False)
    op = cx.orc_params(p)
    steps = 5
    both = cx.to_fft(sk.encrypt_selector_bits([0, 1] * steps, enc_seed=88)).reshape(steps, 2, 2 * p.l, 2, N)
    inputs = list(itertools.product((0, 1), repeat=steps))
    sel = [np.stack([both[t, b] for t, b in enumerate(bits)]) for bits in inputs]
    table = np.arange(steps + 1) % 4
    A = eoc.Automaton
    for name, aut, final, q, tab in (("divisible_by(3)", A.divisible_by(3), None, 2, None),
                                     ("contains([1,0,1])", A.contains([1, 0, 1]), None, 2, None),
                                     ("popcount()", A.popcount(), table_final(eoc, table, 4), 4, [table])):
        final = acceptor_final(eoc, aut) if final is None else final
        out, _ = ao.run(orc, op, aut, final, sel, [aut.start], 0)
        assert out.shape == (len(inputs), 1, 1, p.n + 1)
        got = sk.decrypt_ints(out.reshape(-1, p.n + 1), q)
        want = [aut.evaluate_plain(bits, final=tab) for bits in inputs]
        assert got.tolist() == want, (name, [i for i in range(len(inputs)) if got[i] != want[i]])


def chain_errors(eoc, pset, queries=8, slots=256):
    """phase errors [queries][slots] of slots 0 .. slots-1 behind a CHAIN_STEPS-step all-ones run of the two-state automaton
    that changes state under bit 1 (weights 0) from a pseudo-random full-range final vector: phase(V_0[0]) - phase(F[end])"""
    p = eoc.default_params(pset)
    sk = eoc.SecretKey(p, 13, with_cloud_key=False)
    op = cx.orc_params(p)
    aut = eoc.Automaton([[0, 0, 1, 0], [1, 0, 0, 0]])
    bits = [1] * CHAIN_STEPS
    end, _ = aut.run_plain(bits)
    rng = np.random.default_rng(610 + pset)
    err = np.zeros((queries, slots))
    for k in range(queries):
        F = rng.integers(-2**31, 2**31, (2, 2, N)).astype(np.int32)
        fft = cx.to_fft(sk.encrypt_selector_bits(bits, enc_seed=900 + pset, first_idx=k * CHAIN_STEPS))
        out = ao.run_tlwe(op, aut, F, fft, [0])[0]
        err[k] = wrap32(tlwe_phase(out, sk.tlwe_key)[:slots] - tlwe_phase(F[end], sk.tlwe_key)[:slots]) / 2.0**32
    return p, sk, bits, err


@pytest.mark.parametrize("pset", [0, 1])
def test_chain_noise_matches_the_model(eoc, pset):
    """2 048 coefficients = 8 queries x slots 0 .. 255 of a 24-step all-ones chain.  Variance: around each slot's mean over the
    queries, against automaton_var, within the relative tolerance tests/test_cmux_cpu.py holds cmux_var to, taken at this sample
    count: 5 standard errors of a variance on n samples, sqrt(2 / n) each, plus the 3 % the model is held to -- 8 % there at
    n = 16 384, 18.6 % here at n = 2 048.  Mean: with weights 0 every step leaves its mean at the same slot, so slot j carries
    24 cmux_mean(j), AT the bound for slot 0 and falling by q/2 per key bit passed; a mean over 8 queries of one slot has a
    standard error (about 1e-3 on Set A) several times the bound's slack there, so the observed means are those a test can
    resolve: each query's mean over its 256 slots (model: 24 x the slots' average cmux_mean, about three quarters of the bound;
    s.e. about 2e-4) and the mean of all coefficients.  Each lies under automaton_mean_bound, and the latter agrees with the
    sum of cmux_mean within 4.5 s.e."""
    p, sk, bits, err = chain_errors(eoc, pset)
    n = err.size
    var = float(err.var(axis=0, ddof=1).mean())
    model = noise.automaton_var(p, sk.tlwe_key, bits)
    assert model == pytest.approx(CHAIN_STEPS * noise.cmux_var(p, sk.tlwe_key))
    zeros = noise.automaton_var(p, sk.tlwe_key, [0] * CHAIN_STEPS)
    assert zeros < model and noise.automaton_var(p, sk.tlwe_key, [0] * CHAIN_STEPS, final_var=1e-9) == pytest.approx(zeros + 1e-9)
    tol = 5 * np.sqrt(2.0 / n) + 0.03
    bound = noise.automaton_mean_bound(p, sk.tlwe_key, CHAIN_STEPS)
    q = 2.0 ** (-p.l * p.Bgbit)
    assert bound == pytest.approx(CHAIN_STEPS * (q / 2) * (1 + int(sk.tlwe_key.sum())))
    per_query = err.mean(axis=1)
    want_mean = CHAIN_STEPS * float(noise.cmux_mean(p, sk.tlwe_key, np.arange(err.shape[1])).mean())
    z = (err.mean() - want_mean) / (err.std(axis=0, ddof=1).mean() / np.sqrt(n))
    print(f"pset {pset}: var {var:.4e} model {model:.4e} ratio {var / model:.4f} (tolerance {tol:.3f}); mean {err.mean():.4e} "
          f"model {want_mean:.4e} z {z:.2f}; per-query |mean| max {np.abs(per_query).max():.4e} bound {bound:.4e}")
    assert abs(var / model - 1) < tol
    assert np.abs(per_query).max() < bound and abs(err.mean()) < bound
    assert abs(z) < 4.5


def test_budget_is_monotone_and_covers_the_chain(eoc):
    for pset in (0, 1):
        p = eoc.default_params(pset)
        sk = eoc.SecretKey(p, 14, with_cloud_key=False)
        b = [noise.automaton_budget(p, sk.lwe_key, sk.tlwe_key, m) for m in (2, 4, 8, 16, 64)]
        print(f"pset {pset}: automaton_budget at p = 2, 4, 8, 16, 64: {b}")
        assert all(x >= y for x, y in zip(b, b[1:])) and b[0] > b[-1]
        assert b[0] >= CHAIN_STEPS and b[1] >= CHAIN_STEPS                   # a boolean, and the p = 4 tables of the GPU tests
        enc = noise.compact_var(p, sk.tlwe_key)
        assert noise.automaton_budget(p, sk.lwe_key, sk.tlwe_key, 2, final_var=enc) <= b[0]
        assert noise.automaton_budget(p, sk.lwe_key, sk.tlwe_key, 2, sigmas=8.0) <= b[0]
        # the definition, at the edge
        pr = noise.predict(p, sk.lwe_key, sk.tlwe_key)
        for s, ok in ((b[0], True), (b[0] + 1, False)):
            total = (noise.automaton_mean_bound(p, sk.tlwe_key, s) + abs(pr["ks_mean"])
                     + 6.0 * np.sqrt(noise.automaton_var(p, sk.tlwe_key, [1] * s) + pr["ks_var"]))
            assert (total <= 1.0 / 8) == ok
