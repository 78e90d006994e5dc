"""Every rounding twin launch_leveled() (engine.hip) can dispatch in rounding mode, on the MI355X, with the edge
inputs of the three truncating instance files: k_rcmux, k_rdemux and k_rstep over the six pair shapes, one test id per
instance, named after the kernel.  Ten of the eighteen -- k_rcmux<2,0>, <3,0> and every <L,0> of k_rdemux and k_rstep -- run
nowhere else, and each twin is a kernel of its own, with a run-time L Bgbit < 32 test in front of its one term in <L,0>.

An instance runs at n = 16 on an engine of its own, switched to rounding mode, through the public calls, byte for byte against
tests/leveled_round_oracle.py (rows and references: tests/leveled_round_cases.py; launchers: the truncating files'):
  launch shape    counts 1, 2, 3, 33 and all, a guard item behind every output, the launch counters
  unshifted rows  the truncating files' rows, the dropped-part rows (0, q/2 - 1, q/2, q - 1) and the all-0xFFFFFFFF row; at
                  least one word differs from the truncating reference wherever l Bgbit < 32
  shifted rows    every truncating row less h = 2^(31 - l Bgbit): the CMux's output IS the truncating reference of the
                  unshifted pair; the demultiplexer's out1 is the truncating out1 and its out0 the truncating out0 less h.  (A
                  rotation turns h's sign: the step has no such rows and is compared with leveled_round_oracle.step alone.)
  full scale      the instance's constant selector on digits_min - h and digits_max - h: the contract's top binade
  <4,0>           at (4, 8) h = 0: the output also equals the engine's own mode-off output; the unshifted and shifted rows
                  again at (4, 7), where h = 8 -- the one place where this instance's rounding term is not zero
  built on them   k_rcmux: eoc_table_read_device at (d, log2 W) = (1, 0); k_rdemux: accumulate mode on a pre-filled
                  destination; k_rstep: eoc_automaton_run_device with 1 and 3 steps
Every reference is computed under test_gpu_br_instances.reference: the oracle's recorded maximum is below 2^51 before anything
goes to the device.  Host side, the same references: tests/test_leveled_round_cpu.py."""
import numpy as np
import pytest

import automaton_edge_inputs as aei
import automaton_oracle as ao
import cmux_oracle as cx
import leveled_edge_inputs as lei
import leveled_round_cases as lrc
import leveled_round_oracle as lr
import table_update_oracle as tu
from gpu_util import dev_empty, sync, to_dev, torch_cuda
from test_gpu_automaton import RUN_TRANS, run_device
from test_gpu_automaton_instances import POISON, RUN_LW, RUN_QUERIES, RUN_STARTS, step_device
from test_gpu_br_instances import custom_oracle, custom_params, reference
from test_gpu_cmux_instances import COUNTS, READ_D, READ_LW, cmux_device, convert, differ
from test_gpu_demux_instances import demux_device

pytestmark = pytest.mark.gpu
N = 1024
N_LWE = 16
QUERIES = lrc.QUERIES


def twins(stem):
    return [name.replace("k_cmux", stem) for name in lrc.SHAPES]


@pytest.fixture(scope="module")
def eoc(built_lib):
    torch_cuda()
    import eoc_tfhe_amd
    return eoc_tfhe_amd


def shapes_of(name):
    """(truncating k_cmux name, [(l, Bgbit)]): the instance's own shape, and (4, 7) behind it for <4,0>"""
    base = "k_cmux" + name[name.index("<"):]
    cfg = lrc.SHAPES[base]
    return base, [(cfg["l"], cfg["Bgbit"])] + ([lrc.ALT] if name.endswith("<4,0>") else [])


def rounding_engine(eoc, p, sk=None):
    """an engine of the id's own, in rounding mode"""
    eng = eoc.Engine(p)
    if sk is not None:
        eng.load_cloud_key(sk)
    assert eng.leveled_rounding is False
    eng.leveled_rounding = True
    assert eng.leveled_rounding is True
    return eng


def two_selectors(eng, sk, items):
    """(fft [2], device selectors [items]: item k under the selector of bit k & 1)"""
    sel = sk.encrypt_selector_bits([0, 1], enc_seed=5)
    fft = cx.to_fft(sel)
    d_two = convert(eng, sel)
    assert np.array_equal(d_two.cpu().numpy(), fft * 2.0**-9)
    return fft, d_two, d_two[torch_cuda().arange(items, device="cuda") % 2].contiguous()


def constant(eng, l, K):
    ksel = lei.constant_selector(l, K)[None]
    kfft = cx.to_fft(ksel)
    d_k = convert(eng, ksel)
    assert np.array_equal(d_k.cpu().numpy(), kfft * 2.0**-9)
    return kfft[0], d_k


# ---- k_rcmux -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", twins("k_rcmux"))
def test_rcmux_instance_bit_exact_on_edge_inputs(eoc, name):
    base, shapes = shapes_of(name)
    for l, Bgbit in shapes:
        own = (l, Bgbit) == shapes[0]
        tag = lrc.tag_of(base, l, Bgbit)
        p = custom_params(eoc, l, Bgbit, N_LWE)
        op, h = cx.orc_params(p), lrc.half(l, Bgbit)
        sk = eoc.SecretKey(p, 83, with_cloud_key=own)
        eng = rounding_engine(eoc, p, sk if own else None)

        names, in0, in1, items_t = lrc.cmux_rows(l, Bgbit)
        items = len(in0)
        assert items_t > max(COUNTS) and items % 2 == 0
        fft, _, d_fft = two_selectors(eng, sk, items)
        want_t = lrc.cmux_truncating(tag, op, fft, in0, in1, items_t)
        want_r = lrc.cmux_rounding(tag, op, fft, in0, in1)
        assert (not np.array_equal(want_r[:items_t], want_t)) == (l * Bgbit < 32)

        # -- unshifted rows, every launch shape ------------------------------------------------------------------------------
        for count in (COUNTS if own else (3,)) + (items,):
            got = cmux_device(eng, d_fft, in0, in1, count)
            n_bad, first = differ(got, want_r[:count])
            assert n_bad == 0, (name, (l, Bgbit), count, n_bad, [names[i // 2] for i, _, _ in first], first)
        if h == 0:                                              # (4, 8): the mode changes no word
            eng.leveled_rounding = False
            off = cmux_device(eng, d_fft, in0, in1, items)
            eng.leveled_rounding = True
            assert got.tobytes() == off.tobytes()

        # -- shifted rows: the truncating reference of the unshifted pair ----------------------------------------------------
        shifted = lrc.minus(in1[:items_t], h)
        for count in (3, items_t):
            got = cmux_device(eng, d_fft, in0, shifted, count)
            n_bad, first = differ(got, want_t[:count])
            assert n_bad == 0, (name, (l, Bgbit), "shifted", count, n_bad, [names[i // 2] for i, _, _ in first], first)
        if not own:
            eng.close()
            continue

        # -- full scale ------------------------------------------------------------------------------------------------------
        kfft, d_k = constant(eng, l, lrc.SHAPES[base]["K"])
        f0, f1, want = lrc.cmux_full_scale(base, op, kfft, l, Bgbit)
        got = cmux_device(eng, d_k.expand(2, -1, -1, -1).contiguous(), f0, f1, 2)
        n_bad, first = differ(got, want)
        assert n_bad == 0, (name, "full scale", n_bad, first)

        # -- table read: one tree level, then the rot path at every amount 2N - 2^i --------------------------------------------
        torch = torch_cuda()
        orc = custom_oracle(l, Bgbit, N_LWE, 83)
        assert np.array_equal(sk.ksk, orc.ksk) and np.array_equal(sk.tlwe_key, orc.tlwe_key)
        rng = np.random.default_rng(900 + 10 * l + Bgbit)
        depth = READ_D + 10 - READ_LW
        table = eoc.trivial_table(rng.integers(-2**31, 2**31, N << READ_D))
        last = (1 << depth) - 1
        indices = [0, last, int(rng.integers(1, last))]
        rsel = np.stack([sk.encrypt_index(i, depth, 700, first_idx=k * depth) for k, i in enumerate(indices)])
        rfft = cx.to_fft(rsel)
        d_r = convert(eng, rsel.reshape((-1,) + rsel.shape[2:]))
        d_tab = to_dev(table)
        d_out = dev_empty((len(indices), 1 << READ_LW, N_LWE + 1), torch.int32)
        before = eng.stats()
        eng.table_read_device(d_tab.data_ptr(), READ_D, READ_LW, d_r.data_ptr(), len(indices), d_out.data_ptr())
        sync()
        after = eng.stats()
        eng.close()
        assert after["cmux_launches"] - before["cmux_launches"] == depth
        assert after["keyswitches"] - before["keyswitches"] == len(indices) << READ_LW
        want = reference(("rcmux", base, "read"), lambda: lr.table_read(orc, op, table, READ_D, READ_LW, rfft)[0])
        got = d_out.cpu().numpy()
        assert got.shape == want.shape
        assert np.array_equal(got, want), (name, "table read", np.argwhere((got != want).any(axis=-1)).tolist())
        if h:
            assert not np.array_equal(want, reference(("cmux", base, "read"),
                                                      lambda: cx.table_read(orc, op, table, READ_D, READ_LW, rfft)[0]))


# ---- k_rdemux ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", twins("k_rdemux"))
def test_rdemux_instance_bit_exact_on_edge_inputs(eoc, name):
    base, shapes = shapes_of(name)
    for l, Bgbit in shapes:
        own = (l, Bgbit) == shapes[0]
        tag = lrc.tag_of(base, l, Bgbit)
        p = custom_params(eoc, l, Bgbit, N_LWE)
        op, h = cx.orc_params(p), lrc.half(l, Bgbit)
        sk = eoc.SecretKey(p, 83, with_cloud_key=False)
        eng = rounding_engine(eoc, p)                           # no key is loaded: the call needs none

        names, x, items_t = lrc.demux_rows(l, Bgbit)
        items = len(x)
        assert items_t > max(COUNTS) and items % 2 == 0
        fft, _, d_fft = two_selectors(eng, sk, items)
        want_t = lrc.demux_truncating(tag, op, fft, x, items_t)
        want_r = lrc.demux_rounding(tag, op, fft, x)
        assert (not np.array_equal(want_r[:items_t], want_t)) == (l * Bgbit < 32)
        rng = np.random.default_rng(950 + 10 * l + Bgbit)
        fill = rng.integers(-2**31, 2**31, (2, items + 1, 2, N)).astype(np.int32)

        # -- unshifted rows, every launch shape, stored and accumulated ------------------------------------------------------
        for count in (COUNTS if own else (3,)) + (items,):
            g0, g1 = demux_device(eng, d_fft, x, count)
            for c, got in enumerate((g0, g1)):
                n_bad, first = differ(got, want_r[:count, c])
                assert n_bad == 0, (name, (l, Bgbit), "store", count, c, n_bad, [names[i // 2] for i, _, _ in first], first)
            assert np.array_equal((g0.astype(np.int64) + g1 - x[:count]) % 2**32, np.zeros_like(g0, np.int64))
            a0, a1 = demux_device(eng, d_fft, x, count, base=(fill[0], fill[1]))
            for c, got in enumerate((a0, a1)):
                acc = tu.wrap_i32(fill[c, :count].astype(np.int64) + want_r[:count, c])
                n_bad, first = differ(got, acc)
                assert n_bad == 0, (name, (l, Bgbit), "accumulate", count, c, n_bad, first)
        if h == 0:                                              # (4, 8): the mode changes no word
            eng.leveled_rounding = False
            o0, o1 = demux_device(eng, d_fft, x, items)
            eng.leveled_rounding = True
            assert g0.tobytes() == o0.tobytes() and g1.tobytes() == o1.tobytes()

        # -- shifted rows: out1 the truncating out1, out0 the truncating out0 less h -----------------------------------------
        shifted = lrc.minus(x[:items_t], h)
        for count in (3, items_t):
            g0, g1 = demux_device(eng, d_fft, shifted, count)
            for c, (got, want) in enumerate(((g0, lrc.minus(want_t[:count, 0], h)), (g1, want_t[:count, 1]))):
                n_bad, first = differ(got, want)
                assert n_bad == 0, (name, (l, Bgbit), "shifted", count, c, n_bad, [names[i // 2] for i, _, _ in first], first)
        if not own:
            eng.close()
            continue

        # -- full scale ------------------------------------------------------------------------------------------------------
        kfft, d_k = constant(eng, l, lrc.SHAPES[base]["K"])
        fx, want = lrc.demux_full_scale(base, op, kfft, l, Bgbit)
        g0, g1 = demux_device(eng, d_k.expand(2, -1, -1, -1).contiguous(), fx, 2)
        eng.close()
        for c, got in enumerate((g0, g1)):
            n_bad, first = differ(got, want[:, c])
            assert n_bad == 0, (name, "full scale", c, n_bad, first)


# ---- k_rstep -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", twins("k_rstep"))
def test_rstep_instance_bit_exact_on_edge_inputs(eoc, name):
    torch = torch_cuda()
    base, shapes = shapes_of(name)
    for l, Bgbit in shapes:
        own = (l, Bgbit) == shapes[0]
        tag = lrc.tag_of(base, l, Bgbit)
        p = custom_params(eoc, l, Bgbit, N_LWE)
        op, h = cx.orc_params(p), lrc.half(l, Bgbit)
        sk = eoc.SecretKey(p, 83, with_cloud_key=False)
        eng = rounding_engine(eoc, p)                           # no key is loaded: a step needs none
        fft, d_two, _ = two_selectors(eng, sk, 2)

        # -- edge states, the dropped-part and all-ones pairs behind them: every launch shape --------------------------------
        vectors = lrc.step_vectors(l, Bgbit)
        trans, _, names = vectors[0]
        states = len(names)
        assert states > max(aei.COUNTS) and states % 2 == 0
        cut, want_of = lrc.step_edges(tag, op, fft, vectors)
        differs = 0

        def row_of(c, q):
            return names[q] if q < c - (c & 1) else f"self-loop at {names[q]}"

        for c in (aei.COUNTS if own else (3,)) + (states,):
            t, prev = cut[0, c]
            for b in range(2):                                  # one query, the shared vector
                got = step_device(eng, t, prev, 0, d_two[b:b + 1].contiguous(), 1, 1)[0]
                n_bad, first = differ(got, want_of(0, b, c))
                assert n_bad == 0, (name, (l, Bgbit), "shared", c, b, n_bad, [row_of(c, q) for q, _, _ in first], first)
                if c == states:
                    differs += not np.array_equal(got, ao.step(op, t, prev, fft[b]))
                    if h == 0:                                  # (4, 8): the mode changes no word
                        eng.leveled_rounding = False
                        off = step_device(eng, t, prev, 0, d_two[b:b + 1].contiguous(), 1, 1)[0]
                        eng.leveled_rounding = True
                        assert got.tobytes() == off.tobytes()
            vecs = np.full((QUERIES, c + 1, 2, N), POISON, np.int32)  # three queries, a poisoned sample behind each vector
            for s in range(QUERIES):
                vecs[s, :c] = cut[s, c][1]
            for flip in range(2):
                bits = [(s + flip) & 1 for s in range(QUERIES)]
                pick = torch.tensor([v for bit in bits for v in (bit, 1 - bit)], device="cuda")
                got = step_device(eng, t, vecs, c + 1, d_two[pick].contiguous(), 2, QUERIES)
                for s in range(QUERIES):
                    n_bad, first = differ(got[s], want_of(s, bits[s], c))
                    assert n_bad == 0, (name, (l, Bgbit), "own vectors", c, bits, s, n_bad, [row_of(c, q) for q, _, _ in first], first)
        assert bool(differs) == (l * Bgbit < 32)
        if not own:
            eng.close()
            continue

        # -- full scale: D - h and its negation ------------------------------------------------------------------------------
        kfft, d_k = constant(eng, l, lrc.SHAPES[base]["K"])
        ft, fprev, fnames, want = lrc.step_full_scale(base, op, kfft, l, Bgbit)
        got = step_device(eng, ft, fprev, 0, d_k, 1, 1)[0]
        eng.close()
        n_bad, first = differ(got, want)
        assert n_bad == 0, (name, "full scale", n_bad, [fnames[q] for q, _, _ in first], first)

        # -- run: the cloud key for this part only ---------------------------------------------------------------------------
        sk = eoc.SecretKey(p, 83)
        orc = custom_oracle(l, Bgbit, N_LWE, 83)
        assert np.array_equal(sk.ksk, orc.ksk) and np.array_equal(sk.tlwe_key, orc.tlwe_key)
        eng = rounding_engine(eoc, p, sk)
        rng = np.random.default_rng(1900 + 10 * l + Bgbit)
        final = eoc.trivial_table(rng.integers(-2**31, 2**31, N * len(RUN_TRANS)))
        for steps in (1, 3):
            bits = rng.integers(0, 2, RUN_QUERIES * steps)
            rsel = sk.encrypt_selector_bits(bits, enc_seed=1910 + steps)
            rfft = cx.to_fft(rsel).reshape(RUN_QUERIES, steps, 2 * l, 2, N)
            want = reference(("rstep", base, "run", steps), lambda: lr.run(orc, op, RUN_TRANS, final, rfft, RUN_STARTS, RUN_LW)[0])
            before = eng.stats()["keyswitches"]
            got, launches = run_device(eng, RUN_TRANS, final, convert(eng, rsel), steps, RUN_STARTS, RUN_LW, RUN_QUERIES, N_LWE)
            assert launches == steps and eng.stats()["keyswitches"] - before == RUN_QUERIES * 5 * 2
            assert got.shape == want.shape
            assert np.array_equal(got, want), (name, "run", steps, bits.tolist(), np.argwhere((got != want).any(axis=-1)).tolist())
        eng.close()
