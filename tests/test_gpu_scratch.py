"""The host side's two growth rules on the MI355X.  The engine's scratch rule (scratch_reserve), once per buffer it serves:
refused under stream capture, then the same call outside capture gives the words of that call's existing reference, and a
second identical call grows nothing.  The global context's one staging buffer: a circuit, a table lookup and a circuit again
go through it, with the references' words, and a second round of the same calls grows nothing."""
import numpy as np
import pytest

import cmux_oracle as cx
import compact_oracle as co
import lut2_oracle as l2
import lut_oracle as lo
import oracle_lib as ol
import pack_oracle as po
import test_gpu_cmux as tc
import test_gpu_pack as tp
from gpu_util import dev_empty, sync, to_dev, torch_cuda

pytestmark = pytest.mark.gpu
N = 1024


@pytest.fixture(scope="module")
def eoc(built_lib):
    torch_cuda()
    import eoc_tfhe_amd
    return eoc_tfhe_amd


# Each case: a FRESH Set A engine, run(stream) queues the call, fetch() reads its output back, want = the reference's words,
# what = the buffer's name in the refusal
def case_table_read(eoc):
    """log2_lists = 2, log2_width = 9, one query: both ping-pong buffers, one tree stage each and one rotation"""
    torch = torch_cuda()
    p, sk, pk, orc, _ = tc.keys(eoc, 0)
    d, lw, depth, W = 2, 9, 3, 512
    table, _, _ = tc.make_table(eoc, pk, "ints", d, np.random.default_rng(29), 629)
    sel = tc.index_selectors(sk, [5], depth, enc_seed=729)
    eng = eoc.Engine(p)
    eng.load_cloud_key(sk)
    assert eoc.lib().eoc_engine_reserve(eng.h, W, 64, 0) == 0          # the extracted samples' rows: not what is under test
    d_fft, d_tab = tc.convert(eng, sel), to_dev(table)
    d_out = dev_empty((1, W, p.n + 1), torch.int32)
    ws = np.r_[0:8, 500:508]
    want = co.expand(orc, cx.table_read_tlwe(cx.orc_params(p), table, d, lw, cx.to_fft(sel[0]))[None], ws)
    return dict(eng=eng, what="table workspace", want=want, keep=(d_fft, d_tab),
                run=lambda st: eng.table_read_device(d_tab.data_ptr(), d, lw, d_fft.data_ptr(), 1, d_out.data_ptr(), stream=st),
                fetch=lambda: d_out.cpu().numpy()[0, ws])


def case_pack(eoc):
    torch = torch_cuda()
    p, sk, blob, kfft, _ = tp.keys(eoc, 0)
    cts = sk.encrypt_bits(np.array([1], np.uint8), 51)
    eng = eoc.Engine(p)
    eng.load_packing_key(blob)
    d_in, d_out = to_dev(cts), dev_empty((1, 2, N), torch.int32)
    return dict(eng=eng, what="packing columns", want=po.pack(p.n, kfft, cts), keep=(d_in,),
                run=lambda st: eng.pack_device(d_in.data_ptr(), 1, d_out.data_ptr(), stream=st),
                fetch=lambda: d_out.cpu().numpy())


def case_lut2(eoc):
    """p = 2, function 0 and row 0 of the shared (p, T) = (2, 2) case: a job's words do not depend on its place in a call"""
    torch = torch_cuda()
    params, sk, blob = l2.keys(eoc, 0)[:3]
    case = l2.shared_case(eoc, 0, 2, 2)
    eng = eoc.Engine(params)
    eng.load_cloud_key(sk)
    eng.load_packing_key(blob)
    d_tv = to_dev(case["tv0"][0].reshape(-1, N).copy())
    d_x, d_y = to_dev(case["x"][:1].copy()), to_dev(case["y"][:1].copy())
    d_out = dev_empty((1, 1, params.n + 1), torch.int32)
    return dict(eng=eng, what="two-input lookup workspace", want=case["out"][:1, :1], keep=(d_tv, d_x, d_y),
                run=lambda st: eng.lut2_batch_device(2, 2, d_tv.data_ptr(), 1, d_x.data_ptr(), d_y.data_ptr(), d_out.data_ptr(), 1,
                                                     stream=st),
                fetch=lambda: d_out.cpu().numpy())


def case_seeded(eoc):
    """one seeded selector against the conversion of its host expansion (which uses no scratch)"""
    torch = torch_cuda()
    p = eoc.default_params(0)
    sk = eoc.SecretKey(p, 1, with_cloud_key=False)
    seed, bodies = sk.encrypt_selector_bits_seeded([1], bytes(range(32)), bytes(range(7, 39)), first_idx=0)
    eng = eoc.Engine(p)
    want = tc.convert(eng, eoc.tgsw_seeded_expand_host(p, seed, bodies, 0)).cpu().numpy()
    d_b, d_out = to_dev(bodies), dev_empty((1, 2 * p.l, 2, N), torch.float64)
    return dict(eng=eng, what="seeded-selector staging rows", want=want, keep=(d_b,),
                run=lambda st: eng.tgsw_seeded_to_fft_device(seed, d_b.data_ptr(), 1, d_out.data_ptr(), 0, stream=st),
                fetch=lambda: d_out.cpu().numpy())


CASES = dict(table_read_device=case_table_read, pack_device=case_pack, lut2_batch_device=case_lut2,
             tgsw_seeded_to_fft_device=case_seeded)


@pytest.mark.parametrize("call", list(CASES))
def test_scratch_rule_refuses_capture_then_grows_once(eoc, call):
    torch = torch_cuda()
    c = CASES[call](eoc)
    eng, L = c["eng"], eoc.lib()
    sync()
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    # growth under capture is refused, loudly (an error return, nothing queued), and leaves the engine usable: the pattern of
    # test_gpu_circuits.py::test_mixed_batch_capture_and_replay
    g = torch.cuda.CUDAGraph()
    with pytest.raises(eoc.EocError, match="graph capture: the " + c["what"]):
        with torch.cuda.graph(g, stream=st):
            c["run"](st.cuda_stream)
    sync()
    grows0 = L.eoc_engine_workspace_grows(eng.h)
    c["run"](None)
    sync()
    got = c["fetch"]()
    assert got.shape == c["want"].shape and np.array_equal(got.view(np.uint8), np.ascontiguousarray(c["want"]).view(np.uint8)), call
    grows1 = L.eoc_engine_workspace_grows(eng.h)
    assert grows1 > grows0                                              # the call did need the buffer(s)
    c["run"](None)
    sync()
    assert L.eoc_engine_workspace_grows(eng.h) == grows1
    assert np.array_equal(c["fetch"]().view(np.uint8), got.view(np.uint8))
    eng.close()


def test_circuit_and_table_lookup_share_the_staging_buffer(eoc):
    """one engine on the global context: the 8-bit adder over 4 instances, one table over 4 rows, the adder again, five seeded
    samples expanded -- every word as the oracle's (as the host twin's); a second round of the four calls grows no host-path
    buffer"""
    from eoc_tfhe_amd import circuits
    p = eoc.default_params(0)
    p.n = 40                                                            # short LWE dimension: fast oracle
    sk = eoc.SecretKey(p, 9)
    orc = ol.Oracle(0, 9, n_override=40)
    gates, n_wires, aw, bw, sw = circuits.ripple_carry_adder(8)
    S = 4
    rng = np.random.default_rng(33)
    A, B = rng.integers(0, 256, S), rng.integers(0, 256, S)
    wires0 = np.zeros((n_wires, S, p.n + 1), np.int32)
    for i in range(8):
        wires0[aw[0] + i] = sk.encrypt_bits(((A >> i) & 1).astype(np.uint8), 100 + i, 0)
        wires0[bw[0] + i] = sk.encrypt_bits(((B >> i) & 1).astype(np.uint8), 200 + i, 0)
    ref = wires0.copy()
    for g in gates:                                                     # the oracle, gate by gate, computed once
        ins = [ref[w] if w >= 0 else None for w in (g.in0, g.in1, g.in2)]
        ref[g.out] = orc.gate_batch(g.op, *ins)
    vals = np.arange(S, dtype=np.uint8)
    cts = sk.encrypt_ints(vals, 4, 8401)
    tab = lo.int_table(lambda m: (3 * m + 1) % 4, 4, 4)
    want_lut = lo.lut_batch(orc, eoc.lut_test_polynomial(4, tab), cts)
    seed = bytes(range(32))
    bodies = rng.integers(-2**31, 2**31, 5).astype(np.int32)
    want_seeded = eoc.seeded_expand_host(p, seed, bodies, 3)
    eoc.gpu_shutdown()
    eoc.gpu_init(p, devices=[0])
    try:
        eoc.upload_cloud_key(sk)

        def round_of_four():
            for step in range(3):
                if step == 1:
                    assert np.array_equal(eoc.lut_batch(4, [tab], cts), want_lut)
                    continue
                wires = wires0.copy()
                eoc.circuit_run(gates, wires, S)
                assert np.array_equal(wires, ref), step
            assert np.array_equal(eoc.seeded_expand(seed, bodies, 3), want_seeded)
            return eoc.stats_multi()["host_buffer_grows"]

        grows = round_of_four()
        assert grows >= 1
        assert round_of_four() == grows
        tot = sum(sk.decrypt_bits(ref[sw[0] + i]).astype(np.int64) << i for i in range(9))
        assert np.array_equal(tot, A + B)
    finally:
        eoc.gpu_shutdown()
