"""Dense layers on LWE samples on the MI355X (include/eoc_tfhe_lwe.h): eoc_lwe_matmul_device word for word
against the four-line reference (tests/lwe_matmul_ref.py) at every tail, the accumulator extremes at the largest K, misaligned
buffers, the error ladder, a captured call replayed on new inputs (the protocol of tests/test_gpu_capture.py), one call between
a table lookup and a gate batch on one stream, the host-buffer form, and the two-layer sign network of tests/dinn_case.py on the
hidden="lwe" route and from LWE inputs.  Every comparison of words is exact.  Host side: tests/test_lwe_matmul_cpu.py."""
import numpy as np
import pytest

import dinn_case as dc
import lwe_matmul_ref as ref
from gpu_util import sync, to_dev, torch_cuda

pytestmark = pytest.mark.gpu
POISON = 0x5A5AA5A5
GUARD = 64                                                               # words in front of and behind the output
EOC_ERR_ARG, EOC_ERR_STATE = -1, -6


@pytest.fixture(scope="module")
def eoc(built_lib):
    torch_cuda()
    import eoc_tfhe_amd
    return eoc_tfhe_amd


@pytest.fixture(scope="module")
def eng(eoc):
    e = eoc.Engine(eoc.default_params(0))                                # no key at all
    yield e
    e.close()


def model(eng, w):
    """the device image of weights w: a uint8 tensor that must stay alive while it is used"""
    torch = torch_cuda()
    w = np.asarray(w)
    img = torch.empty(eng.lwe_weights_image_bytes(*w.shape), dtype=torch.uint8, device="cuda")
    assert eng.lwe_weights_to_device(w, img.data_ptr()) == w.shape
    return img


def run(eng, w, cts, bias=None, img=None, shift=0):
    """lwe_matmul_device into a poisoned buffer with GUARD words on either side, which must stay untouched.  shift: words by
    which d_cts, d_out and d_bias are moved off their 16-byte boundary"""
    torch = torch_cuda()
    w, cts = np.asarray(w), np.ascontiguousarray(cts, np.int32)
    (rows, cols), (batch, _, width) = w.shape, cts.shape
    img = model(eng, w) if img is None else img
    d_cts = torch.zeros(cts.size + shift, dtype=torch.int32, device="cuda")
    d_cts[shift:] = to_dev(cts.reshape(-1))
    d_bias = None
    if bias is not None:
        d_bias = torch.zeros(rows + shift, dtype=torch.int32, device="cuda")
        d_bias[shift:] = to_dev(np.asarray(bias, np.int32))
    n = batch * rows * width
    out = torch.full((GUARD + shift + n + GUARD,), POISON, dtype=torch.int32, device="cuda")
    assert out.data_ptr() % 16 == 0 and d_cts.data_ptr() % 16 == 0
    eng.lwe_matmul_device(img.data_ptr(), rows, cols, d_cts.data_ptr() + 4 * shift, width, batch,
                          None if d_bias is None else d_bias.data_ptr() + 4 * shift, out.data_ptr() + 4 * (GUARD + shift))
    sync()
    o = out.cpu().numpy()
    assert (o[:GUARD + shift].view(np.uint32) == POISON).all() and (o[GUARD + shift + n:].view(np.uint32) == POISON).all(), \
        "a guard word around the output was written"
    return o[GUARD + shift:GUARD + shift + n].reshape(batch, rows, width)


SHAPES = [(1, 1, 1, 1), (32, 32, 32, 1), (33, 31, 501, 2), (31, 33, 631, 3), (64, 96, 1025, 1), (5, 1000, 41, 2)]


@pytest.mark.parametrize("rows,cols,width,batch", SHAPES)
def test_words_equal_the_reference(eng, rows, cols, width, batch):
    """the smallest call; exactly one tile each way; one past and one short of a tile in rows and cols at the widths of Set A
    and Set B (16 and 20 column tiles: several workgroups, a last tile of 21 and 23 words); two row tiles, three K steps and
    33 column tiles with one word in the last; a long K with a short tail.  Random words mixed with the limb-edge words,
    random weights mixed with +-127, +-1 and 0; with a bias and without one; guard words around the output"""
    rng = np.random.default_rng(2600 + rows + cols)
    w, cts = ref.weights(rng, rows, cols), ref.words(rng, (batch, cols, width))
    bias = ref.words(rng, rows)
    img = model(eng, w)
    before = eng.lwe_matmul_launches()
    got = run(eng, w, cts, bias, img=img)
    want = ref.lwe_matmul(w, cts, bias)
    assert np.array_equal(got, want), np.argwhere(got != want)[:4].tolist()
    assert np.array_equal(run(eng, w, cts, None, img=img), ref.lwe_matmul(w, cts))
    assert eng.lwe_matmul_launches() - before == 2 and eng.stats()["keyswitches"] == 0


def test_every_edge_word_under_every_edge_weight(eng):
    """each limb-edge word as a whole column of a vector, under a matrix whose rows are the edge weights: a limb that is split
    wrongly shows in its own column"""
    cols = len(ref.EDGE_WEIGHTS)
    w = np.stack([np.roll(ref.EDGE_WEIGHTS, k) for k in range(cols)])
    cts = np.broadcast_to(ref.EDGE_WORDS[None, None, :], (1, cols, len(ref.EDGE_WORDS))).copy()
    assert np.array_equal(run(eng, w, cts), ref.lwe_matmul(w, cts))
    assert np.array_equal(run(eng, -w, cts), ref.lwe_matmul(-w, cts))


@pytest.mark.parametrize("weight,word", [(-127, 0x80808080), (127, 0x7F7F7F7F)])
def test_largest_k_at_the_accumulator_extreme(eng, weight, word):
    """rows = 1, cols = 65 536, width = 1, batch = 1: every limb product is (-127)(-128) resp. 127 * 127, 2 048 K steps"""
    w = np.full((1, 2**16), weight, np.int8)
    cts = np.full((1, 2**16, 1), word, np.int64).astype(np.uint32).view(np.int32)
    got, want = run(eng, w, cts), ref.lwe_matmul(w, cts)
    assert np.array_equal(got, want), (got.tolist(), want.tolist())


def test_misaligned_buffers_give_the_aligned_words(eng):
    """d_cts, d_out and d_bias 4 bytes past a 16-byte boundary, an odd width"""
    rng = np.random.default_rng(2700)
    w, cts, bias = ref.weights(rng, 33, 31), ref.words(rng, (2, 31, 501)), ref.words(rng, 33)
    img = model(eng, w)
    aligned = run(eng, w, cts, bias, img=img)
    assert np.array_equal(run(eng, w, cts, bias, img=img, shift=1), aligned)
    assert np.array_equal(aligned, ref.lwe_matmul(w, cts, bias))


def test_error_ladder(eoc, eng):
    torch, L = torch_cuda(), eoc.lib()
    w = np.ones((2, 5), np.int8)
    img = model(eng, w)
    nbytes = img.numel()
    cts = torch.zeros((3, 5, 7), dtype=torch.int32, device="cuda")
    bias = torch.zeros(2, dtype=torch.int32, device="cuda")
    out = torch.full((3 * 2 * 7 + 64,), 7, dtype=torch.int32, device="cuda")
    before = eng.lwe_matmul_launches()

    def refused(rc, text):
        assert rc == EOC_ERR_ARG and text in L.eoc_last_error(), (rc, L.eoc_last_error())

    # a -128 weight at image build; the image is not written
    bad = w.copy()
    bad[1, 3] = -128
    keep = img.clone()
    refused(L.eoc_lwe_weights_to_device(eng.h, bad.ctypes.data, 2, 5, img.data_ptr(), None), b"weight (1, 3) is -128")
    for rows, cols in ((0, 5), (2, 0), (2**20 + 1, 5), (2, 2**16 + 1)):
        refused(L.eoc_lwe_weights_to_device(eng.h, w.ctypes.data, rows, cols, img.data_ptr(), None), b"rows must lie in [1, 2^20]")
    for a in ((None, w.ctypes.data, img.data_ptr()), (eng.h, None, img.data_ptr()), (eng.h, w.ctypes.data, None)):
        refused(L.eoc_lwe_weights_to_device(a[0], a[1], 2, 5, a[2], None), b"null argument")
    sync()
    assert bool((img == keep).all())
    assert eng.lwe_weights_image_bytes(2, 5) == nbytes == ref.image_bytes(2, 5)
    # the run call: shapes out of range
    ok = dict(e=eng.h, img=img.data_ptr(), rows=2, cols=5, cts=cts.data_ptr(), width=7, batch=3, bias=bias.data_ptr(),
              out=out.data_ptr())

    def call(**kw):
        a = dict(ok, **kw)
        return L.eoc_lwe_matmul_device(a["e"], a["img"], a["rows"], a["cols"], a["cts"], a["width"], a["batch"], a["bias"], a["out"], None)

    for kw in (dict(rows=2**20 + 1), dict(cols=0), dict(cols=2**16 + 1), dict(width=0), dict(width=4097)):
        refused(call(**kw), b"width in [1, 4096]")
    # a null pointer (the bias may be NULL)
    for kw in (dict(e=None), dict(img=None), dict(cts=None), dict(out=None)):
        refused(call(**kw), b"null argument")
    # each overlap: the output on the samples, on the image, on the bias
    refused(call(out=cts.data_ptr() + 64), b"must not overlap")
    refused(call(out=img.data_ptr()), b"must not overlap")
    refused(call(bias=out.data_ptr() + 4 * 3), b"must not overlap")
    refused(call(out=cts.data_ptr() - 4 * (3 * 2 * 7 - 1)), b"must not overlap")           # the output's last word on the first sample word
    # batch x rows = 0 is a no-op, whatever else is passed
    assert call(batch=0) == 0 and call(rows=0) == 0 and call(batch=0, cts=None, out=None) == 0
    sync()
    assert bool((out == 7).all()) and not bool(cts.any()) and eng.lwe_matmul_launches() == before
    # the model load is refused under capture; the run call is not
    st = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=st):
        rc_load = L.eoc_lwe_weights_to_device(eng.h, w.ctypes.data, 2, 5, img.data_ptr(), st.cuda_stream)
        text = L.eoc_last_error()
        rc_run = L.eoc_lwe_matmul_device(eng.h, img.data_ptr(), 2, 5, cts.data_ptr(), 7, 3, None, out.data_ptr(), st.cuda_stream)
    assert rc_load == EOC_ERR_STATE and b"cannot be captured" in text and rc_run == 0
    del g


def test_captured_call_replays_the_reference_words(eoc, eng):
    """one call captured by the protocol of tests/test_gpu_capture.py (its helpers, unchanged): eager on input set 0, the
    capture, then two replays on inputs written in place into the captured buffers, with eager calls of other shapes on other
    buffers in between and the output poisoned ahead of each replay.  The launch counter advances by one per eager call and
    by one for the capture; a replay does not enter the library."""
    import test_gpu_capture as tcap
    torch, L = torch_cuda(), eoc.lib()
    rows, cols, width, batch = 33, 31, 501, 2
    rng = np.random.default_rng(2800)
    w, bias = ref.weights(rng, rows, cols), ref.words(rng, rows)
    inputs = [ref.words(rng, (batch, cols, width)) for _ in range(3)]
    img, d_bias = model(eng, w), to_dev(bias)
    d_cts = to_dev(inputs[0])
    d_out = torch.full((batch, rows, width), POISON, dtype=torch.int32, device="cuda")

    def call(stream):
        eng.lwe_matmul_device(img.data_ptr(), rows, cols, d_cts.data_ptr(), width, batch, d_bias.data_ptr(), d_out.data_ptr(), stream)

    st = tcap.side_stream(torch)
    before = eng.lwe_matmul_launches()
    with torch.cuda.stream(st):
        call(st.cuda_stream)
    st.synchronize()
    assert eng.lwe_matmul_launches() - before == 1
    assert np.array_equal(d_out.cpu().numpy(), ref.lwe_matmul(w, inputs[0], bias))
    grows = L.eoc_engine_workspace_grows(eng.h)
    g = tcap.capture(torch, st, call)
    assert eng.lwe_matmul_launches() - before == 2 and L.eoc_engine_workspace_grows(eng.h) == grows
    other_w = ref.weights(rng, 5, 70)
    for k in (1, 2):
        d_cts.copy_(to_dev(inputs[k]))
        run(eng, other_w, ref.words(rng, (3, 70, 41)), None)              # another shape on other buffers
        d_out.fill_(POISON)
        sync()
        launches = eng.lwe_matmul_launches()
        g.replay()
        sync()
        got = d_out.cpu().numpy()
        assert np.array_equal(got, ref.lwe_matmul(w, inputs[k], bias)), k
        assert eng.lwe_matmul_launches() == launches and L.eoc_engine_workspace_grows(eng.h) == grows
    del g


def test_between_a_lookup_and_a_gate_batch_on_one_stream(eoc):
    """lut_batch_device, lwe_matmul_device, gate_batch_device on one engine and one stream, nothing waited for in between: all
    three results equal those of separate, drained runs"""
    import capture_cases as cc
    torch = torch_cuda()
    p, sk, _, eng = cc.small_keys(eoc, 0, 40, 61)
    rng = np.random.default_rng(2900)
    count = 9
    tv = to_dev(np.resize(ref.words(rng, 1024), (1, 1024)))
    lut_in = to_dev(sk.encrypt_ints(rng.integers(0, 4, count), 4, 2901))
    g0, g1 = to_dev(sk.encrypt_bits(rng.integers(0, 2, count), 2902)), to_dev(sk.encrypt_bits(rng.integers(0, 2, count), 2903))
    w, cts, bias = ref.weights(rng, 7, 9), ref.words(rng, (2, 9, p.n + 1)), ref.words(rng, 7)
    img, d_cts, d_bias = model(eng, w), to_dev(cts), to_dev(bias)

    def outs():
        return (torch.full((count, p.n + 1), POISON, dtype=torch.int32, device="cuda"),
                torch.full((2, 7, p.n + 1), POISON, dtype=torch.int32, device="cuda"),
                torch.full((count, p.n + 1), POISON, dtype=torch.int32, device="cuda"))

    def lut(o, st):
        eng.lut_batch_device(tv.data_ptr(), 1, lut_in.data_ptr(), o.data_ptr(), count, st)

    def mm(o, st):
        eng.lwe_matmul_device(img.data_ptr(), 7, 9, d_cts.data_ptr(), p.n + 1, 2, d_bias.data_ptr(), o.data_ptr(), st)

    def gate(o, st):
        eng.gate_batch_device(eoc.OPS["NAND"], g0.data_ptr(), g1.data_ptr(), None, o.data_ptr(), count, stream=st)

    sep = outs()
    for fn, o in zip((lut, mm, gate), sep):
        fn(o, None)
        sync()
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    tog = outs()
    sync()
    with torch.cuda.stream(st):
        for fn, o in zip((lut, mm, gate), tog):
            fn(o, st.cuda_stream)
    st.synchronize()
    for a, b, name in zip(sep, tog, ("lut", "matmul", "gate")):
        assert np.array_equal(a.cpu().numpy(), b.cpu().numpy()), name
    assert np.array_equal(sep[1].cpu().numpy(), ref.lwe_matmul(w, cts, bias))
    assert not bool((sep[0] == POISON).all()) and not bool((sep[2] == POISON).all())


def test_host_form_on_the_global_context_equals_the_device_call(eoc, eng):
    """eoc_lwe_matmul at (33, 31, n + 1, 5): one engine, then two engines on one device (whole vectors 3 + 2); no key anywhere"""
    p = eoc.default_params(0)
    rng = np.random.default_rng(3000)
    w, cts, bias = ref.weights(rng, 33, 31), ref.words(rng, (5, 31, p.n + 1)), ref.words(rng, 33)
    dev = run(eng, w, cts, bias)
    try:
        eoc.gpu_shutdown()
        eoc.gpu_init(p, devices=[0])
        one = eoc.lwe_matmul(w, cts, bias)
        none = eoc.lwe_matmul(w, cts)
        empty = eoc.lwe_matmul(w, cts[:0], bias)
        eoc.gpu_shutdown()
        eoc.gpu_init(p, devices=[0, 0])
        two = eoc.lwe_matmul(w, cts, bias)
    finally:
        eoc.gpu_shutdown()
    assert np.array_equal(dev, ref.lwe_matmul(w, cts, bias))
    assert np.array_equal(one, dev) and np.array_equal(two, dev) and empty.shape == (0, 33, p.n + 1)
    assert np.array_equal(none, ref.lwe_matmul(w, cts))


def phases(sk, cts):
    c = np.asarray(cts).astype(np.int64)
    return ((c[..., -1] - c[..., :-1] @ np.asarray(sk.lwe_key, np.int64)) + 2**31) % 2**32 - 2**31


def test_two_layer_sign_network_on_the_lwe_route(eoc):
    """Set A, the network and the 64 vectors of tests/dinn_case.py, run_device(hidden="lwe") on an engine that holds the cloud
    key and NO packing key: layer 2's input tensor is layer 1's LUT outputs, its sums equal the reference applied to them word
    for word, and all 64 x 2 outputs decrypt to evaluate_plain"""
    import test_gpu_cmux as tc
    p, sk, pk, _, eng = tc.keys(eoc, 0, dc.KEY_SEED)
    net, x, _ = dc.dinn_case(eoc, p, sk)
    lists = np.stack([pk.encrypt_torus(v * dc.DELTA_IN, 1800 + k) for k, v in enumerate(x)])      # [64][1][2][N]
    launches, ks = eng.lwe_matmul_launches(), eng.stats()["keyswitches"]
    packed = eoc.lib().eoc_engine_packed_samples(eng.h)
    out, layers, ins = net.run_device(eng, lists, return_layers=True, hidden="lwe")
    sync()
    assert eoc.lib().eoc_engine_packed_samples(eng.h) == packed and eng.lwe_matmul_launches() - launches == 1
    # key switches: layer 0's 64 x 8 sums and the two lookups' 64 x 8 + 64 x 2 -- none behind layer 2's sums
    assert eng.stats()["keyswitches"] - ks == 64 * 8 + 64 * 8 + 64 * 2
    l1 = layers[0].cpu().numpy()
    assert ins[1].data_ptr() == layers[0].data_ptr() and l1.shape == (64, 8, p.n + 1)
    # layer 2's lookups read exactly the reference's sums of layer 1's GPU outputs
    torch = torch_cuda()
    want_lin = ref.lwe_matmul(net.layers[1].weights, l1, net.layers[1].bias)
    img = model(eng, net.layers[1].weights)
    lin = torch.empty((64, 2, p.n + 1), dtype=torch.int32, device="cuda")
    eng.lwe_matmul_device(img.data_ptr(), 2, 8, layers[0].data_ptr(), p.n + 1, 64, None, lin.data_ptr())
    relut = torch.empty_like(lin)
    eng.lut_batch_device(to_dev(net.layers[1].tv).data_ptr(), 1, to_dev(want_lin).data_ptr(), relut.data_ptr(), 64 * 2)
    sync()
    assert np.array_equal(lin.cpu().numpy(), want_lin)
    got = out.cpu().numpy()
    assert np.array_equal(relut.cpu().numpy(), got)
    want, pres = net.evaluate_plain(x, return_pre=True)
    ph = phases(sk, got)
    assert got.shape == (64, 2, p.n + 1) and np.array_equal(np.where(ph >= 0, 1, -1) * dc.MU2, want)
    assert np.abs(ph - want).max() / 2.0**32 < 0.05                      # a bootstrap output: sigma ~ 0.004
    assert np.array_equal(np.where(phases(sk, l1) >= 0, 1, -1), np.where(pres[0] + (1 << 20) >= 0, 1, -1))
    # the sums' phases: exactly the weighted phases of layer 1's outputs (the error is sum_k w_k e_k, nothing else)
    w2 = net.layers[1].weights.astype(np.int64)
    assert np.array_equal(phases(sk, want_lin), (np.einsum("rk,bk->br", w2, phases(sk, l1)) + 2**31) % 2**32 - 2**31)


def test_run_device_samples_from_lwe_inputs(eoc):
    """the same network from 64 x 32 inputs encrypted with eoc_lwe_encrypt: layer 0's sums have phase bias + sum w phase(input)
    exactly, under the secret key, and the network decrypts to evaluate_plain"""
    import test_gpu_cmux as tc
    p, sk, _, _, eng = tc.keys(eoc, 0, dc.KEY_SEED)
    net, x, _ = dc.dinn_case(eoc, p, sk)
    L = eoc.lib()
    cts = np.empty((64, 32, p.n + 1), np.int32)
    for b in range(64):
        for k in range(32):
            assert L.eoc_lwe_encrypt(sk.h, 3100, b * 32 + k, int(x[b, k]) * dc.DELTA_IN, p.ks_stdev, cts[b, k].ctypes.data) == 0
    packed, ks = L.eoc_engine_packed_samples(eng.h), eng.stats()["keyswitches"]
    out, layers, ins = net.run_device_samples(eng, cts, return_layers=True)
    sync()
    assert L.eoc_engine_packed_samples(eng.h) == packed and eng.stats()["keyswitches"] - ks == 64 * 8 + 64 * 2   # the lookups' only
    # layer 0: the sums the lookups read, recomputed by the device call, against the reference and in phase
    w0 = net.layers[0].weights
    torch = torch_cuda()
    lin = torch.empty((64, 8, p.n + 1), dtype=torch.int32, device="cuda")
    eng.lwe_matmul_device(model(eng, w0).data_ptr(), 8, 32, ins[0].data_ptr(), p.n + 1, 64, None, lin.data_ptr())
    sync()
    lin = lin.cpu().numpy()
    assert np.array_equal(lin, ref.lwe_matmul(w0, cts, net.layers[0].bias))
    in_ph = phases(sk, cts)                                               # [64][32]
    want_ph = (np.einsum("rk,bk->br", w0.astype(np.int64), in_ph) + 2**31) % 2**32 - 2**31
    assert np.array_equal(phases(sk, lin), want_ph)
    err = (in_ph - x * dc.DELTA_IN) / 2.0**32
    assert np.abs(err).max() < 8 * p.ks_stdev                             # fresh samples: sigma = ks_stdev
    want, pres = net.evaluate_plain(x, return_pre=True)
    got = out.cpu().numpy()
    ph = phases(sk, got)
    assert got.shape == (64, 2, p.n + 1) and np.array_equal(np.where(ph >= 0, 1, -1) * dc.MU2, want)
    assert np.array_equal(np.where(phases(sk, layers[0].cpu().numpy()) >= 0, 1, -1), np.where(pres[0] + (1 << 20) >= 0, 1, -1))
