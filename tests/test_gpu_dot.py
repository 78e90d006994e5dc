"""Inner products with public integer weights on the MI355X: eoc_dot_device against the chunked reference
(tests/c/dot_ref.c through tests/dot_oracle.py) byte for byte at every shape that takes another path, edge words, the key-switch
path against reference + orc_keyswitch, slices, two engines and the global context in key mode 2, errors, a captured
linear_device replayed on new inputs (the protocol of tests/test_gpu_capture.py), and a two-layer sign network end to end.
Host side: tests/test_dot_cpu.py; registers: tests/test_isa_dot.py."""
import numpy as np
import pytest

import compact_oracle as co
import dinn_case as dc
import dot_oracle as do
from gpu_util import sync, to_dev, torch_cuda

pytestmark = pytest.mark.gpu
N = 1024
POISON = 0x5A5AA5A5
EOC_ERR_ARG, EOC_ERR_NO_KEY, EOC_ERR_STATE = -1, -4, -6
INT32_MIN, INT32_MAX = -(2**31), 2**31 - 1
SMALL_N, SMALL_SEED = 40, 63


@pytest.fixture(scope="module")
def eoc(built_lib):
    torch_cuda()
    import eoc_tfhe_amd
    return eoc_tfhe_amd


def small(eoc):
    """(params at n = 40, secret key, oracle with the key-switch key, engine with the cloud key)"""
    import capture_cases as cc
    p, sk, orc, eng = cc.small_keys(eoc, 0, SMALL_N, SMALL_SEED, bk=False)
    co.ksk(orc)
    return p, sk, orc, eng


def model(eng, w):
    """the device image of weights w: a uint8 tensor that must stay alive while it is used"""
    torch = torch_cuda()
    w = np.asarray(w)
    img = torch.empty(eng.weights_image_bytes(*w.shape), dtype=torch.uint8, device="cuda")
    eng.weights_to_device(w, img.data_ptr())
    return img


def run(eng, w, lists, bias=None, linear=False, img=None):
    """dot_device / linear_device into a poisoned buffer with one row behind the output, which must stay untouched"""
    torch = torch_cuda()
    w = np.asarray(w)
    rows, cols = w.shape
    lists = np.ascontiguousarray(lists, np.int32).reshape(-1, do.n_lists(cols), 2, N)
    batch, stride = lists.shape[0], (eng.n + 1 if linear else N + 1)
    img = model(eng, w) if img is None else img
    d_lists = to_dev(lists)
    d_bias = None if bias is None else to_dev(np.asarray(bias, np.int32))
    out = torch.full((batch * rows + 1, stride), POISON, dtype=torch.int32, device="cuda")
    fn = eng.linear_device if linear else eng.dot_device
    fn(img.data_ptr(), rows, cols, d_lists.data_ptr(), batch, None if d_bias is None else d_bias.data_ptr(), out.data_ptr())
    sync()
    o = out.cpu().numpy()
    assert (o[-1].view(np.uint32) == POISON).all(), "the row behind the output was written"
    return o[:-1].reshape(batch, rows, stride)


def rand_lists(rng, batch, cols):
    return rng.integers(INT32_MIN, INT32_MAX, (batch, do.n_lists(cols), 2, N), endpoint=True).astype(np.int32)


def rand_weights(rng, rows, cols):
    """+-127, 0 and random values"""
    w = rng.integers(-127, 128, (rows, cols)).astype(np.int8)
    w.flat[::5] = np.resize(np.array([127, -127, 0], np.int8), w.flat[::5].size)
    return w


def keyswitch_ref(orc, u):
    return np.stack([orc.keyswitch(x) for x in u.reshape(-1, N + 1)]).reshape(u.shape[:-1] + (orc.n + 1,))


SHAPES = [(1, 1, 1), (1, N, 1), (5, N + 3, 3), (2, 8 * N, 1), (2, 8 * N + 1, 2)]


@pytest.mark.parametrize("rows,cols,batch", SHAPES)
def test_dot_equals_the_reference(eoc, rows, cols, batch):
    """the smallest case, one full list, a ragged last list with rows no multiple of the waves per workgroup and several
    vectors, exactly one full chunk, and a chunk of one list behind a full one (two waves add into one row); with a bias and
    with NULL; no key on the engine"""
    p = small(eoc)[0]
    eng = eoc.Engine(p)                                                  # no key
    rng = np.random.default_rng(1000 + cols + rows)
    w, lists = rand_weights(rng, rows, cols), rand_lists(rng, batch, cols)
    bias = rng.integers(INT32_MIN, INT32_MAX, rows, endpoint=True).astype(np.int32)
    img = model(eng, w)
    before = eng.dot_launches()
    eng.set_profiling(True)
    eng.kernel_times()
    got = run(eng, w, lists, bias, img=img)
    times = eng.kernel_times()
    eng.set_profiling(False)
    assert np.array_equal(got, do.dot(w, lists, bias)), (rows, cols, batch)
    assert np.array_equal(run(eng, w, lists, None, img=img), do.dot(w, lists, None))
    assert eng.dot_launches() - before == 2 and eng.stats()["keyswitches"] == 0
    # the transform, the start of the rows and the mask kernel, booked under the key switch
    assert times["keyswitch"]["launches"] == 3 and times["prepare"]["launches"] == times["blind_rotate"]["launches"] == 0
    eng.close()


def test_edge_words(eoc):
    """the full-scale chunk (every weight +127, list words all INT32_MIN, then all INT32_MAX: 2^50.99 before the conversion)
    and list words cycling through 0, -1, INT32_MIN, INT32_MAX under random weights"""
    eng = small(eoc)[3]
    w = np.full((1, 8 * N), 127, np.int8)
    img = model(eng, w)
    for word in (INT32_MIN, INT32_MAX):
        lists = np.full((1, 8, 2, N), word, np.int32)
        assert np.array_equal(run(eng, w, lists, img=img), do.dot(w, lists)), word
    rng = np.random.default_rng(1100)
    w = rand_weights(rng, 3, N + 1)
    lists = np.resize(np.array([0, -1, INT32_MIN, INT32_MAX, -1, 0, INT32_MAX], np.int32), (2, 2, 2, N))
    bias = np.array([INT32_MIN, INT32_MAX, -1], np.int32)
    assert np.array_equal(run(eng, w, lists, bias), do.dot(w, lists, bias))
    assert np.array_equal(run(eng, -w, lists, bias), do.dot(-w, lists, bias))


def test_linear_equals_reference_dot_plus_keyswitch(eoc):
    p, sk, orc, eng = small(eoc)
    rng = np.random.default_rng(1200)
    rows, cols, batch = 5, N + 3, 3
    w, lists = rand_weights(rng, rows, cols), rand_lists(rng, batch, cols)
    bias = rng.integers(INT32_MIN, INT32_MAX, rows, endpoint=True).astype(np.int32)
    before, launches = eng.stats(), eng.dot_launches()
    eng.set_profiling(True)
    eng.kernel_times()
    got = run(eng, w, lists, bias, linear=True)
    times = eng.kernel_times()
    eng.set_profiling(False)
    after = eng.stats()
    assert np.array_equal(got, keyswitch_ref(orc, do.dot(w, lists, bias)))
    assert after["keyswitches"] - before["keyswitches"] == batch * rows and after["bootstraps"] == before["bootstraps"]
    assert eng.dot_launches() - launches == 1
    assert times["keyswitch"]["launches"] == 4 and times["prepare"]["launches"] == times["blind_rotate"]["launches"] == 0
    # the key switch of dot_device's samples is the same thing in two calls
    torch = torch_cuda()
    d_u = to_dev(run(eng, w, lists, bias))
    d_o = torch.empty((batch * rows, p.n + 1), dtype=torch.int32, device="cuda")
    eng.keyswitch_device(d_u.data_ptr(), d_o.data_ptr(), batch * rows)
    sync()
    assert np.array_equal(d_o.cpu().numpy().reshape(got.shape), got)
    # encrypted inputs decrypt to the plain sums: 40 inputs of +-1 at 2^-9, weights in [-3, 3]
    pk = eoc.PublicKey(sk.public_key_bytes())
    x = rng.choice([-1, 1], (4, 40))
    w2 = rng.integers(-3, 4, (6, 40))
    enc = np.stack([pk.encrypt_torus(v * (1 << 23), 1300 + k) for k, v in enumerate(x)])
    out = run(eng, w2, enc, None, linear=True).astype(np.int64)
    ph = out[..., -1] - out[..., :-1] @ np.asarray(sk.lwe_key, np.int64)
    err = ((ph - do.plain_sum(w2, x * (1 << 23)) + 2**31) % 2**32 - 2**31) / 2.0**32
    assert np.abs(err).max() < 0.02, np.abs(err).max()                   # the key switch's noise (sigma ~ 0.002 at n = 40 too)


def test_linear_on_set_b_at_full_size(eoc):
    """(rows, cols, batch) = (4, N, 1) at n = 630: the matrix-core key switch behind the operand rows k_dot_mask wrote"""
    import test_gpu_cmux as tc
    p, sk, pk, orc, eng = tc.keys(eoc, 1)
    co.ksk(orc)
    rng = np.random.default_rng(1400)
    w = rand_weights(rng, 4, N)
    lists = pk.encrypt_torus(rng.integers(-(2**22), 2**22, N), 1401).reshape(1, 1, 2, N)
    assert np.array_equal(run(eng, w, lists, None, linear=True), keyswitch_ref(orc, do.dot(w, lists)))


SLICE_BODY = """
    from test_gpu_dot import run
    p = eoc.default_params(0)
    p.n = 40
    eng = eoc.Engine(p)
    rng = np.random.default_rng(1500)
    w = rng.integers(-127, 128, (3, 1027)).astype(np.int8)
    lists = rng.integers(-2**31, 2**31, (3, 2, 2, 1024)).astype(np.int32)
    np.save(%r, run(eng, w, lists))
    out['launches'] = eng.dot_launches()
    out['grows'] = int(eoc.lib().eoc_engine_workspace_grows(eng.h))
"""


def test_workspace_budget_slices_the_batch(eoc, tmp_path):
    """EOC_TFHE_DOT_WS_BYTES (read at engine creation) at one vector's spectra (L x 16 KiB) and a little: three vectors run as
    three slices, the same words as the unsliced call.  A budget below one vector is refused."""
    import test_gpu_pack as tp
    eng = small(eoc)[3]
    rng = np.random.default_rng(1500)
    w = rng.integers(-127, 128, (3, 1027)).astype(np.int8)
    lists = rng.integers(-2**31, 2**31, (3, 2, 2, 1024)).astype(np.int32)
    before = eng.dot_launches()
    whole = run(eng, w, lists)
    assert eng.dot_launches() - before == 1 and np.array_equal(whole, do.dot(w, lists))
    a = str(tmp_path / "sliced.npy")
    sliced = tp.child(SLICE_BODY % a, env={"EOC_TFHE_DOT_WS_BYTES": str(2 * 16384 + 100)})
    assert sliced["launches"] == 3 and sliced["grows"] == 1
    assert np.array_equal(np.load(a), whole)
    small_budget = tp.child("""
        p = eoc.default_params(0)
        p.n = 40
        eng = eoc.Engine(p)
        x = torch.zeros(1 << 16, dtype=torch.int32, device='cuda')
        img = torch.zeros(eng.weights_image_bytes(1, 1027), dtype=torch.uint8, device='cuda')
        eng.weights_to_device(np.ones((1, 1027), np.int8), img.data_ptr())
        u = torch.zeros(1025, dtype=torch.int32, device='cuda')
        out['rc'] = eoc.lib().eoc_dot_device(eng.h, img.data_ptr(), 1, 1027, x.data_ptr(), 1, None, u.data_ptr(), None)
    """, env={"EOC_TFHE_DOT_WS_BYTES": str(2 * 16384 - 1)})
    assert small_budget["rc"] == EOC_ERR_ARG


def test_global_context_one_and_two_engines_and_key_mode_2(eoc, tmp_path):
    import test_gpu_pack as tp
    p, sk, orc, eng = small(eoc)
    rng = np.random.default_rng(1600)
    w, lists = rand_weights(rng, 3, N + 3), rand_lists(rng, 3, N + 3)
    bias = rng.integers(INT32_MIN, INT32_MAX, 3, endpoint=True).astype(np.int32)
    ref = run(eng, w, lists, bias, linear=True)
    try:
        eoc.gpu_shutdown()
        eoc.gpu_init(p, devices=[0])
        eoc.upload_cloud_key(sk)
        one = eoc.linear(w, lists, bias)
        eoc.gpu_shutdown()
        eoc.gpu_init(p, devices=[0, 0])
        eoc.upload_cloud_key(sk)
        two = eoc.linear(w, lists, bias)
        none = eoc.linear(w, lists)
        per = [e["keyswitches"] for e in eoc.stats_multi()["engines"]]
    finally:
        eoc.gpu_shutdown()
    assert np.array_equal(one, ref) and np.array_equal(two, ref)
    assert np.array_equal(none, run(eng, w, lists, None, linear=True))
    assert per == [2 * 2 * 3, 2 * 1 * 3]                                 # whole vectors per engine: 2 + 1, two calls
    # a server that holds the cloud key alone (key mode 2)
    np.save(tmp_path / "w.npy", w)
    np.save(tmp_path / "lists.npy", lists)
    np.save(tmp_path / "bias.npy", bias)
    sk.export_cloud_key().tofile(tmp_path / "ck.bin")
    server = tp.child("""
        eoc.global_import_cloud_key_blob(np.fromfile(%r, np.uint8))
        out['mode'] = eoc.global_key_mode()
        np.save(%r, eoc.linear(np.load(%r), np.load(%r), np.load(%r)))
        eoc.Tfhe.resetGateKey()
    """ % (str(tmp_path / "ck.bin"), str(tmp_path / "got.npy"), str(tmp_path / "w.npy"), str(tmp_path / "lists.npy"),
           str(tmp_path / "bias.npy")))
    assert server == {"mode": 2}
    assert np.array_equal(np.load(tmp_path / "got.npy"), ref)


def test_errors(eoc):
    torch = torch_cuda()
    L = eoc.lib()
    p, sk, orc, keyed = small(eoc)
    eng = eoc.Engine(p)                                                  # no key
    w = np.ones((2, 5), np.int8)
    img = model(eng, w)
    lists = torch.zeros((3, 1, 2, N), dtype=torch.int32, device="cuda")
    u = torch.full((3 * 2, N + 1), 7, dtype=torch.int32, device="cuda")
    o = torch.full((3 * 2, p.n + 1), 7, dtype=torch.int32, device="cuda")
    args = (img.data_ptr(), 2, 5, lists.data_ptr(), 3, None)
    assert L.eoc_linear_device(eng.h, *args, o.data_ptr(), None) == EOC_ERR_NO_KEY
    assert L.eoc_linear_device(eng.h, img.data_ptr(), 2, 5, lists.data_ptr(), 0, None, o.data_ptr(), None) == EOC_ERR_NO_KEY
    bad = w.copy()
    bad[1, 3] = -128
    assert L.eoc_weights_to_device(eng.h, bad.ctypes.data, 2, 5, img.data_ptr(), None) == EOC_ERR_ARG
    assert b"-128" in L.eoc_last_error()
    for rows, cols in ((0, 5), (2, 0), (2**20 + 1, 5)):
        assert L.eoc_weights_to_device(eng.h, w.ctypes.data, rows, cols, img.data_ptr(), None) == EOC_ERR_ARG
    # overlapping buffers: the output on the lists, on the image, on the bias
    assert L.eoc_dot_device(eng.h, img.data_ptr(), 2, 5, lists.data_ptr(), 3, None, lists.data_ptr() + 64, None) == EOC_ERR_ARG
    assert L.eoc_dot_device(eng.h, img.data_ptr(), 2, 5, lists.data_ptr(), 3, None, img.data_ptr(), None) == EOC_ERR_ARG
    assert L.eoc_dot_device(eng.h, img.data_ptr(), 2, 5, lists.data_ptr(), 3, u.data_ptr() + 4 * (N + 1), u.data_ptr(), None) == EOC_ERR_ARG
    assert L.eoc_linear_device(keyed.h, img.data_ptr(), 2, 5, lists.data_ptr(), 3, None, lists.data_ptr(), None) == EOC_ERR_ARG
    for a in ((None,) + args[1:], args[:3] + (None,) + args[4:]):
        assert L.eoc_dot_device(eng.h, *a, u.data_ptr(), None) == EOC_ERR_ARG
    assert L.eoc_dot_device(eng.h, *args, None, None) == EOC_ERR_ARG
    # batch x rows = 0 is a no-op
    assert L.eoc_dot_device(eng.h, img.data_ptr(), 2, 5, lists.data_ptr(), 0, None, u.data_ptr(), None) == 0
    assert L.eoc_linear_device(keyed.h, img.data_ptr(), 2, 5, lists.data_ptr(), 0, None, o.data_ptr(), None) == 0
    sync()
    assert bool((u == 7).all()) and bool((o == 7).all()) and eng.dot_launches() == 0
    # under capture a workspace that would have to grow is refused, and nothing is launched
    st = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    filler = torch.zeros(64, dtype=torch.int32, device="cuda")
    with torch.cuda.graph(g, stream=st):
        filler.fill_(1)                                                  # the graph is not empty without the refused call
        rc = L.eoc_dot_device(eng.h, *args, u.data_ptr(), st.cuda_stream)
    assert rc == EOC_ERR_STATE and b"graph capture" in L.eoc_last_error()
    sync()
    assert bool((u == 7).all())
    eng.close()


def test_captured_linear_replays_the_reference_words(eoc):
    """tests/test_gpu_capture.py's protocol on linear_device: a reserved engine, one eager call, the capture, then two replays on
    input sets written in place, with eager calls on other live buffers in between; every word against the reference, the grow
    counter unchanged"""
    import capture_cases as cc
    import test_gpu_capture as tcap

    class Linear(cc.Case):
        rows, cols, batch = 5, N + 3, 3
        expect = dict(keyswitches=15)

        def setup(self):
            self.p, self.sk, self.orc, self.eng2 = small(self.eoc)
            self.fresh(self.p).load_cloud_key(self.sk)
            assert self.eoc.lib().eoc_engine_reserve(self.eng.h, 4 * self.rows, 0, 0) == 0
            rng = np.random.default_rng(1700)
            self.w = rand_weights(rng, self.rows, self.cols)
            self.bias = rng.integers(INT32_MIN, INT32_MAX, self.rows, endpoint=True).astype(np.int32)
            self.inp = [rand_lists(rng, self.batch, self.cols) for _ in range(5)]
            self.img = {id(e): model(e, self.w) for e in (self.eng, self.eng2)}
            self.d_bias = to_dev(self.bias)

        def alloc(self, batch=None):
            batch = batch or self.batch
            return dict(lists=self.new((batch, 2, 2, N)), out=self.new((batch, self.rows, self.p.n + 1)))

        def load(self, b, k):
            b["lists"].copy_(to_dev(np.resize(self.inp[k], tuple(b["lists"].shape))))

        def linear(self, eng, b, batch, st):
            eng.linear_device(self.img[id(eng)].data_ptr(), self.rows, self.cols, b["lists"].data_ptr(), batch,
                              self.d_bias.data_ptr(), b["out"].data_ptr(), stream=st)

        def call(self, eng, b, st):
            self.linear(eng, b, self.batch, st)

        def ref(self, k):
            return dict(out=keyswitch_ref(self.orc, do.dot(self.w, self.inp[k], self.bias)))

        def other(self):
            if not hasattr(self, "wide"):
                self.wide = self.alloc(4)                                # operand rows 15 .. 19 left behind, inside the reserve
                self.load(self.wide, 4)
            self.linear(self.eng, self.dbufs[0], 1, None)
            self.linear(self.eng, self.wide, 4, None)

    torch, L = torch_cuda(), eoc.lib()
    c = Linear(eoc)
    eng = c.eng
    st = tcap.side_stream(torch)
    c.set_inputs(0)
    c.poison()
    sync()
    # the list spectra are sized by the widest call the engine will see: the disturbance's four vectors
    c.load(c.dbufs[0], 3)
    wide = c.alloc(4)
    c.linear(eng, wide, 4, None)
    sync()
    st.wait_stream(torch.cuda.current_stream())
    before = eng.stats()
    with torch.cuda.stream(st):
        c.run(st.cuda_stream)
    st.synchronize()
    after = eng.stats()
    for counter, delta in c.expect.items():
        assert after[counter] - before[counter] == delta, counter
    tcap.assert_words(c.fetch(), c.want(0), c, "eager")
    c.set_inputs(0)
    sync()
    grows = L.eoc_engine_workspace_grows(eng.h)
    g = tcap.capture(torch, st, c.run)
    assert L.eoc_engine_workspace_grows(eng.h) == grows
    got = {}
    for k in (1, 2):
        c.set_inputs(k)
        c.disturb()
        c.poison()
        sync()
        assert L.eoc_engine_workspace_grows(eng.h) == grows, "a call after the capture grew a buffer: the graph is void"
        g.replay()
        sync()
        got[k] = c.fetch()
        assert not tcap.still_poisoned(c), (k, "the replay left the poison word in the output")
        tcap.assert_words(got[k], c.want(k), c, f"replay {k}")
    for k in (1, 2):
        assert cc.bytes_equal(got[k]["out"], c.second(k)["out"]), k
    del g
    c.close()


def test_two_layer_sign_network_end_to_end(eoc):
    """Set A: 32 inputs of +-1 (encrypt_torus), a 32 -> 8 sign layer with weights in [-3, 3], pack_device, an 8 -> 2 sign layer
    with weights +-1; the 64 vectors of tests/dinn_case.py, every pre-activation >= 6 predicted sigma from its boundary.  All
    64 x 2 outputs decrypt to evaluate_plain; the words behind layer 1 equal the composed reference (dot reference, orc_keyswitch,
    the LUT oracle) on the first and the last vector."""
    import lut2_oracle as l2
    import lut_oracle as lo
    import test_gpu_pack as tp
    p, sk, blob, _, orc = l2.keys(eoc, 0)
    assert l2.KEY_SEED == dc.KEY_SEED
    eng = tp.keys(eoc, 0)[4]                                             # the same key seed: cloud key and packing key
    net, x, _ = dc.dinn_case(eoc, p, sk)
    pk = eoc.PublicKey(sk.public_key_bytes())
    lists = np.stack([pk.encrypt_torus(v * dc.DELTA_IN, 1800 + k) for k, v in enumerate(x)])      # [64][1][2][N]
    out, layers = net.run_device(eng, lists, return_layers=True)
    sync()
    want, pres = net.evaluate_plain(x, return_pre=True)
    got = out.cpu().numpy()
    assert got.shape == (64, 2, p.n + 1)
    g64 = got.astype(np.int64)
    ph = ((g64[..., -1] - g64[..., :-1] @ np.asarray(sk.lwe_key, np.int64)) + 2**31) % 2**32 - 2**31
    assert np.array_equal(np.where(ph >= 0, 1, -1) * dc.MU2, want)
    assert np.abs(ph - want).max() / 2.0**32 < 0.05                      # a bootstrap output: sigma ~ 0.004
    # layer 1, word for word, on the first and the last vector
    l1 = layers[0].cpu().numpy()
    h1 = np.where(pres[0] + (1 << 20) >= 0, 1, -1)
    g1 = l1.astype(np.int64)
    ph1 = ((g1[..., -1] - g1[..., :-1] @ np.asarray(sk.lwe_key, np.int64)) + 2**31) % 2**32 - 2**31
    assert np.array_equal(np.where(ph1 >= 0, 1, -1), h1)
    for b in (0, 63):
        u = do.dot(net.layers[0].weights, lists[b:b + 1])[0]
        lin = np.stack([orc.keyswitch(s) for s in u])
        assert np.array_equal(l1[b], lo.lut_batch(orc, net.layers[0].tv[None], lin)[0]), b
