"""Convolutions with public int8 kernels on the MI355X: eoc_conv_device against the chunked reference
(tests/c/conv_ref.c through tests/conv_oracle.py) byte for byte at every shape that takes another path and on both template
instances, edge words, the inner product's masks under the word map, the slot-table extraction and the key-switch path against
reference + extraction + orc_keyswitch, slices, captured calls replayed on new inputs, a round trip that needs no key, and a
convolution -> dense sign network end to end.  Host side: tests/test_conv_cpu.py; registers: tests/test_isa_conv.py."""
import numpy as np
import pytest

import compact_oracle as co
import conv_case as ccase
import conv_oracle as cv
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


def table(eng, slots, lists_per_vec):
    """the device slot table: an int32 tensor that must stay alive while it is used"""
    torch = torch_cuda()
    d = torch.empty(len(slots), dtype=torch.int32, device="cuda")
    assert eng.conv_slots_to_device(slots, lists_per_vec, d.data_ptr()) == len(slots)
    return d


def poisoned(rows, stride):
    """[rows + 1][stride] of the poison word: one row behind the output, which must stay untouched"""
    torch = torch_cuda()
    return torch.full((rows + 1, stride), POISON, dtype=torch.int32, device="cuda")


def fetch(out, shape):
    sync()
    o = out.cpu().numpy()
    assert (o[-1].view(np.uint32) == POISON).all(), "the row behind the output was written"
    return o[:-1].reshape(shape)


def run_conv(eng, w, lists, bias=None, img=None):
    w = np.asarray(w)
    rows, cols = w.shape
    lists = np.ascontiguousarray(lists, np.int32).reshape(-1, do.n_lists(cols), 2, N)
    batch = lists.shape[0]
    img = model(eng, w) if img is None else img
    d_lists = to_dev(lists)
    d_bias = None if bias is None else to_dev(np.asarray(bias, np.int32))
    out = poisoned(batch * rows, 2 * N)
    eng.conv_device(img.data_ptr(), rows, cols, d_lists.data_ptr(), batch, None if d_bias is None else d_bias.data_ptr(), out.data_ptr())
    return fetch(out, (batch, rows, 2, N))


def run_linear(eng, w, lists, slots, bias=None):
    w = np.asarray(w)
    rows, cols = w.shape
    lists = np.ascontiguousarray(lists, np.int32).reshape(-1, do.n_lists(cols), 2, N)
    batch = lists.shape[0]
    img, d_slots, d_lists = model(eng, w), table(eng, slots, rows), to_dev(lists)
    d_bias = None if bias is None else to_dev(np.asarray(bias, np.int32))
    out = poisoned(batch * len(slots), eng.n + 1)
    eng.conv_linear_device(img.data_ptr(), rows, cols, d_lists.data_ptr(), batch, None if d_bias is None else d_bias.data_ptr(),
                           d_slots.data_ptr(), len(slots), out.data_ptr())
    return fetch(out, (batch, len(slots), eng.n + 1))


def run_extract(eng, lists, slots):
    lists = np.ascontiguousarray(lists, np.int32)
    batch, per_vec = lists.shape[:2]
    d_slots, d_lists = table(eng, slots, per_vec), to_dev(lists)
    out = poisoned(batch * len(slots), eng.n + 1)
    eng.conv_extract_device(d_lists.data_ptr(), per_vec, batch, d_slots.data_ptr(), len(slots), out.data_ptr())
    return fetch(out, (batch, len(slots), eng.n + 1))


def rand_lists(rng, batch, cols):
    return rng.integers(INT32_MIN, INT32_MAX, (batch, do.n_lists(cols), 2, N), endpoint=True).astype(np.int32)


def rand_weights(rng, rows, cols):
    """+-127, 0 and random values"""
    w = rng.integers(-127, 128, (rows, cols)).astype(np.int8)
    w.flat[::5] = np.resize(np.array([127, -127, 0], np.int8), w.flat[::5].size)
    return w


def extract_keyswitch_ref(orc, out_lists, slots):
    """reference lists [batch][rows][2][N] -> compact_oracle extraction of the table's slots -> orc_keyswitch"""
    return np.stack([co.expand(orc, v, np.asarray(slots, np.int64)) for v in out_lists])


SHAPES = [(0, 1, 1, 1), (0, 5, 1, 3), (0, 2, 8, 1), (0, 3, 9, 2), (1, 3, 9, 2)]


@pytest.mark.parametrize("pset,rows,L,batch", SHAPES)
def test_conv_equals_the_reference(eoc, pset, rows, L, batch):
    """the smallest case, a partial last workgroup (30 waves), exactly one full chunk, and a one-list chunk behind a full one
    (the adding instance behind k_conv_init); cols = (L - 1) N + 3 and L N; no bias and a bias that wraps; no key on the engine"""
    eng = eoc.Engine(eoc.default_params(pset))                           # no key
    for cols in ((L - 1) * N + 3, L * N):
        rng = np.random.default_rng(2000 + cols + rows)
        w, lists = rand_weights(rng, rows, cols), rand_lists(rng, batch, cols)
        bias = np.resize(np.array([INT32_MAX, INT32_MIN, -1], np.int32), rows)
        img = model(eng, w)
        before = eng.conv_launches()
        eng.set_profiling(True)
        eng.kernel_times()
        got = run_conv(eng, w, lists, bias, img=img)
        times = eng.kernel_times()
        eng.set_profiling(False)
        assert got.tobytes() == cv.conv(w, lists, bias).tobytes(), (rows, cols, batch)
        assert run_conv(eng, w, lists, None, img=img).tobytes() == cv.conv(w, lists, None).tobytes(), (rows, cols, batch)
        assert eng.conv_launches() - before == 2 and eng.stats()["keyswitches"] == 0 and eng.dot_launches() == 0
        # the transform, (k_conv_init,) k_conv_lists: booked under the key switch
        assert times["keyswitch"]["launches"] == (2 if L <= 8 else 3)
        assert times["prepare"]["launches"] == times["blind_rotate"]["launches"] == 0
    eng.close()


def test_edge_words(eoc):
    """the full-scale chunk on both polynomials (every weight +127, list words all INT32_MIN, then all INT32_MAX: 2^50.99
    before the conversion) and list words cycling through 0, -1, INT32_MIN, INT32_MAX under random weights"""
    eng = small(eoc)[3]
    w = np.full((1, 8 * N), 127, np.int8)
    img = model(eng, w)
    for word in (INT32_MIN, INT32_MAX):
        lists = np.full((1, 8, 2, N), word, np.int32)
        assert run_conv(eng, w, lists, img=img).tobytes() == cv.conv(w, lists).tobytes(), word
    rng = np.random.default_rng(2100)
    w = rand_weights(rng, 3, N + 1)
    lists = np.resize(np.array([0, -1, INT32_MIN, INT32_MAX, -1, 0, INT32_MAX], np.int32), (2, 2, 2, N))
    bias = np.array([INT32_MIN, INT32_MAX, -1], np.int32)
    assert run_conv(eng, w, lists, bias).tobytes() == cv.conv(w, lists, bias).tobytes()
    assert run_conv(eng, -w, lists, bias).tobytes() == cv.conv(-w, lists, bias).tobytes()


def test_c0_is_the_inner_products_mask_on_the_device(eoc):
    """eoc_conv_device's c0 against eoc_dot_device's masks on the same image and lists, under the word map; two chunks"""
    torch = torch_cuda()
    eng = small(eoc)[3]
    rng = np.random.default_rng(2200)
    rows, cols, batch = 3, 8 * N + 5, 2
    w, lists = rand_weights(rng, rows, cols), rand_lists(rng, batch, cols)
    img = model(eng, w)
    conv = run_conv(eng, w, lists, img=img)
    d_lists = to_dev(lists)
    u = torch.empty((batch, rows, N + 1), dtype=torch.int32, device="cuda")
    eng.dot_device(img.data_ptr(), rows, cols, d_lists.data_ptr(), batch, None, u.data_ptr())
    sync()
    assert cv.to_dot_mask(conv[:, :, 0]).tobytes() == np.ascontiguousarray(u.cpu().numpy()[..., :N]).tobytes()


SLOTS = [0, N - 1, 2 * N + 5, 0, 2 * N + 5] + list(range(N + 40, N + 20, -1)) + [3 * N - 1, 7, N, 2 * N, 511, 512, N + 1023, 2, 1, 2 * N + 1000, 33, 1500]


def test_extraction_and_key_switch_equal_the_reference(eoc):
    """a 37-entry table with slot 0, slot N - 1, slots of the last list, repeats and a descending run: conv_linear_device and
    conv_extract_device against reference lists -> extraction -> orc_keyswitch, byte for byte; the prefix table 0 .. 36 also
    against compact_expand_device on the same lists; counters; errors of the table load"""
    torch = torch_cuda()
    p, sk, orc, eng = small(eoc)
    assert len(SLOTS) == 37 and max(SLOTS) == 3 * N - 1
    rng = np.random.default_rng(2300)
    rows, cols, batch = 3, N + 3, 2
    w, lists = rand_weights(rng, rows, cols), rand_lists(rng, batch, cols)
    bias = rng.integers(INT32_MIN, INT32_MAX, rows, endpoint=True).astype(np.int32)
    ref_lists = cv.conv(w, lists, bias)
    want = extract_keyswitch_ref(orc, ref_lists, SLOTS)
    before, launches = eng.stats(), eng.conv_launches()
    eng.set_profiling(True)
    eng.kernel_times()
    got = run_linear(eng, w, lists, SLOTS, bias)
    times = eng.kernel_times()
    eng.set_profiling(False)
    assert got.tobytes() == want.tobytes()
    assert eng.stats()["keyswitches"] - before["keyswitches"] == batch * 37 and eng.conv_launches() - launches == 1
    assert times["prepare"]["launches"] == times["blind_rotate"]["launches"] == 0 and times["keyswitch"]["launches"] >= 4
    assert run_extract(eng, ref_lists, SLOTS).tobytes() == want.tobytes()
    # the prefix table is k_compact_expand's case
    prefix = list(range(37))
    got = run_extract(eng, ref_lists, prefix)
    assert got.tobytes() == extract_keyswitch_ref(orc, ref_lists, prefix).tobytes()
    for b in range(batch):
        d_l = to_dev(ref_lists[b])
        d_o = torch.empty((37, p.n + 1), dtype=torch.int32, device="cuda")
        eng.compact_expand_device(d_l.data_ptr(), 37, d_o.data_ptr())
        sync()
        assert d_o.cpu().numpy().tobytes() == got[b].tobytes(), b
    # the table load validates: a slot behind the vector's last list, an empty table
    L = eoc.lib()
    d = torch.zeros(4, dtype=torch.int32, device="cuda")
    bad = np.array([0, 3 * N], np.uint32)
    assert L.eoc_conv_slots_to_device(eng.h, bad.ctypes.data, 2, 3, d.data_ptr(), None) == EOC_ERR_ARG
    assert b"slot 1" in L.eoc_last_error()
    assert L.eoc_conv_slots_to_device(eng.h, bad.ctypes.data, 2, 4, d.data_ptr(), None) == 0
    assert L.eoc_conv_slots_to_device(eng.h, bad.ctypes.data, 0, 4, d.data_ptr(), None) == EOC_ERR_ARG


def test_errors(eoc):
    torch = torch_cuda()
    L = eoc.lib()
    p, sk, orc, keyed = small(eoc)
    eng = eoc.Engine(p)                                                  # no key
    w = np.ones((2, 5), np.int8)
    img = model(eng, w)
    lists = torch.zeros((3, 1, 2, N), dtype=torch.int32, device="cuda")
    o = torch.full((3 * 2, 2 * N), 7, dtype=torch.int32, device="cuda")
    k = torch.full((3 * 4, p.n + 1), 7, dtype=torch.int32, device="cuda")
    slots = table(eng, [0, 1, N, N + 1], 2)
    lin = (img.data_ptr(), 2, 5, lists.data_ptr(), 3, None, slots.data_ptr(), 4)
    assert L.eoc_conv_linear_device(eng.h, *lin, k.data_ptr(), None) == EOC_ERR_NO_KEY
    assert L.eoc_conv_extract_device(eng.h, o.data_ptr(), 2, 3, slots.data_ptr(), 4, k.data_ptr(), None) == EOC_ERR_NO_KEY
    for rows, cols in ((0, 5), (2, 0), (2**20 + 1, 5)):
        rc = L.eoc_conv_device(eng.h, img.data_ptr(), rows, cols, lists.data_ptr(), 3, None, o.data_ptr(), None)
        assert rc == (0 if rows == 0 else EOC_ERR_ARG), (rows, cols)
    # overlapping buffers: the output on the lists, on the image, on the bias, on the slot table
    args = (img.data_ptr(), 2, 5, lists.data_ptr(), 3)
    assert L.eoc_conv_device(eng.h, *args, None, lists.data_ptr() + 64, None) == EOC_ERR_ARG
    assert L.eoc_conv_device(eng.h, *args, None, img.data_ptr(), None) == EOC_ERR_ARG
    assert L.eoc_conv_device(eng.h, *args, o.data_ptr() + 8 * N, o.data_ptr(), None) == EOC_ERR_ARG
    assert L.eoc_conv_linear_device(keyed.h, *lin, lists.data_ptr(), None) == EOC_ERR_ARG
    assert L.eoc_conv_linear_device(keyed.h, *lin[:6], k.data_ptr() + 16, 4, k.data_ptr(), None) == EOC_ERR_ARG
    assert L.eoc_conv_extract_device(keyed.h, o.data_ptr(), 2, 3, slots.data_ptr(), 4, o.data_ptr(), None) == EOC_ERR_ARG
    # null pointers, a table that is too long
    assert L.eoc_conv_device(eng.h, None, 2, 5, lists.data_ptr(), 3, None, o.data_ptr(), None) == EOC_ERR_ARG
    assert L.eoc_conv_device(eng.h, img.data_ptr(), 2, 5, None, 3, None, o.data_ptr(), None) == EOC_ERR_ARG
    assert L.eoc_conv_device(eng.h, *args, None, None, None) == EOC_ERR_ARG
    assert L.eoc_conv_linear_device(keyed.h, *lin[:6], None, 4, k.data_ptr(), None) == EOC_ERR_ARG
    assert L.eoc_conv_linear_device(keyed.h, *lin[:7], 2**20 + 1, k.data_ptr(), None) == EOC_ERR_ARG
    assert L.eoc_conv_extract_device(keyed.h, None, 2, 3, slots.data_ptr(), 4, k.data_ptr(), None) == EOC_ERR_ARG
    assert L.eoc_conv_extract_device(keyed.h, o.data_ptr(), 0, 3, slots.data_ptr(), 4, k.data_ptr(), None) == EOC_ERR_ARG
    # nothing to do is a no-op
    assert L.eoc_conv_device(eng.h, *args[:4], 0, None, o.data_ptr(), None) == 0
    assert L.eoc_conv_linear_device(keyed.h, *lin[:7], 0, k.data_ptr(), None) == 0
    assert L.eoc_conv_extract_device(keyed.h, o.data_ptr(), 2, 0, slots.data_ptr(), 4, k.data_ptr(), None) == 0
    sync()
    assert bool((o == 7).all()) and bool((k == 7).all()) and eng.conv_launches() == 0
    eng.close()


SLICE_BODY = """
    import capture_cases as cc
    from test_gpu_conv import run_conv, run_linear, SLOTS, SMALL_N, SMALL_SEED
    p, sk, orc, eng = cc.small_keys(eoc, 0, SMALL_N, SMALL_SEED, bk=False)
    rng = np.random.default_rng(2500)
    w = rng.integers(-127, 128, (3, 1027)).astype(np.int8)
    lists = rng.integers(-2**31, 2**31, (5, 2, 2, 1024)).astype(np.int32)
    np.save(%r, run_conv(eng, w, lists))
    out['conv'] = eng.conv_launches()
    np.save(%r, run_linear(eng, w, lists, SLOTS))
    out['linear'] = eng.conv_launches() - out['conv']
"""


def test_workspace_budget_slices_the_batch(eoc, tmp_path):
    """EOC_TFHE_DOT_WS_BYTES (read at engine creation) at two vectors of conv_linear_device (per vector 2 x 16 KiB of spectra
    and 3 x 8 KiB of output lists) and a little: its five vectors run as three slices, conv_device's (spectra alone: three
    vectors fit) as two, the same words as the unsliced calls.  A budget below one vector is refused."""
    import test_gpu_pack as tp
    eng = small(eoc)[3]
    rng = np.random.default_rng(2500)
    w = rng.integers(-127, 128, (3, 1027)).astype(np.int8)
    lists = rng.integers(-2**31, 2**31, (5, 2, 2, 1024)).astype(np.int32)
    before = eng.conv_launches()
    whole, whole_lin = run_conv(eng, w, lists), run_linear(eng, w, lists, SLOTS)
    assert eng.conv_launches() - before == 2 and whole.tobytes() == cv.conv(w, lists).tobytes()
    a, b = str(tmp_path / "conv.npy"), str(tmp_path / "linear.npy")
    per_vec = 2 * 16384 + 3 * 8192
    sliced = tp.child(SLICE_BODY % (a, b), env={"EOC_TFHE_DOT_WS_BYTES": str(2 * per_vec + 100)})
    assert sliced == {"conv": 2, "linear": 3}
    assert np.load(a).tobytes() == whole.tobytes() and np.load(b).tobytes() == whole_lin.tobytes()
    small_budget = tp.child("""
        import capture_cases as cc
        p, sk, orc, eng = cc.small_keys(eoc, 0, 40, 63, bk=False)
        x = torch.zeros(2 * 2 * 2 * 1024, dtype=torch.int32, device='cuda')
        img = torch.zeros(eng.weights_image_bytes(3, 1027), dtype=torch.uint8, device='cuda')
        eng.weights_to_device(np.ones((3, 1027), np.int8), img.data_ptr())
        t = torch.zeros(4, dtype=torch.int32, device='cuda')
        o = torch.zeros(3 * 2 * 1024, dtype=torch.int32, device='cuda')
        L = eoc.lib()
        out['linear'] = L.eoc_conv_linear_device(eng.h, img.data_ptr(), 3, 1027, x.data_ptr(), 1, None, t.data_ptr(), 4, o.data_ptr(), None)
        out['conv'] = L.eoc_conv_device(eng.h, img.data_ptr(), 3, 1027, x.data_ptr(), 1, None, o.data_ptr(), None)
    """, env={"EOC_TFHE_DOT_WS_BYTES": str(per_vec - 1)})
    assert small_budget == {"linear": EOC_ERR_ARG, "conv": 0}            # the spectra alone fit


def test_captured_calls_replay_the_eager_words(eoc):
    """after one eager call of the shape (which sizes the scratch buffers), conv_device and conv_linear_device are captured
    into one graph and replayed on two new input sets written in place, with eager calls on other buffers in between: every
    word equals the eager call's and the reference's, the grow counter stays.  A capture that would grow a scratch buffer is
    refused (EOC_ERR_STATE) and nothing grew."""
    torch, L = torch_cuda(), eoc.lib()
    p, sk, orc, eng2 = small(eoc)
    eng = eoc.Engine(p)
    eng.load_cloud_key(sk)
    rng = np.random.default_rng(2600)
    rows, cols, batch = 3, 8 * N + 3, 2                                  # two chunks: k_conv_init and the adding instance
    w = rand_weights(rng, rows, cols)
    bias = to_dev(rng.integers(INT32_MIN, INT32_MAX, rows, endpoint=True).astype(np.int32))
    inp = [rand_lists(rng, batch, cols) for _ in range(4)]
    img, slots = model(eng, w), table(eng, SLOTS, rows)
    lists = to_dev(inp[0])
    out_l = torch.full((batch, rows, 2, N), POISON, dtype=torch.int32, device="cuda")
    out_k = torch.full((batch, 37, p.n + 1), POISON, dtype=torch.int32, device="cuda")

    def call(d_lists, d_l, d_k, n, st):
        eng.conv_device(img.data_ptr(), rows, cols, d_lists.data_ptr(), n, bias.data_ptr(), d_l.data_ptr(), stream=st)
        eng.conv_linear_device(img.data_ptr(), rows, cols, d_lists.data_ptr(), n, bias.data_ptr(), slots.data_ptr(), 37,
                               d_k.data_ptr(), stream=st)

    # a capture on the fresh engine would have to grow the list spectra: refused, nothing grew, nothing written
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    grows = L.eoc_engine_workspace_grows(eng.h)
    g0 = torch.cuda.CUDAGraph()
    filler = torch.zeros(64, dtype=torch.int32, device="cuda")
    with torch.cuda.graph(g0, stream=st):
        filler.fill_(1)                                                  # the graph is not empty without the refused calls
        rc1 = L.eoc_conv_device(eng.h, img.data_ptr(), rows, cols, lists.data_ptr(), batch, None, out_l.data_ptr(), st.cuda_stream)
        err1 = L.eoc_last_error()
        rc2 = L.eoc_conv_linear_device(eng.h, img.data_ptr(), rows, cols, lists.data_ptr(), batch, None, slots.data_ptr(), 37,
                                       out_k.data_ptr(), st.cuda_stream)
    assert rc1 == rc2 == EOC_ERR_STATE and b"graph capture" in err1
    sync()
    assert L.eoc_engine_workspace_grows(eng.h) == grows and eng.conv_launches() == 0
    assert bool((out_l.view(torch.int32) == POISON).all()) and bool((out_k == POISON).all())
    del g0
    # eager: sizes the scratch buffers; the words of every input set, eagerly, for the comparison
    eager = []
    for k in range(3):
        lists.copy_(to_dev(inp[k]))
        call(lists, out_l, out_k, batch, None)
        sync()
        eager.append((out_l.cpu().numpy(), out_k.cpu().numpy()))
    ref_lists = cv.conv(w, inp[1], bias.cpu().numpy())
    assert eager[1][0].tobytes() == ref_lists.tobytes()
    assert eager[1][1].tobytes() == extract_keyswitch_ref(orc, ref_lists, SLOTS).tobytes()
    lists.copy_(to_dev(inp[0]))
    sync()
    st.wait_stream(torch.cuda.current_stream())
    grows = L.eoc_engine_workspace_grows(eng.h)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=st):
        call(lists, out_l, out_k, batch, st.cuda_stream)
    assert L.eoc_engine_workspace_grows(eng.h) == grows
    other = (to_dev(inp[3][:1]), torch.empty((1, rows, 2, N), dtype=torch.int32, device="cuda"),
             torch.empty((1, 37, p.n + 1), dtype=torch.int32, device="cuda"))
    for k in (1, 2):
        lists.copy_(to_dev(inp[k]))
        call(*other, 1, None)                                            # an eager call of a narrower shape in between
        out_l.fill_(POISON)
        out_k.fill_(POISON)
        sync()
        assert L.eoc_engine_workspace_grows(eng.h) == grows, "a call after the capture grew a buffer: the graph is void"
        g.replay()
        sync()
        assert out_l.cpu().numpy().tobytes() == eager[k][0].tobytes(), k
        assert out_k.cpu().numpy().tobytes() == eager[k][1].tobytes(), k
    del g
    eng.close()


def test_round_trip_without_a_key(eoc):
    """PublicKey.encrypt_torus -> conv_device on an engine with no cloud key -> SecretKey.list_phases: every slot of both
    output channels, wrap slots included, within 6 sqrt(noise.linear_var) of the plain (negacyclic) correlation +
    noise.linear_offset of the slot's row"""
    from eoc_tfhe_amd import noise
    p = eoc.default_params(0)
    sk = eoc.SecretKey(p, 5, with_cloud_key=False)
    pk = eoc.PublicKey(sk.public_key_bytes())
    eng = eoc.Engine(p)
    rng = np.random.default_rng(2700)
    w = np.zeros((2, N), np.int8)
    w[:, :9] = rng.integers(-3, 4, (2, 9))
    x = rng.integers(-8, 9, N)
    delta = 1 << 20
    lists = pk.encrypt_torus(x * delta, 2701).reshape(1, 1, 2, N)
    got = run_conv(eng, w, lists)
    eng.close()
    phases = sk.list_phases(got[0]).astype(np.int64)                     # [2][N]
    off = noise.compact_offset(sk.tlwe_key, pk)
    cvar = noise.compact_var(p, sk.tlwe_key, pk)
    for r in range(2):
        rows = cv.shifted_rows(w[r], range(N))                           # [N][N]: the row of every slot
        plain = rows @ (x * delta)
        err = ((phases[r] - plain + 2**31) % 2**32 - 2**31) / 2.0**32 - rows.astype(np.float64) @ off
        for t in (0, N - 1):
            assert rows[t].astype(np.float64) @ off == pytest.approx(noise.linear_offset(p, sk, noise.conv_row(w[r], t)), abs=1e-15)
        sigma = np.sqrt(noise.linear_var(p, w[r], cvar))
        print(f"channel {r}: largest |error - offset| = {np.abs(err).max() / sigma:.2f} sigma over {N} slots")
        assert np.abs(err).max() <= 6 * sigma, (r, np.abs(err).max() / sigma)


def test_convolution_network_end_to_end(eoc):
    """Set A, tests/conv_case.py: 16 images 8 x 8 of +-1, a ConvLayer of 2 filters 3 x 3 with a sign activation on the 36 valid
    positions, one pack per (vector, channel), a DenseLayer of 2 rows with three +-1 weights each, sign.  All 16 x 2 outputs
    decrypt to evaluate_plain; the 72 words behind layer 0 equal the composed reference (conv reference, extraction,
    orc_keyswitch, the LUT oracle) on the first and the last vector."""
    import lut2_oracle as l2
    import lut_oracle as lo
    import test_gpu_pack as tp
    p, sk, blob, _, orc = l2.keys(eoc, 0)
    assert l2.KEY_SEED == ccase.KEY_SEED
    co.ksk(orc)
    eng = tp.keys(eoc, 0)[4]                                             # the same key seed: cloud key and packing key
    net, x, xin = ccase.conv_case()
    pk = eoc.PublicKey(sk.public_key_bytes())
    lists = np.stack([pk.encrypt_torus(v * ccase.DELTA_IN, 2800 + k) for k, v in enumerate(xin)])      # [16][1][2][N]
    before = eng.conv_launches()
    out, layers = net.run_device(eng, lists, return_layers=True)
    sync()
    assert eng.conv_launches() - before == 1
    want, pres = net.evaluate_plain(xin, return_pre=True)
    got = out.cpu().numpy()
    assert got.shape == (ccase.VECTORS, 2, p.n + 1)
    s = np.asarray(sk.lwe_key, np.int64)
    g64 = got.astype(np.int64)
    ph = ((g64[..., -1] - g64[..., :-1] @ s) + 2**31) % 2**32 - 2**31
    assert np.array_equal(np.where(ph >= 0, 1, -1) * ccase.MU2, want)
    assert np.abs(ph - want).max() / 2.0**32 < 0.05                      # a bootstrap output: sigma ~ 0.004
    # layer 0: signs of all 16 x 72 outputs, and the words of the first and the last vector
    l0 = layers[0].cpu().numpy()
    assert l0.shape == (ccase.VECTORS, 72, p.n + 1)
    g0 = l0.astype(np.int64)
    ph0 = ((g0[..., -1] - g0[..., :-1] @ s) + 2**31) % 2**32 - 2**31
    assert np.array_equal(np.where(ph0 >= 0, 1, -1), np.where(pres[0] + (1 << 20) >= 0, 1, -1))
    conv = net.layers[0]
    for b in (0, ccase.VECTORS - 1):
        u = cv.conv(conv.weights, lists[b:b + 1])[0]
        lin = co.expand(orc, u, conv.slot_table().astype(np.int64))
        assert l0[b].tobytes() == lo.lut_batch(orc, conv.tv[None], lin)[0].tobytes(), b
