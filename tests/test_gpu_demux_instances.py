"""Every k_demux instance launch_leveled() (engine.hip) can dispatch, on the MI355X, with the edge words of
tests/leveled_edge_inputs.py taken as x itself (the demultiplexer decomposes the sample, not a difference): one test id per
instance, named after the kernel.

An instance runs on a real key at n = 16 (no key is used by the call) through eoc_demux_device:
  edge words    every row of cmux_differences -- cell ends of every digit position, all digits -Bg/2 and Bg/2 - 1, single
                coefficients at the lane / register borders, the alternating words -- under real selectors of 0 and of 1, at
                counts 1, 2, 3, 33 and all (two items per workgroup: a lone item, a full workgroup, a dead pair in the last
                one, a longer odd grid); both outputs word for word, the word behind each output untouched
  accumulate    the same items added into a random pre-filled destination
  full scale    a selector of one constant word (cmux_full_scale) on digits_min and digits_max: the top binade of the
                conversion contract, which on the demultiplexer is a condition on its inputs as it is on the CMux's
against the reference (tests/table_update_oracle.py).  Every reference is computed under test_gpu_br_instances.reference:
the oracle's recorded maximum is reset first and asserted below 2^51 before anything is sent to the device."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import cmux_oracle as cx
import leveled_edge_inputs as lei
import oracle_lib as ol
import table_update_oracle as tu
from gpu_util import dev_empty, sync, to_dev, torch_cuda
from test_gpu_br_instances import custom_params, reference

pytestmark = pytest.mark.gpu
N = 1024
N_LWE = 16
COUNTS = (1, 2, 3, 33)
FILL0, FILL1 = 0x5A5A5A5A, 0x3C3C3C3C
INSTANCES = {name.replace("k_cmux", "k_demux"): cfg for name, cfg in lei.cmux_full_scale.items()}


@pytest.fixture(scope="module")
def eoc(built_lib):
    torch_cuda()
    import eoc_tfhe_amd
    return eoc_tfhe_amd


def pool_map(fn, count, threads=16):
    with ThreadPoolExecutor(threads) as ex:                    # ctypes drops the GIL inside the references
        return list(ex.map(fn, range(count)))


def convert(eng, sel):
    sel = np.ascontiguousarray(sel, np.int32)
    d_sel = to_dev(sel)
    d_fft = dev_empty(sel.shape, torch_cuda().float64)
    eng.tgsw_to_fft_device(d_sel.data_ptr(), sel.shape[0], d_fft.data_ptr())
    sync()
    return d_fft


def demux_device(eng, d_fft, x, count, base=None):
    """(out0, out1) [count][2][N] of the first `count` items.  Store mode (base None): the buffers hold one item more, which
    must keep its fill.  Accumulate mode: base = (b0, b1) pre-fills, and the item behind must keep its pre-fill."""
    torch = torch_cuda()
    d_x = to_dev(x[:count])
    if base is None:
        d0 = torch.full((count + 1, 2, N), FILL0, dtype=torch.int32, device="cuda")
        d1 = torch.full((count + 1, 2, N), FILL1, dtype=torch.int32, device="cuda")
    else:
        d0, d1 = to_dev(base[0][:count + 1]), to_dev(base[1][:count + 1])
    before = eng.stats()
    eng.demux_device(d_fft.data_ptr(), d_x.data_ptr(), d0.data_ptr(), d1.data_ptr(), count, accumulate=base is not None)
    sync()
    after = eng.stats()
    assert after["demux_launches"] - before["demux_launches"] == 1 and after["cmux_launches"] == before["cmux_launches"]
    o0, o1 = d0.cpu().numpy(), d1.cpu().numpy()
    if base is None:
        assert (o0[count] == FILL0).all() and (o1[count] == FILL1).all()
    else:
        assert np.array_equal(o0[count], base[0][count]) and np.array_equal(o1[count], base[1][count])
    return o0[:count], o1[:count]


def differ(got, want):
    bad = np.argwhere(got != want)
    return len(np.unique(bad[:, 0])), bad[:6].tolist()


@pytest.mark.parametrize("name", list(INSTANCES))
def test_instance_bit_exact_on_edge_inputs(eoc, name):
    cfg = INSTANCES[name]
    l, Bgbit = cfg["l"], cfg["Bgbit"]
    p = custom_params(eoc, l, Bgbit, N_LWE)
    op = cx.orc_params(p)
    sk = eoc.SecretKey(p, 83, with_cloud_key=False)
    eng = eoc.Engine(p)                                         # no key is loaded: the call needs none

    # -- edge words: item 2 s + b is sample s under the selector of bit b ---------------------------------------------------
    diffs = lei.cmux_differences(l, Bgbit)
    names = [nm for nm, a in diffs.items() for _ in range(a.shape[0])]
    x = np.repeat(np.concatenate([a.view(np.int32) for a in diffs.values()]), 2, axis=0)
    items = x.shape[0]
    assert items > max(COUNTS) and items % 2 == 0
    sel = sk.encrypt_selector_bits([0, 1], enc_seed=5)
    fft = cx.to_fft(sel)
    d_two = convert(eng, sel)
    assert np.array_equal(d_two.cpu().numpy(), fft * 2.0**-9)
    d_fft = d_two[torch_cuda().arange(items, device="cuda") % 2].contiguous()
    want = reference(("demux", name, "edges"),
                     lambda: np.stack(pool_map(lambda k: np.stack(tu.demux(op, fft[k % 2], x[k])), items)))
    rng = np.random.default_rng(950 + 10 * l + Bgbit)
    base = rng.integers(-2**31, 2**31, (2, items + 1, 2, N)).astype(np.int32)
    for count in COUNTS + (items,):
        g0, g1 = demux_device(eng, d_fft, x, count)
        for c, got in enumerate((g0, g1)):
            n_bad, first = differ(got, want[:count, c])
            assert n_bad == 0, (name, "store", count, c, n_bad, [names[i // 2] for i, _, _ in first], first)
        assert np.array_equal((g0.astype(np.int64) + g1 - x[:count]) % 2**32, np.zeros_like(g0, np.int64))
        a0, a1 = demux_device(eng, d_fft, x, count, base=(base[0], base[1]))
        for c, got in enumerate((a0, a1)):
            acc = tu.wrap_i32(base[c, :count].astype(np.int64) + want[:count, c])
            n_bad, first = differ(got, acc)
            assert n_bad == 0, (name, "accumulate", count, c, n_bad, first)

    # -- full scale: the contract's top binade --------------------------------------------------------------------------------
    ksel = lei.constant_selector(l, cfg["K"])[None]
    kfft = cx.to_fft(ksel)
    d_k = convert(eng, ksel)
    assert np.array_equal(d_k.cpu().numpy(), kfft * 2.0**-9)
    fx = np.concatenate([diffs["digits_min"], diffs["digits_max"]]).view(np.int32)

    def full_scale():
        L = ol.lib()
        out = np.stack([np.stack(tu.demux(op, kfft[0], fx[k])) for k in range(2)])
        mx = L.orc_dbg_max_conv(0)                              # reference() reset it and asserts the contract behind this
        assert cfg["lo"] <= mx < cfg["hi"], (name, np.log2(mx))
        return out
    want = reference(("demux", name, "full scale"), full_scale)
    g0, g1 = demux_device(eng, d_k.expand(2, -1, -1, -1).contiguous(), fx, 2)
    eng.close()
    for c, got in enumerate((g0, g1)):
        n_bad, first = differ(got, want[:, c])
        assert n_bad == 0, (name, "full scale", c, n_bad, first)
