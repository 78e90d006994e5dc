"""Every k_cmux instance launch_leveled() (engine.hip) can dispatch, on the MI355X, with the edge inputs of
tests/leveled_edge_inputs.py: one test id per instance, named after the kernel.  <2,0> and <3,0> run nowhere else.

An instance runs on a real key at n = 16 (only the key switch behind a table read uses n) through the public calls:
  edge differences  eoc_cmux_device on every row of cmux_inputs -- cell ends of every digit position, all digits -Bg/2 and
                    Bg/2 - 1, single coefficients at the lane / register borders, the wrapping alternating pair -- under real
                    selectors of 0 and of 1, at counts 1, 2, 3, 33 and all (kCmuxItemsPerWG = 2: a lone item, a full
                    workgroup, a dead pair in the last one, a longer odd grid)
  full scale        a selector of one constant word (cmux_full_scale) through eoc_tgsw_to_fft_device, bit-identical to the
                    oracle's transform, on digits_min and digits_max: the top binade of the conversion contract
  table read        eoc_table_read_device at (d, log2 W) = (1, 0): one tree level and all ten rotations X^(2N - 2^i)
and is compared with the reference (tests/cmux_oracle.py) word for word.  Nothing is decrypted: exotic shapes are noisy, and
parity does not depend on the noise.  Every reference is computed under test_gpu_br_instances.reference: the oracle's
recorded maximum is below 2^51 (include/eoc_tfhe_gpu.h), so no input beyond the contract reaches the device.
Host side of the inputs: tests/test_leveled_edge_inputs_cpu.py."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import cmux_oracle as cx
import leveled_edge_inputs as lei
import oracle_lib as ol
from gpu_util import dev_empty, sync, to_dev, torch_cuda
from test_gpu_br_instances import custom_oracle, custom_params, reference

pytestmark = pytest.mark.gpu
N = 1024
N_LWE = 16
COUNTS = (1, 2, 3, 33)
READ_D, READ_LW = 1, 0


@pytest.fixture(scope="module")
def eoc(built_lib):
    torch_cuda()
    import eoc_tfhe_amd
    return eoc_tfhe_amd


def pool_map(fn, count, threads=16):
    with ThreadPoolExecutor(threads) as ex:                    # ctypes drops the GIL inside the references
        return list(ex.map(fn, range(count)))


def convert(eng, sel):
    """selectors [count][2l][2][N] int32 -> device tensor [count][2l][2][N] float64 (512 complex per polynomial)"""
    sel = np.ascontiguousarray(sel, np.int32)
    d_sel = to_dev(sel)
    d_fft = dev_empty(sel.shape, torch_cuda().float64)
    assert d_fft[0].numel() * 8 == eng.tgsw_fft_bytes
    eng.tgsw_to_fft_device(d_sel.data_ptr(), sel.shape[0], d_fft.data_ptr())
    sync()
    return d_fft


def cmux_device(eng, d_fft, in0, in1, count, fill=0x5A5A5A5A):
    """out [count][2][N] of the first `count` items; the output buffer holds one item more, which must keep its fill"""
    torch = torch_cuda()
    d0, d1 = to_dev(in0[:count]), to_dev(in1[:count])
    d_out = torch.full((count + 1, 2, N), fill, dtype=torch.int32, device="cuda")
    before = eng.stats()["cmux_launches"]
    eng.cmux_device(d_fft.data_ptr(), d0.data_ptr(), d1.data_ptr(), d_out.data_ptr(), count)
    sync()
    assert eng.stats()["cmux_launches"] - before == 1
    out = d_out.cpu().numpy()
    assert (out[count] == fill).all()
    return out[:count]


def differ(got, want):
    """(number of differing items, the first few (item, polynomial, coefficient))"""
    bad = np.argwhere(got != want)
    return len(np.unique(bad[:, 0])), bad[:6].tolist()


@pytest.mark.parametrize("name", list(lei.cmux_full_scale))
def test_instance_bit_exact_on_edge_inputs(eoc, name):
    cfg = lei.cmux_full_scale[name]
    l, Bgbit = cfg["l"], cfg["Bgbit"]
    p = custom_params(eoc, l, Bgbit, N_LWE)
    op = cx.orc_params(p)
    sk = eoc.SecretKey(p, 83)
    orc = custom_oracle(l, Bgbit, N_LWE, 83)
    assert np.array_equal(sk.ksk, orc.ksk) and np.array_equal(sk.tlwe_key, orc.tlwe_key)
    eng = eoc.Engine(p)
    eng.load_cloud_key(sk)

    # -- edge differences: item 2 s + b is sample s under the selector of bit b ---------------------------------------------
    ins = lei.cmux_inputs(l, Bgbit)
    names = [nm for nm, (a, _) in ins.items() for _ in range(a.shape[0])]
    in0 = np.repeat(np.concatenate([a for a, _ in ins.values()]), 2, axis=0)
    in1 = np.repeat(np.concatenate([b for _, b in ins.values()]), 2, axis=0)
    items = in0.shape[0]
    assert items > max(COUNTS) and items % 2 == 0
    sel = sk.encrypt_selector_bits([0, 1], enc_seed=5)
    fft = cx.to_fft(sel)
    d_two = convert(eng, sel)
    assert np.array_equal(d_two.cpu().numpy(), fft * 2.0**-9)
    d_fft = d_two[torch_cuda().arange(items, device="cuda") % 2].contiguous()
    want = reference(("cmux", name, "edges"),
                     lambda: np.stack(pool_map(lambda k: cx.cmux(op, fft[k % 2], in0[k], in1[k]), items)))
    for count in COUNTS + (items,):
        got = cmux_device(eng, d_fft, in0, in1, count)
        n_bad, first = differ(got, want[:count])
        assert n_bad == 0, (name, count, n_bad, [names[i // 2] for i, _, _ in first], first)
        if count == items:
            zero = [k for k in range(items) if names[k // 2] == "zero"]
            assert len(zero) == 2 and np.array_equal(got[zero], in0[zero])

    # -- full scale: the contract's top binade --------------------------------------------------------------------------------
    ksel = lei.constant_selector(l, cfg["K"])[None]
    kfft = cx.to_fft(ksel)
    d_k = convert(eng, ksel)
    assert np.array_equal(d_k.cpu().numpy(), kfft * 2.0**-9)
    f0 = np.concatenate([ins["digits_min"][0], ins["digits_max"][0]])
    f1 = np.concatenate([ins["digits_min"][1], ins["digits_max"][1]])

    def full_scale():
        L = ol.lib()
        out = np.stack([cx.cmux(op, kfft[0], f0[k], f1[k]) for k in range(2)])
        mx = L.orc_dbg_max_conv(0)                              # reference() reset it and asserts the contract behind this
        assert cfg["lo"] <= mx < cfg["hi"], (name, np.log2(mx))
        return out
    want = reference(("cmux", name, "full scale"), full_scale)
    got = cmux_device(eng, d_k.expand(2, -1, -1, -1).contiguous(), f0, f1, 2)
    n_bad, first = differ(got, want)
    assert n_bad == 0, (name, "full scale", n_bad, first)

    # -- table read: one tree level, then the rot path at every amount 2N - 2^i ---------------------------------------------
    torch = torch_cuda()
    rng = np.random.default_rng(900 + 10 * l + Bgbit)
    depth = READ_D + 10 - READ_LW
    table = eoc.trivial_table(rng.integers(-2**31, 2**31, N << READ_D))
    assert table.shape == (1 << READ_D, 2, N)
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
    want = reference(("cmux", name, "read"), lambda: cx.table_read(orc, op, table, READ_D, READ_LW, rfft)[0])
    got = d_out.cpu().numpy()
    assert got.shape == want.shape
    assert np.array_equal(got, want), (name, "table read", np.argwhere((got != want).any(axis=-1)).tolist())
