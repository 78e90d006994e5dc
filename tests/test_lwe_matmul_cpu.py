"""Dense layers on LWE samples, host side (include/eoc_tfhe_lwe.h): the new header as C and its five symbols, the
image size rule, both limb rules in numpy against the reference on the edge words, and the pricing of the hidden="lwe" route on
the network of tests/dinn_case.py.  The kernel's registers: tests/test_lwe_matmul_ledger_cpu.py; the device: tests/
test_gpu_lwe_matmul.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import dinn_case as dc
import lwe_matmul_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("eoc_lwe_weights_image_bytes", "eoc_lwe_weights_to_device", "eoc_lwe_matmul_device", "eoc_engine_lwe_matmul_launches",
           "eoc_lwe_matmul")


@pytest.fixture(scope="module")
def eoc(built_lib):
    import eoc_tfhe_amd
    return eoc_tfhe_amd


def test_header_compiles_as_c_and_the_symbols_are_exported(eoc, tmp_path):
    src = tmp_path / "use.c"
    # typed pointers: a declaration that differs from the documented signature does not compile (the flags of the build's
    # own C compile of the Lua binding)
    src.write_text("""#include "eoc_tfhe_lwe.h"
size_t (*p0)(size_t, size_t) = eoc_lwe_weights_image_bytes;
int (*p1)(eoc_engine *, const int8_t *, size_t, size_t, void *, void *) = eoc_lwe_weights_to_device;
int (*p2)(eoc_engine *, const void *, size_t, size_t, const int32_t *, size_t, size_t, const int32_t *, int32_t *, void *) =
    eoc_lwe_matmul_device;
uint64_t (*p3)(eoc_engine *) = eoc_engine_lwe_matmul_launches;
int (*p4)(const int8_t *, size_t, size_t, const int32_t *, size_t, size_t, const int32_t *, int32_t *) = eoc_lwe_matmul;
""")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-c", "-I" + os.path.join(ROOT, "include"), str(src), "-o",
                           str(tmp_path / "use.o")])
    L = eoc.lib()
    assert all(hasattr(L, s) for s in SYMBOLS)
    assert all(hasattr(eoc.Engine, m) for m in ("lwe_weights_image_bytes", "lwe_weights_to_device", "lwe_matmul_device",
                                                "lwe_matmul_launches")) and callable(eoc.lwe_matmul)
    # the Lua registry stays as it is: no binding of this unit
    import test_binding_surfaces as tb
    assert len(tb.lua_registered()) == 34 and not [n for n in tb.lua_registered() | tb.node_exported() if "lwe" in n.lower()]


def test_null_engine_and_null_buffers_answer_without_a_device(eoc):
    L = eoc.lib()
    buf = np.zeros(64, np.int32)
    p = buf.ctypes.data
    assert L.eoc_lwe_weights_to_device(None, p, 1, 1, p, None) == -1 and b"null" in L.eoc_last_error()
    assert L.eoc_lwe_matmul_device(None, p, 1, 1, p, 1, 1, None, p, None) == -1 and b"null" in L.eoc_last_error()
    assert L.eoc_engine_lwe_matmul_launches(None) == 0
    for args in ((None, 1, 1, p, 1, 1, None, p), (p, 1, 1, None, 1, 1, None, p), (p, 1, 1, p, 1, 1, None, None)):
        assert L.eoc_lwe_matmul(*args) == -1 and b"eoc_lwe_matmul: null" in L.eoc_last_error()


@pytest.mark.parametrize("rows,cols", [(0, 1), (1, 0), (2**20 + 1, 1), (1, 2**16 + 1), (0, 0), (2**40, 2**40)])
def test_image_bytes_is_zero_for_a_refused_shape(eoc, rows, cols):
    assert eoc.lib().eoc_lwe_weights_image_bytes(rows, cols) == 0 == ref.image_bytes(rows, cols)


@pytest.mark.parametrize("rows,cols", [(1, 1), (32, 32), (33, 31), (31, 33), (64, 96), (5, 1000), (1, 2**16), (2**20, 1),
                                       (2**20, 2**16)])
def test_image_bytes_is_the_documented_size(eoc, rows, cols):
    assert eoc.lib().eoc_lwe_weights_image_bytes(rows, cols) == ref.image_bytes(rows, cols) > 0


@pytest.mark.parametrize("rule", [ref.limbs_carry, ref.limbs_carry_free])
def test_limb_rules_recombine_to_the_reference(rule):
    """every edge word alone, under every edge weight; the shapes of the GPU test on mixed words; and the accumulator extremes
    at the largest K"""
    limbs, const = rule(ref.EDGE_WORDS)
    back = (sum(l << (8 * j) for j, l in enumerate(limbs)) + const) & ref.MASK
    assert np.array_equal(back.astype(np.uint32).view(np.int32), ref.EDGE_WORDS)
    w = ref.EDGE_WEIGHTS.reshape(-1, 1)
    for word in ref.EDGE_WORDS:
        cts = np.full((1, 1, 3), word, np.int32)
        assert np.array_equal(ref.lwe_matmul_by_limbs(w, cts, rule), ref.lwe_matmul(w, cts)), hex(int(word) & ref.MASK)
    rng = np.random.default_rng(2500)
    for rows, cols, width, batch in ((33, 31, 51, 2), (5, 1000, 41, 2)):
        w, cts = ref.weights(rng, rows, cols), ref.words(rng, (batch, cols, width))
        assert np.array_equal(ref.lwe_matmul_by_limbs(w, cts, rule), ref.lwe_matmul(w, cts))
    for weight, word in ((-127, 0x80808080), (127, 0x7F7F7F7F), (127, 0x80808080), (-127, 0x7F7F7F7F)):
        w = np.full((1, 2**16), weight, np.int8)
        cts = np.full((1, 2**16, 1), word, np.int64).astype(np.uint32).view(np.int32)
        assert np.array_equal(ref.lwe_matmul_by_limbs(w, cts, rule), ref.lwe_matmul(w, cts))


def test_reference_adds_the_bias_on_the_body_word_only():
    rng = np.random.default_rng(2501)
    w, cts = ref.weights(rng, 3, 4), ref.words(rng, (2, 4, 5))
    bias = np.array([-2**31, 2**31 - 1, 7], np.int32)
    d = ref.lwe_matmul(w, cts, bias).astype(np.int64) - ref.lwe_matmul(w, cts).astype(np.int64)
    assert not d[..., :-1].any() and np.array_equal(d[..., -1] & ref.MASK, np.broadcast_to(bias.astype(np.int64) & ref.MASK, (2, 3)))


@pytest.fixture(scope="module")
def case(eoc):
    p = eoc.default_params(0)
    sk = eoc.SecretKey(p, dc.KEY_SEED, with_cloud_key=False)
    net, x, _ = dc.dinn_case(eoc, p, sk)
    return p, sk, net, x


def test_lwe_linear_var_is_the_weights_norm_times_the_input_variance(eoc):
    from eoc_tfhe_amd import noise
    assert noise.lwe_linear_var([3, -4, 0], 2.0) == 50.0 and noise.lwe_linear_var(np.zeros(5), 1.0) == 0.0


def test_lwe_route_is_priced_no_worse_and_keeps_every_vector(eoc, case):
    """hidden="lwe" gives every hidden row a sigma no larger than hidden="pack"; all 64 vectors of the case keep MIN_SIGMA under
    the "lwe" pricing -- on lists in front of layer 0 (run_device(hidden="lwe")) and on fresh samples (run_device_samples):
    the condition for the GPU end-to-end tests to leave no vector out"""
    from eoc_tfhe_amd import noise
    p, sk, net, x = case
    pk = eoc.PublicKey(sk.public_key_bytes())
    pack = net.layer_sigma(p, sk.lwe_key, sk.tlwe_key, pk)
    lwe = net.layer_sigma(p, sk.lwe_key, sk.tlwe_key, pk, hidden="lwe")
    assert np.array_equal(pack[0][0], lwe[0][0]) and np.array_equal(pack[0][1], lwe[0][1])     # layer 0 reads the same lists
    assert (lwe[1][0] <= pack[1][0]).all() and (lwe[1][0] < pack[1][0]).any()
    pr = noise.predict(p, sk.lwe_key, sk.tlwe_key)
    w = net.layers[1].weights.astype(np.float64)
    want = np.sqrt((w * w).sum(1) * pr["total_var"] + noise.modswitch_var(sk.lwe_key))          # no pack_var, no ks_var
    assert np.allclose(lwe[1][0], want, rtol=1e-12) and np.allclose(lwe[1][1], np.abs(w.sum(1) * pr["total_mean"]), rtol=1e-12)
    # the defaults are today's behaviour
    assert all(np.array_equal(a, b) for s, t in zip(pack, net.layer_sigma(p, sk.lwe_key, sk.tlwe_key, pk, hidden="pack"))
               for a, b in zip(s, t))
    assert len(x) == dc.VECTORS
    lists_route = net.check(p, sk.lwe_key, sk.tlwe_key, x=x, pk=pk, hidden="lwe")["vector_sigma"]
    assert lists_route.shape == (dc.VECTORS,) and lists_route.min() >= dc.MIN_SIGMA, lists_route.min()
    fresh = float(p.ks_stdev) ** 2
    samples_route = net.check(p, sk.lwe_key, sk.tlwe_key, x=x, hidden="lwe", input_var=fresh)["vector_sigma"]
    assert samples_route.min() >= dc.MIN_SIGMA, samples_route.min()
    s0 = net.layer_sigma(p, sk.lwe_key, sk.tlwe_key, hidden="lwe", input_var=fresh)[0]
    w0 = net.layers[0].weights.astype(np.float64)
    assert np.allclose(s0[0], np.sqrt((w0 * w0).sum(1) * fresh + noise.modswitch_var(sk.lwe_key)), rtol=1e-12) and not s0[1].any()
    with pytest.raises(ValueError):
        net.layer_sigma(p, sk.lwe_key, sk.tlwe_key, hidden="lists")


def test_run_device_samples_refuses_a_conv_network(eoc):
    from eoc_tfhe_amd import dinn
    conv = dinn.ConvLayer(dinn.conv2d_weights(np.ones((1, 1, 2, 2), np.int8), 4), dinn.conv_slots(4, 4, 2, 2), None,
                          dinn.sign_test_polynomial(1 << 29))
    net = dinn.Network([conv], 1 << 24)
    with pytest.raises(ValueError, match="DenseLayer-only"):
        net.run_device_samples(None, np.zeros((1, 1024, 501), np.int32))
    # a link behind a ConvLayer keeps the pack under hidden="lwe"
    dense = dinn.DenseLayer(np.ones((2, 1024), np.int8), None, dinn.sign_test_polynomial(1 << 29))
    net2 = dinn.Network([conv, dense], 1 << 24)
    assert not net2._lwe_link(1, "lwe") and not net2._lwe_link(0, "lwe")
