"""The network of the end-to-end test of tests/test_gpu_dot.py, drawn on the CPU (tests/test_dot_cpu.py checks that the draw
terminates quickly): 32 inputs of +-1 at delta = 2^-8, a 32 -> 8 sign layer with weights in [-3, 3] whose outputs are +-1/36,
a pack, and an 8 -> 2 sign layer with weights +-1.  Weights are drawn until every row of layer 1 stays inside the range
(sum |w| < 64: Network.check raises otherwise); input vectors are drawn and kept only if Network.check puts every
pre-activation of both layers at least MIN_SIGMA predicted standard deviations from its decision boundary, until 64 are kept;
none is left out afterwards.  Test-side only."""
import numpy as np

from eoc_tfhe_amd import dinn

KEY_SEED = 1                                                    # tests/lut2_oracle.py's KEY_SEED: the Set A keys the GPU tests share
DELTA_IN = 1 << 24
MU1 = (1 << 32) // 36
MU2 = 1 << 29
MIN_SIGMA = 6.0
VECTORS = 64
BLOCK = 20000
MAX_DRAWS = 200000


def dinn_case(eoc, params, sk):
    """(network, x [64][32] of +-1, vectors drawn)"""
    rng = np.random.default_rng(20261)
    pk = eoc.PublicKey(sk.public_key_bytes())
    while True:
        net = dinn.Network([dinn.DenseLayer(rng.integers(-3, 4, (8, 32)), None, dinn.sign_test_polynomial(MU1)),
                            dinn.DenseLayer(rng.choice([-1, 1], (2, 8)), None, dinn.sign_test_polynomial(MU2))], DELTA_IN)
        try:
            net.check(params, sk.lwe_key, sk.tlwe_key)
            break
        except ValueError:
            continue
    kept, draws = [], 0
    while sum(len(k) for k in kept) < VECTORS:
        assert draws < MAX_DRAWS, "the draw does not terminate: the margins are too tight for these weights"
        x = rng.choice([-1, 1], (BLOCK, 32))
        draws += BLOCK
        sig = net.check(params, sk.lwe_key, sk.tlwe_key, x=x, pk=pk)["vector_sigma"]
        kept.append(x[sig >= MIN_SIGMA])
    return net, np.concatenate(kept)[:VECTORS], draws
