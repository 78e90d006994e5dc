"""The network of the end-to-end test of tests/test_gpu_conv.py, drawn on the CPU (tests/test_conv_cpu.py prices it): 8 x 8
images of +-1 at DELTA_IN, one channel; a ConvLayer of 2 filters 3 x 3 with taps +-1 and a sign activation of value MU1 on the
36 valid positions; a pack per (vector, channel); a DenseLayer of 2 rows, each with exactly three +-1 weights on distinct
filled slots, sign activation MU2.  Odd tap counts make every pre-activation an odd multiple of its step (DELTA_IN, MU1), so no
vector sits on a decision boundary and none is rejected: the 16 vectors are the first 16 drawn.

The two constants.  Ranges: 9 DELTA_IN = 0.2109 and 3 MU1 = 0.2250, both below 1/4.  Margins: the smallest |pre-activation|
is one step, DELTA_IN = 0.0234 in front of layer 0 (sigma 2.93e-3: 9 taps on fresh lists + key switch + mod switch) and MU1 =
0.075 in front of layer 1 (sigma 7.82e-3: three bootstrap outputs behind a pack + key switch + mod switch); less the boundary's
place at -1/4N and the predicted |mean|, Network.check prices them at 7.92 and 9.53 sigma under the Set A key of seed 1, and
every one of the 16 vectors at 7.92 (tests/test_conv_cpu.py prints them and asserts >= 6).  Test-side only."""
import numpy as np

from eoc_tfhe_amd import dinn

KEY_SEED = 1                                                    # tests/lut2_oracle.py's KEY_SEED: the Set A keys the GPU tests share
HEIGHT = WIDTH = 8
KH = KW = 3
DELTA_IN = 3 << 25                                              # 3 * 2^-7
MU1 = 322122547                                                 # 0.075 * 2^32, rounded
MU2 = 1 << 29
MIN_SIGMA = 6.0
VECTORS = 16


def conv_case():
    """(network, x [16][1][64] of +-1, the same padded to [16][N] for evaluate_plain / encrypt_torus)"""
    rng = np.random.default_rng(20262)
    taps = rng.choice([-1, 1], (2, 1, KH, KW))
    slots = dinn.conv_slots(HEIGHT, WIDTH, KH, KW)
    conv = dinn.ConvLayer(dinn.conv2d_weights(taps, WIDTH), slots, None, dinn.sign_test_polynomial(MU1))
    w2 = np.zeros((2, 2 * slots.size), np.int64)
    for r in range(2):
        w2[r, rng.choice(2 * slots.size, 3, replace=False)] = rng.choice([-1, 1], 3)
    dense = dinn.DenseLayer(dinn.pad_dense_weights(w2, 2, slots.size), None, dinn.sign_test_polynomial(MU2))
    net = dinn.Network([conv, dense], DELTA_IN)
    x = rng.choice([-1, 1], (VECTORS, 1, HEIGHT * WIDTH))
    return net, x, conv.pad_input(x)
