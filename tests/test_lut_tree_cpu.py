"""Multi-digit table lookups, host side (no GPU): the exact pack's reference (tests/tv_pack_exact_oracle.py)
against the exact integer evaluation of the existing rule, the operand order of k_pks_limbs / k_tvpack_mm / k_tv_spread
restated in numpy, the level-1 test polynomials and their refusals, and the composed reference's output noise against
noise.lut_tree_var / lut_tree_mean.  GPU side: tests/test_gpu_tvpack_mm.py, tests/test_gpu_lut_tree.py; registers:
tests/test_isa_lut_tree.py."""
import numpy as np
import pytest

import lut2_oracle as l2
import lut_tree_oracle as lt
import pack_oracle as po
import tv_pack_exact_oracle as tpe
from eoc_tfhe_amd import noise
from test_ks_limbs_cpu import limbs_of

N = 1024
EOC_OK, EOC_ERR_ARG = 0, -1
EDGE = np.array([-2**31, 2**31 - 1, 0, -1, 0x7FFF, 0x8000, -0x8000, -0x8001], np.int64)
ALLOWED_T = [(p, T) for p in (2, 4, 8) for T in (1, 2, 4, 8) if p % T == 0 and (T == 1 or p * T <= 16)]
ALLOWED = [(p, d, T) for p, T in ALLOWED_T for d in (2, 3, 4) if p ** (d - 1) <= 64]


@pytest.fixture(scope="module")
def eoc(built_lib):
    import eoc_tfhe_amd
    return eoc_tfhe_amd


def edge_case(n, p, seed):
    """random key rows [n][4][2][N] and values [p][n+1], with INT32_MIN and the other edge words in both"""
    rng = np.random.default_rng(seed)
    rows = rng.integers(-2**31, 2**31, (n, 4, 2, N))
    rows[:, :, :, ::97] = -2**31
    rows[:, :, :, 5::101] = 2**31 - 1
    vals = rng.integers(-2**31, 2**31, (p, n + 1))
    vals[0, :] = EDGE[np.arange(n + 1) % len(EDGE)]                         # the sample that is also negated
    vals[p - 1, :] = EDGE[(np.arange(n + 1) + 3) % len(EDGE)]
    return rows.astype(np.int32), vals.astype(np.int32)


@pytest.mark.parametrize("n", [1, 7, 17])
@pytest.mark.parametrize("p", [2, 4, 8])
def test_reference_equals_the_exact_evaluation_of_the_existing_rule(p, n):
    rows, vals = edge_case(n, p, 100 * n + p)
    want = po.pack_list_exact(n, rows, l2.tv_batch(vals, p), 0, po.n_chunks(n))
    got = tpe.tv_pack_exact(n, rows, vals[None, :, None, :], p)[0, 0]
    assert np.array_equal(got, want), np.argwhere(got != want)[:4]


def test_windows_tile_the_ring_as_tv_batch_does():
    for p in (2, 4, 8):
        j, neg = l2.tv_slots(p)
        cover = np.full(N, -1)
        for s, (lo, hi) in enumerate(tpe.windows(p)):
            assert (cover[lo:hi] == -1).all()
            cover[lo:hi] = s
        assert np.array_equal(cover, np.where(neg, p, j))


# -- the kernels' operand order, restated ------------------------------------------------------------------------------------
def digit_dword(a):
    """tvp_digit_dword: the four digits of a mask word as four signed bytes, digit j in byte 4 - j"""
    a = np.asarray(a, np.int64) & 0xFFFFFFFF
    t = ((a + 0x88888000) & 0xFFFFFFFF) >> 16
    u = (t | (t << 8)) & 0x00FF00FF
    u = ((u | (u << 4)) & 0x0F0F0F0F) ^ 0x08080808
    return (u | ((u & 0x08080808) * 0x1E)) & 0xFFFFFFFF


def test_digit_dword_holds_the_signed_digits():
    words = np.concatenate([EDGE, np.arange(-70000, 70000, 7), np.random.default_rng(2).integers(-2**31, 2**31, 100000)])
    dw = digit_dword(words)
    d = po.digits(words)                                                    # [4][...], digit j at index j - 1
    for j in range(1, 5):
        byte = ((dw >> (8 * (4 - j))) & 0xFF).astype(np.uint8).view(np.int8)
        assert np.array_equal(byte, d[j - 1]), j


def limb_image(rows, n):
    """k_pks_limbs: int8 [ksteps][64 column tiles][4 limbs][64 lanes][16 bytes]"""
    ksteps = (n + 7) // 8
    img = np.zeros((ksteps, 64, 4, 64, 16), np.int8)
    planes = limbs_of(np.asarray(rows, np.int32))                           # 4 x [n][4][2][N]
    for lane in range(64):
        h, r = lane >> 5, lane & 31
        for q in range(4):
            for jj in range(4):
                m = 8 * np.arange(ksteps) + 4 * h + q
                ok = m < n
                for limb in range(4):
                    cols = planes[limb][np.minimum(m, n - 1), 4 - jj - 1].reshape(ksteps, 2 * N)[:, r::32]  # [ksteps][64 tiles]
                    img[:, :, limb, lane, 4 * q + jj] = np.where(ok[:, None], cols, 0)
    return img


@pytest.mark.parametrize("n", [1, 7, 8, 9, 17])
def test_kernel_operand_order_gives_the_constant_slot_samples(n):
    """k_tvpack_mm lane by lane: A bytes from digit_dword of mask words m = 8 step + 4 h + q, B bytes from the limb image, the
    instruction pairing equal (h, byte) slots of row r and column r; C recombined in wrapping 32 bits and negated"""
    p = 4
    rows, vals = edge_case(n, p, 7 + n)
    u = tpe.samples(vals[None])[0]                                          # [p + 1][n+1]
    img = limb_image(rows, n).astype(np.int64)
    ksteps = img.shape[0]
    M = u.shape[0]
    a = np.zeros((M, ksteps, 2, 16), np.int64)                              # [row][step][h][byte]
    for h in range(2):
        for q in range(4):
            m = 8 * np.arange(ksteps) + 4 * h + q
            dw = np.where(m < n, digit_dword(u[:, np.minimum(m, n - 1)]), 0)   # [M][ksteps]
            for jj in range(4):
                a[:, :, h, 4 * q + jj] = ((dw >> (8 * jj)) & 0xFF).astype(np.uint8).view(np.int8)
    b = img.reshape(ksteps, 64, 4, 2, 32, 16)                               # [step][tile][limb][h][r][byte]
    acc = np.einsum("mshb,stlhrb->mltr", a, b)                              # [M][limb][tile][r]
    assert np.abs(acc).max() < 1 << 22
    S = -sum(acc[:, limb] << (8 * limb) for limb in range(4)).reshape(M, 2 * N)
    S[:, N] += u[:, n]                                                       # k_tv_spread adds b_s at X^0
    got = (S & 0xFFFFFFFF).astype(np.uint32).view(np.int32).reshape(M, 2, N)
    assert np.array_equal(got, tpe.const_slot(n, rows, u))


def test_spread_by_prefix_sums_is_the_negacyclic_window_product():
    """k_tv_spread's E(t) rule against schoolbook negacyclic products with the 0/1 window polynomials"""
    rng = np.random.default_rng(9)
    for p in (2, 4, 8):
        S = rng.integers(-2**31, 2**31, (p + 1, 2, N))
        S[0, 0, :4] = EDGE[:4]
        want = np.zeros((2, N), np.int64)
        for s, (lo, hi) in enumerate(tpe.windows(p)):
            win = np.zeros(N, np.int64)
            win[lo:hi] = 1
            for c in range(2):
                full = np.convolve(win, S[s, c])
                want[c] += full[:N]
                want[c, :N - 1] -= full[N:]
        want = (want & 0xFFFFFFFF).astype(np.uint32).view(np.int32)
        assert np.array_equal(tpe.spread(S.astype(np.int32), p), want)


# -- level-1 polynomials and refusals -------------------------------------------------------------------------------------------
def test_allowed_shapes():
    assert len(ALLOWED) == 19 and (8, 3, 2) in ALLOWED and (4, 4, 4) in ALLOWED and (8, 4, 1) not in ALLOWED


@pytest.mark.parametrize("p,d,T", ALLOWED)
def test_level1_polynomials_equal_the_twin(eoc, p, d, T):
    table = np.random.default_rng(100 * p + 10 * d + T).integers(-2**31, 2**31, (p,) * d).astype(np.int32)
    tv = eoc.lut_tree_test_polynomials(p, d, table, T)
    assert tv.shape == (p ** (d - 1) // T, N) and tv.dtype == np.int32
    assert np.array_equal(tv, lt.test_polynomials(eoc, p, d, table, T))
    if d == 2:
        assert np.array_equal(tv, eoc.lut2_test_polynomials(p, table, T))
    assert np.array_equal(eoc.lut_tree_test_polynomials(p, d, table, 0), eoc.lut_tree_test_polynomials(p, d, table, 1))


def test_table_order_j2_fastest(eoc):
    """p = 2, d = 3: polynomial J = j_2 + 2 j_3 is the lookup x_1 -> table[x_1][j_2][j_3]"""
    table = (np.arange(8, dtype=np.int64) << 28).astype(np.int32).reshape(2, 2, 2)
    tv = eoc.lut_tree_test_polynomials(2, 3, table)
    for j2 in range(2):
        for j3 in range(2):
            assert np.array_equal(tv[j2 + 2 * j3], eoc.lut_test_polynomial(2, table[:, j2, j3]))


def test_refusals(eoc):
    L = eoc.lib()
    tab, tv = np.zeros(8**4, np.int32), np.zeros(64 * N, np.int32)
    t, v = tab.ctypes.data, tv.ctypes.data
    bad = [(p, 2, 1) for p in (0, 1, 3, 16)] + [(4, 1, 1), (4, 5, 1), (4, 0, 1), (8, 4, 1), (2, 3, 4), (4, 3, 8), (8, 3, 4), (4, 3, 3), (4, 3, -1)]
    for p, d, T in bad:
        assert L.eoc_lut_tree_test_polynomials(p, d, T, t, v) == EOC_ERR_ARG, (p, d, T)
    assert L.eoc_lut_tree_test_polynomials(4, 3, 1, None, v) == EOC_ERR_ARG
    assert L.eoc_lut_tree_test_polynomials(4, 3, 1, t, None) == EOC_ERR_ARG
    for p, d, T in ALLOWED:
        assert L.eoc_lut_tree_test_polynomials(p, d, T, t, v) == EOC_OK, (p, d, T)
    with pytest.raises(eoc.EocError):
        eoc.lut_tree_test_polynomials(4, 3, np.zeros((4, 4), np.int32))
    with pytest.raises(eoc.EocError):
        eoc.lut_tree_test_polynomials(8, 4, np.zeros(8**4, np.int32))
    # the engine entry points check their arguments before they need a device
    a = np.zeros((4, 501), np.int32).ctypes.data
    assert L.eoc_lut_tree_batch_device(None, 4, 3, 1, a, 1, a, a, 4, None) == EOC_ERR_ARG
    assert L.eoc_tv_pack_exact_device(None, 4, a, 1, 4, a, None) == EOC_ERR_ARG


# -- noise --------------------------------------------------------------------------------------------------------------------------
def test_model_composition(eoc):
    params = eoc.default_params(0)
    sk = eoc.SecretKey(params, l2.KEY_SEED, with_cloud_key=False)
    args = (params, sk.lwe_key, sk.tlwe_key)
    pr = noise.predict(*args)
    assert noise.lut_tree_var(*args, 2) == pytest.approx(noise.lut2_var(*args))
    assert noise.lut_tree_mean(*args, 2) == pytest.approx(noise.lut2_mean(*args))
    step = noise.pack_var(params, sk.lwe_key, N) + noise.br_enc_var(*args) + pr["ks_var"]
    for d in (3, 4):
        assert noise.lut_tree_var(*args, d) == pytest.approx(pr["total_var"] + (d - 1) * step)
        m = noise.lut_tree_margin_sigma(4, d, 2, *args)
        assert len(m) == d and m[0] == pytest.approx(noise.lut2_margin_sigma(4, 2, *args)[0])
        assert all(x == pytest.approx(noise.lut2_margin_sigma(4, 2, *args)[1]) for x in m[1:])


def _errors(sk, out, want, p):
    ph = (np.asarray(out, np.int64)[:, -1] - np.asarray(out, np.int64)[:, :-1] @ sk.lwe_key.astype(np.int64))
    msg = (want.astype(np.int64) << 32) // (2 * p)
    return ((((ph - msg) + 2**31) % 2**32) - 2**31) / 2.0**32


def test_reference_noise_matches_lut_tree_var(eoc):
    """S = 128 reference rows, Set A, p = 2, d = 3, T = 1, random digits: the output error's variance within
    1 +- 3.5 sqrt(2 / (S - 1)) of noise.lut_tree_var and its mean within 4 standard errors of noise.lut_tree_mean (the bound rule
    of tests/test_lut2_cpu.py); every row decodes.  F is the parity: every level-1 column is a permutation
    (lut2_oracle.SUM_LO says why that matters)."""
    S, p, d = 128, 2, 3
    params, sk, blob, _, orc = l2.keys(eoc, 0)
    rng = np.random.default_rng(77)
    xs = rng.integers(0, p, (d, S)).astype(np.uint8)
    digits = np.stack([sk.encrypt_ints(xs[k], p, 5100 + k) for k in range(d)])
    F = lambda a, b, c: a ^ b ^ c                                            # noqa: E731
    tv0 = eoc.lut_tree_test_polynomials(p, d, lt.torus_table(F, p, d))[None]
    out = lt.lut_tree_batch(orc, po.blob_rows(blob, params.n), p, d, 1, tv0, digits)[0]
    want = (xs[0] ^ xs[1] ^ xs[2]).astype(np.uint8)
    assert np.array_equal(sk.decrypt_ints(out, p), want)
    err = _errors(sk, out, want, p)
    var_pred = noise.lut_tree_var(params, sk.lwe_key, sk.tlwe_key, d, sk.ksk)
    mean_pred = noise.lut_tree_mean(params, sk.lwe_key, sk.tlwe_key, d, sk.ksk)
    ratio = err.var(ddof=1) / var_pred
    z = (err.mean() - mean_pred) / (err.std(ddof=1) / np.sqrt(S))
    print(f"sigma {err.std():.4e} predicted {np.sqrt(var_pred):.4e} variance ratio {ratio:.4f}; mean {err.mean():.3e} predicted "
          f"{mean_pred:.3e} ({z:+.2f} se)")
    assert abs(ratio - 1) <= 3.5 * np.sqrt(2.0 / (S - 1)), ratio
    assert abs(z) <= 4, z
