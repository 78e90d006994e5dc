"""Two-input table lookups composed from the references that exist: the byte-for-byte reference of
eoc_tv_pack_device, eoc_lut_enc_batch_device and eoc_lut2_batch_device, and the fixed keys, seeds and inputs the CPU and GPU
tests share.

  level 1   lut_oracle.bootstrap (T = 1) / lut_many_oracle.bootstrap_many (T > 1) on x against the p public tables
  the pack  pack_oracle.pack_list on the N-row batch of repeated / negated samples (tv_batch): that batch IS the definition
            of eoc_tv_pack_device's output
  level 2   lut_oracle.bootstrap's composition with ACC = X^(2N - barb) (c0, c1): both polynomials of the list rotated

Test-side only."""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import lut_many_oracle as lmo
import lut_oracle as lo
import oracle_lib as ol
import pack_oracle as po

N = 1024
KEY_SEED = 1                       # the key of every shared case (tests/test_gpu_pack.py's engines use it too)
MIN_SIGMA = 6.0                    # decode assertions only at this margin or more on both levels (tests/test_gpu_int_circuit.py)


def _neg32(a):
    return (0 - np.asarray(a, np.int64)).astype(np.uint32).view(np.int32)


# -- the pack ----------------------------------------------------------------------------------------------------------------
def tv_slots(p):
    """(sample index, negated) of every coefficient of a test-polynomial list: eoc_lut_test_polynomial's rule"""
    k = np.arange(N)
    top = N - N // (2 * p)
    return np.where(k < top, (k * p + N // 2) // N, 0), k >= top


def tv_batch(vals, p):
    """the N-row batch [N][n+1] whose packing key switch is the list of `vals` [p][n+1]: sample j(k) in row k, the last
    N / (2p) rows sample 0 negated word by word"""
    vals = np.asarray(vals, np.int32)
    j, neg = tv_slots(p)
    rows = vals[j].copy()
    rows[neg] = _neg32(rows[neg])
    return np.ascontiguousarray(rows)


def tv_pack(n, kfft, vals, p, threads=16):
    """eoc_tv_pack_device: vals [n_funcs][p][count][n+1] -> lists [n_funcs][count][2][N]"""
    vals = np.asarray(vals, np.int32)
    F, _, S, _ = vals.shape
    with ThreadPoolExecutor(threads) as ex:
        out = list(ex.map(lambda fs: po.pack_list(n, kfft, tv_batch(vals[fs // S, :, fs % S], p)), range(F * S)))
    return np.stack(out).reshape(F, S, 2, N)


# -- level 2 -----------------------------------------------------------------------------------------------------------------
def bootstrap_enc(orc, lst, t):
    """KeySwitch(Extract(BlindRotate(t) from ACC = X^(-barb) (c0, c1))) on the oracle: lst [2][N], t [n+1] -> [n+1]"""
    L, p, n = orc.L, orc.p, orc.n
    bara, barb = np.zeros(n, np.int32), np.zeros(1, np.int32)
    L.orc_modswitch_sample(C.byref(p), np.ascontiguousarray(t, np.int32), bara, barb)
    rot = (2 * N - int(barb[0])) & (2 * N - 1)
    acc = np.zeros(2 * N, np.int32)
    acc[:N] = lo.rotate(lst[0], rot)
    acc[N:] = lo.rotate(lst[1], rot)
    step = orc.kpl * 2 * N
    base = orc.bkfft.ctypes.data
    for i in range(n):
        if bara[i]:
            L.orc_blind_rotate_step(C.byref(p), C.c_void_p(base + i * step * 8), None, int(bara[i]), acc, 1)
    u = np.zeros(N + 1, np.int32)
    u[0] = acc[0]
    u[1:N] = _neg32(acc[N - np.arange(1, N)])
    u[N] = acc[N]
    return orc.keyswitch(u)


def pool_map(fn, count, threads=16):
    with ThreadPoolExecutor(threads) as ex:                    # ctypes drops the GIL inside the oracle
        return list(ex.map(fn, range(count)))


def lut_enc_batch(orc, lists, cts, per_row):
    """eoc_lut_enc_batch_device: per_row False: lists [G][2][N] -> [G][count][n+1]; True: lists [G][count][2][N]"""
    cts = np.asarray(cts, np.int32).reshape(-1, orc.n + 1)
    S = cts.shape[0]
    lists = np.asarray(lists, np.int32).reshape((-1, S, 2, N) if per_row else (-1, 2, N))
    G = lists.shape[0]
    out = pool_map(lambda k: bootstrap_enc(orc, lists[k // S, k % S] if per_row else lists[k // S], cts[k % S]), G * S)
    return np.stack(out).reshape(G, S, orc.n + 1)


def lut_enc_rows(orc, lists, rows):
    """lut_enc_batch (per_row False) for thousands of rows of a SMALL n (tests/test_gpu_lut2_instances.py): the numpy parts
    for all rows at once, so that a thread's loop is ctypes calls only, as test_gpu_br_instances.oracle_lut does for public
    polynomials.  The first and last rows are checked against bootstrap_enc itself."""
    L, p, n = orc.L, orc.p, orc.n
    rows = np.asarray(rows, np.int32)
    lists = np.asarray(lists, np.int32).reshape(-1, 2, N)
    R, G = rows.shape[0], lists.shape[0]
    bar = lmo.modswitch_coarse(rows, 1)
    rot = (2 * N - bar[:, n].astype(np.int64)) & (2 * N - 1)
    idx = (np.arange(N)[None, :] - rot[:, None]) & (2 * N - 1)
    step = orc.kpl * 2 * N * 8
    base = orc.bkfft.ctypes.data
    out = np.zeros((G, R, n + 1), np.int32)

    def chunk(g, r0, r1):
        acc = np.zeros((r1 - r0, 2 * N), np.int32)
        for q in range(2):
            c = lists[g, q].astype(np.int64)
            acc[:, q * N:(q + 1) * N] = (np.concatenate([c, -c])[idx[r0:r1]] & 0xFFFFFFFF).astype(np.uint32).view(np.int32)
        for k, r in enumerate(range(r0, r1)):
            for i in range(n):
                if bar[r, i]:
                    L.orc_blind_rotate_step(C.byref(p), C.c_void_p(base + i * step), None, int(bar[r, i]), acc[k], 1)
        a = acc[:, :N].astype(np.int64)
        ext = np.concatenate([a, -a], axis=1)
        u = np.zeros((r1 - r0, N + 1), np.int32)
        u[:, :N] = (ext[:, (2 * N - np.arange(N)) & (2 * N - 1)] & 0xFFFFFFFF).astype(np.uint32).view(np.int32)
        u[:, N] = acc[:, N]
        for k in range(r1 - r0):
            out[g, r0 + k] = orc.keyswitch(u[k])

    cuts = np.linspace(0, R, 17).astype(int)
    with ThreadPoolExecutor(16) as ex:
        list(ex.map(lambda a: chunk(*a), [(g, cuts[k], cuts[k + 1]) for g in range(G) for k in range(16) if cuts[k] < cuts[k + 1]]))
    few = np.r_[0:2, R - 1]
    assert np.array_equal(out[:, few], lut_enc_batch(orc, lists, rows[few], False))
    return out


# -- the composed call -------------------------------------------------------------------------------------------------------
def lut2_tables(F, p, p_out=None):
    """Torus32 output values [p][p] of F: Z_p x Z_p -> Z_p_out in the integer encoding, table[x][y]"""
    p_out = p if p_out is None else p_out
    t = [[((int(F(x, y)) % p_out) << 32) // (2 * p_out) for y in range(p)] for x in range(p)]
    return np.array(t, np.uint64).astype(np.uint32).view(np.int32)


def level1(orc, p, T, tv0, x):
    """vals [n_funcs][p][count][n+1]: tv0 [n_funcs][p / T][N] on every row of x"""
    tv0 = np.asarray(tv0, np.int32).reshape(-1, p // T, N)
    x = np.asarray(x, np.int32).reshape(-1, orc.n + 1)
    F, S, G = tv0.shape[0], x.shape[0], p // T
    if T == 1:
        out = pool_map(lambda k: lo.bootstrap(orc, tv0[k // (G * S), (k // S) % G], x[k % S]), F * G * S)
        return np.stack(out).reshape(F, p, S, orc.n + 1)
    out = pool_map(lambda k: lmo.bootstrap_many(orc, tv0[k // (G * S), (k // S) % G], x[k % S], T), F * G * S)
    return np.stack(out).reshape(F, G, S, T, orc.n + 1).transpose(0, 1, 3, 2, 4).reshape(F, p, S, orc.n + 1)


def lut2_batch(orc, kfft, p, T, tv0, x, y, parts=False):
    """eoc_lut2_batch_device: [n_funcs][count][n+1]; parts: (vals, lists, out)"""
    vals = level1(orc, p, T, tv0, x)
    lists = tv_pack(orc.n, kfft, vals, p)
    out = lut_enc_batch(orc, lists, y, True)
    return (vals, lists, out) if parts else out


# -- shared keys, inputs and references ----------------------------------------------------------------------------------------
PROD_LO = lambda x, y: (x * y) % 4                   # noqa: E731  the digit product's low and high base-4 digits
PROD_HI = lambda x, y: (x * y) // 4                  # noqa: E731
# The noise measurements take the digit SUM instead: a blind rotation of a CONSTANT test polynomial adds no noise at all (the
# rotated difference (X^a - 1) ACC is zero in every step), and the product's column y = 0 is the zero polynomial, so a quarter
# of the product's rows would carry no level-1 noise (measured on the reference: 0.78 of predict()['total_var']).  Every
# column x -> x + y of the sum is a permutation, the generic case the model describes.
SUM_LO = lambda x, y: (x + y) % 4                    # noqa: E731
_CACHE = {}


def cached(key, compute):
    """computed once per process, shared by the tests that need it, never written to"""
    if key not in _CACHE:
        v = compute()
        for a in (v if isinstance(v, tuple) else (v.values() if isinstance(v, dict) else (v,))):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _CACHE[key] = v
    return _CACHE[key]


def keys(eoc, pset):
    """(params, secret key with the cloud key, packing-key blob, its reference spectra, oracle with the same keys)"""
    def make():
        p = eoc.default_params(pset)
        sk = eoc.SecretKey(p, KEY_SEED)
        blob = sk.packing_key_bytes()
        orc = ol.Oracle(pset, KEY_SEED)
        assert np.array_equal(sk.bk, orc.bk) and np.array_equal(sk.ksk, orc.ksk)
        return p, sk, blob, po.key_fft(po.blob_rows(blob, p.n)), orc
    return cached(("keys", pset), make)


def functions(p):
    """the two functions of every shared case: at p = 4 the digit product's low and high digit"""
    if p == 4:
        return [PROD_LO, PROD_HI]
    return [lambda x, y: (x * y + 1) % p, lambda x, y: max(x, y)]


def all_pairs(p, rows=None):
    """(x, y) values: every pair of Z_p x Z_p, or the first `rows` of a fixed shuffle of them"""
    xy = np.array([(x, y) for x in range(p) for y in range(p)], np.uint8)
    if rows is not None:
        xy = xy[np.random.default_rng(p).permutation(len(xy))[:rows]]
    return xy[:, 0].copy(), xy[:, 1].copy()


def shared_case(eoc, pset, p, T, rows=None):
    """dict of a shared case: inputs (fixed seeds), level-1 polynomials, and the reference's three stages"""
    def make():
        params, sk, _, kfft, orc = keys(eoc, pset)
        xv, yv = all_pairs(p, rows)
        x, y = sk.encrypt_ints(xv, p, 1400 + 10 * pset + p), sk.encrypt_ints(yv, p, 2400 + 10 * pset + p)
        fs = functions(p)
        tv0 = np.stack([eoc.lut2_test_polynomials(p, lut2_tables(f, p), T) for f in fs])
        vals, lists, out = lut2_batch(orc, kfft, p, T, tv0, x, y, parts=True)
        want = np.array([[f(int(a), int(b)) % p for a, b in zip(xv, yv)] for f in fs], np.uint8)
        return dict(p=p, T=T, xv=xv, yv=yv, x=x, y=y, tv0=tv0, vals=vals, lists=lists, out=out, want=want)
    return cached(("case", pset, p, T, rows), make)


def decodable(eoc, noise, pset, p, T):
    """the decode rule: both levels of the case at MIN_SIGMA or more by noise.lut2_margin_sigma (gate-output input variance)"""
    params, sk = keys(eoc, pset)[:2]
    return min(noise.lut2_margin_sigma(p, T, params, sk.lwe_key, sk.tlwe_key)) >= MIN_SIGMA
