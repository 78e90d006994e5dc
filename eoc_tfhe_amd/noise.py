"""Predicted output noise of one gate bootstrap, for a GIVEN key (pure numpy; no GPU, no oracle).

This is the quantitative anchor of the parity statement: upstream libtfhe is absent from the
reference tree, so what ties this path to TFHE as published is (a) bit-exact agreement with the CPU restatement and
(b) agreement of the measured output noise -- mean AND variance, before and after the key switch -- with what the
CGGI analysis predicts for the conventions of SURVEY.md Appendix A.  A wrong gadget offset, a rounding instead of
upstream's truncating decomposition, a wrong key-switch precision offset or a mis-scaled key row moves one of the four
numbers below by tens of per cent while every gate still decrypts.

All quantities are in torus units (int32 / 2^32).  N = 1024, k = 1.

Blind rotation (tfhe_blindRotateAndExtract_FFT), error of the extracted sample under the
extracted key, over many input ciphertexts and ONE key:

  V_BR = n_eff * 2l * N * E[d^2] * sigma_eff^2           (the TLWE-zero rows of BK_i, every step; E[d^2] = (Bg^2 + 2)/12:
                                                          digits uniform on [-Bg/2, Bg/2), mean -1/2.  As `predict` computes
                                                          it: sigma_eff^2 = sigma_bk^2 - sigma_bk sqrt(2/pi) 2^-32 + 2^-64/3
                                                          -- gaussian32 truncates toward zero -- and n_eff = (n - 1 + f0)
                                                          (1 - 1/2N): step 0 works on the trivial accumulator and counts as
                                                          the fraction f0 of a regular step; a step whose amount is 0 adds
                                                          nothing)
       + w_eff * (1 + |s'|) * q^2 / 12                    (w_eff = w - s_0, w = Hamming weight of the LWE key: step 0's
                                                          remainder is exactly zero; |s'| = weight of the TLWE key; the
                                                          decomposition's remainder, q = Bg^-l)
       + (w_eff - 1) * (q/2)^2 * G(s')                    (the remainder is a TRUNCATION: upstream's offset
                                                          sum_p (Bg/2) 2^(32 - p Bgbit) centres the digits, not the
                                                          remainder, which is uniform on [0, q) with mean q/2; the LAST
                                                          active step contributes the constant M_BR below, not variance)

The third term is what CGGI's worst-case bound hides and the average-case textbook formula omits.  At a step with
s_i = 1 the update adds  -(low_b - low_a * s')  to the accumulator, low_x[j] in [0, q).  Its mean is the polynomial
-(q/2) J*(1 - s'), J = 1 + X + ... + X^(N-1); later steps multiply it by X^rho with rho uniform on [0, 2N) (the
remaining rotation), so coefficient 0 of the result picks +-((q/2) (J*(1 - s'))[r]) for a uniform r:
G(s') = mean_r ((J*(1-s'))[r])^2, about N^2/12 -- N/2 times the variance term next to it.  For the LAST step with
s_i = 1 nothing rotates any more (rho = 0): a deterministic bias

  M_BR = -(q/2) * (1 + |s'| - 2 s'_0).

(At 262 144 samples a third, input-dependent mean term resolves: step 0 multiplies constant band digits by the FIXED noise
of its rows -- about 50 (q/2), zero over uniform rotations.  tools/noise_mean_diag.py simulates
it from the key and matches the measured means per input class; `predict` keeps the input-independent M_BR.)

Key switch (lweKeySwitch; A.6), added error for ONE key whose rows have noises e[i][j][d]
(d = 1..base-1; d = 0 is "no row", e = 0), digits uniform:

  V_KS = sum_{i,j} ( mean_d e^2 - (mean_d e)^2 )  +  |s'| * 2^(-2 (t basebit + 1)) / 3
  M_KS = - sum_{i,j} mean_d e[i][j][d]            (res = (0, b') - sum of rows: the phase loses msg + e per row)

The textbook average over keys, kN t (1 - 1/base) sigma_ks^2, is ~ 4/3 of V_KS for a fixed key: a quarter of the
rows' second moment is the per-key constant M_KS, not spread.

How much of this is fitted: the three refinements (sigma_eff, n_eff / f0, w_eff) were added in round 5 while looking at
twelve 262 144-sample cases -- keys 1, 2, 3, 4, 5, 9 on both parameter sets (profiles/r05_noise_262144.txt) -- so the
0.9986 +- 0.0029 agreement on THOSE keys is partly tuned (each refinement is derived, none has a free parameter, but which
ones to derive was chosen by looking).  Key 77 was never looked at while the model was written: it is the asserted
HOLD-OUT of tests/test_gpu_noise.py and tests/test_noise_cpu.py.  Measured once the model was frozen, at 262 144
samples (profiles/r06_noise_holdout_262144.txt, keys 77 and 78, both sets): V_BR ratios 0.9999, 1.0011, 0.9951, 1.0013, V_KS
ratios 1.0006, 0.9972, 0.9990, 0.9960 (standard error 0.0028), all predicted means within 1.5 standard errors.
"""
import numpy as np

N = 1024


def _wrap32(x):
    return ((np.asarray(x, np.int64) + 2**31) % 2**32) - 2**31


def ksk_noise(ksk, lwe_key, tlwe_key, ks_t, ks_basebit):
    """e[i*t + j][d-1]: noise of key-switch row (i, j, d) in torus units (phase minus message)."""
    base = 1 << ks_basebit
    ksk = np.asarray(ksk, np.int64).reshape(N * ks_t * (base - 1), -1)
    s = np.asarray(lwe_key, np.int64)
    s1 = np.asarray(tlwe_key, np.int64)
    ph = _wrap32(ksk[:, -1] - ksk[:, :-1] @ s)
    r = np.arange(ksk.shape[0])
    d = r % (base - 1) + 1
    j = (r // (base - 1)) % ks_t
    i = r // ((base - 1) * ks_t)
    msg = _wrap32(s1[i] * (d << (32 - (j + 1) * ks_basebit)))
    return (_wrap32(ph - msg) / 2.0**32).reshape(N * ks_t, base - 1)


def predict(params, lwe_key, tlwe_key, ksk=None):
    """dict of predicted means / variances (torus units) for this key; `ksk` = [N t (base-1)][n+1] torus rows
    (None: the key-switch part uses the average-key textbook formula and a zero mean)."""
    n, l, Bgbit = int(params.n), int(params.l), int(params.Bgbit)
    t, bb = int(params.ks_t), int(params.ks_basebit)
    Bg, base = 1 << Bgbit, 1 << bb
    s = np.asarray(lwe_key, np.int64)
    s1 = np.asarray(tlwe_key, np.int64)
    w, hw = int(s.sum()), int(s1.sum())
    q = 2.0 ** (-l * Bgbit)
    # J * (1 - s') in Z[X]/(X^N + 1): coefficient r = sum_{m <= r} v_m - sum_{m > r} v_m
    v = -s1.astype(np.float64)
    v[0] += 1.0
    pre = np.cumsum(v)
    Jv = 2.0 * pre - pre[-1]
    out = {}
    # (a) gaussian32 converts sigma * z to Torus32 by TRUNCATION toward zero (dtot32 = int32(int64(frac * 2^32)),
    #     upstream's conversion): the stored noise is sign(x) floor(|x|), variance sigma^2 - sigma sqrt(2/pi) u + u^2/3 with
    #     u = 2^-32 -- 2.6 % below sigma^2 for Set A's sigma_bk (30.8 units), 0.6 % for Set B's (128 units); measured on the
    #     keys' rows: 0.9736 / 0.9924
    u = 2.0**-32
    sig = float(params.bk_stdev)
    sig2 = sig * sig - sig * np.sqrt(2.0 / np.pi) * u + u * u / 3.0
    # (b) STEP 0 sees the trivial accumulator (0, X^-b testvector): its mask polynomial decomposes to all-zero digits and its
    #     body to ~N/2 digits of 2 mu / h_1, so that step adds about (N/2) (2 mu / h_1)^2 / (2l N E[d^2]) of a regular step's
    #     row noise (9 % for Set A), and its remainder is exactly zero (no truncation term from it when s_0 = 1).  From step 1
    #     on the accumulator's mask is the pseudo-random sum of key-row masks -- a regular step whether s_0 was 0 or 1
    Ed2 = (Bg * Bg + 2) / 12.0
    d_triv = (1 << 30) >> (32 - Bgbit) if Bgbit <= 30 else 0          # first digit of +-2 mu = 2^30
    triv_frac = min(1.0, 0.5 * d_triv * d_triv / (2 * l * Ed2))
    n_eff = (n - (1.0 - triv_frac)) * (1.0 - 1.0 / (2 * N))          # step 0 only: after it the accumulator's MASK is
    w_eff = max(w - int(s[0]), 0)                                     # pseudo-random whatever s_0 is, and every later step regular
    out["br_var_rows"] = n_eff * 2 * l * N * Ed2 * sig2
    out["br_var_remainder"] = w_eff * (1 + hw) * q * q / 12.0
    # the LAST active step is rotated by nothing: its term is the constant M_BR (the mean below), not variance
    out["br_var_truncation_bias"] = max(w_eff - 1, 0) * (q / 2) ** 2 * float((Jv**2).mean())
    out["br_var"] = out["br_var_rows"] + out["br_var_remainder"] + out["br_var_truncation_bias"]
    out["br_mean"] = -(q / 2) * float(Jv[0])
    out["br_var_textbook"] = (n * 2 * l * N * (Bg * Bg / 12.0) * float(params.bk_stdev) ** 2
                              + n * (1 + N / 2) * q * q / 12.0)        # the average-case formula WITHOUT the truncation term
    ks_round = hw * 2.0 ** (-2 * (t * bb + 1)) / 3.0
    out["ks_var_textbook"] = N * t * (1 - 1.0 / base) * float(params.ks_stdev) ** 2 + ks_round
    if ksk is not None:
        e = ksk_noise(ksk, s, s1, t, bb)
        m1 = e.sum(1) / base
        m2 = (e**2).sum(1) / base
        out["ks_var"] = float((m2 - m1**2).sum()) + ks_round
        # res = (0, b') - sum of rows: phase(res) = b' - sum (msg + e) = phase(u) + rounding - sum e
        out["ks_mean"] = -float(m1.sum())
    else:
        out["ks_var"] = out["ks_var_textbook"]
        out["ks_mean"] = 0.0
    out["total_var"] = out["br_var"] + out["ks_var"]
    out["total_mean"] = out["br_mean"] + out["ks_mean"]
    return out


def rotation_amounts(t_rows):
    """modSwitchFromTorus32(., 2N) of every word of the LWE samples `t_rows` [count][n+1]: the blind
    rotation's abar_0..abar_{n-1} and barb (last column)."""
    t = np.asarray(t_rows, np.int64) & 0xFFFFFFFF
    return ((t + (1 << 20)) >> 21) & (2 * N - 1)


def br_conditional_mean(params, lwe_key, tlwe_key, t_rows):
    """What the truncating decomposition adds to EACH sample, given only public data and the key: sum over the steps with
    s_i = 1 (step 0 excepted: its accumulator is the trivial one, its remainder exactly zero) of coefficient 0 of
    X^rho_i * M, M = -(q/2) J*(1 - s'), rho_i = sum of the LATER active steps' rotation amounts (mod 2N).  [count] torus units.

    The measured error of a sample regresses on this with slope 1 and correlation sqrt(V_truncation / V_BR) (0.58 for
    Set A): a sample-by-sample check of the order in which the steps' rotations accumulate and of the remainder's sign
    and size -- which the variance alone does not see (steps taken in the opposite order give slope 0, a remainder of the
    other sign slope -1; the rotation's DIRECTION is not resolved: M is antisymmetric about N/2 to leading order)."""
    n, l, Bgbit = int(params.n), int(params.l), int(params.Bgbit)
    s = np.asarray(lwe_key, np.int64)
    s1 = np.asarray(tlwe_key, np.int64)
    q = 2.0 ** (-l * Bgbit)
    v = -s1.astype(np.float64)
    v[0] += 1.0
    pre = np.cumsum(v)
    M = -(q / 2) * (2.0 * pre - pre[-1])
    act = np.flatnonzero(s)
    A = rotation_amounts(t_rows)[:, :n][:, act]
    rc = np.cumsum(A[:, ::-1], axis=1)[:, ::-1]
    rho = (rc - A) % (2 * N)
    # (X^rho M)[0]: rho = 0 -> M[0]; 0 < rho < N -> -M[N - rho]; rho = N -> -M[0]; N < rho < 2N -> +M[2N - rho]
    idx = np.where(rho % N == 0, 0, np.where(rho < N, N - rho, 2 * N - rho))
    sgn = np.where(rho == 0, 1.0, np.where(rho <= N, -1.0, 1.0))
    contrib = sgn * M[idx]
    if len(act) and act[0] == 0:
        contrib[:, :1] = 0.0          # step 0 works on the trivial accumulator: its remainder is exactly zero
    return contrib.sum(1)


def br_early_term(params, lwe_key, tlwe_key, bk, t_rows, mu=1 << 29, chunk=16384):
    """STEP 0 sees the trivial accumulator (0, X^-barb testvector): the digits of (X^abar_0 - 1) ACC are the CONSTANT
    +-2 mu / h_1 on a band (first digit of the body polynomial only), so that step adds  (2 mu / h_1) * sum_band +-e_0  with the
    FIXED noise e_0 of row (q = 1, p = 1) of BK_0, rotated by the active steps behind it.  Deterministic given the key and the
    public rotation amounts; zero over uniform rotations, of the order of 50 (q/2) over NAND's three phase classes
    (DESIGN.md 2.3).  (After step 0 the accumulator's mask is a pseudo-random sum of key-row masks whether s_0 is 0 or 1:
    every later step is a regular one.)  `bk` = the torus rows [n][2l][2][N] (SecretKey.bk).  [count] torus units."""
    n, l, Bgbit = int(params.n), int(params.l), int(params.Bgbit)
    s = np.asarray(lwe_key, np.int64)
    s1 = np.asarray(tlwe_key, np.int64)
    bk = np.asarray(bk).reshape(n, 2 * l, 2, N)
    ones = np.flatnonzero(s)
    bara = rotation_amounts(t_rows)
    out = np.zeros(bara.shape[0])
    if not len(ones):
        return out
    i0 = 0          # step 0 only
    dig = float((2 * mu) >> (32 - Bgbit))
    S = np.zeros((N, N))                                   # a @ S = a * s' in Z[X]/(X^N + 1)
    for m_ in range(N):
        col = np.roll(s1.astype(np.float64), m_)
        col[:m_] *= -1
        S[m_, :] = col
    ext = []
    for i in range(i0 + 1):
        a_, b_ = bk[i, l, 0].astype(np.float64), bk[i, l, 1].astype(np.int64)   # row (q = 1, p = 1)
        ph = b_ - np.rint(a_ @ S).astype(np.int64)
        if s[i]:
            ph[0] -= 1 << (32 - Bgbit)                      # the row's message: s_i h_1 on the body's constant coefficient
        ei = _wrap32(ph) / 2.0**32
        ext.append(np.concatenate(([ei[0]], -ei[:0:-1], [-ei[0]], ei[:0:-1])))   # (X^k e_i)[0], k in [0, 2N)
    jj = np.arange(N)[None, :]
    act_after = [ones[ones > i] for i in range(i0 + 1)]
    for lo in range(0, bara.shape[0], chunk):
        B = bara[lo:lo + chunk]
        bb = B[:, n][:, None]

        def sign_of(j):                                     # coefficient j of X^(2N - barb) testvector, 2N-periodic extension
            return np.where(((j - (2 * N - bb)) % (2 * N)) < N, 1, -1)
        for i in range(i0 + 1):
            ab = B[:, i][:, None]
            k = (sign_of(jj - ab) - sign_of(jj)) // 2
            rho = (B[:, act_after[i]].sum(1) % (2 * N))[:, None]
            out[lo:lo + chunk] += dig * (k * ext[i][(jj + rho) % (2 * N)]).sum(1)
    return out


def regress(e_br, cond_mean, pred=None):
    """slope / correlation of the measured blind-rotation error on its per-sample conditional mean (+ the correlation the
    prediction implies and the slope's standard error)"""
    x = cond_mean - cond_mean.mean()
    y = e_br - e_br.mean()
    r = float((x * y).sum() / np.sqrt((x * x).sum() * (y * y).sum()))
    out = {"br_cm_slope": float((x * y).sum() / (x * x).sum()), "br_cm_corr": r,
           "br_cm_slope_se": float(np.sqrt(max(1.0 - r * r, 0.0) / max(r * r, 1e-30) / len(x)))}
    if pred is not None:
        out["br_cm_corr_pred"] = float(np.sqrt(pred["br_var_truncation_bias"] / pred["br_var"]))
    return out


def residual_mean(e_br, cond_mean, early=None):
    """mean of what the per-sample model leaves of the blind rotation's error (measured - conditional mean - early term), and
    its z: the sharpest mean test there is -- the model removes a third of the variance and all of the known bias"""
    res = e_br - cond_mean - (0.0 if early is None else early)
    return {"br_resid_mean": float(res.mean()), "br_resid_z": float(res.mean() / (res.std() / np.sqrt(len(res)))),
            "br_model_mean": float((cond_mean + (0.0 if early is None else early)).mean())}


def measure(u, out, lwe_key, tlwe_key):
    """errors of blind-rotation outputs `u` [count][N+1] under the extracted key and of the key-switched
    samples `out` [count][n+1] under the LWE key, against the nearest of +-1/8.  Returns (e_br, e_ks, e_total) in
    torus units; e_ks = e_total - e_br is the key switch's own contribution, sample by sample."""
    s = np.asarray(lwe_key, np.int64)
    s1 = np.asarray(tlwe_key, np.int64)
    u = np.asarray(u, np.int64).reshape(-1, N + 1)
    out = np.asarray(out, np.int64).reshape(u.shape[0], -1)
    phu = _wrap32(u[:, N] - u[:, :N] @ s1)
    pho = _wrap32(out[:, -1] - out[:, :-1] @ s)
    sign = np.where(phu > 0, 1, -1)
    e_br = (phu - sign * 2**29) / 2.0**32
    e_tot = (pho - sign * 2**29) / 2.0**32
    return e_br, e_tot - e_br, e_tot


def compare(pred, e_br, e_ks, e_tot):
    """measured / predicted summary (what the tests assert on and bench.py prints)"""
    cnt = len(e_br)
    return {
        "count": int(cnt),
        "br_var": float(e_br.var()), "br_var_pred": pred["br_var"], "br_ratio": float(e_br.var() / pred["br_var"]),
        "br_ratio_textbook": float(e_br.var() / pred["br_var_textbook"]),
        "br_mean": float(e_br.mean()), "br_mean_pred": pred["br_mean"],
        "br_mean_z": float((e_br.mean() - pred["br_mean"]) / (e_br.std() / np.sqrt(cnt))),
        "ks_var": float(e_ks.var()), "ks_var_pred": pred["ks_var"], "ks_ratio": float(e_ks.var() / pred["ks_var"]),
        "ks_ratio_textbook": float(e_ks.var() / pred["ks_var_textbook"]),
        "ks_mean": float(e_ks.mean()), "ks_mean_pred": pred["ks_mean"],
        "ks_mean_z": float((e_ks.mean() - pred["ks_mean"]) / (e_ks.std() / np.sqrt(cnt))),
        "total_std": float(e_tot.std()), "total_std_pred": float(np.sqrt(pred["total_var"])),
        "max_abs_err": float(np.abs(e_tot).max()),
    }


def modswitch_var(lwe_key, n_tables=1):
    """variance (torus units) of the mod switch to 2N of a sample under `lwe_key`, every amount rounded to the grid of
    T = n_tables (many-LUT bootstrapping): b and the |s| active a_i each carry a rounding error uniform
    over a step of T / (2N), (1 + |s|) T^2 / (48 N^2) in all -- T = 1 is the gate bootstrap's mod switch"""
    w = int(np.asarray(lwe_key, np.int64).sum())
    return (1 + w) * float(n_tables) ** 2 / (48.0 * N * N)


def lut_margin_sigma(params, lwe_key, tlwe_key, p, n_tables=1, inputs=1):
    """decision margin of a table lookup at message space p, in predicted standard deviations at the
    blind rotation's input: 1/(4p) over sqrt(inputs x V_out + V_ms(T)).  The input is the sum of `inputs` bootstrap outputs
    (each of variance predict()['total_var'], average-key key switch), mod-switched on the grid of T = n_tables.  The
    OUTPUT noise of a many-LUT lookup is the gate bootstrap's: the grid only widens the rounding at the input."""
    v_out = predict(params, lwe_key, tlwe_key)["total_var"]
    return (1.0 / (4 * int(p))) / float(np.sqrt(inputs * v_out + modswitch_var(lwe_key, n_tables)))


def lut_margin_sigma_var(p, n_tables, input_var, lwe_key):
    """the general form of lut_margin_sigma (integer circuits): 1/(4p) over sqrt(input_var + V_ms(T)), where
    input_var is the variance (torus units) of the sample in front of the mod switch -- sum_k w_k^2 V(in_k) behind a linear
    stage with weights w.  lut_margin_sigma(params, ..., p, T, inputs=k) = lut_margin_sigma_var(p, T, k V_out, lwe_key)."""
    return (1.0 / (4 * int(p))) / float(np.sqrt(float(input_var) + modswitch_var(lwe_key, n_tables)))


def _sig2(params):
    """variance of one gaussian32 draw at bk_stdev, truncation toward zero included (as `predict` computes it)"""
    u = 2.0**-32
    sig = float(params.bk_stdev)
    return sig * sig - sig * np.sqrt(2.0 / np.pi) * u + u * u / 3.0


def pk_noise(pk, tlwe_key):
    """e = B - A s' of a compact public key (PublicKey / its EOCPK1 blob, or an (A, B) pair), [N] torus units"""
    if isinstance(pk, (bytes, bytearray)):
        w = np.frombuffer(bytes(pk), np.int32)
        A, B = w[-2 * N:-N], w[-N:]
    elif hasattr(pk, "A"):
        A, B = pk.A, pk.B
    else:
        A, B = pk
    A = np.asarray(A, np.int64)
    s1 = np.asarray(tlwe_key, np.int64)
    # (A s')[j] = sum_m s'_m (X^m A)[j], (X^m A)[j] = A[j - m] (j >= m), -A[j - m + N] (j < m)
    As = np.zeros(N, np.int64)
    for m in np.flatnonzero(s1):
        As += np.concatenate((-A[N - m:], A[:N - m]))
    return _wrap32(np.asarray(B, np.int64) - As) / 2.0**32


def compact_offset(tlwe_key, pk):
    """mean error of slot j of a compact list under this public key, [N] torus units: u e with binary u of mean 1/2 gives
    (1/2) (J e)[j], J = 1 + X + ... + X^(N-1), i.e. (1/2) (sum_{m <= j} e_m - sum_{m > j} e_m).  The lists' own e1, e2
    have mean 0."""
    e = pk_noise(pk, tlwe_key)
    pre = np.cumsum(e)
    return 0.5 * (2.0 * pre - pre[-1])


def compact_var(params, tlwe_key, pk=None):
    """variance (torus units) of the error of one extracted compact-list sample under s', around its slot's mean
    (compact_offset), over the lists' randomness.  Error of slot j: (u e)[j] + e2[j] - (e1 s')[j].
      u e     binary u (variance 1/4 per coefficient): ||e||^2 / 4 -- from the key's own e when `pk` is given, N sigma^2 / 4
              (its expectation) otherwise
      e2      sigma^2
      e1 s'   |s'| sigma^2
    sigma^2 is the truncation-corrected variance of gaussian32 at bk_stdev, as in `predict`.  The key switch adds
    predict(...)['ks_var'] and ['ks_mean'] on top: the two sums are independent."""
    s1 = np.asarray(tlwe_key, np.int64)
    sig2 = _sig2(params)
    ue = float((pk_noise(pk, tlwe_key) ** 2).sum()) / 4.0 if pk is not None else N * sig2 / 4.0
    return ue + sig2 + float(s1.sum()) * sig2


# ---- leveled operations: CMux and encrypted-index table reads ------------------------------------------------
def _Jv(tlwe_key):
    """J * (1 - s') in Z[X]/(X^N + 1), J = 1 + X + ... + X^(N-1), as `predict` forms it: about 1 + |s'| - 2 (ones of s' up to j)"""
    v = -np.asarray(tlwe_key, np.int64).astype(np.float64)
    v[0] += 1.0
    pre = np.cumsum(v)
    return 2.0 * pre - pre[-1]


def cmux_var(params, tlwe_key, bit=1):
    """variance (torus units) one CMux  out = A + C (x) (B - A)  adds to every coefficient of the phase, for a fixed key, over
    the selector's randomness and pseudo-random full-range inputs -- the two per-step terms of `predict`:
      rows       2l N E[d^2] sigma_eff^2: the 2l TLWE-zero rows of the selector times the digits (E[d^2] = (Bg^2 + 2) / 12,
                 sigma_eff^2 the truncation-corrected variance of gaussian32 at bk_stdev)
      remainder  (1 + |s'|) q^2 / 12, q = Bg^-l: what the decomposition drops, low_b - low_a s' -- only where the bit is 1
                 (a selector of 0 multiplies it by nothing)
    This is the spread around the CMux's mean.  The mean is not zero where the bit is 1: see cmux_mean.
    The rounding mode of the leveled calls has the same variance, which is why this function takes no
    `rounding`: the mode adds a constant to the decomposed word, so the dropped part is uniform on an interval of the same
    length q, [-q/2, q/2) instead of [0, q), and the digits run over the same Bg values; only the mean moves."""
    l, Bgbit = int(params.l), int(params.Bgbit)
    Bg = 1 << Bgbit
    q = 2.0 ** (-l * Bgbit)
    hw = int(np.asarray(tlwe_key, np.int64).sum())
    return 2 * l * N * ((Bg * Bg + 2) / 12.0) * _sig2(params) + (1 if bit else 0) * (1 + hw) * q * q / 12.0


def _dropped_mean(params, rounding=False):
    """mean (torus units) of the part of a pseudo-random word that the gadget drops: q/2 when it truncates (uniform on
    [0, q)); -2^-33, half an LSB of Torus32, in the rounding mode (uniform on the integers of [-q/2, q/2)), which
    changes nothing where l Bgbit = 32"""
    lb = int(params.l) * int(params.Bgbit)
    return -(2.0 ** -33) if rounding and lb < 32 else 2.0 ** (-lb) / 2


def cmux_mean(params, tlwe_key, slot=0, bit=1, rounding=False):
    """mean error (torus units) of coefficient `slot` behind one CMux whose bit is 1: the decomposition TRUNCATES, the dropped
    parts low_x[j] are uniform on [0, q) with mean q/2, and the output loses low_b - low_a s': -(q/2) (J (1 - s'))[slot], the
    polynomial whose coefficient 0 is the blind rotation's M_BR (`predict`).  About -(q/2) (1 + |s'|) at slot 0, falling
    linearly to +(q/2) (|s'| - 1) at slot N - 1.  `slot` may be an array.  Zero where the bit is 0.
    rounding=True: the leveled calls' rounding mode (eoc_engine_set_leveled_rounding), whose dropped parts are uniform on
    [-q/2, q/2) with mean -1/2 LSB: the residual is 2^-33 (J (1 - s'))[slot], the same polynomial 2^(32 - l Bgbit) times
    smaller and of the other sign."""
    return -_dropped_mean(params, rounding) * _Jv(tlwe_key)[np.asarray(slot)] * (1 if bit else 0)


def table_read_var(params, lwe_key, tlwe_key, depth, table_var=0.0, ksk=None):
    """variance (torus units) of a table-read output (eoc_table_read_device) around its mean: table_var (0 for a trivial
    table, compact_var for a public-key-encrypted one) + depth x cmux_var + the key switch's (`predict`; `ksk` as there)"""
    return float(table_var) + int(depth) * cmux_var(params, tlwe_key) + predict(params, lwe_key, tlwe_key, ksk)["ks_var"]


def table_read_slots(index, log2_lists, log2_width):
    """the slot offsets at which the CMuxes of a read with index bit 1 leave their mean, for output slot 0: a tree level does
    not move slots, rotation i (bit i set) moves slot W 2^i to 0.  Returns the list of slots, seen from output slot 0."""
    d, r, W = int(log2_lists), 10 - int(log2_width), 1 << int(log2_width)
    idx = int(index)
    rot_bits = [i for i in range(r) if (idx >> i) & 1]
    s = W * (idx & ((1 << r) - 1))
    out = [s] * sum((idx >> (r + v)) & 1 for v in range(d))     # tree levels act on the slot the entry starts at
    for k, i in enumerate(rot_bits):                             # behind rotation i the entry starts at the sum of the later ones
        out.append(sum(W << j for j in rot_bits[k + 1:]))
    return out


def table_read_mean(params, tlwe_key, index, log2_lists, log2_width, w=0, rounding=False):
    """mean error (torus units) of slot w of the read of entry `index`, before the key switch's own mean: the sum of cmux_mean
    over the CMuxes whose bit is 1, each at the slot the entry occupied behind it.  Up to depth x (q/2) (1 + |s'|) in
    magnitude: unlike a blind rotation's, these means are not spread by later rotations.  rounding: as
    cmux_mean's."""
    slots = np.asarray(table_read_slots(index, log2_lists, log2_width), np.int64) + int(w)
    return float(cmux_mean(params, tlwe_key, slots, rounding=rounding).sum()) if len(slots) else 0.0


# ---- encrypted-index table updates: rotations and a demultiplexer tree -------------------------------------------
# One update sends a value x through r rotations  x <- x + C_i (x) (X^(W 2^i) x - x)  and d demux stages  E = C (x) x,
# child(2j + 1) = E, child(2j) = x - E.  With eps = phase(C (x) D) - bit phase(D) (mean cmux_mean, variance cmux_var(bit)):
#   rotation, any bit     the error gains eps; a bit of 1 also moves what is there by W 2^i slots
#   stage, bit 1          child 2j + 1 = x + eps        child 2j = -eps: an encryption of 0 whose error is eps NEGATED, and
#                                                       whatever error x carried is gone with x
#   stage, bit 0          child 2j + 1 = eps (rows only, mean 0; x's error is gone)        child 2j = x - eps
# The models below assume a value with a pseudo-random mask (a packed or public-key list); for a trivial value the first
# external product decomposes a sample without low parts and has neither remainder nor mean, so they bound it from above.
def _update_bits(index, log2_lists, log2_width):
    d, r = int(log2_lists), 10 - int(log2_width)
    idx = int(index)
    return d, r, 1 << int(log2_width), [(idx >> k) & 1 for k in range(r + d)]


def table_update_var(params, tlwe_key, index, log2_lists, log2_width, lst=None, value_var=0.0):
    """variance (torus units) ONE update (eoc_table_update_device) of entry `index` adds to a slot of list `lst`, around
    table_update_mean.  lst None or the selected list (index >> r): value_var (the value's own noise: 0 for a trivial value,
    compact_var / pack_var for a list) + cmux_var(bit) over the r + d external products -- every slot of that list, the entry's
    and the others'.  Another list: only the external products between its branch point and the leaf count, and a stage
    whose output does not contain its input (module comment) starts the sum afresh."""
    d, r, W, bits = _update_bits(index, log2_lists, log2_width)
    sel = int(index) >> r
    lst = sel if lst is None else int(lst)
    v = float(value_var) + sum(cmux_var(params, tlwe_key, b) for b in bits[:r])
    for t in range(d):
        b, g = bits[r + d - 1 - t], (lst >> (d - 1 - t)) & 1
        keeps = g == b                      # child 2j + 1 under bit 1, child 2j under bit 0: the input + / - eps
        v = (v if keeps else 0.0) + cmux_var(params, tlwe_key, b)
    return v


def table_update_mean(params, tlwe_key, index, log2_lists, log2_width, slot=None, lst=None, rounding=False):
    """mean error (torus units) ONE update of entry `index` adds to slot `slot` (0 .. N-1, default the entry's first slot) of
    list `lst` (default the selected one).  Rotation i with bit 1 leaves cmux_mean at every slot behind it, and the later
    rotations with bit 1 carry it along (negated where it wraps past X^N = -1): seen from the final slot it sits at
    slot - sum of the later shifts.  A stage under bit 1 leaves cmux_mean(slot) in child 2j + 1 and -cmux_mean(slot) in child
    2j, whose other errors are gone; a stage under bit 0 has no mean and clears child 2j + 1.  Linear in the number of
    updates of one list: the term that bounds how often a list can be updated before a refresh.  rounding: as cmux_mean's."""
    d, r, W, bits = _update_bits(index, log2_lists, log2_width)
    sel = int(index) >> r
    lst = sel if lst is None else int(lst)
    slot = W * (int(index) & ((1 << r) - 1)) if slot is None else int(slot)
    m = 0.0
    for i in range(r):
        if not bits[i]:
            continue
        pos = (slot - sum((W << k) for k in range(i + 1, r) if bits[k])) % (2 * N)
        m += float(cmux_mean(params, tlwe_key, pos % N, rounding=rounding)) * (-1.0 if pos >= N else 1.0)
    here = float(cmux_mean(params, tlwe_key, slot, rounding=rounding))
    for t in range(d):
        b, g = bits[r + d - 1 - t], (lst >> (d - 1 - t)) & 1
        if b:
            m = m + here if g else -here
        elif g:
            m = 0.0
    return m


def table_update_budget(params, lwe_key, tlwe_key, p, log2_lists, log2_width, sigmas=6.0, value_var=0.0, table_var=0.0,
                        ksk=None, rounding=False):
    """how many updates a TABLE tolerates before a read of it no longer decodes with margin -- every update reaches every
    list: the selected one gains the value and the most noise, the others an encryption of 0 with at most as much (the bound
    below covers both, so U counts updates at any index): the largest U with
        |mean| + sigmas sqrt(variance) <= 1 / (4p)        (half a step of the grid m / (2p) decrypt_ints rounds on)
    for the worst index (every bit 1), where variance = table_var + U table_update_var + table_read_var(depth) and
    |mean| = (U + 1) depth (q/2) (1 + |s'|) + |ks_mean|: every update and the read leave their largest mean at the slot.
    0 if not even the read alone fits.  Computed from the model; nothing fitted.  rounding=True: updates and read in the
    leveled calls' rounding mode, |mean| = (U + 1) depth 2^-33 (1 + |s'|) + |ks_mean|; the variances are the same."""
    d, lw = int(log2_lists), int(log2_width)
    depth = d + 10 - lw
    worst = (1 << depth) - 1
    hw = int(np.asarray(tlwe_key, np.int64).sum())
    m1 = depth * abs(_dropped_mean(params, rounding)) * (1 + hw)
    v1 = table_update_var(params, tlwe_key, worst, d, lw, value_var=value_var)
    pr = predict(params, lwe_key, tlwe_key, ksk)
    v0 = float(table_var) + table_read_var(params, lwe_key, tlwe_key, depth, 0.0, ksk)
    margin = 1.0 / (4 * int(p))

    def fits(u):
        return (u + 1) * m1 + abs(pr["ks_mean"]) + float(sigmas) * np.sqrt(v0 + u * v1) <= margin
    if not fits(0):
        return 0
    lo, hi = 0, 1
    while fits(hi) and hi < 1 << 40:
        lo, hi = hi, hi * 2
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if fits(mid) else (lo, mid)
    return lo


# ---- finite automata on encrypted bit strings: a chain of CMux steps ----------------------------------------------
# A run is `steps` CMuxes in a row on the path the input selects, V_t[q] = A + C_t (x) (B - A) with A, B rotated successors and
# no bootstrap in between: every step adds its own error to what it selects, so BOTH the variance and the mean of the output's
# error grow linearly in the number of steps.  A rotation X^(-w) permutes the coefficients of an error polynomial and negates
# those that wrap: variances are unchanged, and a mean polynomial keeps its entries' magnitudes at other slots.
def automaton_var(params, tlwe_key, bits, final_var=0.0):
    """variance (torus units) of every coefficient of the output of an automaton run (eoc_automaton_run_device) over the input
    `bits`, before the key switch, around its mean: final_var (0 for a trivial final vector, compact_var for a public-key-
    encrypted one) + the sum of cmux_var(bit) over the steps.  Linear in the number of steps, as the mean is
    (automaton_mean_bound): nothing refreshes the sample between steps."""
    return float(final_var) + float(sum(cmux_var(params, tlwe_key, int(b) & 1) for b in bits))


def automaton_mean_bound(params, tlwe_key, steps, rounding=False):
    """bound on |mean error| (torus units) of any slot of a run of `steps` steps, before the key switch: steps (q/2)(1 + |s'|).
    One step whose bit is 1 leaves cmux_mean, a polynomial whose entries are at most (q/2)(1 + |s'|) in magnitude; the later
    steps' rotations permute and negate its entries, so the per-step bound holds at whatever slot is read.  Linear in the
    number of steps, as the variance is (automaton_var).  rounding=True: steps 2^-33 (1 + |s'|), the rounding mode's residual
    (cmux_mean)."""
    hw = int(np.asarray(tlwe_key, np.int64).sum())
    return int(steps) * abs(_dropped_mean(params, rounding)) * (1 + hw)


def automaton_budget(params, lwe_key, tlwe_key, p, sigmas=6.0, final_var=0.0, ksk=None, rounding=False):
    """how many steps (input bits) a run tolerates before its key-switched output no longer decodes with margin on the message
    space p (p = 2: a boolean at +-1/8): the largest number of steps with
        automaton_mean_bound(steps) + |ks_mean| + sigmas sqrt(automaton_var(all-ones, steps) + ks_var) <= 1 / (4p)
    Mean and variance both grow linearly in the steps; on the default sets the mean term is the one that binds.  0 if not even
    the key switch alone fits.  Computed from the model (`predict`, cmux_var); nothing fitted.  rounding=True: the run in the
    leveled calls' rounding mode, where the mean bound is 2^(32 - l Bgbit) times smaller and the variance binds."""
    pr = predict(params, lwe_key, tlwe_key, ksk)
    v1 = cmux_var(params, tlwe_key, 1)
    margin = 1.0 / (4 * int(p))

    def fits(s):
        return (automaton_mean_bound(params, tlwe_key, s, rounding) + abs(pr["ks_mean"])
                + float(sigmas) * np.sqrt(float(final_var) + s * v1 + pr["ks_var"]) <= margin)
    if not fits(0):
        return 0
    lo, hi = 0, 1
    while fits(hi) and hi < 1 << 40:
        lo, hi = hi, hi * 2
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if fits(mid) else (lo, mid)
    return lo


# ---- packing key switch: LWE samples into compact lists ----------------------------------------------------------
PACK_T, PACK_BASEBIT = 4, 4


def pack_var(params, lwe_key, filled=N):
    """variance (torus units) the packing key switch (eoc_pack_device) ADDS to the phase of every packed sample, for a fixed
    key, over the packing key's randomness and pseudo-random full-range masks:
      rows       n 4 filled E[d^2] sigma_eff^2: the n x 4 TLWE rows times the digit polynomials, which have `filled`
                 non-zero coefficients (the occupied slots of the list); E[d^2] = (16^2 + 2) / 12, sigma_eff^2 the
                 truncation-corrected variance of gaussian32 at bk_stdev, as in `predict`
      rounding   |s| 2^-32 / 12: the mask words are rounded to 16 bits (uniform on [-2^-17, 2^-17)) where s_m = 1
    The decomposition ROUNDS (the 2^15 of the key switch's precision offset), so unlike a CMux the operation leaves no mean:
    pack_mean = 0."""
    n = int(params.n)
    hw = int(np.asarray(lwe_key, np.int64).sum())
    Bg = 1 << PACK_BASEBIT
    return n * PACK_T * int(filled) * ((Bg * Bg + 2) / 12.0) * _sig2(params) + hw * 2.0**-32 / 12.0


def pack_mean(params=None, lwe_key=None, filled=N):
    """mean (torus units) the packing key switch adds, over keys: 0 -- a rounding decomposition and zero-mean rows.  For ONE
    key the slots carry the small fixed offsets of pack_offset, whose mean over keys is 0."""
    return 0.0


def pack_offset(row_phases, lwe_key, filled=N):
    """what a FIXED packing key adds to slot i on average, [N] torus units (compact_offset's sibling; nothing fitted).  The
    signed digits are uniform on [-8, 8): their mean is -1/2, not 0, on the `filled` occupied coefficients.  A list loses
    sum D_{m,j} e_{m,j} (e the rows' noise), so slot i keeps (1/2) (P E)[i] with P = 1 + X + ... + X^(filled-1) and
    E = sum_{m,j} e_{m,j}.  Over keys this has mean 0 and standard deviation (1/2) sqrt(4 n filled) sigma -- 5e-6 on Set A,
    a twentieth of sqrt(pack_var) -- so it shows only in the mean of many thousand samples under one key.
    row_phases: [n][4][N] int, the phases of the packing key's rows under s' (SecretKey.list_phases of the blob's rows)."""
    ph = np.asarray(row_phases, np.int64).reshape(-1, PACK_T, N).copy()
    s = np.asarray(lwe_key, np.int64)
    for j in range(1, PACK_T + 1):
        ph[:, j - 1, 0] -= s << (32 - PACK_BASEBIT * j)
    E = (_wrap32(ph) / 2.0**32).sum(axis=(0, 1))
    f = int(filled)
    pre = np.concatenate(([0.0], np.cumsum(E)))                          # pre[k] = E[0] + ... + E[k-1]
    i = np.arange(N)
    lo = np.maximum(i - f + 1, 0)                                        # + E[lo .. i]
    plus = pre[i + 1] - pre[lo]
    a, b = np.minimum(i + 1 + N - f, N), N                               # - E[i - k + N] for i < k < filled
    minus = np.where(f > i + 1, pre[b] - pre[np.maximum(a, i + 1)], 0.0)
    return 0.5 * (plus - minus)


# ---- two-input table lookups: blind rotation from an encrypted polynomial ---------------------------------------
def br_enc_var(params, lwe_key, tlwe_key):
    """variance (torus units) a blind rotation ADDS when its accumulator starts from an ENCRYPTED TLWE sample (k_br_enc*):
    the three terms of `predict` with step 0 a REGULAR step.  `predict` discounts step 0 because the gate accumulator
    (0, X^-b tv) has an all-zero mask and a body of constant digits; an encrypted seed's mask is already pseudo-random, so
      rows        n (1 - 1/2N) 2l N E[d^2] sigma_eff^2        every step counts whole (n_eff = n (1 - 1/2N): an amount of 0 adds nothing)
      remainder   w (1 + |s'|) q^2 / 12                        w_eff = w: step 0 has a remainder too when s_0 = 1
      truncation  (w - 1) (q/2)^2 G(s')                        the last active step is the constant br_mean, as in `predict`
    Nothing fitted."""
    n, l, Bgbit = int(params.n), int(params.l), int(params.Bgbit)
    Bg = 1 << Bgbit
    q = 2.0 ** (-l * Bgbit)
    w = int(np.asarray(lwe_key, np.int64).sum())
    hw = int(np.asarray(tlwe_key, np.int64).sum())
    Jv = _Jv(tlwe_key)
    rows = n * (1.0 - 1.0 / (2 * N)) * 2 * l * N * ((Bg * Bg + 2) / 12.0) * _sig2(params)
    return rows + w * (1 + hw) * q * q / 12.0 + max(w - 1, 0) * (q / 2) ** 2 * float((Jv**2).mean())


def lut2_var(params, lwe_key, tlwe_key, ksk=None):
    """variance (torus units) of the error of a two-input lookup's output (eoc_lut2_batch_device) around lut2_mean, for a fixed
    key: the level-1 output that sits in the packed polynomial (predict()['total_var']) + the packing key switch of a full
    list (pack_var(params, lwe_key, N)) + a regular blind rotation (br_enc_var) + the key switch (predict()['ks_var'])."""
    pr = predict(params, lwe_key, tlwe_key, ksk)
    return pr["total_var"] + pack_var(params, lwe_key, N) + br_enc_var(params, lwe_key, tlwe_key) + pr["ks_var"]


def lut2_mean(params, lwe_key, tlwe_key, ksk=None):
    """mean error (torus units) of a two-input lookup's output: the level-1 output's total_mean + the level-2 blind rotation's
    br_mean + its key switch's ks_mean; the pack's mean is 0"""
    pr = predict(params, lwe_key, tlwe_key, ksk)
    return pr["total_mean"] + pr["br_mean"] + pr["ks_mean"]


def lut2_margin_sigma(p, n_tables, params, lwe_key, tlwe_key, x_var=None, y_var=None):
    """(level-1 margin, level-2 margin) of a two-input lookup at message space p, in predicted standard deviations: level 1
    mod-switches x on the grid of T = n_tables, level 2 mod-switches y on the grid of 1.  x_var / y_var: variance of the
    samples in front of the call (None: a gate-bootstrap output, predict()['total_var'])."""
    v_out = predict(params, lwe_key, tlwe_key)["total_var"]
    vx = v_out if x_var is None else float(x_var)
    vy = v_out if y_var is None else float(y_var)
    return (lut_margin_sigma_var(p, max(int(n_tables), 1), vx, lwe_key), lut_margin_sigma_var(p, 1, vy, lwe_key))


# ---- multi-digit table lookups: deeper trees -----------------------------------------------------------------------
def lut_tree_var(params, lwe_key, tlwe_key, d, ksk=None):
    """variance (torus units) of the error of a d-digit lookup's output (eoc_lut_tree_batch_device) around lut_tree_mean, for a
    fixed key, lut2_var's composition once per further digit: the level-1 output (predict()['total_var']) + (d - 1) x (the
    pack of a full list + a regular blind rotation + the key switch).  The exact pack evaluates eoc_tv_pack_device's rule
    without the transforms' rounding, so pack_var stands unchanged.  d = 2 is lut2_var.  Nothing fitted."""
    pr = predict(params, lwe_key, tlwe_key, ksk)
    per_level = pack_var(params, lwe_key, N) + br_enc_var(params, lwe_key, tlwe_key) + pr["ks_var"]
    return pr["total_var"] + (int(d) - 1) * per_level


def lut_tree_mean(params, lwe_key, tlwe_key, d, ksk=None):
    """mean error (torus units) of a d-digit lookup's output: the level-1 output's total_mean + (d - 1) x (a blind rotation's
    br_mean + its key switch's ks_mean); the packs' mean is 0.  d = 2 is lut2_mean."""
    pr = predict(params, lwe_key, tlwe_key, ksk)
    return pr["total_mean"] + (int(d) - 1) * (pr["br_mean"] + pr["ks_mean"])


def lut_tree_margin_sigma(p, d, n_tables, params, lwe_key, tlwe_key, digit_vars=None):
    """one margin per level of a d-digit lookup at message space p, in predicted standard deviations: level 1 mod-switches
    x_1 on the grid of T = n_tables, every level k >= 2 is a T = 1 lookup on x_k.  digit_vars: the variances of the d digit
    samples in front of the call (None, or None entries: a gate-bootstrap output, predict()['total_var'])."""
    v_out = predict(params, lwe_key, tlwe_key)["total_var"]
    dv = [None] * int(d) if digit_vars is None else list(digit_vars)
    if len(dv) != int(d):
        raise ValueError("lut_tree_margin_sigma: one variance per digit")
    dv = [v_out if v is None else float(v) for v in dv]
    return tuple(lut_margin_sigma_var(p, max(int(n_tables), 1) if k == 0 else 1, dv[k], lwe_key) for k in range(int(d)))


# ---- inner products with public integer weights on compact lists ---------------------------------------------
def linear_var(params, w_row, slot_var):
    """variance (torus units) of the phase of one output of eoc_dot_device around its mean: ||w||^2 slot_var for independent
    slots of variance slot_var each -- for the slots of fresh lists, which share u and e1, the variance over lists AND rows of
    independent zero-mean weights; one fixed row: linear_var_row (compact_var for fresh lists; a bootstrap output's total_var + pack_var behind
    eoc_pack_device).  The operation itself adds nothing: the body is an exact integer sum and the mask differs from the
    exact product by the conversion's few units of 2^-32 per chunk.  eoc_linear_device's key switch adds predict()['ks_var']
    and ['ks_mean'] on top."""
    w = np.asarray(w_row, np.float64).ravel()
    return float((w * w).sum()) * float(slot_var)


def lwe_linear_var(w_row, input_var):
    """variance (torus units) of the phase of one output of eoc_lwe_matmul_device: ||w||^2 input_var for
    independent input samples of variance input_var each.  Nothing else enters: the output's error is exactly
    sum_k w_k e_k -- no packing error on the inputs, no key switch behind the sum.  A bootstrap output has
    predict()['total_var'] (and mean total_mean, which the sum multiplies by sum_k w_k); a fresh sample of eoc_lwe_encrypt or
    eoc_encrypt_ints has params.ks_stdev ** 2."""
    w = np.asarray(w_row, np.float64).ravel()
    return float((w * w).sum()) * float(input_var)


def linear_offset(params, pk_or_key, w_row, tlwe_key=None):
    """mean error (torus units) of one output of eoc_dot_device on FRESH lists under one public key: every list's slots
    carry compact_offset (a fresh binary u per list has mean 1/2, the key's e is the same for all of them), so the output
    carries sum_k w_k compact_offset[k mod N] = (1/2) sum_l (V_l J e)[0] -- derived from the key, nothing fitted.
    pk_or_key: a SecretKey (its own public key and TLWE key are used), or a PublicKey / EOCPK1 blob / (A, B) pair together
    with tlwe_key."""
    if tlwe_key is None:
        tlwe_key, pk = pk_or_key.tlwe_key, pk_or_key.public_key_bytes()
    else:
        pk = pk_or_key
    off = compact_offset(tlwe_key, pk)
    w = np.asarray(w_row, np.float64).ravel()
    return float((w * off[np.arange(w.size) % N]).sum())


def linear_var_row(params, w_row, tlwe_key, pk):
    """linear_var for ONE weight row on fresh lists under one key, exactly: the output's error is coefficient 0 of
    V (u e + e2 - e1 s') summed over the lists, so its variance over the lists' randomness is
      sum_l ||V_l e||^2 / 4 + ||w||^2 sigma^2 + sum_l ||V_l s'||^2 sigma^2.
    linear_var(compact_var) is its mean over rows of independent zero-mean weights; over 200 random rows a single row is 0.66 - 2.10 of it
    (standard deviation 0.29, either default set), because s' and a binary u have mean 1/2: V (1/2) J is the running sum of the weights, a
    random walk whose energy does not average out inside one row.  Nothing is fitted."""
    w = np.asarray(w_row, np.float64).ravel()
    e = pk_noise(pk, tlwe_key)
    s1 = np.asarray(tlwe_key, np.float64)
    sig2 = _sig2(params)
    out = float((w * w).sum()) * sig2
    for l0 in range(0, w.size, N):
        wl = np.zeros(N)
        wl[:min(N, w.size - l0)] = w[l0:l0 + N]
        V = np.concatenate(([wl[0]], -wl[:0:-1]))                      # V[0] = w[0], V[N - k] = -w[k]
        for poly, scale in ((e, 0.25), (s1, sig2)):
            full = np.convolve(V, poly)
            r = full[:N].copy()
            r[:N - 1] -= full[N:]
            out += scale * float((r * r).sum())
    return out


# ---- convolutions with public int8 kernels on compact lists ------------------------------------------------------
def conv_row(w_row, t):
    """the effective inner-product row of slot t of one output channel of eoc_conv_device: slot t has phase
    bias + sum_l sum_k w[l N + k] x_l[t + k] with the negacyclic wrap, i.e. the inner product of the inputs with
      w_eff[l N + m] = w[l N + m - t] (m >= t),  -w[l N + m - t + N] (m < t),
    per list (w_row is padded with zeros to whole lists).  linear_var, linear_var_row and linear_offset of this row price the
    slot -- the weight polynomial of w_eff is X^t V up to the sign of the wrap, nothing is fitted.  float64 [L N]."""
    t = int(t)
    if not 0 <= t < N:
        raise ValueError(f"conv_row: slot {t} outside [0, {N})")
    w = np.asarray(w_row, np.float64).ravel()
    w = np.concatenate((w, np.zeros(-w.size % N))).reshape(-1, N)
    return (np.concatenate((-w[:, N - t:], w[:, :N - t]), axis=1) if t else w).reshape(-1)
