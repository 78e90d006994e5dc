// kernels.hip.h -- hand-written HIP kernels (gfx950 / CDNA4) for the TFHE gate-bootstrapping path.
//
// Replaces, on the device, the upstream libtfhe CPU functions listed in SURVEY.md 8a:
//   k_prepare        bootsNAND... linear stage + modSwitchFromTorus32 loop of tfhe_bootstrap_woKS_FFT
//   k_blind_rotate   tfhe_blindRotateAndExtract_FFT / tfhe_blindRotate_FFT / tfhe_MuxRotate_FFT /
//                    tLweMulByXaiMinusOne / tGswTorus32PolynomialDecompH / IntPolynomial_ifft /
//                    tLweFFTAddMulRTo / tLweFromFFTConvert / tLweAddTo / tLweExtractLweSample
//   k_keyswitch      lweKeySwitch
//   k_fft_fwd_polys  tGswToFFTConvert (key load)
//
// Arithmetic contract (DESIGN.md "Canonical transform v3"): every floating-point operation below is a
// separately rounded IEEE-754 binary64 +, -, * or an explicit fma; the file MUST be compiled with
// -ffp-contract=off.  The data-flow graph is the oracle's radix-2 graph:
//   forward  evaluation tree of X^512 - i on c_j = p_j + i p_{j+512} (no twist pass; natural order in,
//            bit-reversed root index out); stage 0 is written on exact integer sums (4 fma per butterfly),
//            every later butterfly is (u + w v, u - w v) in the 6-operation fused form
//            a' = u + w v by 4 fma, b' = fma(2, u, -a');
//   inverse  decimation in time with conjugate twiddles, three register-constant stages as exact moves, then
//            the un-twist by conj(E[j]) and the conversion Torus32(int64(.)) (truncation, as upstream).
// Three radix-2 stages are executed per register pass (8 points per lane, one 512-point transform per wave64).
// The twiddles of a pass are 1 + 2 + 4 per lane, but the second of every sibling pair is i times the first
// (E[k + 512] = i E[k] holds exactly in the table), so a pass LOADS four and applies the other three through
// operand swaps and sign modifiers: bit-identical, 4 instead of 7 ds_read_b128 and 16 instead of 28 registers.
//
// Wave layouts of the 512 complex points (e = 9-bit index):
//   L0: reg r = e[8:6], lane = e[5:0]           (input of forward / output of inverse)
//   L1: reg r = e[5:3], lane = e[8:6]*8 + e[2:0]
//   L2: reg r = e[2:0], lane = e[8:3]           (spectrum layout; stored at sigma(e) = r*64 + lane)
// The two transposes go through a per-wave LDS scratch with conflict-free address maps f01 / f12.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

namespace eoc {

typedef double d2 __attribute__((ext_vector_type(2))); // (re, im)

constexpr int kN = 1024;
constexpr int kNH = 512;
constexpr int kScr = 568;      // d2 elements of per-wave transpose scratch (f01 needs 72*7+64)
// twiddle tables in LDS (d2 entries), FOUR per lane and pass {A, B0, C0, C2}: the stage twiddles are
// A | B0, i B0 | C0, i C0, C2, i C2
constexpr int kTwF1 = 0;                    // forward pass 1 [4][8]  (by lane >> 3)
constexpr int kTwF2 = 32;                   // forward pass 2 [4][64] (by lane)
constexpr int kTwI1 = 32 + 256;             // inverse middle pass [4][8] (by lane & 7)
constexpr int kTwI0 = 32 + 256 + 32;        // inverse last pass [4][64] (by lane)
constexpr int kTwEntries = 32 + 256 + 32 + 256;

#define EOC_FMA(a, b, c) __builtin_fma((a), (b), (c))

// register constants of the forward transform's first pass: E[256] = (c, c), E[128], E[64], E[320]
// (checked against canon_twiddles.h when an engine is created)
#define EOC_SQRT_HALF 0x1.6a09e667f3bcdp-1
#define EOC_E128_RE 0x1.d906bcf328d46p-1
#define EOC_E128_IM 0x1.87de2a6aea963p-2
#define EOC_E64_RE 0x1.f6297cff75cb0p-1
#define EOC_E64_IM 0x1.8f8b83c69a60bp-3
#define EOC_E320_RE 0x1.1c73b39ae68c8p-1
#define EOC_E320_IM 0x1.a9b66290ea1a3p-1

__device__ __forceinline__ d2 cmulc(d2 a, d2 w)
{ // a * conj(w)
    d2 r;
    r.x = EOC_FMA(a.x, w.x, a.y * w.y);
    r.y = EOC_FMA(a.y, w.x, -(a.x * w.y));
    return r;
}

// --- radix-2 butterflies (u, v) -> (u + t v, u - t v), fused form ---------------------------------
#define EOC_BFLY_TAIL()                      \
    a = n;                                   \
    b.x = EOC_FMA(2.0, u.x, -n.x);           \
    b.y = EOC_FMA(2.0, u.y, -n.y)
__device__ __forceinline__ void ct_w(d2 &a, d2 &b, d2 w)
{ // t = w
    d2 u = a, n;
    n.x = EOC_FMA(-w.y, b.y, EOC_FMA(w.x, b.x, u.x));
    n.y = EOC_FMA(w.x, b.y, EOC_FMA(w.y, b.x, u.y));
    EOC_BFLY_TAIL();
}
__device__ __forceinline__ void ct_iw(d2 &a, d2 &b, d2 w)
{ // t = i w = (-w.im, w.re)
    d2 u = a, n;
    n.x = EOC_FMA(-w.x, b.y, EOC_FMA(-w.y, b.x, u.x));
    n.y = EOC_FMA(-w.y, b.y, EOC_FMA(w.x, b.x, u.y));
    EOC_BFLY_TAIL();
}
__device__ __forceinline__ void ct_wc(d2 &a, d2 &b, d2 w)
{ // t = conj(w)
    d2 u = a, n;
    n.x = EOC_FMA(w.y, b.y, EOC_FMA(w.x, b.x, u.x));
    n.y = EOC_FMA(w.x, b.y, EOC_FMA(-w.y, b.x, u.y));
    EOC_BFLY_TAIL();
}
__device__ __forceinline__ void ct_iwc(d2 &a, d2 &b, d2 w)
{ // t = conj(i w) = (-w.im, -w.re)
    d2 u = a, n;
    n.x = EOC_FMA(w.x, b.y, EOC_FMA(-w.y, b.x, u.x));
    n.y = EOC_FMA(-w.y, b.y, EOC_FMA(-w.x, b.x, u.y));
    EOC_BFLY_TAIL();
}
__device__ __forceinline__ void ct_1(d2 &a, d2 &b)
{ // t = 1 (register-constant stages of the inverse only)
    d2 u = a, v = b;
    a = u + v;
    b = u - v;
}
__device__ __forceinline__ void ct_ic(d2 &a, d2 &b)
{ // t = conj(i): t v = (v.y, -v.x)
    d2 u = a, t;
    t.x = b.y;
    t.y = -b.x;
    a = u + t;
    b = u - t;
}

// --- LDS address maps ---------------------------------------------------------------------------
// f12: XOR swizzle, conflict-free for ds_read_b128 (16-lane groups, 64 banks) AND ds_write_b128 (8-lane
// groups, 32 banks) in both the L1 and the L2 access pattern (brute-forced against the bank model of
// MI355X_MICROARCH.md)
__device__ __forceinline__ int f12(int e) { return e ^ (((e >> 3) & 7) | (((e >> 6) & 1) << 3)); }

// compiler-level ordering between a wave's own LDS writes and cross-lane reads (the hardware
// executes one wave's LDS operations in order, so no s_barrier is needed inside a wave)
__device__ __forceinline__ void wave_lds_fence()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ---- forward transform, in pieces ---------------------------------------------------------------
// stage 0 on exact integer-valued doubles: u = (a, b), v = (p, q), dm = p - q, dp = p + q
__device__ __forceinline__ void fwd_stage0(d2 &lo, d2 &hi, double a, double b, double dm, double dp)
{
    lo.x = EOC_FMA(EOC_SQRT_HALF, dm, a);
    lo.y = EOC_FMA(EOC_SQRT_HALF, dp, b);
    hi.x = EOC_FMA(-EOC_SQRT_HALF, dm, a);
    hi.y = EOC_FMA(-EOC_SQRT_HALF, dp, b);
}
__device__ __forceinline__ void fwd_pass0_tail(d2 (&x)[8])
{ // stages 1, 2 (bits 7, 6): rho(1,0) = E[128], rho(1,1) = i E[128]; rho(2,.) = E[64], i E[64], E[320], i E[320]
    const d2 w1 = {EOC_E128_RE, EOC_E128_IM}, w2 = {EOC_E64_RE, EOC_E64_IM}, w3 = {EOC_E320_RE, EOC_E320_IM};
    ct_w(x[0], x[2], w1);
    ct_w(x[1], x[3], w1);
    ct_iw(x[4], x[6], w1);
    ct_iw(x[5], x[7], w1);
    ct_w(x[0], x[1], w2);
    ct_iw(x[2], x[3], w2);
    ct_w(x[4], x[5], w3);
    ct_iw(x[6], x[7], w3);
}

// ---- gadget decomposition and the external product's arithmetic: the ONE copy every kernel uses ---------------------
// Constants of the signed decomposition into l digits of Bgbit bits.  The digit words carry an offset, Bg/2 at every
// digit position, so digit p is a bit field of the word, biased: u = digit + Bg/2 in [0, Bg).
// as_double(2^52 | u) - (2^52 + Bg/2) is the digit, exactly (bias1); the stage-0 sums p - q and p + q are formed on the
// biased integers and converted the same way (bias2).
// The offset itself is NOT here: each kernel sums it in three lines of its own text, from Bgbit alone, and builds its
// Gadget behind that sum.  Measured with tools/isa_diff.py against the parent: with the sum inside make_gadget (as a loop
// or loop-free), the step loop's entry test of k_blind_rotate_wide<10> came out inverted (4 changed lines) and
// k_cmux<2,10> / <3,7> changed in 173 / 141 lines; with the sum in the kernels but behind make_gadget, the run-time-base
// instances k_cmux<2,0> / <3,0> / <4,0> changed in 410-468 lines; as written now, every k_cmux, wide and gadget-length
// 1, 3, 4 pair instance is byte-identical.  The cause was not established.
template <int BGBIT> // > 0: the base is known at compile time (digit extraction becomes one bit-field extract); 0: run time
struct Gadget {
    int Bgbit;
    uint32_t Bg, maskBg, halfBg;
    double bias1, bias2;
    __device__ __forceinline__ int shift(int p) const { return 32 - p * Bgbit; } // of digit p = 1..l in a digit word
};
template <int BGBIT>
__device__ __forceinline__ Gadget<BGBIT> make_gadget(int Bgbit_rt)
{
    const int Bgbit = BGBIT > 0 ? BGBIT : Bgbit_rt;
    Gadget<BGBIT> g;
    g.Bgbit = Bgbit;
    g.Bg = 1u << Bgbit;
    g.maskBg = g.Bg - 1;
    g.halfBg = g.Bg >> 1;
    g.bias1 = 4503599627370496.0 + (double)g.halfBg;
    g.bias2 = 4503599627370496.0 + (double)g.Bg;
    return g;
}
// The digit pass: the digit at `shift` of the 16 coefficients of this lane (digit words lo[r]: coefficient lane + 64 r,
// hi[r]: lane + 64 r + 512) and the first pass of its forward transform (stages 0-2).  EOC_GADGET_BG / _MASK: a
// compile-time base is named as a constant, as a kernel's own text would name it, and a run-time one is read from the
// struct at each use (measured: read from the struct, k_blind_rotate_wide<10> changed in 64 lines; copied into two
// locals first, k_blind_rotate_wide<0> changed in 144 lines inside the step loop)
#define EOC_GADGET_BG(g) (BGBIT > 0 ? 1u << BGBIT : (g).Bg)
#define EOC_GADGET_MASK(g) (BGBIT > 0 ? (1u << BGBIT) - 1 : (g).maskBg)
template <int BGBIT>
__device__ __forceinline__ void digit_pass(const uint32_t *lo, const uint32_t *hi, int shift, const Gadget<BGBIT> &g,
                                           d2 (&x)[8])
{
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const uint32_t ua = (lo[r] >> shift) & EOC_GADGET_MASK(g), ub = (hi[r] >> shift) & EOC_GADGET_MASK(g);
        const uint32_t up = (lo[r + 4] >> shift) & EOC_GADGET_MASK(g), uq = (hi[r + 4] >> shift) & EOC_GADGET_MASK(g);
        const double a = __hiloint2double(0x43300000, (int)ua) - g.bias1;
        const double b = __hiloint2double(0x43300000, (int)ub) - g.bias1;
        const double dm = __hiloint2double(0x43300000, (int)(up - uq + EOC_GADGET_BG(g))) - g.bias2;
        const double dp = __hiloint2double(0x43300000, (int)(up + uq)) - g.bias2;
        fwd_stage0(x[r], x[r + 4], a, b, dm, dp);
    }
    fwd_pass0_tail(x);
}
#undef EOC_GADGET_BG
#undef EOC_GADGET_MASK
// The complex multiply-accumulate of the chains, in the canonical nesting (oracle/tfhe_oracle.c, compiled like this file
// with -ffp-contract=off): the first term of a chain is a product, one multiplication and one fused multiply-add per
// component (cmul0); every later term is two nested fused multiply-adds per component, the x.x product innermost (cmac1).
// This nesting is the bit-parity contract with the oracle: change it here and there, or nowhere.
__device__ __forceinline__ d2 cmul0(d2 x, d2 b)
{
    d2 o;
    o.x = EOC_FMA(-x.y, b.y, x.x * b.x);
    o.y = EOC_FMA(x.y, b.x, x.x * b.y);
    return o;
}
__device__ __forceinline__ d2 cmac1(d2 x, d2 b, d2 acc)
{
    d2 o;
    o.x = EOC_FMA(-x.y, b.y, EOC_FMA(x.x, b.x, acc.x));
    o.y = EOC_FMA(x.y, b.x, EOC_FMA(x.x, b.y, acc.y));
    return o;
}
__device__ __forceinline__ void cmac8(bool first, const d2 (&x)[8], const d2 (&b)[8], d2 (&acc)[8])
{ // the eight bins of a lane; `first`: this term starts the chain (acc is not read)
#pragma unroll
    for (int r = 0; r < 8; r++) {
        if (first) acc[r] = cmul0(x[r], b[r]);
        else acc[r] = cmac1(x[r], b[r], acc[r]);
    }
}

// the four loaded twiddles of a table-driven pass; `stride` = 8 (pass 1, q = table + (lane >> 3)) or 64 (pass 2)
__device__ __forceinline__ void tw_load(d2 (&t)[4], const d2 *q, int stride)
{
#pragma unroll
    for (int k = 0; k < 4; k++) t[k] = q[k * stride];
}
__device__ __forceinline__ void fwd_pass12(d2 (&x)[8], const d2 (&t)[4])
{ // three radix-2 stages on the 8 register points: twiddles A | B0, i B0 | C0, i C0, C2, i C2
    ct_w(x[0], x[4], t[0]);
    ct_w(x[1], x[5], t[0]);
    ct_w(x[2], x[6], t[0]);
    ct_w(x[3], x[7], t[0]);
    ct_w(x[0], x[2], t[1]);
    ct_w(x[1], x[3], t[1]);
    ct_iw(x[4], x[6], t[1]);
    ct_iw(x[5], x[7], t[1]);
    ct_w(x[0], x[1], t[2]);
    ct_iw(x[2], x[3], t[2]);
    ct_w(x[4], x[5], t[3]);
    ct_iw(x[6], x[7], t[3]);
}
// transposes: write in the source layout, read in the destination layout.  One wave's LDS operations
// execute in issue order, so a later write to the same scratch cannot overtake an earlier read.
__device__ __forceinline__ void t01_write(const d2 (&x)[8], d2 *scr, int lane)
{
#pragma unroll
    for (int r = 0; r < 8; r++) scr[72 * r + lane] = x[r];
    wave_lds_fence();
}
__device__ __forceinline__ void t01_read(d2 (&x)[8], const d2 *scr, int lane)
{
    const int hi = lane >> 3, lo = lane & 7;
#pragma unroll
    for (int r = 0; r < 8; r++) x[r] = scr[72 * hi + 8 * r + lo];
    wave_lds_fence();
}
__device__ __forceinline__ void t12_write(const d2 (&x)[8], d2 *scr, int lane)
{
    const int hi = lane >> 3, lo = lane & 7;
#pragma unroll
    for (int r = 0; r < 8; r++) scr[f12(hi * 64 + r * 8 + lo)] = x[r];
    wave_lds_fence();
}
__device__ __forceinline__ void t12_read(d2 (&x)[8], const d2 *scr, int lane)
{
#pragma unroll
    for (int r = 0; r < 8; r++) x[r] = scr[f12(lane * 8 + r)];
    wave_lds_fence();
}

// one forward transform after its first pass: x[] in L0 (stages 0-2 done) -> x[] in L2.  The second twiddle set is
// requested under the second transpose (register-lean: this form runs next to the live spectra of a finished pair)
__device__ __forceinline__ void fft_fwd_rest(d2 (&x)[8], const d2 *tw, d2 *scr, int lane)
{
    d2 t1[4], t2[4];
    tw_load(t1, tw + kTwF1 + (lane >> 3), 8);
    t01_write(x, scr, lane);
    t01_read(x, scr, lane);
    fwd_pass12(x, t1);
    t12_write(x, scr, lane);
    tw_load(t2, tw + kTwF2 + lane, 64);
    t12_read(x, scr, lane);
    fwd_pass12(x, t2);
}
// EOC_SB: scheduling barriers that pin the phase order of the skewed pair below (the machine scheduler otherwise sinks
// the early twiddle reads under the transposes and waits for BOTH transposes before the first register pass).
// EOC_SGB: the stores of one transform's transpose are interleaved one by one with the other transform's register pass
// (sched_group_barrier pipelines): a ds_write_b128 holds the CU's LDS store path for about 13 cycles, and a wave that
// issues eight of them back to back is issue-blocked for all of them (SQ_WAIT_INST_LDS was 22 % of the wave cycles)
#define EOC_SB() __builtin_amdgcn_sched_barrier(0)
#define EOC_SGB(mask, n) __builtin_amdgcn_sched_group_barrier((mask), (n), 0)
#define EOC_M_VALU 0x002
#define EOC_M_DSR 0x100
#define EOC_M_DSW 0x200
// T2 != nullptr: the last pass's four twiddles are resident in registers (loop-invariant, kept by the caller);
// T1 != nullptr: the first table pass's too, and the pair then reads no table at all.
// before_last() runs between the last transpose and b's last register pass, pinned there: the caller's first key-row
// requests, which then fly under that pass
struct FwdNoHook {
    __device__ __forceinline__ void operator()() const {}
};
template <class MakeB, class BeforeLast = FwdNoHook>
__device__ __forceinline__ void fft_fwd_rest_x2(d2 (&xa)[8], d2 (&xb)[8], MakeB make_b, const d2 *tw, d2 *scr, int lane,
                                                const d2 (*T2)[4] = nullptr, const d2 (*T1)[4] = nullptr,
                                                BeforeLast before_last = BeforeLast())
{
    d2 t1[4], t2[4];
    EOC_SB();
    // region B: first pass of b, a's stores spread through it; then a's reads
    if (T1) {
#pragma unroll
        for (int k = 0; k < 4; k++) t1[k] = (*T1)[k];
    } else {
        tw_load(t1, tw + kTwF1 + (lane >> 3), 8);
    }
    wave_lds_fence();
    t01_write(xa, scr, lane);
    make_b();
    t01_read(xa, scr, lane);
    if (!T1) EOC_SGB(EOC_M_DSR, 4);
#pragma unroll
    for (int k = 0; k < 8; k++) {
        EOC_SGB(EOC_M_DSW, 1);
        EOC_SGB(EOC_M_VALU, 10);
    }
    EOC_SGB(EOC_M_VALU, 64);
    EOC_SGB(EOC_M_DSR, 8);
    EOC_SB();
    // region C: second pass of a; b's stores spread through its first half, then b's reads and the last twiddle set
    t01_write(xb, scr, lane);
    t01_read(xb, scr, lane);
    if (T2) {
#pragma unroll
        for (int k = 0; k < 4; k++) t2[k] = (*T2)[k];
    } else {
        tw_load(t2, tw + kTwF2 + lane, 64);
    }
    wave_lds_fence();
    fwd_pass12(xa, t1);
#pragma unroll
    for (int k = 0; k < 8; k++) {
        EOC_SGB(EOC_M_DSW, 1);
        EOC_SGB(EOC_M_VALU, 4);
    }
    if (T2) EOC_SGB(EOC_M_DSR, 8);
    else EOC_SGB(EOC_M_DSR, 12);
    EOC_SGB(EOC_M_VALU, 40);
    EOC_SB();
    // region D: second pass of b under a's second transpose
    t12_write(xa, scr, lane);
    t12_read(xa, scr, lane);
    fwd_pass12(xb, t1);
#pragma unroll
    for (int k = 0; k < 8; k++) {
        EOC_SGB(EOC_M_DSW, 1);
        EOC_SGB(EOC_M_VALU, 4);
    }
    EOC_SGB(EOC_M_DSR, 8);
    EOC_SGB(EOC_M_VALU, 40);
    EOC_SB();
    // region E: third pass of a under b's second transpose
    t12_write(xb, scr, lane);
    t12_read(xb, scr, lane);
    fwd_pass12(xa, t2);
#pragma unroll
    for (int k = 0; k < 8; k++) {
        EOC_SGB(EOC_M_DSW, 1);
        EOC_SGB(EOC_M_VALU, 4);
    }
    EOC_SGB(EOC_M_DSR, 8);
    EOC_SGB(EOC_M_VALU, 40);
    EOC_SB();
    if constexpr (!std::is_same<BeforeLast, FwdNoHook>::value) {
        before_last();
        EOC_SB();
    }
    fwd_pass12(xb, t2);
}

// ---- inverse transform, in pieces: x[] in L2 -> x[] in L0 (before the un-twist); decimation in time,
// conjugate twiddles ---------------------------------------------------------------------------------
__device__ __forceinline__ void inv_pass2(d2 (&x)[8])
{ // stages 8,7,6 (bits 0,1,2): register constants; w = 1 and w = conj(i) are exact moves
    const d2 wc = {EOC_SQRT_HALF, EOC_SQRT_HALF}; // W[64]; W[192] = i W[64]
    ct_1(x[0], x[1]);
    ct_1(x[2], x[3]);
    ct_1(x[4], x[5]);
    ct_1(x[6], x[7]);
    ct_1(x[0], x[2]);
    ct_ic(x[1], x[3]);
    ct_1(x[4], x[6]);
    ct_ic(x[5], x[7]);
    ct_1(x[0], x[4]);
    ct_wc(x[1], x[5], wc);
    ct_ic(x[2], x[6]);
    ct_iwc(x[3], x[7], wc);
}
__device__ __forceinline__ void inv_pass10(d2 (&x)[8], const d2 (&t)[4])
{ // three DIT stages, twiddles conj of: m6 | m4, i m4 | m0, m1, i m0, i m1   (t = {m6, m4, m0, m1})
    ct_wc(x[0], x[1], t[0]);
    ct_wc(x[2], x[3], t[0]);
    ct_wc(x[4], x[5], t[0]);
    ct_wc(x[6], x[7], t[0]);
    ct_wc(x[0], x[2], t[1]);
    ct_iwc(x[1], x[3], t[1]);
    ct_wc(x[4], x[6], t[1]);
    ct_iwc(x[5], x[7], t[1]);
    ct_wc(x[0], x[4], t[2]);
    ct_wc(x[1], x[5], t[3]);
    ct_iwc(x[2], x[6], t[2]);
    ct_iwc(x[3], x[7], t[3]);
}
__device__ __forceinline__ void t21_read(d2 (&x)[8], const d2 *scr, int lane)
{
    const int hi = lane >> 3, lo = lane & 7;
#pragma unroll
    for (int r = 0; r < 8; r++) x[r] = scr[f12(hi * 64 + r * 8 + lo)];
    wave_lds_fence();
}
__device__ __forceinline__ void t10_read(d2 (&x)[8], const d2 *scr, int lane)
{
#pragma unroll
    for (int r = 0; r < 8; r++) x[r] = scr[72 * r + lane];
    wave_lds_fence();
}
// inverse transform + un-twist factors: the twiddles of both table passes and the 8 un-twist factors are requested
// under the first transpose, so that no table read sits between a transpose read and its use.  The eight stores of each
// transpose leave in the order the last stage of the register pass completes its butterflies -- (0,4) (1,5) (2,6) (3,7) --
// and are spread through that stage (sched_group_barrier), as the forward pair does
// T1 != nullptr: the first table pass's four twiddles are resident in registers.  RESIDENT: so are the last pass's (*T0)
// and the eight un-twist factors, which `ut` then already holds, and the transform reads no table at all
template <bool RESIDENT = false>
__device__ __forceinline__ void fft_inv_wave(d2 (&x)[8], d2 (&ut)[8], const d2 *tw, const d2 *s_twist, d2 *scr, int lane,
                                             const d2 (*T1)[4] = nullptr, const d2 (*T0)[4] = nullptr)
{
    d2 t1[4], t0[4];
    EOC_SB();
    if (T1) {
#pragma unroll
        for (int k = 0; k < 4; k++) t1[k] = (*T1)[k];
    } else {
        tw_load(t1, tw + kTwI1 + (lane & 7), 8);
    }
    inv_pass2(x);
    {
        constexpr int ord[8] = {0, 4, 1, 5, 2, 6, 3, 7};
#pragma unroll
        for (int q = 0; q < 8; q++) scr[f12(lane * 8 + ord[q])] = x[ord[q]];
        wave_lds_fence();
    }
    t21_read(x, scr, lane);
    EOC_SGB(EOC_M_VALU, 32);                                     // stages 8 and 7
    EOC_SGB(EOC_M_VALU, 4);  EOC_SGB(EOC_M_DSW, 2);              // (0,4): w = 1
    EOC_SGB(EOC_M_VALU, 6);  EOC_SGB(EOC_M_DSW, 2);              // (1,5)
    EOC_SGB(EOC_M_VALU, 4);  EOC_SGB(EOC_M_DSW, 2);              // (2,6): w = conj(i)
    EOC_SGB(EOC_M_VALU, 6);  EOC_SGB(EOC_M_DSW, 2);              // (3,7)
    EOC_SGB(EOC_M_DSR, 8);
    if constexpr (RESIDENT) {
#pragma unroll
        for (int k = 0; k < 4; k++) t0[k] = (*T0)[k];
    } else {
        tw_load(t0, tw + kTwI0 + lane, 64);
#pragma unroll
        for (int r = 0; r < 8; r++) ut[r] = s_twist[lane + 64 * r];
    }
    wave_lds_fence();
    EOC_SB();
    inv_pass10(x, t1);
    {
        constexpr int ord[8] = {0, 4, 1, 5, 2, 6, 3, 7};
        const int hi = lane >> 3, lo = lane & 7;
#pragma unroll
        for (int q = 0; q < 8; q++) scr[72 * hi + 8 * ord[q] + lo] = x[ord[q]];
        wave_lds_fence();
    }
    t10_read(x, scr, lane);
    EOC_SGB(EOC_M_VALU, 48);                                     // first two stages of the pass
#pragma unroll
    for (int k = 0; k < 4; k++) {
        EOC_SGB(EOC_M_VALU, 6);
        EOC_SGB(EOC_M_DSW, 2);
    }
    EOC_SGB(EOC_M_DSR, 8);
    EOC_SB();
    inv_pass10(x, t0);
}

// Torus32(int64(v)) for |v| < 2^51: t = trunc(v) (exact), t + 1.5 * 2^52 is exact and carries t mod 2^32 in its
// low dword.  Two operations.  (An external product is bounded by 2 l N (Bg/2) 2^31 <= 2^52 in exact arithmetic and
// is statistically near 2^45; tests/ hold the oracle's high-water mark below 2^51.)
__device__ __forceinline__ uint32_t wrap_trunc(double v)
{
    double m = __builtin_trunc(v) + 6755399441055744.0;
    return (uint32_t)__double2loint(m);
}

// copy the two constant tables into LDS (called by all threads of the workgroup, followed by __syncthreads)
__device__ __forceinline__ void load_tables(d2 *s_tw, d2 *s_twist, const d2 *g_tw, const d2 *g_twist, int tid, int nthreads)
{
    for (int i = tid; i < kTwEntries; i += nthreads) s_tw[i] = g_tw[i];
    for (int i = tid; i < kNH; i += nthreads) s_twist[i] = g_twist[i];
}

// =================================================================================================
// K4 / debug: forward transform of `count` integer polynomials, one wave each
// =================================================================================================
// `scale` must be a power of two (exact): 1 for the plain transform, 2^-9 for the key image so that the
// inverse transform's 1/512 is already in the products (bit-identical to scaling at the end)
__global__ __launch_bounds__(256) void k_fft_fwd_polys(const int32_t *__restrict__ polys,
                                                        double *__restrict__ specs, size_t count,
                                                        const d2 *__restrict__ g_tw,
                                                        const d2 *__restrict__ g_twist, double scale)
{
    __shared__ d2 s_tw[kTwEntries];
    __shared__ d2 s_scr[4][kScr];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    for (int i = tid; i < kTwEntries; i += 256) s_tw[i] = g_tw[i];
    (void)g_twist;
    __syncthreads();
    size_t poly = (size_t)blockIdx.x * 4 + w;
    if (poly >= count) return;
    const int32_t *p = polys + poly * kN;
    d2 x[8];
#pragma unroll
    for (int r = 0; r < 4; r++) { // full-range torus inputs: the integer sums are formed in binary64 (exact, < 2^33)
        int j = lane + 64 * r;
        double a = (double)p[j], b = (double)p[j + kNH], pp = (double)p[j + 256], q = (double)p[j + 256 + kNH];
        fwd_stage0(x[r], x[r + 4], a, b, pp - q, pp + q);
    }
    fwd_pass0_tail(x);
    fft_fwd_rest(x, s_tw, s_scr[w], lane);
    d2 *o = reinterpret_cast<d2 *>(specs) + poly * kNH;
#pragma unroll
    for (int r = 0; r < 8; r++) o[r * 64 + lane] = x[r] * scale;
}

__global__ __launch_bounds__(256) void k_fft_inv_polys(const double *__restrict__ specs,
                                                        int32_t *__restrict__ polys, size_t count,
                                                        const d2 *__restrict__ g_tw,
                                                        const d2 *__restrict__ g_twist)
{
    __shared__ d2 s_tw[kTwEntries];
    __shared__ d2 s_twist[kNH];
    __shared__ d2 s_scr[4][kScr];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    load_tables(s_tw, s_twist, g_tw, g_twist, tid, 256);
    __syncthreads();
    size_t poly = (size_t)blockIdx.x * 4 + w;
    if (poly >= count) return;
    const d2 *in = reinterpret_cast<const d2 *>(specs) + poly * kNH;
    d2 x[8];
#pragma unroll
    for (int r = 0; r < 8; r++) x[r] = in[r * 64 + lane];
    d2 ut[8];
    fft_inv_wave(x, ut, s_tw, s_twist, s_scr[w], lane);
    int32_t *p = polys + poly * kN;
#pragma unroll
    for (int r = 0; r < 8; r++) {
        int j = lane + 64 * r;
        d2 y = cmulc(x[r], ut[r] * 0x1p-9);
        p[j] = (int32_t)wrap_trunc(y.x);
        p[j + kNH] = (int32_t)wrap_trunc(y.y);
    }
}

// =================================================================================================
// K1: gate linear stage + mod-switch.   t = (0,cst) + s0*in0 + s1*in1  ->  bara/barb in [0, 2N)
// =================================================================================================
struct GateDesc {
    int32_t op;        // eoc_op, or OP_RAW
    uint32_t job_base; // first blind-rotate job of this gate (jobs are [variant][instance])
    const int32_t *in0, *in1, *in2;
    int32_t *out;
};
constexpr int OP_MUX = 10, OP_NOT = 11, OP_COPY = 12, OP_CONST0 = 13, OP_CONST1 = 14, OP_RAW = 100;
// extension gates (include/eoc_tfhe_gpu.h): one bootstrap behind a linear stage over THREE operands (in0, in1, in2).  Their
// rotation amounts come from k_prepare (a launch of its own): the blind rotation's folded prologue stays the two-operand
// code it was, so the hot kernels' ISA does not change for them
constexpr int OP_MAJ = 15, OP_XOR3 = 16;
__device__ __forceinline__ int gate_lin3(int op) { return op == OP_MAJ ? 1 : (op == OP_XOR3 ? -2 : 0); } // sign of ALL three
// OP_MULTI (internal, mixed batches): one gate descriptor over rows of DIFFERENT two-input opcodes (0..9) -- only the
// linear stage differs between them, so the whole opcode-sorted block runs as one level (full launches instead of one
// partly filled launch per opcode).  `in2` then points at one 32-bit word per row whose top four bits are the row's
// opcode (the gather permutation: original index | op << 28).
constexpr int OP_MULTI = 101;
constexpr uint32_t kPermIndexMask = 0x0FFFFFFFu;
// the opcode field above the mask is 4 bits wide: the host stores opcodes 0..9 there (the only ones OP_MULTI rows can have)
static_assert(OP_MUX - 1 <= (~kPermIndexMask >> 28), "two-input opcodes must fit the permutation's opcode field");
__device__ __forceinline__ int desc_op(const GateDesc &d, uint32_t inst)
{
    return d.op == OP_MULTI ? (int)(reinterpret_cast<const uint32_t *>(d.in2)[inst] >> 28) : d.op;
}

__device__ __forceinline__ void gate_lin(int op, int &cst8, int &s0, int &s1)
{
    // (cst in eighths, s0, s1) -- SURVEY.md 8a a1
    switch (op) {
    case 0: cst8 = 1; s0 = -1; s1 = -1; break;  // NAND
    case 1: cst8 = -1; s0 = 1; s1 = 1; break;   // AND
    case 2: cst8 = 1; s0 = 1; s1 = 1; break;    // OR
    case 3: cst8 = -1; s0 = -1; s1 = -1; break; // NOR
    case 4: cst8 = 2; s0 = 2; s1 = 2; break;    // XOR
    case 5: cst8 = -2; s0 = -2; s1 = -2; break; // XNOR
    case 6: cst8 = -1; s0 = -1; s1 = 1; break;  // ANDNY
    case 7: cst8 = -1; s0 = 1; s1 = -1; break;  // ANDYN
    case 8: cst8 = 1; s0 = -1; s1 = 1; break;   // ORNY
    case 9: cst8 = 1; s0 = 1; s1 = -1; break;   // ORYN
    default: cst8 = 0; s0 = 1; s1 = 0; break;   // RAW: t = in0
    }
}

// grid: x = jobs of the widest gate (S or 2S; the large dimension goes on x), y = ceil((n+1)/256),
//       z = gates of this level
__global__ __launch_bounds__(256) void k_prepare(const GateDesc *__restrict__ descs, int n, uint32_t S,
                                                 uint16_t *__restrict__ bara, int bara_stride)
{
    const GateDesc d = descs[blockIdx.z];
    const uint32_t y = blockIdx.x;
    const uint32_t variant = y / S, s = y - variant * S;
    if (variant >= (d.op == OP_MUX ? 2u : 1u)) return;
    const int m = blockIdx.y * 256 + threadIdx.x;
    if (m > n) return;
    int op = desc_op(d, s);
    const int32_t *a = d.in0, *b = d.in1;
    if (d.op == OP_MUX) { // u1 = AND(a,b), u2 = ANDNY(a,c)
        op = variant ? 6 : 1;
        b = variant ? d.in2 : d.in1;
    }
    int cst8, s0, s1;
    gate_lin(op, cst8, s0, s1);
    const size_t off = (size_t)s * (n + 1) + m;
    uint32_t t;
    if (const int s3 = gate_lin3(op)) // MAJ: a + b + c; XOR3: -2 (a + b + c); no constant
        t = (uint32_t)s3 * ((uint32_t)a[off] + (uint32_t)b[off] + (uint32_t)d.in2[off]);
    else {
        t = (uint32_t)s0 * (uint32_t)a[off];
        if (s1) t += (uint32_t)s1 * (uint32_t)b[off];
        if (m == n) t += (uint32_t)cst8 << 29;
    }
    // modSwitchFromTorus32(t, 2N), N = 1024: round(t * 2048 / 2^32) mod 2048
    bara[(size_t)(d.job_base + y) * bara_stride + m] = (uint16_t)(((t + (1u << 20)) >> 21) & 2047u);
}

// Many-LUT levels: modSwitchFromTorus32 rounded to the grid of T = 2^theta, every word of the OP_RAW row
// in0[s] -> a multiple of T in [0, 2N): ((t + 2^(20 + theta)) >> (21 + theta)) << theta.  theta = 0 is k_prepare's rounding.
// A kernel of its own: k_prepare runs in every gate level and stays as it is.  grid: x = S, y = ceil((n+1)/256), z = tables
__global__ __launch_bounds__(256) void k_modswitch_coarse(const GateDesc *__restrict__ descs, int n, int theta,
                                                          uint16_t *__restrict__ bara, int bara_stride)
{
    const GateDesc d = descs[blockIdx.z];
    const uint32_t s = blockIdx.x;
    const int m = blockIdx.y * 256 + threadIdx.x;
    if (m > n) return;
    const uint32_t t = (uint32_t)d.in0[(size_t)s * (n + 1) + m];
    bara[(size_t)(d.job_base + s) * bara_stride + m] = (uint16_t)((((t + (1u << (20 + theta))) >> (21 + theta)) << theta) & 2047u);
}

// Integer circuits: the linear stage of a netlist node, t = sum_k w[k] in[k][s] + (0, ..., 0, cst) in wrapping
// int32, over up to four operand rows -- GateDesc has no room for weights and keeps its 40 bytes, so the nodes travel as
// descriptors of their own (two GateDesc slots of the descriptor ring each).  BOOT: the mod switch onto the 2^theta-grid
// behind it (k_modswitch_coarse's rounding; theta = 0 is k_prepare's) -> the node's rows of rotation amounts; otherwise a
// free node, out[s] = t.  MAXT = the largest term count among the launch's nodes: the operand loop is unrolled to it and a
// node issues one load per term it has (the count is uniform over the workgroup).  Kernels of their own: k_prepare and
// k_modswitch_coarse run in shipped paths and stay as they are.  grid: x = rows, y = ceil((n+1)/256), z = nodes
struct LinDesc {
    const int32_t *in[4]; // operand rows (row 0 of the launch's slice)
    int32_t w[4];
    int32_t cst;          // Torus32, added to word n (b)
    uint32_t job_base;    // BOOT: first blind-rotate job of the node (jobs are [node][row])
    int32_t *out;         // free node: output rows
    int32_t theta;        // BOOT: T = 2^theta tables
    int32_t n_terms;      // 1 .. 4
    int32_t pad[2];
};
static_assert(sizeof(LinDesc) == 2 * sizeof(GateDesc), "a LinDesc takes two slots of the descriptor ring");
template <int MAXT, bool BOOT>
__global__ __launch_bounds__(256) void k_lin_modswitch(const LinDesc *__restrict__ descs, int n, uint16_t *__restrict__ bara,
                                                       int bara_stride)
{
    const LinDesc &d = descs[blockIdx.z];
    const uint32_t s = blockIdx.x;
    const int m = blockIdx.y * 256 + threadIdx.x;
    if (m > n) return;
    const size_t off = (size_t)s * (n + 1) + m;
    const int nt = d.n_terms;
    uint32_t t = (uint32_t)d.w[0] * (uint32_t)d.in[0][off];
#pragma unroll
    for (int k = 1; k < MAXT; k++)
        if (k < nt) t += (uint32_t)d.w[k] * (uint32_t)d.in[k][off];
    if (m == n) t += (uint32_t)d.cst;
    if constexpr (BOOT) {
        const int theta = d.theta;
        bara[(size_t)(d.job_base + s) * bara_stride + m] = (uint16_t)((((t + (1u << (20 + theta))) >> (21 + theta)) << theta) & 2047u);
    } else d.out[off] = (int32_t)t;
}

// The _tv and many-LUT kernels map job j to polynomial (job0 + j) / rows of ONE contiguous array: the polynomials of an
// integer circuit's nodes are copied into level order, once per call.  grid: x = nodes; idx[node] = row of `tv`
__global__ __launch_bounds__(256) void k_tv_gather(const int32_t *__restrict__ tv, const int32_t *__restrict__ idx,
                                                   int32_t *__restrict__ staged)
{
    const int32_t *src = tv + (size_t)idx[blockIdx.x] * kN;
    int32_t *dst = staged + (size_t)blockIdx.x * kN;
#pragma unroll
    for (int j = 0; j < kN / 256; j++) dst[threadIdx.x + 256 * j] = src[threadIdx.x + 256 * j];
}

// The folded prologue writes the job's row of rotation amounts with vector stores; the step loop reads it back.
// SHIPPED FORM (SABAR = false): behind the workgroup barrier the row is copied ONCE into LDS (vector loads: writer and
// reader share the CU's vector L1 and the barrier carries a workgroup-scope release / acquire -- inside the formal memory
// model) and every step reads its amount with one ds_read_u16 of a wave-uniform address + v_readfirstlane.  VERDICT r5 asked
// for vector loads + v_readfirstlane in the loop (measured in round 5: +0.3 % Set A / +0.6 % Set B); that form keeps the
// loaded word and its address in VGPRs across a step, which the 256-register kernels do not have (the run-time-base gadget-
// length-3 instance spilled 16 registers, the wide kernel up to 40); the LDS copy needs neither (register counts equal to
// the scalar form's) and puts one extra LDS read per step on a pipe that serves ~250.
// SCALAR FORM (SABAR = true, EOC_TFHE_SCALAR_ABAR=1): scalar loads through the constant address space.  The scalar cache is
// not coherent with vector stores: the vector L1 is write-through, a store is complete -- vmcnt decremented -- when this
// XCD's L2 has it; the scalar cache fills from that same L2 and is emptied by s_dcache_inv behind the barrier.  So:
// compiler-level release fence, an explicit s_waitcnt vmcnt(0) (a workgroup-scope fence alone emits none outside
// threadgroup-split mode), the workgroup barrier, s_dcache_inv, and s_waitcnt lgkmcnt(0) so that no later s_load can be
// issued past the invalidate (scalar memory operations may complete out of order).  Rows are bara_stride =
// a multiple of 32 entries = 64 bytes apart, so two jobs never share a scalar-cache line.  An agent-scope release would
// also be correct but emits buffer_wbl2 -- an L2 write-back per workgroup (+18 us per 1024-job launch).  This form relies
// on cache behaviour outside the memory model; it is kept as a measured alternative, not the default.
// EOC_TFHE_NO_FOLD=1 restores the separate k_prepare launch (a kernel boundary orders everything) for either form.
__device__ __forceinline__ void eoc_row_stores_to_l2()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}
// scalar form only, behind the workgroup barrier: drop the scalar cache's (possibly stale) lines and let nothing pass
__device__ __forceinline__ void eoc_scalar_cache_acquire()
{
    __builtin_amdgcn_s_dcache_inv();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
}

// the same for ONE job inside the blind rotation (levels without MUX): thread `t` of `nt` writes entries t, t + nt, ... of
// the job's row; the caller orders the stores before its loads of the row (the workgroup barrier; the scalar form adds
// eoc_row_stores_to_l2 in front of it and eoc_scalar_cache_acquire behind it)
__device__ __forceinline__ void prepare_row(const GateDesc &d, uint32_t inst, int n, uint16_t *row, int t, int nt)
{
    int cst8, s0, s1;
    gate_lin(desc_op(d, inst), cst8, s0, s1);
    typedef const __attribute__((address_space(1))) int32_t *gi32p; // operand rows are global memory (device or mapped host)
    const gi32p a = (gi32p)(uintptr_t)(d.in0 + (size_t)inst * (n + 1));
    const gi32p b = s1 ? (gi32p)(uintptr_t)(d.in1 + (size_t)inst * (n + 1)) : a; // one-operand forms carry no second row
    for (int m = t; m <= n; m += nt) {
        uint32_t v = (uint32_t)s0 * (uint32_t)a[m];
        if (s1) v += (uint32_t)s1 * (uint32_t)b[m];
        if (m == n) v += (uint32_t)cst8 << 29;
        row[m] = (uint16_t)(((v + (1u << 20)) >> 21) & 2047u);
    }
}

// NOT / COPY: no bootstrap.  grid: x = ceil(S*(n+1)/256), y = gates
__global__ __launch_bounds__(256) void k_free_gates(const GateDesc *__restrict__ descs, size_t total, int rowlen, int32_t mu)
{
    const GateDesc d = descs[blockIdx.y];
    size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    if (d.op >= OP_CONST0) { // bootsCONSTANT: (0, ..., 0, +-mu), no input
        const bool is_b = (int)(i % (size_t)rowlen) == rowlen - 1;
        d.out[i] = is_b ? (d.op == OP_CONST1 ? mu : (int32_t)(0u - (uint32_t)mu)) : 0;
        return;
    }
    uint32_t v = (uint32_t)d.in0[i];
    d.out[i] = (int32_t)(d.op == OP_NOT ? 0u - v : v);
}


// mixed batches in arbitrary opcode order: rows are gathered into opcode-sorted order, evaluated run by
// run, and scattered back.  perm[i] = original index of the i-th gate in sorted order.
// grid: x = rows, y = ceil(rowlen / 256)
__global__ __launch_bounds__(256) void k_gather_rows(const int32_t *__restrict__ src, int32_t *__restrict__ dst,
                                                     const uint32_t *__restrict__ perm, int rowlen, int scatter)
{
    const int m = blockIdx.y * 256 + threadIdx.x;
    if (m >= rowlen) return;
    const size_t i = blockIdx.x, j = perm[i] & kPermIndexMask; // the top four bits carry the row's opcode (OP_MULTI)
    if (scatter) dst[j * rowlen + m] = src[i * rowlen + m];
    else dst[i * rowlen + m] = src[j * rowlen + m];
}


// Wave-priority alternation between the two waves sharing a SIMD (see the step loop): one step per phase, the
// later-placed wave holds the high priority kPrioDuty sixteenths of the steps.  The host enables it per launch
// (BRArgs::prio_duty).  Everything that was measured and rejected on this kernel is recorded in DESIGN.md 5.1; the
// timing-only ablations are patches under tools/patches/ (tools/variants.sh applies them to a scratch copy).
constexpr int kPrioDuty = 11;

// In-kernel stamps (diagnostic build only, -DEOC_STAMPS): per-wave cycle shares of the step's
// segments.  Never enabled in the shipped library; the values leave through a buffer of their own.
#ifdef EOC_STAMPS
#define EOC_STAMP(k)                                                                      \
    do {                                                                                  \
        __builtin_amdgcn_sched_barrier(0);                                                \
        unsigned long long _t;                                                            \
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(_t)::"memory");       \
        __builtin_amdgcn_sched_barrier(0);                                                \
        st_acc[k] += _t - st_prev;                                                        \
        st_prev = _t;                                                                     \
    } while (0)
#else
#define EOC_STAMP(k) do { } while (0)
#endif

// =================================================================================================
// K2: blind rotate + sample extract.  One workgroup = ONE ciphertext = a wave pair (h = 0,1), four workgroups per
// CU (35.6 KB of LDS each), so that s_barrier couples only the two waves that exchange data (with two ciphertexts per
// workgroup the barriers cost 6 % of the launch).  Wave h owns accumulator polynomial h, decomposes it, runs the l forward
// transforms of its digits, multiplies them by rows (h, p) of BK_i for the OTHER output polynomial and hands
// that partial chain to its partner through LDS; it then continues the chain it received from the partner with
// its own digits (rows (h, p), output polynomial h), runs the inverse transform of the sum and updates ACC_h.
// Accumulation order of output polynomial c (canonical, oracle/tfhe_oracle.c): terms (q_in = 1 - c, p = 1..l)
// first, then (q_in = c, p = 1..l); first term a product, every later one four fused multiply-adds.
// =================================================================================================
struct BRArgs {
    const double *bkfft;  // [n][2l][2][512] complex, bin order sigma, scaled by 2^-9
    uint16_t *bara;       // [jobs][stride], entry n = barb (written by k_prepare, or by this kernel's prologue: `prep`)
    int32_t *u;           // [jobs][N+1]
    uint32_t njobs;
    int n, Bgbit, bara_stride;
    int32_t mu;
    unsigned long long *stamps; // diagnostic build only: [waves][16] cycle sums per segment
    int prio_duty;              // < 0: leave wave priorities alone; else see the loop (single-round launches)
    // folded key-switch set-up (levels without MUX): the epilogue writes the key-switch operand and the output row
    // itself, k_ks_init is not launched and the extracted sample never goes to memory
    const GateDesc *ks_descs;   // non-null = fold; gate of job j is j / ks_S (jobs are [gate][instance])
    GateDesc desc0;             // single-gate levels (the plain batch call): the descriptor travels as a kernel argument,
    int inline_desc;            // `ks_descs` is then a non-null dummy and no descriptor copy precedes the launch
    int prep;                   // fold only: the prologue derives the job's rotation amounts from the gate's operand rows
                                // itself (bootsNAND... linear stage + modSwitchFromTorus32), k_prepare is not launched
    uint32_t *ubar;             // [jobs][N], row-major: the epilogue's stores are lane-contiguous (256 B per instruction)
    uint32_t ks_S, ks_prec_offset, job0; // job0: first job of this launch within the level
    // step range of this launch: the n steps of a blind rotation may be cut into consecutive launches; every boundary
    // brings all workgroups of the chip back to the same step (the accumulator travels through `acc_state`)
    int step_begin, step_end;
    int32_t *acc_state;         // [jobs][2][N], only used when the range is a proper part of [0, n)
};

// LDS: the two tables (not loaded by the gadget-length-2 instances, which keep their values in registers; the layout and
// the four workgroups per CU are the same for all) + one 9 KB scratch per wave.  The accumulator lives in registers (racc[16]); the scratch holds it
// as a signed 2N-periodic image ext[k] = ACC[k], ext[k + N] = -ACC[k] (8 KB) only for the sample extraction after the
// last step, which reads it by index.
// (X^abar - 1) * ACC without an accumulator image: coefficient lane + 64 r of ACC lives in racc[r];
// entry k of the signed 2N-periodic extension, k = lane' + 64 r' (r' < 32), is +racc[r'] (r' < 16) or -racc[r' - 16] of
// lane lane'.  Entry (lane + 64 r) - abar with abar = 64 Q + s is lane (lane - s) mod 64, register r - Q - (lane < s):
// one ds_bpermute_b32 per register moves the lanes, the register shift Q is wave-uniform and selects one of 32
// compile-time renamings of the block below.
template <int Q>
__device__ __forceinline__ void rot_digits(const uint32_t (&t)[16], const uint32_t (&racc)[16], bool borrow, uint32_t offset,
                                           uint32_t (&d)[16])
{
#pragma unroll
    for (int r = 0; r < 16; r++) {
        const int k0 = (r - Q) & 31, k1 = (r - Q - 1) & 31;
        const uint32_t a0 = t[k0 & 15], a1 = t[k1 & 15];
        const uint32_t A = offset - racc[r];
        const bool n0 = k0 >= 16, n1 = k1 >= 16;
        if (n0 == n1) {
            const uint32_t w = borrow ? a1 : a0;
            d[r] = n0 ? A - w : A + w;
        } else {
            const uint32_t d0 = n0 ? A - a0 : A + a0, d1 = n1 ? A - a1 : A + a1;
            d[r] = borrow ? d1 : d0;
        }
    }
}
constexpr int kAbarLds = 2048;                                  // one job's rotation amounts (n + 1 <= 1024 entries of 16 bits)
constexpr int kBRLds = (kTwEntries + kNH + 2 * kScr) * 16 + kAbarLds; // 37 632 bytes: four workgroups per CU

// BGBIT > 0: gadget base known at compile time (digit extraction becomes one bit-field extract); 0: run time.
// Register budget (hipcc 7.2, -Rpass-analysis=kernel-resource-usage): <2,10> 252 VGPRs, <3,7> 256, <1> 162, <2> 256, <3> 256,
// none of them spills.  Gadget length 2 holds ALL loop-invariant table values in registers (96: four twiddle sets and the
// eight un-twist factors) and reads no table in the step loop; what pays for them is that no whole key row is ever live
// there: the rows are streamed through the chains bin block by bin block, three blocks (24 registers) ahead, and the
// partner's chain leaves for the scratch block by block (blind_rotate_pair.inc).  Its earlier form is k_br_lds* below.  Gadget length 4 (no default parameter set uses it) is a SLOW CORRECTNESS PATH: four live spectra
// exceed the 256 registers of a wave at two waves per SIMD, its kernel spills (324 VGPRs to scratch) and runs several
// times slower per transform; it is bit-exact (tests/test_gpu_parity.py) and nothing else is claimed for it.

// Two kernel names share one body (blind_rotate_pair.inc, included into each so that it is compiled as the kernel's own
// code).  What is known about sharing code between these kernels, measured with tools/isa_diff.py on the assembly of every
// instance against the parent commit's:
//   * the whole body moved into a __device__ function compiled to different code for the gate kernels; the L-generic
//     external product as a force-inlined function template (row loader passed by value or by reference) changed
//     k_blind_rotate<3,7> in 249 lines (SGPRs 89 -> 87), k_br_lds<2,10> in 57, k_cmux<2,10> in 950 and k_cmux<3,7> in 300.
//     The same texts as includes (blind_rotate_pair.inc, blind_rotate_wide.inc, ext_product_pair.inc) change none of them;
//   * the small force-inlined helpers Gadget, digit_pass, cmul0 / cmac1 / cmac8 leave every instance of a default
//     parameter set byte-identical, provided a compile-time gadget base is named as a constant inside digit_pass
//     (Gadget<BGBIT>), as the kernel's text named it: read from the struct, k_blind_rotate_wide<10> changed in 64 lines;
//   * the measured exceptions: the rotation block (16 ds_bpermute + the 32-way rot_digits switch) as a function renames
//     registers in k_blind_rotate<2,10> and changes the length of twenty other instances, and the three-line sum of the
//     gadget offset as a helper inverts the step loop's entry test (see Gadget).  Both stay in the kernels' text;
//   * the leveled kernels' frame (k_cmux, k_demux, k_automaton_step: LDS carve, wave roles, the dead pair's rule, gadget,
//     row loader, product) as a struct returned by a force-inlined function, the row loader a function template called from
//     the lambda, tried on k_demux alone: the 125 other kernels identical, all six k_demux instances changed in 26 to 184
//     lines (equal metadata, length within 3 instructions).  As included text (leveled_pair.inc) all eighteen are identical
//     -- in the order the kernels had it: the same lines with the gadget's sum ahead of the kernel's operand pointers, so
//     that two parts would do instead of three, changed all eighteen in 42 to 365 lines.  Of the small pieces, the row
//     loader (load_selector_row) and the store phases' cmulc + wrap_trunc pair (leveled_words) change nothing as
//     force-inlined functions; the negacyclic gather does (EOC_NEGACYCLIC, a macro);
//   * the three leveled kernels' whole texts as included text (leveled_kernels.inc, included twice each: the truncating
//     kernel and its rounding twin): all eighteen shipped instances and the 120 other kernels identical;
//   * kernels are compared modulo the function's number in the code object (tools/isa_diff.py drops it from the block
//     labels): a new kernel may be plain and may stand where it belongs, here and in engine.hip.
// The body's constant TV selects the accumulator: false = the gate test vector (mu, ..., mu),
// true = a test polynomial per job.  The gate kernel's name, template arguments and argument list are what
// tests/test_isa_guard.py and the profiles look up and what the shipped code was measured as: they do not change.
template <int L, int BGBIT = 0, bool SABAR = false>
__global__ __launch_bounds__(128, 2) void k_blind_rotate(BRArgs A, const d2 *__restrict__ g_tw,
                                                         const d2 *__restrict__ g_twist)
{
    constexpr bool TV = false, MANY = false, TLDS = false, ENC = false;
    const int32_t *const tv = nullptr;
    const uint32_t tv_rows = 1, n_tables = 1;
#include "blind_rotate_pair.inc"
}
// Programmable bootstrapping: job j starts from test polynomial tv[(job0 + j) / tv_rows] ([tables][N] int32), read once
// in the prologue; the step loop and the epilogue are the gate kernel's.
template <int L, int BGBIT = 0, bool SABAR = false>
__global__ __launch_bounds__(128, 2) void k_blind_rotate_tv(BRArgs A, const d2 *__restrict__ g_tw,
                                                            const d2 *__restrict__ g_twist, const int32_t *__restrict__ tv,
                                                            uint32_t tv_rows)
{
    constexpr bool TV = true, MANY = false, TLDS = false, ENC = false;
    const uint32_t n_tables = 1;
#include "blind_rotate_pair.inc"
}
// Many-LUT bootstrapping: the _tv kernel's prologue and step loop on rotation amounts of the T-grid
// (k_modswitch_coarse), and n_tables = T sample extractions at indices 0 .. T - 1 of the one accumulator instead of one:
// slot j of job (table g, row s) is workspace row (g T + j) tv_rows + s, which the key switch reads as n_luts x T
// descriptors.  No folded key-switch set-up (ks_descs must be null).  The name avoids "k_blind_rotate": the ISA tests
// count the kernels of that name.
template <int L, int BGBIT = 0, bool SABAR = false>
__global__ __launch_bounds__(128, 2) void k_lut_many(BRArgs A, const d2 *__restrict__ g_tw, const d2 *__restrict__ g_twist,
                                                     const int32_t *__restrict__ tv, uint32_t tv_rows, uint32_t n_tables)
{
    constexpr bool TV = true, MANY = true, TLDS = false, ENC = false;
#include "blind_rotate_pair.inc"
}
// Blind rotation from an ENCRYPTED polynomial: job j starts from ACC = X^(2N - barb) (c0, c1), (c0, c1) the
// TLWE list tv[(job0 + j) / tv_rows] ([lists][2][N] int32, the layout of the packing key switch); wave h seeds polynomial
// h.  Step loop and epilogue are the _tv kernel's.  The name avoids "k_blind_rotate" and "k_lut_many" (the ISA tests count
// those); this family has no earlier-form twin.
template <int L, int BGBIT = 0, bool SABAR = false>
__global__ __launch_bounds__(128, 2) void k_br_enc(BRArgs A, const d2 *__restrict__ g_tw, const d2 *__restrict__ g_twist,
                                                   const int32_t *__restrict__ tv, uint32_t tv_rows)
{
    constexpr bool TV = true, MANY = false, TLDS = false, ENC = true;
    const uint32_t n_tables = 1;
#include "blind_rotate_pair.inc"
}

// The three families once more for gadget length 2 in their EARLIER form (TLDS: three of the five loop-invariant table
// sets are read from LDS in every step, whole key rows are requested at the top of the step), kept for comparisons inside
// one build: EOC_TFHE_BR_TABLES_LDS=1 selects them.  The names avoid "k_blind_rotate" and "k_lut_many": the ISA tests
// count the kernels of those names.
template <int L, int BGBIT = 0, bool SABAR = false>
__global__ __launch_bounds__(128, 2) void k_br_lds(BRArgs A, const d2 *__restrict__ g_tw, const d2 *__restrict__ g_twist)
{
    constexpr bool TV = false, MANY = false, TLDS = true, ENC = false;
    const int32_t *const tv = nullptr;
    const uint32_t tv_rows = 1, n_tables = 1;
#include "blind_rotate_pair.inc"
}
template <int L, int BGBIT = 0, bool SABAR = false>
__global__ __launch_bounds__(128, 2) void k_br_lds_tv(BRArgs A, const d2 *__restrict__ g_tw, const d2 *__restrict__ g_twist,
                                                      const int32_t *__restrict__ tv, uint32_t tv_rows)
{
    constexpr bool TV = true, MANY = false, TLDS = true, ENC = false;
    const uint32_t n_tables = 1;
#include "blind_rotate_pair.inc"
}
template <int L, int BGBIT = 0, bool SABAR = false>
__global__ __launch_bounds__(128, 2) void k_br_lds_many(BRArgs A, const d2 *__restrict__ g_tw, const d2 *__restrict__ g_twist,
                                                        const int32_t *__restrict__ tv, uint32_t tv_rows, uint32_t n_tables)
{
    constexpr bool TV = true, MANY = true, TLDS = true, ENC = false;
#include "blind_rotate_pair.inc"
}

// =================================================================================================
// K2w: blind rotate + sample extract, WIDE form (gadget length 2): ONE WAVE = ONE CIPHERTEXT.  For launches of at
// least twice the pair kernel's resident set, two waves per SIMD can come from two ciphertexts instead of one wave
// pair: the wave owns both accumulator polynomials, runs the four forward transforms of a step as two skewed pairs and
// the two inverse transforms as a third, and needs no partner -- no exchange of partial chains through LDS (16 of 112
// ds_write_b128 and 16 of 144 ds_read_b128 per ciphertext-step), no s_barrier in the step loop, no wait for a partner on
// another SIMD (timing-only ablation on the pair kernel, tools/patches/abl_noexchange.patch: -14 %).
// Results are bit-identical to k_blind_rotate: the same transforms, and the accumulation of output polynomial c runs
// in the canonical order (oracle/tfhe_oracle.c) -- terms (q_in = 1 - c, p = 1, 2) first, then (q_in = c, p = 1, 2) --
// which needs all four spectra live when the chains start (128 registers): the key rows are therefore streamed bin
// block by bin block (r = 0..7: eight 16-byte loads, one per row, then the eight chain steps of that block), so that
// a chain value replaces two spectrum values as the loop advances.  Gadget length 3 would need six live spectra and
// stays on the pair kernel.
// Workgroup = two independent ciphertexts (128 threads, the pair kernel's 35.6 KB of LDS: tables + one scratch per wave).
// =================================================================================================
// two inverse transforms skewed on one scratch (a's transposes under b's register passes and vice versa); the un-twist
// factors are read once for both.  Arithmetic per transform identical to fft_inv_wave.
__device__ __forceinline__ void fft_inv_x2(d2 (&xa)[8], d2 (&xb)[8], d2 (&ut)[8], const d2 *tw, const d2 *s_twist, d2 *scr,
                                           int lane)
{
    d2 t1[4], t0[4];
    const int hi = lane >> 3, lo = lane & 7;
    EOC_SB();
    tw_load(t1, tw + kTwI1 + (lane & 7), 8);
    inv_pass2(xa);
    EOC_SB();
    // region B: register-constant pass of b, a's first transpose spread through it
#pragma unroll
    for (int r = 0; r < 8; r++) scr[f12(lane * 8 + r)] = xa[r];
    wave_lds_fence();
    inv_pass2(xb);
    t21_read(xa, scr, lane);
#pragma unroll
    for (int k = 0; k < 8; k++) {
        EOC_SGB(EOC_M_DSW, 1);
        EOC_SGB(EOC_M_VALU, 5);
    }
    EOC_SGB(EOC_M_VALU, 16);
    EOC_SGB(EOC_M_DSR, 8);
    EOC_SB();
    // region C: middle pass of a, b's first transpose spread through it; then b's reads and the last twiddle set
#pragma unroll
    for (int r = 0; r < 8; r++) scr[f12(lane * 8 + r)] = xb[r];
    wave_lds_fence();
    t21_read(xb, scr, lane);
    tw_load(t0, tw + kTwI0 + lane, 64);
    wave_lds_fence();
    inv_pass10(xa, t1);
#pragma unroll
    for (int k = 0; k < 8; k++) {
        EOC_SGB(EOC_M_DSW, 1);
        EOC_SGB(EOC_M_VALU, 4);
    }
    EOC_SGB(EOC_M_DSR, 12);
    EOC_SGB(EOC_M_VALU, 40);
    EOC_SB();
    // region D: middle pass of b under a's second transpose
#pragma unroll
    for (int r = 0; r < 8; r++) scr[72 * hi + 8 * r + lo] = xa[r];
    wave_lds_fence();
    t10_read(xa, scr, lane);
    inv_pass10(xb, t1);
#pragma unroll
    for (int k = 0; k < 8; k++) {
        EOC_SGB(EOC_M_DSW, 1);
        EOC_SGB(EOC_M_VALU, 4);
    }
    EOC_SGB(EOC_M_DSR, 8);
    EOC_SGB(EOC_M_VALU, 40);
    EOC_SB();
    // region E: last pass of a under b's second transpose; the un-twist factors
#pragma unroll
    for (int r = 0; r < 8; r++) scr[72 * hi + 8 * r + lo] = xb[r];
    wave_lds_fence();
    t10_read(xb, scr, lane);
#pragma unroll
    for (int r = 0; r < 8; r++) ut[r] = s_twist[lane + 64 * r];
    wave_lds_fence();
    inv_pass10(xa, t0);
#pragma unroll
    for (int k = 0; k < 8; k++) {
        EOC_SGB(EOC_M_DSW, 1);
        EOC_SGB(EOC_M_VALU, 4);
    }
    EOC_SGB(EOC_M_DSR, 16);
    EOC_SGB(EOC_M_VALU, 40);
    EOC_SB();
    inv_pass10(xb, t0);
}

constexpr int kBRWideJobsPerWG = 2;
constexpr int kBRWideLds = (kTwEntries + kNH + kBRWideJobsPerWG * kScr) * 16 + kBRWideJobsPerWG * kAbarLds;


// the two kernel names over one body (blind_rotate_wide.inc), as for the pair kernel
template <int BGBIT = 0, bool SABAR = false>
__global__ __launch_bounds__(64 * kBRWideJobsPerWG, 2) void k_blind_rotate_wide(BRArgs A, const d2 *__restrict__ g_tw,
                                                              const d2 *__restrict__ g_twist)
{
    constexpr bool TV = false, MANY = false, ENC = false;
    const int32_t *const tv = nullptr;
    const uint32_t tv_rows = 1, n_tables = 1;
#include "blind_rotate_wide.inc"
}
template <int BGBIT = 0, bool SABAR = false>
__global__ __launch_bounds__(64 * kBRWideJobsPerWG, 2) void k_blind_rotate_wide_tv(BRArgs A, const d2 *__restrict__ g_tw,
                                                                 const d2 *__restrict__ g_twist,
                                                                 const int32_t *__restrict__ tv, uint32_t tv_rows)
{
    constexpr bool TV = true, MANY = false, ENC = false;
    const uint32_t n_tables = 1;
#include "blind_rotate_wide.inc"
}
// the many-LUT twin of the wide kernel (see k_lut_many)
template <int BGBIT = 0, bool SABAR = false>
__global__ __launch_bounds__(64 * kBRWideJobsPerWG, 2) void k_lut_many_wide(BRArgs A, const d2 *__restrict__ g_tw,
                                                                            const d2 *__restrict__ g_twist,
                                                                            const int32_t *__restrict__ tv, uint32_t tv_rows,
                                                                            uint32_t n_tables)
{
    constexpr bool TV = true, MANY = true, ENC = false;
#include "blind_rotate_wide.inc"
}
// the wide twin of k_br_enc: the wave seeds both accumulators from the job's list
template <int BGBIT = 0, bool SABAR = false>
__global__ __launch_bounds__(64 * kBRWideJobsPerWG, 2) void k_br_enc_wide(BRArgs A, const d2 *__restrict__ g_tw,
                                                                          const d2 *__restrict__ g_twist,
                                                                          const int32_t *__restrict__ tv, uint32_t tv_rows)
{
    constexpr bool TV = true, MANY = false, ENC = true;
    const uint32_t n_tables = 1;
#include "blind_rotate_wide.inc"
}

// =================================================================================================
// K3: key switch (lweKeySwitch), two launches.
//   k_ks_init      per ciphertext: ubar[job][i] = u_i + 2^(31 - t*basebit)  (sum of the two extracted
//                  samples + (0, mu) for MUX), out = (0, ..., 0, b')
//   k_keyswitch_waves   basebit 2, even t: 64 ciphertexts per workgroup (one per lane), two digits per LDS look-up
//                  through a table of row sums, partial sums of the i-slices through LDS and a few integer atomics
//   k_keyswitch_generic any other (basebit, t): the plain one-thread-per-output-word form
//   k_keyswitch_mfma    basebit 2, t 8 (both default sets; what launch_keyswitch takes): the same sum as four int8 matrix
//                  products on the matrix cores, from the limb image k_ksk_limbs derives at key install
// KSK device image: [N*t][base-1][n1p], rows padded with zeros to n1p (multiple of 256).
// =================================================================================================
constexpr int KS_GT = 64; // ciphertexts per workgroup (one per lane)

struct KSArgs {
    const int32_t *ksk;
    const int32_t *u;   // [jobs][N+1]
    uint32_t *ubar;     // [jobs][N] row-major
    int n, n1p, t, basebit;
    uint32_t S;
    GateDesc desc0;     // single-gate levels: the descriptor as a kernel argument (see BRArgs)
    int inline_desc;
    int32_t mu;
};

// grid: x = S, y = gates
__global__ __launch_bounds__(256) void k_ks_init(const GateDesc *__restrict__ descs, KSArgs A)
{
    const GateDesc d = A.inline_desc ? A.desc0 : descs[blockIdx.y];
    const uint32_t s = blockIdx.x;
    const uint32_t job = d.job_base + s;
    const int32_t *u1 = A.u + (size_t)job * (kN + 1);
    const bool mux = d.op == OP_MUX;
    const int32_t *u2 = u1 + (size_t)A.S * (kN + 1);
    const uint32_t prec_offset = 1u << (32 - (1 + A.basebit * A.t));
    for (int j = threadIdx.x; j < kN; j += 256) {
        uint32_t v = (uint32_t)u1[j];
        if (mux) v += (uint32_t)u2[j];
        A.ubar[(size_t)job * kN + j] = v + prec_offset;
    }
    int32_t *o = d.out + (size_t)s * (A.n + 1);
    for (int m = threadIdx.x; m < A.n; m += 256) o[m] = 0;
    if (threadIdx.x == 0) {
        uint32_t b = (uint32_t)u1[kN];
        if (mux) b += (uint32_t)u2[kN] + (uint32_t)A.mu;
        o[A.n] = (int32_t)b;
    }
}

typedef int i4 __attribute__((ext_vector_type(4)));

// ---- k_keyswitch_waves<T, NWV, IW>: basebit 2, even t (both default sets) ------------------------------------------
// One lane = one ciphertext.  A workgroup is (tile of 64 ciphertexts) x (ONE block of 64 key columns) x (a slice of
// NWV * IW indices i); its NWV waves split the SLICE: wave w walks IW indices of its own.
//   * Two digits per look-up.  For digits j, j + 1 of index i the wave first combines the 3 + 3 candidate key rows into
//     the table of their 16 sums, S[d1][d2] = row_j[d1] + row_{j+1}[d2] (64 columns, 4.3 KB, double-buffered in LDS;
//     d1 = d2 = 0 is the zero row), built by its own lanes with lane = COLUMN: six coalesced dword loads (exactly the
//     wave's 256-byte strips of the six rows), nine additions, and the fifteen non-zero rows leave through
//     ds_write_addtid_b32 -- the LDS store whose address is M0 + offset + 4 * lane, no address register: a 256-byte row
//     in 2 cycles of the CU's store path against 13.6 for a ds_write_b128 (tools/ubench_addtid.hip pins its addressing:
//     lane within the wave, no 16-bit wrap of the sum, one wait state after the SALU write of M0).
//     Every lane then selects with the 4-bit nibble of its operand word that holds
//     both digits of ITS ciphertext and does ONE look-up and ONE subtraction per column for the pair:
//     acc -= S[nibble]  ==  acc -= row_j[d1]; acc -= row_{j+1}[d2]  in wrapping int32 arithmetic -- bit-identical, at half
//     the subtractions and half the LDS reads per ciphertext of the one-digit form (rows are skewed by 16 B so that the 16
//     table rows cover the 64 banks: lanes with equal nibbles share an address, others never share a bank).
//   * No barrier in the stage loop: the table is the wave's own (a wave's LDS operations execute in order).
//   * The NWV partial sums of a workgroup are added through LDS (tree: the upper half of the waves parks its
//     accumulators, the lower half adds), so only the kN / (NWV IW) = 2...8 slices meet in the output row through integer
//     atomics (exact, order independent), 256 contiguous bytes per atomic instruction.
// History (Set A, 1024 gates): round 3's kernel -- one digit per look-up, the candidate rows of 4 digits staged per
// workgroup barrier, one i-slice x all columns per workgroup, 32 atomics per output word -- took 0.212 ms: integer issue
// and the LDS pipe were loaded exactly alike (4 bytes from LDS per subtraction) and 16.8 M atomics arrived together at the
// end of the kernel (33 us, timing-only ablation).  Pair tables alone: 0.180 ms; with one i-range per wave: 0.133 ms; tables
// built through ds_write_addtid_b32 instead of ds_write_b128: 0.122 ms (Set B: 0.363 -> 0.304 -> 0.196 -> 0.178 ms).  An XCD-aware workgroup order (all tiles of a slice on one XCD) changed nothing:
// the 50 MB key image is served by the Infinity Cache either way.
template <int T, int NWV, int IW>
struct KS3Cfg {
    static constexpr int NT = 64 * NWV;
    static constexpr int ROWI = 64 + 4;                  // table row stride in ints (16-B skew: 16 rows cover the 64 banks)
    static constexpr int TABI = 16 * ROWI;               // one table, ints
    static constexpr int WAVE_I = 2 * TABI;              // two tables per wave
    static constexpr int RED_I = 64 * ROWI;              // one wave's partial sums [64 ciphertexts][64 columns + 4]
    static constexpr int TAB_BYTES = NWV * WAVE_I * 4, RED_BYTES = (NWV > 1 ? NWV / 2 : 1) * RED_I * 4;
    static constexpr int LDS_BYTES = TAB_BYTES > RED_BYTES ? TAB_BYTES : RED_BYTES;
    static constexpr int NPAIR = T / 2;
    static constexpr int NSTAGE = IW * NPAIR;
    static constexpr int SLICE_I = NWV * IW;             // indices i per workgroup
    static constexpr int NS = kN / SLICE_I;              // slices (= atomics per output word)
};

// grid: x = ntiles * (n1p / 64) * NS, y = gates; block = 64 NWV
template <int T, int NWV, int IW>
__global__ __launch_bounds__(64 * NWV, 4) void k_keyswitch_waves(const GateDesc *__restrict__ descs, KSArgs A)
{
    typedef KS3Cfg<T, NWV, IW> C;
    static_assert(T % 2 == 0 && kN % C::SLICE_I == 0 && (NWV & (NWV - 1)) == 0, "shape");
    static_assert((NWV * C::WAVE_I - C::TABI) * 4 < 65536, "ds_write_addtid_b32 takes its base from M0[15:0]");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    int *s_all = reinterpret_cast<int *>(smem);
    // ds_write_addtid_b32 adds M0[15:0]: the static_assert above bounds the largest base ONLY IF the dynamic block starts at
    // LDS offset 0, i.e. the kernel has no static __shared__ object -- trap instead of silently wrapping if that ever changes
    if ((uint32_t)(uintptr_t)smem != 0u) __builtin_trap();

    const GateDesc d = A.inline_desc ? A.desc0 : descs[blockIdx.y];
    const uint32_t ntiles = (A.S + 63) / 64, ncb = (uint32_t)A.n1p / 64u;
    const uint32_t tile = blockIdx.x % ntiles, rest = blockIdx.x / ntiles;
    const uint32_t cb = rest % ncb, slice = rest / ncb;
    const uint32_t s0 = tile * 64;
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const bool valid = s0 + lane < A.S;
    const uint32_t job = d.job_base + (valid ? s0 + lane : A.S - 1);
    const int i0 = (int)slice * C::SLICE_I + w * IW; // this wave's indices: [i0, i0 + IW)

    int *s_tab = s_all + w * C::WAVE_I; // this wave's two tables [2][16][ROWI]
    const size_t n1p = (size_t)A.n1p;
    // Table building, lane = column.  Stage st covers i = i0 + st / NPAIR, digits j0 = 2 (st % NPAIR) and j0 + 1: six
    // adjacent key rows, of which this wave needs the 256-byte strip of its column block.  Everything in the stage loop is
    // unconditional (the last stage re-loads itself): one basic block, so that look-ups and subtractions stay in the order
    // written.  M0 is saved and restored around the add-TID stores (the compiler does not expect it to change).
    int kr[6];
    for (int k = lane; k < 2 * C::ROWI; k += 64) s_tab[(k / C::ROWI) * C::TABI + k % C::ROWI] = 0; // the two zero rows
    const uint32_t tab_lds = (uint32_t)(uintptr_t)s_tab;
    auto stage_load = [&](int st) {
        const int i = i0 + st / C::NPAIR, j0 = 2 * (st % C::NPAIR);
        const int *src = A.ksk + ((size_t)i * T + j0) * 3 * n1p + cb * 64 + lane;
#pragma unroll
        for (int k = 0; k < 6; k++) kr[k] = src[k * n1p];
    };
#define EOC_KS_ROW(BUF, D1, D2) ((BUF) * C::TABI * 4 + ((D1) * 4 + (D2)) * C::ROWI * 4)
    auto stage_store = [&](int buf) {
        const int a1 = kr[0], a2 = kr[1], a3 = kr[2], b1 = kr[3], b2 = kr[4], b3 = kr[5];
        const uint32_t base = tab_lds + (uint32_t)buf * (C::TABI * 4);
        uint32_t m0_saved;
        asm volatile("s_mov_b32 %0, m0\n\t"
                     "s_mov_b32 m0, %1\n\t"
                     "s_nop 1\n\t" /* an SALU write of M0 needs a wait state before an add-TID LDS instruction reads it */
                     "ds_write_addtid_b32 %2 offset:%17\n\t"
                     "ds_write_addtid_b32 %3 offset:%18\n\t"
                     "ds_write_addtid_b32 %4 offset:%19\n\t"
                     "ds_write_addtid_b32 %5 offset:%20\n\t"
                     "ds_write_addtid_b32 %6 offset:%21\n\t"
                     "ds_write_addtid_b32 %7 offset:%22\n\t"
                     "ds_write_addtid_b32 %8 offset:%23\n\t"
                     "ds_write_addtid_b32 %9 offset:%24\n\t"
                     "ds_write_addtid_b32 %10 offset:%25\n\t"
                     "ds_write_addtid_b32 %11 offset:%26\n\t"
                     "ds_write_addtid_b32 %12 offset:%27\n\t"
                     "ds_write_addtid_b32 %13 offset:%28\n\t"
                     "ds_write_addtid_b32 %14 offset:%29\n\t"
                     "ds_write_addtid_b32 %15 offset:%30\n\t"
                     "ds_write_addtid_b32 %16 offset:%31\n\t"
                     "s_mov_b32 m0, %0"
                     : "=&s"(m0_saved)
                     : "s"(base), "v"(b1), "v"(b2), "v"(b3), "v"(a1), "v"(a1 + b1), "v"(a1 + b2), "v"(a1 + b3), "v"(a2),
                       "v"(a2 + b1), "v"(a2 + b2), "v"(a2 + b3), "v"(a3), "v"(a3 + b1), "v"(a3 + b2), "v"(a3 + b3),
                       "n"(EOC_KS_ROW(0, 0, 1)), "n"(EOC_KS_ROW(0, 0, 2)), "n"(EOC_KS_ROW(0, 0, 3)), "n"(EOC_KS_ROW(0, 1, 0)),
                       "n"(EOC_KS_ROW(0, 1, 1)), "n"(EOC_KS_ROW(0, 1, 2)), "n"(EOC_KS_ROW(0, 1, 3)), "n"(EOC_KS_ROW(0, 2, 0)),
                       "n"(EOC_KS_ROW(0, 2, 1)), "n"(EOC_KS_ROW(0, 2, 2)), "n"(EOC_KS_ROW(0, 2, 3)), "n"(EOC_KS_ROW(0, 3, 0)),
                       "n"(EOC_KS_ROW(0, 3, 1)), "n"(EOC_KS_ROW(0, 3, 2)), "n"(EOC_KS_ROW(0, 3, 3))
                     : "memory"); // (an "m0" clobber is refused -- "reserved register" -- so M0 is saved and restored by
                                  // hand inside the block; the trailing s_mov m0 is followed by the block's own consumers
                                  // only after a wave_lds_fence, never by an M0-reading instruction of the compiler's)
    };
#undef EOC_KS_ROW

    i4 acc[16];
#pragma unroll
    for (int c = 0; c < 16; c++) acc[c] = (i4){0, 0, 0, 0};

    stage_load(0);
    stage_store(0);
    wave_lds_fence();
    // this lane's IW operand words are IW * 4 contiguous bytes of its ciphertext's row (the blind rotation's epilogue
    // writes rows, coalesced): read 16 bytes every fourth index -- the tile is transposed on load, one lane per row
    typedef uint32_t u4 __attribute__((ext_vector_type(4)));
    const u4 *ubp = reinterpret_cast<const u4 *>(A.ubar + (size_t)job * kN + i0);
    u4 ub4 = ubp[0];
#pragma unroll 1
    for (int ii = 0; ii < IW; ii++) {
        const int k4 = ii & 3;
        const uint32_t ub = k4 == 0 ? ub4.x : (k4 == 1 ? ub4.y : (k4 == 2 ? ub4.z : ub4.w));
        u4 ub4n = ub4;
        if (k4 == 3 && ii + 1 < IW) ub4n = ubp[(ii + 1) >> 2];
#pragma unroll 1
        for (int q = 0; q < C::NPAIR; q++) {
            const int st = ii * C::NPAIR + q;
            const int buf = st & 1;
            stage_load(st + 1 < C::NSTAGE ? st + 1 : st);
            const uint32_t nib = (ub >> (28 - 4 * q)) & 15u; // digits 2q and 2q + 1 of this lane's ciphertext
            const i4 *row = reinterpret_cast<const i4 *>(s_tab + buf * C::TABI + (int)nib * C::ROWI);
#pragma unroll
            for (int c0 = 0; c0 < 16; c0 += 8) {
                i4 v[8];
#pragma unroll
                for (int c = 0; c < 8; c++) v[c] = row[c0 + c];
#pragma unroll
                for (int c = 0; c < 8; c++) acc[c0 + c] -= v[c];
                __builtin_amdgcn_sched_barrier(0);
            }
            stage_store(buf ^ 1);
            wave_lds_fence();
        }
        ub4 = ub4n;
    }

    // the workgroup's NWV partial sums -> one: the upper half of the waves parks its accumulators in LDS, the lower half adds
    __syncthreads(); // every wave is done with its tables
#pragma unroll
    for (int h = NWV / 2; h >= 1; h /= 2) {
        if (w >= h && w < 2 * h) {
            int *r = s_all + (w - h) * C::RED_I + lane * C::ROWI;
#pragma unroll
            for (int c = 0; c < 16; c++) *reinterpret_cast<i4 *>(r + 4 * c) = acc[c];
        }
        __syncthreads();
        if (w < h) {
            const int *r = s_all + w * C::RED_I + lane * C::ROWI;
#pragma unroll
            for (int c = 0; c < 16; c++) acc[c] += *reinterpret_cast<const i4 *>(r + 4 * c);
        }
        __syncthreads();
    }
    if (w == 0) {
        int *r = s_all + lane * C::ROWI;
#pragma unroll
        for (int c = 0; c < 16; c++) *reinterpret_cast<i4 *>(r + 4 * c) = acc[c];
    }
    __syncthreads();
    // output: wave w takes 64 / NWV ciphertexts, lane = column (256 contiguous bytes per atomic instruction)
    const int col = (int)cb * 64 + lane;
#pragma unroll 4
    for (int k = 0; k < 64 / NWV; k++) {
        const int ct = w * (64 / NWV) + k;
        const int v = s_all[ct * C::ROWI + lane];
        if (v != 0 && s0 + ct < A.S && col <= A.n) atomicAdd(d.out + (size_t)(s0 + ct) * (A.n + 1) + col, v);
    }
}

// Key switch for any (basebit <= 4, t) the kernel above is not instantiated for (both default parameter sets use
// basebit 2, t 8 and never come here): one thread per output word, rows read straight from the key image.  A plain,
// slow, exact form -- lweKeySwitchTranslate_fromArray as written.  The output row holds (0, ..., 0, b')
// when it starts (k_ks_init or the blind rotate's epilogue wrote it).  grid: x = S, y = gates; block = 256
__global__ __launch_bounds__(256) void k_keyswitch_generic(const GateDesc *__restrict__ descs, KSArgs A)
{
    const GateDesc d = A.inline_desc ? A.desc0 : descs[blockIdx.y];
    const uint32_t s = blockIdx.x, job = d.job_base + s;
    const int base1 = (1 << A.basebit) - 1;
    int32_t *o = d.out + (size_t)s * (A.n + 1);
    for (int m = threadIdx.x; m <= A.n; m += 256) {
        uint32_t acc = (uint32_t)o[m];
        for (int i = 0; i < kN; i++) {
            const uint32_t ub = A.ubar[(size_t)job * kN + i];
            for (int j = 0; j < A.t; j++) {
                const uint32_t dg = (ub >> (32 - (j + 1) * A.basebit)) & (uint32_t)base1;
                if (dg) acc -= (uint32_t)A.ksk[(((size_t)i * A.t + j) * base1 + (dg - 1)) * A.n1p + m];
            }
        }
        o[m] = (int32_t)acc;
    }
}

// ---- k_keyswitch_mfma<NWV>: basebit 2, t 8 (both default sets) on the matrix cores --------------------------------
// The key switch is the one dense contraction of the path:  out[c][col] = b[c] - sum_k OneHot[c][k] * KSK[k][col],
// k = (i, j, d), an integer matrix product mod 2^32.  With every key word split into four signed byte limbs,
//   l_0 = ((v + 128) & 255) - 128,  v <- (v - l_0) >> 8,  ...      v == l_0 + l_1 2^8 + l_2 2^16 + l_3 2^24  (mod 2^32),
// it is four int8 products with int32 accumulators (at most kN t = 8192 terms of magnitude <= 128: |acc| <= 2^20), and
//   out = b - (acc_0 + (acc_1 << 8) + (acc_2 << 16) + (acc_3 << 24))   in wrapping 32-bit arithmetic
// equals the row sums of k_keyswitch_waves word for word: integers, so neither the order of the terms nor the way the
// partial sums of the K-slices meet (integer atomics, as above) can change a bit.
//   * K order: k = (i t + j) 4 + d with an all-zero d = 0 slot, so one (i, j) group is one dword of an operand fragment and
//     one v_mfma_i32_32x32x32_i8 (K = 32) is exactly one index i.  Lane l = (h = l >> 5, r = l & 31) holds 16 bytes of A
//     (row r) and of B (column r): its slot (h, byte 4 q + d) is digit j = 4 h + q, value d, in BOTH operands.  The
//     instruction pairs A's and B's bytes of equal (h, byte), so the product does not depend on which k the hardware
//     calls such a slot (tools/ubench_ks_mfma.hip compares every output word with k_keyswitch_waves).
//   * A is never stored: a lane reads its ciphertext's operand word ubar[job][i] and forms the one-hot dword of digit j
//     as 1 << (8 d), three vector instructions.
//   * B is the limb image built by k_ksk_limbs at key install: [i][column tile of 32][limb][lane][16 B], so that a
//     fragment is one 16-byte load per lane, 1 KiB contiguous per wave, and the 4 fragments (limbs) of a (tile, i) 4 KiB.
//   * Workgroup = NWV waves stacked along M (64 ciphertexts each: 2 x 4 tiles of 32 x 32, A reused over the four limbs, B over
//     the two row tiles) x one column tile x one slice of the indices i.  The B fragments of 4 indices (16 KiB) are staged
//     per step through LDS (two buffers, one barrier per step; the global loads of step s + 1 fly during step s), each
//     fragment feeding 2 NWV MFMAs.  The four limbs of a column sit at the same lane of four accumulator tiles (C/D: col =
//     lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 h), so the recombination is in-lane.
// grid: x = mtiles * (n1p / 32) * nsl, y = gates; block = 64 NWV.  nsl divides kN / 4.
typedef int i16 __attribute__((ext_vector_type(16)));
constexpr int KSM_KI = 4; // indices i per staged step (one 16-byte read of a ciphertext's operand row)

template <int NWV>
__global__ __launch_bounds__(64 * NWV, 2) void k_keyswitch_mfma(const GateDesc *__restrict__ descs, KSArgs A,
                                                                 const i4 *__restrict__ limbs, int nsl)
{
    constexpr int MT = 64 * NWV;                 // ciphertexts per workgroup
    constexpr int CHUNKS = KSM_KI * 4;           // 1 KiB fragments per step
    constexpr int NLD = CHUNKS / NWV;            // ... of which each wave fetches this many
    static_assert(CHUNKS % NWV == 0, "shape");
    __shared__ i4 s_b[2][CHUNKS * 64];

    const GateDesc d = A.inline_desc ? A.desc0 : descs[blockIdx.y];
    const uint32_t ntiles = (A.S + MT - 1) / MT, nct = (uint32_t)A.n1p / 32u;
    const uint32_t tile = blockIdx.x % ntiles, rest = blockIdx.x / ntiles;
    const uint32_t ct = rest % nct, slice = rest / nct;
    const int per = kN / nsl, nstage = per / KSM_KI;
    const int ibeg = (int)slice * per;
    const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, h = lane >> 5;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t row0 = tile * MT + (uint32_t)w * 64u;

    typedef uint32_t u4 __attribute__((ext_vector_type(4)));
    const u4 *ubp[2];
#pragma unroll
    for (int m = 0; m < 2; m++) {
        const uint32_t s = row0 + 32u * m + r;
        const uint32_t job = d.job_base + (s < A.S ? s : A.S - 1);
        ubp[m] = reinterpret_cast<const u4 *>(A.ubar + (size_t)job * kN + ibeg);
    }
    // chunk c = ki * 4 + limb of step st: limbs[((ibeg + 4 st + ki) nct + ct) 256 + limb 64 + lane]
    const i4 *bsrc = limbs + ((size_t)ibeg * nct + ct) * 256 + lane;
    i4 stg[NLD];
    auto stage_load = [&](int st) {
#pragma unroll
        for (int x = 0; x < NLD; x++) {
            const int c = w + NWV * x;
            stg[x] = bsrc[((size_t)(st * KSM_KI + (c >> 2)) * nct) * 256 + (c & 3) * 64];
        }
    };
    auto stage_store = [&](int buf) {
#pragma unroll
        for (int x = 0; x < NLD; x++) s_b[buf][(w + NWV * x) * 64 + lane] = stg[x];
    };

    i16 acc[2][4];
#pragma unroll
    for (int m = 0; m < 2; m++)
#pragma unroll
        for (int k = 0; k < 4; k++)
#pragma unroll
            for (int q = 0; q < 16; q++) acc[m][k][q] = 0;

    stage_load(0);
    u4 ubc[2] = {ubp[0][0], ubp[1][0]};
    stage_store(0);
    stage_load(nstage > 1 ? 1 : 0);
    __syncthreads();
    const int sh0 = 27 - 8 * h; // digit j = 4 h + q sits at bits 31 - 2 j, 30 - 2 j: 8 d = (ub >> (27 - 2 j)) & 24
#pragma unroll 1
    for (int st = 0; st < nstage; st++) {
        const int buf = st & 1;
        const int stn = st + 1 < nstage ? st + 1 : st;
        const u4 ubn[2] = {ubp[0][stn], ubp[1][stn]};
#pragma unroll
        for (int ki = 0; ki < KSM_KI; ki++) {
            i4 b[4], a[2];
#pragma unroll
            for (int k = 0; k < 4; k++) b[k] = s_b[buf][(ki * 4 + k) * 64 + lane];
#pragma unroll
            for (int m = 0; m < 2; m++) {
                const uint32_t ub = ubc[m][ki];
#pragma unroll
                for (int q = 0; q < 4; q++) a[m][q] = (int)(1u << ((ub >> (sh0 - 2 * q)) & 24u));
            }
#pragma unroll
            for (int m = 0; m < 2; m++)
#pragma unroll
                for (int k = 0; k < 4; k++)
                    acc[m][k] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[m], b[k], acc[m][k], 0, 0, 0);
        }
        // unconditional (the last steps re-load the last one and store it where nobody reads): the number of loads in
        // flight is then the same on every path and the waits stay counted instead of draining the fresh loads
        stage_store(buf ^ 1); // (its readers of step st - 1 are behind the last barrier)
        stage_load(st + 2 < nstage ? st + 2 : nstage - 1);
        __syncthreads();
        ubc[0] = ubn[0];
        ubc[1] = ubn[1];
    }

    // out -= acc_0 + (acc_1 << 8) + (acc_2 << 16) + (acc_3 << 24); an atomic instruction covers two rows of 32 columns
    const int col = (int)ct * 32 + r;
    if (col <= A.n) {
#pragma unroll
        for (int m = 0; m < 2; m++)
#pragma unroll
            for (int q = 0; q < 16; q++) {
                const uint32_t s = row0 + 32u * m + (uint32_t)((q & 3) + 8 * (q >> 2) + 4 * h);
                const uint32_t v = (uint32_t)acc[m][0][q] + ((uint32_t)acc[m][1][q] << 8) + ((uint32_t)acc[m][2][q] << 16) +
                                   ((uint32_t)acc[m][3][q] << 24);
                if (v != 0 && s < A.S) atomicAdd(d.out + (size_t)s * (A.n + 1) + col, (int)(0u - v));
            }
    }
}

// The limb image of a [kN 8][3][n1p] key image (basebit 2, t 8): one thread per dword = one (i, j) group of one column
// and limb, bytes d = 0 (zero), 1, 2, 3.  grid: kN * (n1p / 32) * 4 workgroups of 256 (one 1 KiB fragment each)
__global__ __launch_bounds__(256) void k_ksk_limbs(const int32_t *__restrict__ ksk, uint32_t *__restrict__ limbs, int n1p)
{
    const uint32_t nct = (uint32_t)n1p / 32u;
    const uint32_t limb = blockIdx.x & 3u, ct = (blockIdx.x >> 2) % nct, i = (blockIdx.x >> 2) / nct;
    const int q = threadIdx.x & 3, lane = threadIdx.x >> 2, r = lane & 31, h = lane >> 5;
    const int j = 4 * h + q;
    const int32_t *row = ksk + ((size_t)i * 8 + j) * 3 * n1p + ct * 32 + r;
    uint32_t o = 0;
#pragma unroll
    for (int dg = 1; dg <= 3; dg++) {
        int32_t v = row[(size_t)(dg - 1) * n1p];
        int32_t l = 0;
        for (uint32_t k = 0; k <= limb; k++) {
            l = (int32_t)(((uint32_t)v + 128u) & 255u) - 128;
            v = (int32_t)((uint32_t)v - (uint32_t)l) >> 8;
        }
        o |= ((uint32_t)l & 255u) << (8 * dg);
    }
    limbs[(size_t)blockIdx.x * 256 + threadIdx.x] = o;
}

static inline size_t ks_limb_bytes(int n1p) { return (size_t)kN * (size_t)(n1p / 32) * 4096; }
static inline void ks_limbs_launch(const int32_t *ksk, void *limbs, int n1p, hipStream_t st)
{
    hipLaunchKernelGGL(k_ksk_limbs, dim3((unsigned)(kN * (n1p / 32) * 4)), dim3(256), 0, st, ksk,
                       static_cast<uint32_t *>(limbs), n1p);
}

// Waves per workgroup and K-slices of a k_keyswitch_mfma launch over `S` ciphertexts per gate: enough slices that one gate
// group gives every SIMD its two waves (2048 waves), at least 8 staged steps per slice.
struct KSMPlan {
    int nwv, nsl;
    unsigned gx;
};
static inline KSMPlan ks_mfma_plan(uint32_t S, int n1p)
{
    KSMPlan p;
    p.nwv = 4;
    const unsigned ntiles = (S + 64 * p.nwv - 1) / (64 * p.nwv), nct = (unsigned)n1p / 32u;
    p.nsl = 1;
    while (p.nsl < 32 && ntiles * nct * p.nsl * p.nwv < 2048u) p.nsl *= 2;
    p.gx = ntiles * nct * (unsigned)p.nsl;
    return p;
}
static inline void ks_mfma_launch(const KSMPlan &pl, uint32_t ngates, const GateDesc *descs, const KSArgs &a,
                                  const void *limbs, hipStream_t st)
{
    const i4 *lp = static_cast<const i4 *>(limbs);
    // the plan's nwv is 4: the <8> instance no plan could pick is no longer compiled
    hipLaunchKernelGGL(k_keyswitch_mfma<4>, dim3(pl.gx, ngates), dim3(256), 0, st, descs, a, lp, pl.nsl);
}

// =================================================================================================
// Compact public-key lists: sample extraction straight into the key switch's operand.
// A list is one TLWE sample (c0, c1) [2][N]; slot j of it is the LWE sample under s' with
//   a'_i = c0[j - i] (i <= j), -c0[N + j - i] (i > j),  b' = c1[j]      (the X^m a convention of the bootstrapping key)
// This kernel does for such a sample what k_ks_init does for an extracted one: ubar[s][i] = a'_i + 2^(31 - t basebit) and
// out[s] = (0, ..., 0, b'); the key switch then runs unchanged with its operand already in place.  A workgroup serves
// kCompactSlotsPerWG consecutive slots of ONE list and stages the list's c0 (4 KiB) in LDS once for all of them; lane i of
// a row reads c0[(j - i) mod N], consecutive lanes consecutive (descending) words: no bank conflict.
// grid: x = ((first mod G) + S + G - 1) / G; block = 256.  Sample s is slot `first + s` of `lists` (counted from slot 0 of
// list 0); workgroup w covers the G-aligned slots [G (first / G + w), + G), G divides N, and skips those outside the call.
// =================================================================================================
constexpr int kCompactSlotsPerWG = 16;
__global__ __launch_bounds__(256) void k_compact_expand(const int32_t *__restrict__ lists, uint64_t first, uint32_t S,
                                                        uint32_t *__restrict__ ubar, int32_t *__restrict__ out, int n,
                                                        uint32_t prec_offset)
{
    static_assert(kN % kCompactSlotsPerWG == 0, "a workgroup's slots lie inside one list");
    __shared__ int32_t s_c0[kN];
    const uint64_t g0 = (first / kCompactSlotsPerWG + blockIdx.x) * kCompactSlotsPerWG;
    const int32_t *list = lists + (g0 / kN) * (uint64_t)(2 * kN);
    for (int k = threadIdx.x; k < kN; k += 256) s_c0[k] = list[k];
    __syncthreads();
    for (int q = 0; q < kCompactSlotsPerWG; q++) {
        const uint64_t g = g0 + q;
        if (g < first || g >= first + S) continue;
        const uint32_t s = (uint32_t)(g - first);
        const int j = (int)(g % kN);
        uint32_t *row = ubar + (size_t)s * kN;
        for (int i = threadIdx.x; i < kN; i += 256) {
            const uint32_t v = (uint32_t)s_c0[(j - i) & (kN - 1)];
            row[i] = (i <= j ? v : 0u - v) + prec_offset;
        }
        int32_t *o = out + (size_t)s * (n + 1);
        for (int m = threadIdx.x; m < n; m += 256) o[m] = 0;
        if (threadIdx.x == 0) o[n] = list[kN + j];
    }
}

// =================================================================================================
// Leveled operations: the CMux of an encrypted-index table read.
//   out = A + C (x) (X^rot B - A),  rot in [0, 2N)
// A, B: TLWE samples [2][N] in global memory; C: a converted selector [2l][2][512] complex (one row block of the
// bootstrapping key's FFT image, scaled by 2^-9).  The external product is the blind rotation's, the same text
// (ext_product_pair.inc, in the canonical order of oracle/tfhe_oracle.c): with A = B the item is one blind-rotation step
// with abar = rot, bit for bit, by construction.
// Mapping: one wave PAIR per item, as k_blind_rotate -- wave h owns input polynomial h (difference, decomposition, the l
// forward transforms) and output polynomial h (the chain the partner started, continued with the own digits, the inverse
// transform, + A_h).  Wave h reads and writes polynomial h only.  kCmuxItemsPerWG pairs share one workgroup and its copy of
// the twiddle tables; the pairs of a workgroup meet at the two exchange barriers (a pair past the end of the grid computes
// the last item again and stores nothing, so every barrier is reached by all waves).  Nothing here is loop-invariant, so
// the tables are read from LDS in every pass, as the pair kernel's gadget-length-3 instance does.
// This mapping, the LDS plan, the dead pair's rule and the product are the leveled frame, leveled_pair.inc: one text that
// k_cmux, k_demux and k_automaton_step include around their operand pointers, their load phase and their store phase.
// grid: x = ceil(nx / kCmuxItemsPerWG), y = ny; item (x, y) is addressed by strides in int32 (samples) / d2 (selectors).
// =================================================================================================
constexpr int kCmuxItemsPerWG = 2;
constexpr int kCmuxLds = (kTwEntries + kNH + 2 * kCmuxItemsPerWG * kScr) * 16; // 53 760 bytes: two workgroups per CU

struct CmuxArgs {
    const d2 *sel;             // converted selectors
    const int32_t *in0, *in1;  // A, B
    int32_t *out;
    size_t sel_x, sel_y;       // strides per item along x / y, in d2
    size_t in0_x, in0_y, in1_x, in1_y, out_x, out_y; // ... in int32
    uint32_t nx;               // items along x
    int rot;                   // B is multiplied by X^rot
    int Bgbit;
};

// The small pieces of the leveled kernels (their frame is leveled_pair.inc).
// Rows (h, p) of the converted selector `sel` for output polynomial c: 16 bytes per lane, 1 KiB contiguous per wave and
// instruction
template <int L> __device__ __forceinline__ void load_selector_row(const d2 *sel, int h, int lane, int p, int c, d2 (&b)[8])
{
    const d2 *row = sel + ((size_t)(h * L + (p - 1)) * 2 + c) * kNH + lane;
#pragma unroll
    for (int r = 0; r < 8; r++) b[r] = row[r * 64];
}
// register r of the product, un-twisted and truncated: coefficients lane + 64 r (x) and lane + 64 r + 512 (y) of C (x) x
__device__ __forceinline__ uint2 leveled_words(const d2 &s, const d2 &u)
{
    const d2 y = cmulc(s, u); // 1/512 is in the selector's image
    return make_uint2(wrap_trunc(y.x), wrap_trunc(y.y));
}
// Position idx of the 2N-period of a polynomial of the ring X^N = -1, from v = its coefficient idx mod N: the upper half of
// the period is negated.  A macro: as a force-inlined function, of (p, idx) or of (idx, v) alone, it leaves every k_cmux
// byte-identical and changes every k_automaton_step in 45 to 680 lines (tools/isa_diff.py).
#define EOC_NEGACYCLIC(idx, v) (((idx) & kN) ? 0u - (v) : (v))

// The kernel's text is in leveled_kernels.inc, included twice: k_cmux<L, BGBIT> with the oracle's truncating gadget, and
// k_rcmux<L, BGBIT>, its rounding twin: the same lines with 2^(31 - L Bgbit) more in the gadget's offset.
#define EOC_LEVELED_KERNEL 1
#define EOC_LEVELED_ROUND 0
#include "leveled_kernels.inc"
#define EOC_LEVELED_KERNEL 1
#define EOC_LEVELED_ROUND 1
#include "leveled_kernels.inc"

// k_compact_expand's sibling behind a table read: sample (q, w), w < W, is slot w of query q's TLWE sample
// `lists + q * list_stride` and becomes key-switch operand row q W + w (ubar) and output row q W + w (0, ..., 0, b').  The
// same staging of c0 in LDS and the same lane-contiguous stores.  grid: x = ceil(W / kCompactSlotsPerWG), y = queries
__global__ __launch_bounds__(256) void k_tlwe_extract(const int32_t *__restrict__ lists, size_t list_stride, uint32_t W,
                                                      uint32_t *__restrict__ ubar, int32_t *__restrict__ out, int n,
                                                      uint32_t prec_offset)
{
    __shared__ int32_t s_c0[kN];
    const int32_t *list = lists + (size_t)blockIdx.y * list_stride;
    for (int k = threadIdx.x; k < kN; k += 256) s_c0[k] = list[k];
    __syncthreads();
    for (int q = 0; q < kCompactSlotsPerWG; q++) {
        const uint32_t j = blockIdx.x * kCompactSlotsPerWG + q;
        if (j >= W) break;
        const size_t s = (size_t)blockIdx.y * W + j;
        uint32_t *row = ubar + s * kN;
        for (int i = threadIdx.x; i < kN; i += 256) {
            const uint32_t v = (uint32_t)s_c0[((int)j - i) & (kN - 1)];
            row[i] = (i <= (int)j ? v : 0u - v) + prec_offset;
        }
        int32_t *o = out + s * (n + 1);
        for (int m = threadIdx.x; m < n; m += 256) o[m] = 0;
        if (threadIdx.x == 0) o[n] = list[kN + j];
    }
}

// =================================================================================================
// Packing key switch: LWE samples (a_i, b_i) under the LWE key s -> compact TLWE lists under s'; sample i
// goes to slot i mod N of list i / N.  With A_m(X) = sum_i a_{i,m} X^i and B(X) = sum_i b_i X^i a list is
//   (0, B) - sum_m sum_{j = 1..4} D_{m,j}(X) Row(m, j),   Row(m, j) a TLWE encryption of s_m 2^(32 - 4j) under s',
// D_{m,j} the j-th signed base-16 digit polynomial of A_m + 2^15 (a ROUNDING decomposition to 16 bits).
// Format rule: the rows of 16 consecutive key indices (a chunk) are accumulated in the spectral domain, m ascending then j
// ascending, per output polynomial; every chunk is inverse-transformed and converted once (|.| <= 64 * 8 * 1024 * 2^31 =
// 2^50 < 2^51: wrap_trunc's contract holds unconditionally) and the int32 result is subtracted from the list.  Chunks
// combine by integer addition, so their order -- and the atomics below -- cannot change a bit.
// =================================================================================================
constexpr int kPackT = 4, kPackBasebit = 4;   // decomposition of the packing key (part of the EOCPKS1 format)
constexpr int kPackChunk = 16;                // key indices per inverse transform (part of the format)
constexpr int kPackTile = 64;

// The mask columns as polynomials: cols[list][m][i] = a_{list N + i, m} (0 past `count`), a 64 x 64 tile transpose through
// LDS, both sides 256 contiguous bytes per wave and instruction; column n (the b_i) goes to c1 of the output list and c0 is
// cleared: lists[list] = (0, B).  grid: x = N / 64 sample tiles, y = ceil((n + 1) / 64) column tiles, z = lists of the
// slice; block = 256.  `in`, `lists` and `count` are those of the slice (sample 0 = slot 0 of list 0).
__global__ __launch_bounds__(256) void k_pack_gather(const int32_t *__restrict__ in, size_t count, int n,
                                                     int32_t *__restrict__ cols, int32_t *__restrict__ lists)
{
    __shared__ int32_t s_tile[kPackTile][kPackTile + 1];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int i0 = blockIdx.x * kPackTile, m0 = blockIdx.y * kPackTile;
    const size_t list = blockIdx.z, s0 = list * kN + i0;
    for (int r = ty; r < kPackTile; r += 4) {
        const size_t s = s0 + r;
        const int m = m0 + tx;
        s_tile[r][tx] = (s < count && m <= n) ? in[s * ((size_t)n + 1) + m] : 0;
    }
    __syncthreads();
    for (int r = ty; r < kPackTile; r += 4) {
        const int m = m0 + r;
        const int32_t v = s_tile[tx][r];
        if (m < n) cols[(list * n + m) * kN + i0 + tx] = v;
        else if (m == n) lists[list * 2 * kN + kN + i0 + tx] = v;
    }
    if (blockIdx.y == 0 && ty == 0) lists[list * 2 * kN + i0 + tx] = 0;
}

// One WAVE per (list, chunk): both spectral accumulators stay in registers (64 VGPRs), the four digit transforms of a key
// index run two at a time through fft_fwd_rest_x2 on the wave's own scratch, and nothing is exchanged between waves: one
// barrier (the tables), none in the row loop.  Key rows [n][4][2][512] complex (k_fft_fwd_polys at scale 2^-9, as the
// selectors of k_cmux) are read 16 bytes per lane, 1 KiB per wave and instruction, and multiplied in bin block by bin
// block as k_blind_rotate_wide does: whole rows held next to two accumulators and two transforms do not fit 256 registers.
// The first row of a chunk starts both chains as a plain product (cmul0, as every chain), so the first key index is
// peeled off the loop.  Results leave as vector integer atomics of the negated words.
// grid: x = ceil(items / 4), items = lists x chunks; block = 256.
constexpr int kPackWavesPerWG = 4;
constexpr int kPackLds = (kTwEntries + kNH + kPackWavesPerWG * kScr) * 16; // 53 760 bytes: two workgroups per CU

__global__ __launch_bounds__(64 * kPackWavesPerWG, 2) void k_pack_rows(const int32_t *__restrict__ cols,
                                                                       const d2 *__restrict__ key, int32_t *__restrict__ lists,
                                                                       int n, uint32_t nchunks, uint32_t items,
                                                                       const d2 *__restrict__ g_tw,
                                                                       const d2 *__restrict__ g_twist)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    d2 *s_tw = reinterpret_cast<d2 *>(smem);
    d2 *s_twist = s_tw + kTwEntries;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    d2 *scr = s_twist + kNH + wv * kScr;
    load_tables(s_tw, s_twist, g_tw, g_twist, tid, 64 * kPackWavesPerWG);
    __syncthreads(); // the tables; the only barrier
    const uint32_t item = blockIdx.x * kPackWavesPerWG + (uint32_t)wv;
    if (item >= items) return;
    const uint32_t list = item / nchunks, chunk = item - list * nchunks;
    const int m_first = (int)chunk * kPackChunk, m_end = min(m_first + kPackChunk, n);

    const Gadget<kPackBasebit> gd = make_gadget<kPackBasebit>(0);
    uint32_t offset = 1u << (31 - kPackT * kPackBasebit); // the rounding term 2^15 ...
#pragma unroll
    for (int p = 1; p <= kPackT; p++) offset += gd.halfBg << gd.shift(p); // ... and DecompH's offset

    uint32_t dlo[8], dhi[8];
    auto make_x0 = [&](int p, d2 (&x)[8]) __attribute__((always_inline)) { digit_pass(dlo, dhi, gd.shift(p), gd, x); };
    d2 S0[8], S1[8];
    auto key_index = [&](int m, auto first_tag) __attribute__((always_inline)) {
        constexpr bool kFirst = decltype(first_tag)::value;
        const int32_t *pa = cols + ((size_t)list * n + m) * kN;
#pragma unroll
        for (int r = 0; r < 8; r++) {
            dlo[r] = (uint32_t)pa[lane + 64 * r] + offset;
            dhi[r] = (uint32_t)pa[lane + 64 * r + kNH] + offset;
        }
        const d2 *rows = key + (size_t)m * kPackT * 2 * kNH + lane; // Row(m, j) polynomial c at ((j - 1) * 2 + c) * 512
        d2 xa[8], xb[8];
#pragma unroll
        for (int j0 = 1; j0 < kPackT; j0 += 2) {
            make_x0(j0, xa);
            fft_fwd_rest_x2(xa, xb, [&]() __attribute__((always_inline)) { make_x0(j0 + 1, xb); }, s_tw, scr, lane);
            // both chains, bin block by bin block: row (m, j0), then row (m, j0 + 1)
#pragma unroll
            for (int r = 0; r < 8; r++) {
                const d2 a0 = rows[((j0 - 1) * 2 + 0) * kNH + r * 64], a1 = rows[((j0 - 1) * 2 + 1) * kNH + r * 64];
                const d2 b0 = rows[(j0 * 2 + 0) * kNH + r * 64], b1 = rows[(j0 * 2 + 1) * kNH + r * 64];
                const d2 s0 = (kFirst && j0 == 1) ? cmul0(xa[r], a0) : cmac1(xa[r], a0, S0[r]);
                const d2 s1 = (kFirst && j0 == 1) ? cmul0(xa[r], a1) : cmac1(xa[r], a1, S1[r]);
                S0[r] = cmac1(xb[r], b0, s0);
                S1[r] = cmac1(xb[r], b1, s1);
            }
        }
    };
    key_index(m_first, std::true_type());
#pragma unroll 1
    for (int m = m_first + 1; m < m_end; m++) key_index(m, std::false_type());

    int32_t *po = lists + (size_t)list * 2 * kN;
    d2 ut[8];
    fft_inv_wave(S0, ut, s_tw, s_twist, scr, lane);
#pragma unroll
    for (int r = 0; r < 8; r++) {
        const int j = lane + 64 * r;
        const d2 y = cmulc(S0[r], ut[r]); // 1/512 is in the key image
        atomicAdd(po + j, (int)(0u - wrap_trunc(y.x)));
        atomicAdd(po + j + kNH, (int)(0u - wrap_trunc(y.y)));
    }
    fft_inv_wave(S1, ut, s_tw, s_twist, scr, lane);
#pragma unroll
    for (int r = 0; r < 8; r++) {
        const int j = lane + 64 * r;
        const d2 y = cmulc(S1[r], ut[r]);
        atomicAdd(po + kN + j, (int)(0u - wrap_trunc(y.x)));
        atomicAdd(po + kN + j + kNH, (int)(0u - wrap_trunc(y.y)));
    }
}

// The same two outputs for a TEST-POLYNOMIAL list: list (f, s) holds the p values v_0 .. v_(p-1) of row s
// of function f, in[((f p + j) rows + s)][n + 1], each over a window of N / p coefficients by the rule of
// eoc_lut_test_polynomial: coefficient k < N - N / (2p) takes sample j(k) = floor((k p + N / 2) / N), the last N / (2p)
// coefficients take sample 0 negated (word-wise).  The words are those of k_pack_gather on the N-row batch of repeated /
// negated samples, which never exists in memory.  p in {2, 4, 8}: every window boundary is a multiple of 64, so a tile of 64
// coefficients reads ONE sample: a wave loads 64 mask words (256 contiguous bytes) and stores, per key index, 64 copies of
// one of them (256 contiguous bytes): no transpose, no LDS.  grid: x = N / 64 coefficient tiles, y = ceil((n + 1) / 64)
// column tiles, z = lists of the slice (list = f rows + s - list0); block = 256 (wave w: columns w, w + 4, ...).  A template
// over the message space p.
template <int p>
__global__ __launch_bounds__(256) void k_tvpack_cols(const int32_t *__restrict__ in, uint32_t rows, uint32_t list0, int n,
                                                     int32_t *__restrict__ cols, int32_t *__restrict__ lists)
{
    static_assert(p == 2 || p == 4 || p == 8, "window boundaries are multiples of the tile only for these");
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int i0 = blockIdx.x * kPackTile, m0 = blockIdx.y * kPackTile;
    const size_t list = blockIdx.z;
    const uint32_t gl = list0 + (uint32_t)list, f = gl / rows, s = gl - f * rows;
    const bool neg = i0 >= kN - kN / (2 * p);
    const int j = neg ? 0 : (i0 * p + kN / 2) / kN;
    const int32_t *row = in + (((size_t)f * p + j) * rows + s) * ((size_t)n + 1);
    const int m = m0 + tx;
    const uint32_t w = m <= n ? (uint32_t)row[m] : 0u;
    const int32_t mine = (int32_t)(neg ? 0u - w : w);
    for (int r = ty; r < kPackTile; r += 4) {
        const int mr = m0 + r;
        const int32_t v = __shfl(mine, r, 64);
        if (mr < n) cols[(list * n + mr) * kN + i0 + tx] = v;
        else if (mr == n) lists[list * 2 * kN + kN + i0 + tx] = v;
    }
    if (blockIdx.y == 0 && ty == 0) lists[list * 2 * kN + i0 + tx] = 0;
}

// ---- the EXACT test-polynomial pack on the matrix cores ----------------------------------------------
// The digit polynomials of k_tvpack_cols' batch are piecewise constant: p + 1 distinct samples per list (the p values and
// value 0 negated), each spread over one window of coefficients.  So the list factors, in wrapping 32-bit integers, into
//   S_s  = (0, b_s X^0) - sum_m sum_j d_(s,m,j) Row(m, j)       an integer matrix product: M = samples, K = 4 n, 2 N columns
//   list = sum_s Win_s(X) S_s                                   negacyclic sums over public windows of ones
// Win_0 = X^0 .. X^(h-1), Win_s = X^(s w - h) .. X^(s w + h - 1) (0 < s < p), Win_p = X^(N-h) .. X^(N-1), h = N / 2p, w = N / p.
// The product runs as k_keyswitch_mfma's does: the int32 key rows split into four signed byte limbs (k_ksk_limbs' rule), four
// int8 products with int32 accumulators (at most 4 n terms of magnitude <= 8 x 128: |acc| < 2^22), recombined in-lane.

// The limb image of the packing key's int32 rows [n][4][2][N]: [K step of 8 key indices][column tile of 32][limb][lane][16 B].
// Lane (h = lane >> 5, r = lane & 31) holds column 32 ct + r of the 2 N columns (polynomial c0 first); its byte 4 q + jj is
// Row(m, j) with m = 8 step + 4 h + q and j = 4 - jj: the order in which tvp_digit_dword leaves the digits of one mask word.
// Key indices m >= n are zero rows.  One thread per dword; grid: ksteps * 64 * 4 workgroups of 256 (one 1 KiB fragment each)
constexpr int kTvpCols = 2 * kN, kTvpColTiles = kTvpCols / 32;
__global__ __launch_bounds__(256) void k_pks_limbs(const int32_t *__restrict__ rows, uint32_t *__restrict__ limbs, int n)
{
    const uint32_t limb = blockIdx.x & 3u, ct = (blockIdx.x >> 2) % kTvpColTiles, step = (blockIdx.x >> 2) / kTvpColTiles;
    const int q = threadIdx.x & 3, lane = threadIdx.x >> 2, r = lane & 31, h = lane >> 5;
    const int m = 8 * (int)step + 4 * h + q;
    const int col = (int)ct * 32 + r;
    uint32_t o = 0;
    if (m < n) {
#pragma unroll
        for (int jj = 0; jj < 4; jj++) {
            const int j = 4 - jj;
            int32_t v = rows[(((size_t)m * kPackT + (j - 1)) * 2 + (col >> 10)) * kN + (col & (kN - 1))];
            int32_t l = 0;
            for (uint32_t k = 0; k <= limb; k++) {
                l = (int32_t)(((uint32_t)v + 128u) & 255u) - 128;
                v = (int32_t)((uint32_t)v - (uint32_t)l) >> 8;
            }
            o |= ((uint32_t)l & 255u) << (8 * jj);
        }
    }
    limbs[(size_t)blockIdx.x * 256 + threadIdx.x] = o;
}
static inline int tvp_ksteps(int n) { return (n + 7) / 8; }
static inline size_t tvp_limb_bytes(int n) { return (size_t)tvp_ksteps(n) * kTvpColTiles * 4096; }

// The four signed base-16 digits of one mask word as four signed bytes: digit j (bits 32 - 4 j .. 35 - 4 j of
// a + 2^15 + sum 8 2^(32 - 4 j), minus 8) in byte 4 - j
__device__ __forceinline__ int tvp_digit_dword(uint32_t a)
{
    const uint32_t t = (a + 0x88888000u) >> 16;
    uint32_t u = (t | (t << 8)) & 0x00FF00FFu;
    u = ((u | (u << 4)) & 0x0F0F0F0Fu) ^ 0x08080808u; // nibble - 8 = (nibble ^ 8) sign-extended from bit 3 ...
    return (int)(u | ((u & 0x08080808u) * 0x1Eu));    // ... 8 x 0x1E = 0xF0: no carry between the bytes
}

// S[row][2 N] = -(sum_m sum_j d Row(m, j)) for the rows (list l, sample s) = l (p + 1) + s of a slice of lists; sample s < p is
// value s of the list's row, sample p is value 0 negated word by word (formed here, never stored).  A is never stored: lane
// (h, r) reads the mask words m = 8 step + 4 h + q, q < 4, of its row and forms one digit dword each, so one K = 32 instruction
// covers 8 key indices; m >= n gives zero digits against the image's zero rows.  Workgroup = NWV waves stacked along M (64 rows
// each: 2 x 4 tiles of 32 x 32, A reused over the limbs, B over the two row tiles) x one column tile x all of K; the four 1 KiB
// fragments of a step go through LDS (two buffers, one barrier per step, the loads of step s + 2 in flight during step s).
// No K slices: every word of S is written exactly once, by a plain store.
// vals: [n_funcs][p][rows][n + 1]; list l of the slice is (f, row) = divmod(list0 + l, rows).
// grid: x = ceil(M / (64 NWV)) * 64, column tile fastest (workgroups b and b + 8 share an L2: 8 of the 64 column tiles each)
template <int NWV>
__global__ __launch_bounds__(64 * NWV, 2) void k_tvpack_mm(const int32_t *__restrict__ vals, uint32_t rows, uint32_t list0,
                                                            uint32_t M, int p, int n, const i4 *__restrict__ limbs, int ksteps,
                                                            int32_t *__restrict__ S)
{
    static_assert(NWV == 4, "one 1 KiB fragment (limb) per wave and step");
    constexpr int MT = 64 * NWV;
    __shared__ i4 s_b[2][4 * 64];

    const uint32_t ct = blockIdx.x % kTvpColTiles, tile = blockIdx.x / kTvpColTiles;
    const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, h = lane >> 5;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t row0 = tile * MT + (uint32_t)w * 64u;

    const int32_t *ap[2];
    bool neg[2];
#pragma unroll
    for (int m = 0; m < 2; m++) {
        uint32_t row = row0 + 32u * m + r;
        row = row < M ? row : M - 1;
        const uint32_t l = row / (uint32_t)(p + 1), s = row - l * (uint32_t)(p + 1);
        const uint32_t gl = list0 + l, f = gl / rows, sr = gl - f * rows;
        neg[m] = s == (uint32_t)p;
        ap[m] = vals + (((size_t)f * p + (neg[m] ? 0u : s)) * rows + sr) * ((size_t)n + 1) + 4 * h;
    }
    // the digit dwords of K step `st`: mask words m = 8 st + 4 h + q of both row tiles
    auto a_load = [&](int st, i4 (&a)[2]) {
#pragma unroll
        for (int m = 0; m < 2; m++)
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const int idx = 8 * st + q; // + 4 h in ap
                const bool in = idx + 4 * h < n;
                const uint32_t wd = in ? (uint32_t)ap[m][idx] : 0u;
                a[m][q] = in ? tvp_digit_dword(neg[m] ? 0u - wd : wd) : 0;
            }
    };
    const i4 *bsrc = limbs + ((size_t)ct * 4 + w) * 64 + lane; // wave w fetches limb w of every step
    auto b_load = [&](int st) { return bsrc[(size_t)st * kTvpColTiles * 256]; };

    i16 acc[2][4];
#pragma unroll
    for (int m = 0; m < 2; m++)
#pragma unroll
        for (int k = 0; k < 4; k++)
#pragma unroll
            for (int q = 0; q < 16; q++) acc[m][k][q] = 0;

    i4 stg = b_load(0), ac[2], an[2];
    a_load(0, ac);
    s_b[0][w * 64 + lane] = stg;
    stg = b_load(ksteps > 1 ? 1 : 0);
    __syncthreads();
#pragma unroll 1
    for (int st = 0; st < ksteps; st++) {
        const int buf = st & 1;
        a_load(st + 1 < ksteps ? st + 1 : st, an);
        i4 b[4];
#pragma unroll
        for (int k = 0; k < 4; k++) b[k] = s_b[buf][k * 64 + lane];
#pragma unroll
        for (int m = 0; m < 2; m++)
#pragma unroll
            for (int k = 0; k < 4; k++) acc[m][k] = __builtin_amdgcn_mfma_i32_32x32x32_i8(ac[m], b[k], acc[m][k], 0, 0, 0);
        // unconditional, as in k_keyswitch_mfma: the last steps re-load the last fragment and store it where nobody reads
        s_b[buf ^ 1][w * 64 + lane] = stg; // (its readers of step st - 1 are behind the last barrier)
        stg = b_load(st + 2 < ksteps ? st + 2 : ksteps - 1);
        __syncthreads();
        ac[0] = an[0];
        ac[1] = an[1];
    }

    // S = -(acc_0 + (acc_1 << 8) + (acc_2 << 16) + (acc_3 << 24)); a store instruction covers two rows of 32 columns
    const int col = (int)ct * 32 + r;
#pragma unroll
    for (int m = 0; m < 2; m++)
#pragma unroll
        for (int q = 0; q < 16; q++) {
            const uint32_t row = row0 + 32u * m + (uint32_t)((q & 3) + 8 * (q >> 2) + 4 * h);
            const uint32_t v = (uint32_t)acc[m][0][q] + ((uint32_t)acc[m][1][q] << 8) + ((uint32_t)acc[m][2][q] << 16) +
                               ((uint32_t)acc[m][3][q] << 24);
            if (row < M) S[(size_t)row * kTvpCols + col] = (int32_t)(0u - v);
        }
}

// list[c] = sum_s Win_s(X) (S_s[c] + [c = 1] b_s X^0) for one polynomial c of one list: per sample the inclusive prefix sums
// C[t] of the 1 024 words (four consecutive words per thread, a wave scan, the wave totals through LDS); with S~[t] = S[t]
// (t >= 0), -S[t + N] (t < 0) and E(t) = sum_(u = -N .. t) S~[u] = -C[t + N] (t < 0), C[t] - C[N - 1] (t >= 0), a window
// [lo, hi) gives coefficient k the running-sum difference E(k - lo) - E(k - hi).  The list is WRITTEN (plain stores, 256
// contiguous bytes per wave and instruction), not accumulated into.  grid: x = 2 * lists of the slice; block = 256.
template <int p>
__global__ __launch_bounds__(256) void k_tv_spread(const int32_t *__restrict__ S, const int32_t *__restrict__ vals, uint32_t rows,
                                                   uint32_t list0, int n, int32_t *__restrict__ lists)
{
    static_assert(p == 2 || p == 4 || p == 8, "the message spaces of k_tvpack_cols");
    constexpr int hw = kN / (2 * p), wd = kN / p;
    typedef uint32_t u4 __attribute__((ext_vector_type(4)));
    __shared__ u4 s_c[kN / 4];
    __shared__ uint32_t s_w[4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const uint32_t l = blockIdx.x >> 1, c = blockIdx.x & 1u;
    const uint32_t gl = list0 + l, f = gl / rows, sr = gl - f * rows;
    const uint32_t *sc = reinterpret_cast<const uint32_t *>(s_c);
    uint32_t out[4] = {0, 0, 0, 0};
#pragma unroll 1
    for (int s = 0; s <= p; s++) {
        u4 x = *reinterpret_cast<const u4 *>(S + (((size_t)l * (p + 1) + s) * 2 + c) * kN + 4 * tid);
        if (c == 1 && tid == 0) {
            const uint32_t b = (uint32_t)vals[(((size_t)f * p + (s < p ? s : 0)) * rows + sr) * ((size_t)n + 1) + n];
            x.x += s < p ? b : 0u - b;
        }
        x.y += x.x;
        x.z += x.y;
        x.w += x.z;
        uint32_t t = x.w;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t o = __shfl_up(t, d, 64);
            if (lane >= d) t += o;
        }
        if (lane == 63) s_w[wv] = t;
        __syncthreads(); // also: the readers of s_c of sample s - 1 are done
        uint32_t base = t - x.w;
        for (int k = 0; k < wv; k++) base += s_w[k];
        s_c[tid] = x + base;
        __syncthreads(); // also: the readers of s_w are done before sample s + 1 writes it
        const uint32_t total = sc[kN - 1];
        const int lo = s == 0 ? 0 : (s == p ? kN - hw : s * wd - hw), hi = s == p ? kN : s * wd + hw;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int k = tid + 256 * i, t0 = k - lo, t1 = k - hi;
            const uint32_t e0 = t0 < 0 ? 0u - sc[t0 + kN] : sc[t0] - total;
            const uint32_t e1 = t1 < 0 ? 0u - sc[t1 + kN] : sc[t1] - total;
            out[i] += e0 - e1;
        }
    }
#pragma unroll
    for (int i = 0; i < 4; i++) lists[((size_t)l * 2 + c) * kN + tid + 256 * i] = (int32_t)out[i];
}

// =================================================================================================
// Encrypted-index table updates: the demultiplexer, a table read's CMux run backwards.
//   E = C (x) x,  out1 = E,  out0 = x - E (word by word)
// x: a TLWE sample [2][N]; C: a converted selector, as k_cmux's.  E is k_cmux's external product with in0 = 0, in1 = x,
// rot = 0 before the add -- the same text (ext_product_pair.inc), so the two agree bit for bit by construction.  The mapping,
// the LDS plan and the dead pair's rule are the leveled frame (leveled_pair.inc, described above k_cmux): wave h decomposes
// offset + x_h (no difference, no rotation), produces E_h and writes polynomial h of BOTH children.  x is not held across the
// product: x - E is formed at store time from a reload of x (8 KiB per item, L2-resident), which is what keeps the second
// output out of the register count.
// accumulate = 0: plain stores (out0 / out1 may not overlap x).  accumulate = 1: vector integer atomicAdd into the
// destination, lane-contiguous (256 bytes per wave and instruction) as k_pack_rows leaves its results: the last stage of an
// update adds its leaves straight into the table, every word an integer sum, so colliding queries and any order of arrival
// give the same words.
// grid: x = ceil(nx / kCmuxItemsPerWG) parents, y = ny; item (x, y) by strides in int32 (samples) / d2 (selectors).
// =================================================================================================
struct DemuxArgs {
    const d2 *sel;            // converted selectors
    const int32_t *in;        // x
    int32_t *out0, *out1;     // x - E, E
    size_t sel_x, sel_y;      // strides per item along x / y, in d2
    size_t in_x, in_y, out_x, out_y; // ... in int32 (out0 and out1 share theirs)
    uint32_t nx;              // items along x
    int accumulate;           // 0: store, 1: atomicAdd
    int Bgbit;
};

// k_demux<L, BGBIT> and its rounding twin k_rdemux<L, BGBIT>: one text, leveled_kernels.inc
#define EOC_LEVELED_KERNEL 2
#define EOC_LEVELED_ROUND 0
#include "leveled_kernels.inc"
#define EOC_LEVELED_KERNEL 2
#define EOC_LEVELED_ROUND 1
#include "leveled_kernels.inc"

// table[0] += sample_q for q = 0 .. queries - 1: the update of a one-list table, where no demultiplexer runs (DESIGN.md
// 15).  V = 4: one 16-byte load per lane (both pointers 16-byte aligned); V = 1: word loads.  Integer atomics either way:
// queries meet on the one list.  grid: x = 2N / (256 V), y = queries; block = 256.
template <int V>
__global__ __launch_bounds__(256) void k_sample_add(const int32_t *__restrict__ in, int32_t *__restrict__ list)
{
    static_assert(V == 1 || V == 4, "a word or 16 bytes per lane");
    const size_t k = ((size_t)blockIdx.x * 256 + threadIdx.x) * V;
    const int32_t *src = in + (size_t)blockIdx.y * 2 * kN + k;
    if constexpr (V == 4) {
        const int4 v = *reinterpret_cast<const int4 *>(src);
        atomicAdd(list + k, v.x);
        atomicAdd(list + k + 1, v.y);
        atomicAdd(list + k + 2, v.z);
        atomicAdd(list + k + 3, v.w);
    } else {
        atomicAdd(list + k, src[0]);
    }
}

// =================================================================================================
// Seeded ciphertexts, selectors and cloud key: the masks of rows, regenerated from a public seed.
// Row r of a call has the ChaCha20 stream (seed, tag, first_idx + r) of host.cpp's Stream: sub-key = words 0 .. 7 of block
// ChaCha20(seed, counter tag << 32, nonce idx), mask word j = the ODD word 2 (j mod 8) + 1 of block ChaCha20(sub-key,
// counter j / 8, nonce 0) (the high half of the stream's j-th 64-bit word): a block yields 8 mask words.  Integer ARX
// only: 32-bit adds, xors and rotates (v_alignbit_b32), and the 64-bit block counter with its carry into the high word.
// Mapping: a workgroup serves R consecutive rows (R = what fits the 32 KiB image, at most 32).  Lane r < R computes row r's
// sub-key into LDS -- one block per row, against len / 8 data blocks --, then every lane computes whole blocks (item = row x
// block, consecutive lanes consecutive blocks) and puts the 8 kept words into the LDS image of the rows; the image leaves with
// lane-contiguous stores.  Three shapes:
//   LWE   out [rows][len + 1], rows 4-byte aligned only (2 004-byte stride on Set A): mask in columns 0 .. len - 1, the body
//         in column len.  The R rows of a workgroup are ONE contiguous span of the output: dword stores, consecutive lanes
//         consecutive words.
//   KSK   out [rows][stride], stride = eoc_ksk_row_stride (a multiple of 256 words): the engine's padded key-switch-key
//         image, body in column len, zeros behind it (the whole row is written).  dwordx4 stores.
//   RING  out [rows][2][N]: a = the stream's N words, b = the row's body [N], copied.  Rows are 16-byte aligned: dwordx4
//         stores, 1 KiB contiguous per wave and instruction.
// A partial last block (len mod 8 != 0) stores its leading words only.  No atomics, no buffer stores, no scratch: every
// array below is indexed by unrolled constants.
// grid: x = ceil(rows / R); block = 256.
// =================================================================================================
constexpr int kSeedImgWords = 8192; // the LDS image of a workgroup's rows
constexpr int kSeedMaxRows = 32;
enum { SEED_LWE = 0, SEED_KSK = 1, SEED_RING = 2 };

struct SeedArgs {
    uint32_t seed[8];
    uint64_t first_idx; // stream index of row 0
    uint64_t rows;
    uint32_t tag;
    uint32_t len;       // mask words per row
    uint32_t R;         // rows per workgroup
    uint32_t stride;    // words per output row (LWE: len + 1, KSK: the padded stride; RING: unused)
    const int32_t *bodies; // LWE / KSK: [rows]; RING: [rows][N]
    int32_t *out;
};

__device__ __forceinline__ uint32_t cc_rotl(uint32_t x, int k) { return (x << k) | (x >> (32 - k)); }
// the 20 rounds on x, in place
__device__ __forceinline__ void chacha20_rounds(uint32_t (&x)[16])
{
#define EOC_CC_QR(a, b, c, d)                                                                   \
    x[a] += x[b]; x[d] = cc_rotl(x[d] ^ x[a], 16); x[c] += x[d]; x[b] = cc_rotl(x[b] ^ x[c], 12); \
    x[a] += x[b]; x[d] = cc_rotl(x[d] ^ x[a], 8);  x[c] += x[d]; x[b] = cc_rotl(x[b] ^ x[c], 7)
#pragma unroll 1
    for (int r = 0; r < 10; r++) {
        EOC_CC_QR(0, 4, 8, 12); EOC_CC_QR(1, 5, 9, 13); EOC_CC_QR(2, 6, 10, 14); EOC_CC_QR(3, 7, 11, 15);
        EOC_CC_QR(0, 5, 10, 15); EOC_CC_QR(1, 6, 11, 12); EOC_CC_QR(2, 7, 8, 13); EOC_CC_QR(3, 4, 9, 14);
    }
#undef EOC_CC_QR
}
// original ChaCha layout: constants | key | 64-bit block counter | 64-bit nonce (host.cpp, chacha20_block)
__device__ __forceinline__ void chacha20_init(uint32_t (&x)[16], const uint32_t (&key)[8], uint64_t counter, uint64_t nonce)
{
    x[0] = 0x61707865u; x[1] = 0x3320646eu; x[2] = 0x79622d32u; x[3] = 0x6b206574u;
#pragma unroll
    for (int k = 0; k < 8; k++) x[4 + k] = key[k];
    x[12] = (uint32_t)counter; x[13] = (uint32_t)(counter >> 32);
    x[14] = (uint32_t)nonce; x[15] = (uint32_t)(nonce >> 32);
}

template <int MODE>
__global__ __launch_bounds__(256) void k_seed_masks(SeedArgs A)
{
    __shared__ __attribute__((aligned(16))) uint32_t s_img[kSeedImgWords];
    __shared__ uint32_t s_sub[kSeedMaxRows][8];
    const uint32_t tid = threadIdx.x;
    const uint64_t row0 = (uint64_t)blockIdx.x * A.R;
    const uint64_t left = A.rows - row0;
    const uint32_t R = left < A.R ? (uint32_t)left : A.R;
    const uint32_t istride = MODE == SEED_RING ? (uint32_t)kN : A.stride;

    if (tid < R) { // the row's sub-key: the tag sits in the high counter word, the stream index is the nonce
        uint32_t x[16];
        chacha20_init(x, A.seed, (uint64_t)A.tag << 32, A.first_idx + row0 + tid);
        chacha20_rounds(x);
        // the first half of the block: constants + x, then key words 0 .. 3 + x
        s_sub[tid][0] = x[0] + 0x61707865u;
        s_sub[tid][1] = x[1] + 0x3320646eu;
        s_sub[tid][2] = x[2] + 0x79622d32u;
        s_sub[tid][3] = x[3] + 0x6b206574u;
#pragma unroll
        for (int k = 0; k < 4; k++) s_sub[tid][4 + k] = x[4 + k] + A.seed[k];
    }
    if (MODE != SEED_RING) { // body in column len; the key image's padding is zero
        for (uint32_t r = tid; r < R; r += 256) s_img[r * istride + A.len] = (uint32_t)A.bodies[row0 + r];
        if (MODE == SEED_KSK) {
            const uint32_t pad = istride - A.len - 1;
            for (uint32_t i = tid; i < R * pad; i += 256) s_img[(i / pad) * istride + A.len + 1 + i % pad] = 0u;
        }
    }
    __syncthreads();

    const uint32_t nb = (A.len + 7) / 8;
    for (uint32_t it = tid; it < R * nb; it += 256) {
        const uint32_t r = it / nb, b = it - r * nb;
        uint32_t key[8], x[16];
#pragma unroll
        for (int k = 0; k < 8; k++) key[k] = s_sub[r][k];
        chacha20_init(x, key, (uint64_t)b, 0);
        chacha20_rounds(x);
        // the odd words: 1, 3 are constants + x, 5 .. 11 key words + x, 13 the high counter word (0) + x, 15 the nonce (0) + x
        const uint32_t w[8] = {x[1] + 0x3320646eu, x[3] + 0x6b206574u, x[5] + key[1], x[7] + key[3],
                               x[9] + key[5],      x[11] + key[7],     x[13],         x[15]};
        uint32_t *dst = s_img + r * istride + b * 8;
        if (b * 8 + 8 <= A.len) {
#pragma unroll
            for (int k = 0; k < 8; k++) dst[k] = w[k];
        } else {
#pragma unroll
            for (int k = 0; k < 8; k++)
                if (b * 8 + k < A.len) dst[k] = w[k];
        }
    }
    __syncthreads();

    if (MODE == SEED_LWE) { // rows row0 .. row0 + R - 1 are one span of the output
        int32_t *o = A.out + row0 * istride;
        for (uint32_t i = tid; i < R * istride; i += 256) o[i] = (int32_t)s_img[i];
    } else if (MODE == SEED_KSK) {
        uint4 *o = reinterpret_cast<uint4 *>(A.out + row0 * istride);
        const uint4 *img = reinterpret_cast<const uint4 *>(s_img);
        for (uint32_t i = tid; i < R * (istride / 4); i += 256) o[i] = img[i];
    } else {
        const uint4 *img = reinterpret_cast<const uint4 *>(s_img);
        for (uint32_t i = tid; i < R * (kN / 4); i += 256) {
            const uint64_t row = row0 + (i >> 8);
            const uint32_t c = i & 255;
            uint4 *o = reinterpret_cast<uint4 *>(A.out + row * (2 * kN));
            o[c] = img[i];
            o[kN / 4 + c] = reinterpret_cast<const uint4 *>(A.bodies + row * kN)[c];
        }
    }
}

// block i of [n_blocks][16] = ChaCha20(key, counter + i, nonce): the block function above, all 16 words (known-answer tests).
template <int WORDS>
__global__ __launch_bounds__(256) void k_chacha20_blocks(SeedArgs A, uint64_t counter, uint64_t nonce, uint32_t *__restrict__ out)
{
    static_assert(WORDS == 16, "whole blocks");
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= A.rows) return;
    uint32_t x[16], s[16];
    chacha20_init(x, A.seed, counter + i, nonce);
#pragma unroll
    for (int k = 0; k < 16; k++) s[k] = x[k];
    chacha20_rounds(x);
    uint4 *o = reinterpret_cast<uint4 *>(out + i * 16);
#pragma unroll
    for (int k = 0; k < 4; k++)
        o[k] = make_uint4(x[4 * k] + s[4 * k], x[4 * k + 1] + s[4 * k + 1], x[4 * k + 2] + s[4 * k + 2], x[4 * k + 3] + s[4 * k + 3]);
}

// =================================================================================================
// Finite automata on encrypted bit strings: one backward step over all states.
//   next[q] = A + C (x) (B - A),  A = X^(-w0(q)) prev[next0(q)],  B = X^(-w1(q)) prev[next1(q)]
// prev, next: state vectors [states][2][N] of TLWE samples per query; C: the query's converted selector of this step's input
// bit (one per query, shared by its states); the transition record {next0, w0, next1, w1} of state q is public, validated on
// the host (next in [0, states), w in [0, 2N)) and read once per wave pair through a uniform address.  The external product
// is k_cmux's -- the same text (ext_product_pair.inc) --, so a step equals the CMux of the two rotated successors bit for bit
// by construction.  The mapping, the LDS plan and the dead pair's rule are the leveled frame (leveled_pair.inc, described
// above k_cmux); BOTH operands are gathered and rotated by index arithmetic on their loads (coefficient j of X^(-w) P is
// P[(j + w) mod 2N], negated in the upper half of the period), lane-contiguous up to the one wrap; A is not held across the
// product but reloaded at store time, as k_cmux reloads in0.
// prev_y = 0 reads one shared vector for every query (the first step reads the final vector in place).  next may not
// overlap prev: a state may be its own successor, so the driver alternates two buffers.
// grid: x = ceil(nx / kCmuxItemsPerWG) states, y = queries.
// =================================================================================================
struct AutoTrans {
    int32_t next0, w0, next1, w1; // successor and weight under bit 0 / bit 1
};
static_assert(sizeof(AutoTrans) == 16, "one 16-byte record per state");

struct AutoStepArgs {
    const d2 *sel;          // converted selectors, one per query
    const AutoTrans *trans; // [nx] records, validated by the host
    const int32_t *prev;    // [states][2][N] per query
    int32_t *next;          // [nx][2][N] per query
    size_t sel_y;           // strides per query, in d2 ...
    size_t prev_y, next_y;  // ... and in int32 (prev_y = 0: one vector for all queries)
    uint32_t nx;            // states along x
    int Bgbit;
};

// k_automaton_step<L, BGBIT> and its rounding twin k_rstep<L, BGBIT>: one text, leveled_kernels.inc
#define EOC_LEVELED_KERNEL 3
#define EOC_LEVELED_ROUND 0
#include "leveled_kernels.inc"
#define EOC_LEVELED_KERNEL 3
#define EOC_LEVELED_ROUND 1
#include "leveled_kernels.inc"
#undef EOC_NEGACYCLIC

// =================================================================================================
// Inner products with public integer weights: output sample (b, r) is the LWE sample under s' with phase
//   bias[r] + sum_k w[r][k] phase(slot k of vector b),
// vector b = L compact lists [L][2][N], input k in slot k mod N of list k / N, w int8 in [-127, 127].  With the weight
// polynomial V_{r,l}: V[0] = w[r][lN], V[N - k] = -w[r][lN + k], coefficient 0 of V C is sum_k w_k C[k], so the sample is
// slot 0 of sum_l V_{r,l} (c0, c1)_{b,l}: mask a'_0 = P0[0], a'_i = -P0[N - i] with P0 = sum_l V_{r,l} c0_{b,l}, and body
// b' = bias[r] + sum_k w[r][k] c1_b[k], an exact wrapping integer sum (no transform).
// Format rule: the products of 8 consecutive lists (a chunk) are accumulated in the spectral domain, l ascending, the
// weight spectrum (k_fft_fwd_polys at scale 1) in the digit's place and the list spectrum (k_fft_fwd_polys at scale 2^-9)
// in the key row's; every chunk is inverse-transformed and converted once (|.| <= 8 * 1024 * 127 * 2^31 < 2^51:
// wrap_trunc's contract holds unconditionally).  Chunks combine by integer addition, so their order -- and the atomics
// below -- cannot change a bit.
// =================================================================================================
constexpr int kDotChunk = 8;      // lists per inverse transform (part of the format)
constexpr int kDotWavesPerWG = 4;
constexpr int kDotLds = (kTwEntries + kNH + kDotWavesPerWG * kScr) * 16; // 53 760 bytes: two workgroups per CU

// Start of every output sample and the whole body: one workgroup per sample s = b rows + r of the slice.  The mask row
// mask[s mask_stride + i], i < N, is filled with `fill` (0, or the key switch's 2^(31 - t basebit): k_dot_mask then adds
// the mask words and the row is the key switch's operand, as k_compact_expand leaves it); body[s body_stride + m] = 0 for
// m < nzero and body[s body_stride + body_at] = b'.  wts: the zero-padded weights [rows][L N] int8 behind the spectra of
// the device image; lists: [batch][L][2][N].  grid: x = samples; block = 256.
// Both kernels are templates (OPERAND: the key-switch form, whose body row is cleared in front of b'; CHUNK: the format's
// chunk).
template <bool OPERAND>
__global__ __launch_bounds__(256) void k_dot_init(const int8_t *__restrict__ wts, const int32_t *__restrict__ lists,
                                                   const int32_t *__restrict__ bias, uint32_t rows, uint32_t L,
                                                   uint32_t *__restrict__ mask, size_t mask_stride, uint32_t fill,
                                                   int32_t *__restrict__ body, size_t body_stride, int nzero, int body_at)
{
    __shared__ uint32_t s_part[4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const uint32_t s = blockIdx.x, b = s / rows, r = s - b * rows;
    const int8_t *w = wts + (size_t)r * L * kN;
    const int32_t *c1 = lists + (size_t)b * L * 2 * kN + kN;
    uint32_t acc = 0;
    for (uint32_t l = 0; l < L; l++)
        for (int j = tid; j < kN; j += 256)
            acc += (uint32_t)(int32_t)w[(size_t)l * kN + j] * (uint32_t)c1[(size_t)l * 2 * kN + j];
#pragma unroll
    for (int o = 32; o; o >>= 1) acc += __shfl_down(acc, o, 64);
    if (lane == 0) s_part[wv] = acc;
    uint32_t *row = mask + (size_t)s * mask_stride;
    for (int i = tid; i < kN; i += 256) row[i] = fill;
    int32_t *o = body + (size_t)s * body_stride;
    if constexpr (OPERAND) // the key switch's output row (0, ..., 0, b'); the sample form has its mask there
        for (int m = tid; m < nzero; m += 256) o[m] = 0;
    __syncthreads();
    if (tid == 0) o[body_at] = (int32_t)((bias ? (uint32_t)bias[r] : 0u) + s_part[0] + s_part[1] + s_part[2] + s_part[3]);
}

// One WAVE per (sample, chunk), as k_pack_rows: the one spectral accumulator stays in registers, nothing is exchanged
// between waves, one barrier (the tables).  wspec [rows][L][512] complex, lspec [batch][L][2][512] complex (both
// polynomials of every list are transformed by the one k_fft_fwd_polys launch; polynomial 0 is read), both 16 bytes per
// lane, 1 KiB per wave and instruction.  The first list of a chunk starts the chain as a plain product (cmul0, as every
// chain).  Coefficient j of the chunk's product goes to mask word (N - j) mod N, negated for j > 0: vector integer atomics,
// lane-contiguous (descending).
// grid: x = ceil(items / 4), items = samples x chunks; block = 256.
template <int CHUNK>
__global__ __launch_bounds__(64 * kDotWavesPerWG, 2) void k_dot_mask(const d2 *__restrict__ wspec, const d2 *__restrict__ lspec,
                                                                     uint32_t *__restrict__ mask, size_t mask_stride,
                                                                     uint32_t rows, uint32_t L, uint32_t nchunks,
                                                                     uint32_t items, const d2 *__restrict__ g_tw,
                                                                     const d2 *__restrict__ g_twist)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    d2 *s_tw = reinterpret_cast<d2 *>(smem);
    d2 *s_twist = s_tw + kTwEntries;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    d2 *scr = s_twist + kNH + wv * kScr;
    load_tables(s_tw, s_twist, g_tw, g_twist, tid, 64 * kDotWavesPerWG);
    __syncthreads(); // the tables; the only barrier
    const uint32_t item = blockIdx.x * kDotWavesPerWG + (uint32_t)wv;
    if (item >= items) return;
    const uint32_t s = item / nchunks, chunk = item - s * nchunks;
    const uint32_t b = s / rows, r = s - b * rows;
    const uint32_t l_first = chunk * CHUNK, l_end = min(l_first + (uint32_t)CHUNK, L);

    const d2 *pw = wspec + ((size_t)r * L + l_first) * kNH + lane;
    const d2 *pc = lspec + ((size_t)b * L + l_first) * 2 * kNH + lane;
    d2 S[8];
#pragma unroll
    for (int q = 0; q < 8; q++) S[q] = cmul0(pw[q * 64], pc[q * 64]);
#pragma unroll 1
    for (uint32_t l = l_first + 1; l < l_end; l++) {
        pw += kNH;
        pc += 2 * kNH;
#pragma unroll
        for (int q = 0; q < 8; q++) S[q] = cmac1(pw[q * 64], pc[q * 64], S[q]);
    }

    int *po = reinterpret_cast<int *>(mask + (size_t)s * mask_stride);
    d2 ut[8];
    fft_inv_wave(S, ut, s_tw, s_twist, scr, lane);
#pragma unroll
    for (int q = 0; q < 8; q++) {
        const int j = lane + 64 * q;
        const d2 y = cmulc(S[q], ut[q]); // 1/512 is in the list image
        const uint32_t vx = wrap_trunc(y.x), vy = wrap_trunc(y.y);
        atomicAdd(po + ((kN - j) & (kN - 1)), (int)(j ? 0u - vx : vx));
        atomicAdd(po + (kNH - j), (int)(0u - vy));
    }
}

// =================================================================================================
// Convolutions with public int8 kernels: the WHOLE product the inner product takes one slot of.  Same
// weights, same image, same lists, same format rule; output (vector b, row r) is the TLWE list
//   ( sum_l V_{r,l} c0_{b,l} ,  bias[r] + sum_l V_{r,l} c1_{b,l} )                                        [2][N] int32
// whose slot t has phase bias[r] + sum_l sum_k w[r][lN + k] x_l[t + k], terms with t + k >= N entering negated (the
// negacyclic wrap): a cross-correlation of input channel l (list l) with filter (r, l).  Both polynomials go through the
// chunks of the inner product (8 lists, l ascending, cmul0 / cmac1, one inverse transform and one wrap_trunc per chunk
// and polynomial; chunks combine by wrapping integer addition; the bias is added to every word of c1).  c0 is the
// inner product's P0: word j here is mask word (N - j) mod N there, negated for j > 0, bit for bit.
// All three kernels are templates (CHUNK: the format's chunk; SINGLE: one chunk per output; THREADS, G: the block and the
// table entries per workgroup).
// =================================================================================================

// Start of every output list when several chunks add into it: c0 = 0, c1 = bias[r] in every word.  One workgroup per
// list s = b rows + r of the slice, lane-contiguous words.  grid: x = lists; block = THREADS.
template <int THREADS>
__global__ __launch_bounds__(THREADS) void k_conv_init(const int32_t *__restrict__ bias, uint32_t rows, int32_t *__restrict__ out)
{
    const uint32_t s = blockIdx.x, r = s % rows;
    const uint32_t bv = bias ? (uint32_t)bias[r] : 0u;
    int32_t *o = out + (size_t)s * (2 * kN);
    for (int i = threadIdx.x; i < kN; i += THREADS) {
        o[i] = 0;
        o[kN + i] = (int32_t)bv;
    }
}

// One WAVE per (output list, chunk, polynomial): k_dot_mask's frame (4 waves per workgroup, kDotLds, one barrier, one
// spectral accumulator in registers, the shared device functions only).  The polynomial is the fastest-varying part of the
// item index: the two waves that read the same weight rows sit in one workgroup.  wspec [rows][L][512] complex, lspec
// [batch][L][2][512] complex -- both polynomials of the one k_fft_fwd_polys launch are read.  Coefficient j of the chunk's
// product goes to word j of its polynomial.  SINGLE (nchunks == 1): plain vector stores with the bias folded in, no init
// launch, no atomics; otherwise vector integer atomics on the lists k_conv_init started.
// grid: x = ceil(items / 4), items = lists x chunks x 2; block = 256.
template <int CHUNK, bool SINGLE>
__global__ __launch_bounds__(64 * kDotWavesPerWG, 2) void k_conv_lists(const d2 *__restrict__ wspec, const d2 *__restrict__ lspec,
                                                                       const int32_t *__restrict__ bias, int32_t *__restrict__ out,
                                                                       uint32_t rows, uint32_t L, uint32_t nchunks, uint32_t items,
                                                                       const d2 *__restrict__ g_tw, const d2 *__restrict__ g_twist)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    d2 *s_tw = reinterpret_cast<d2 *>(smem);
    d2 *s_twist = s_tw + kTwEntries;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    d2 *scr = s_twist + kNH + wv * kScr;
    load_tables(s_tw, s_twist, g_tw, g_twist, tid, 64 * kDotWavesPerWG);
    __syncthreads(); // the tables; the only barrier
    const uint32_t item = blockIdx.x * kDotWavesPerWG + (uint32_t)wv;
    if (item >= items) return;
    const uint32_t poly = item & 1u, sc = item >> 1;
    const uint32_t s = SINGLE ? sc : sc / nchunks, chunk = SINGLE ? 0u : sc - s * nchunks;
    const uint32_t b = s / rows, r = s - b * rows;
    const uint32_t l_first = chunk * CHUNK, l_end = min(l_first + (uint32_t)CHUNK, L);

    const d2 *pw = wspec + ((size_t)r * L + l_first) * kNH + lane;
    const d2 *pc = lspec + (((size_t)b * L + l_first) * 2 + poly) * kNH + lane;
    d2 S[8];
#pragma unroll
    for (int q = 0; q < 8; q++) S[q] = cmul0(pw[q * 64], pc[q * 64]);
#pragma unroll 1
    for (uint32_t l = l_first + 1; l < l_end; l++) {
        pw += kNH;
        pc += 2 * kNH;
#pragma unroll
        for (int q = 0; q < 8; q++) S[q] = cmac1(pw[q * 64], pc[q * 64], S[q]);
    }

    int *po = out + ((size_t)s * 2 + poly) * kN;
    uint32_t bv = 0u;
    if constexpr (SINGLE) bv = (poly && bias) ? (uint32_t)bias[r] : 0u;
    d2 ut[8];
    fft_inv_wave(S, ut, s_tw, s_twist, scr, lane);
#pragma unroll
    for (int q = 0; q < 8; q++) {
        const int j = lane + 64 * q;
        const d2 y = cmulc(S[q], ut[q]); // 1/512 is in the list image
        const uint32_t vx = wrap_trunc(y.x), vy = wrap_trunc(y.y);
        if constexpr (SINGLE) {
            po[j] = (int)(vx + bv);
            po[j + kNH] = (int)(vy + bv);
        } else {
            atomicAdd(po + j, (int)vx);
            atomicAdd(po + j + kNH, (int)vy);
        }
    }
}

// k_compact_expand with a public slot table: sample (b, s), s < n_slots, is slot slots[s] mod N of list slots[s] / N of
// vector b's `lists_per_vec` lists, and becomes key-switch operand row b n_slots + s (ubar: a'_i + 2^(31 - t basebit)) and
// output row b n_slots + s (0, ..., 0, b').  The table is validated when it is loaded (eoc_conv_slots_to_device); a list
// index past the vector is held to its last list all the same, so no table can make the kernel read outside the vector.
// Slots may be unordered and may repeat.  A workgroup serves G consecutive table entries of one vector and stages c0 of
// the list at hand in LDS, again whenever the list changes (the table is uniform over the workgroup, so every thread
// reaches the same barriers); the same lane-contiguous loads and stores as k_compact_expand.
// grid: x = ceil(n_slots / G), y = vectors of the slice; block = 256.
template <int G>
__global__ __launch_bounds__(256) void k_conv_extract(const int32_t *__restrict__ lists, uint32_t lists_per_vec,
                                                      const uint32_t *__restrict__ slots, uint32_t n_slots,
                                                      uint32_t *__restrict__ ubar, int32_t *__restrict__ out, int n,
                                                      uint32_t prec_offset)
{
    __shared__ int32_t s_c0[kN];
    const int32_t *vec = lists + (size_t)blockIdx.y * lists_per_vec * (2 * kN);
    uint32_t staged = 0xFFFFFFFFu;
    const int32_t *list = vec;
    for (int q = 0; q < G; q++) {
        const uint32_t t = blockIdx.x * G + q;
        if (t >= n_slots) break;
        const uint32_t slot = slots[t];
        const uint32_t li = min(slot / (uint32_t)kN, lists_per_vec - 1u);
        const int j = (int)(slot % (uint32_t)kN);
        if (li != staged) {
            __syncthreads(); // every row of the list staged before is written
            list = vec + (size_t)li * (2 * kN);
            for (int k = threadIdx.x; k < kN; k += 256) s_c0[k] = list[k];
            __syncthreads();
            staged = li;
        }
        const size_t s = (size_t)blockIdx.y * n_slots + t;
        uint32_t *row = ubar + s * kN;
        for (int i = threadIdx.x; i < kN; i += 256) {
            const uint32_t v = (uint32_t)s_c0[(j - i) & (kN - 1)];
            row[i] = (i <= j ? v : 0u - v) + prec_offset;
        }
        int32_t *o = out + s * (n + 1);
        for (int m = threadIdx.x; m < n; m += 256) o[m] = 0;
        if (threadIdx.x == 0) o[n] = list[kN + j];
    }
}

} // namespace eoc
