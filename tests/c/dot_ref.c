/* dot_ref.c -- test-side reference of the inner product with public integer weights behind eoc_dot_device.
 *
 * One output sample (vector b, row r): the LWE sample [N+1] under s' of phase bias + sum_k w[k] phase(slot k).  The weight
 * polynomial of list l is V[0] = w[lN], V[N - k] = -w[lN + k]; the mask is slot 0 of P0 = sum_l V_l c0_l, a'_0 = P0[0],
 * a'_i = -P0[N - i], and the body is bias + sum_k w[k] c1[k] as a wrapping integer sum.  Inside a chunk of 8 lists the
 * products are accumulated in the spectral domain, l ascending, the weight spectrum in the digit's place and the list
 * spectrum in the key row's -- first term a plain product, every later term four explicit fused multiply-adds (cmux_ref.c's
 * nesting) -- then ONE inverse transform and conversion, added as int32.  The transforms are liboracle.so's.
 * Compiled by tests/dot_oracle.py with gcc -ffp-contract=off: every fma below is written out. */
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "tfhe_oracle.h"

#define DOT_CHUNK 8

/* w: the row's weights, zero-padded to [L N] int8; lists: the vector's lists [L][2][N]; out: [N+1].
 * Only chunks [chunk_lo, chunk_hi) enter the mask (all of them: 0, (L + 7) / 8); the body is always whole.
 * hwm (may be NULL): the largest |value| any chunk held before its conversion is folded into *hwm. */
void dot_ref_sample(const int8_t *w, int L, const int32_t *lists, int32_t bias, int chunk_lo, int chunk_hi, int32_t *out,
                    double *hwm)
{
    uint32_t P0[ORC_N];
    uint32_t body = (uint32_t)bias;
    memset(P0, 0, sizeof P0);
    for (int l = 0; l < L; l++)
        for (int k = 0; k < ORC_N; k++)
            body += (uint32_t)(int32_t)w[(size_t)l * ORC_N + k] * (uint32_t)lists[((size_t)l * 2 + 1) * ORC_N + k];
    for (int c = chunk_lo; c < chunk_hi; c++) {
        static _Thread_local double S[ORC_N], X[ORC_N], B[ORC_N], raw[ORC_N];
        const int l_end = (c + 1) * DOT_CHUNK < L ? (c + 1) * DOT_CHUNK : L;
        for (int l = c * DOT_CHUNK; l < l_end; l++) {
            int32_t V[ORC_N];
            V[0] = w[(size_t)l * ORC_N];
            for (int k = 1; k < ORC_N; k++) V[ORC_N - k] = -(int32_t)w[(size_t)l * ORC_N + k];
            orc_fft_fwd(V, X);
            orc_fft_fwd(lists + (size_t)l * 2 * ORC_N, B);
            for (int e = 0; e < ORC_NH; e++) {
                const double dr = X[2 * e], di = X[2 * e + 1], br = B[2 * e], bi = B[2 * e + 1];
                if (l == c * DOT_CHUNK) {
                    S[2 * e] = fma(-di, bi, dr * br);
                    S[2 * e + 1] = fma(di, br, dr * bi);
                } else {
                    S[2 * e] = fma(-di, bi, fma(dr, br, S[2 * e]));
                    S[2 * e + 1] = fma(di, br, fma(dr, bi, S[2 * e + 1]));
                }
            }
        }
        int32_t r[ORC_N];
        orc_fft_inv(S, r);
        for (int i = 0; i < ORC_N; i++) P0[i] += (uint32_t)r[i];
        if (hwm) {
            orc_fft_inv_raw(S, raw);
            for (int i = 0; i < ORC_N; i++)
                if (fabs(raw[i]) > *hwm) *hwm = fabs(raw[i]);
        }
    }
    uint32_t *o = (uint32_t *)out;
    o[0] = P0[0];
    for (int i = 1; i < ORC_N; i++) o[i] = 0u - P0[ORC_N - i];
    o[ORC_N] = body;
}
