/* conv_ref.c -- test-side reference of the convolution with public int8 kernels behind eoc_conv_device.
 *
 * One output list (vector b, row r): the TLWE list [2][N]
 *     ( sum_l V_l c0_l ,  bias + sum_l V_l c1_l ),   V_l[0] = w[lN], V_l[N - k] = -w[lN + k],
 * whose slot t has phase bias + sum_l sum_k w[lN + k] x_l[t + k], negacyclically.  It is dot_ref.c's rule with the whole
 * product kept and c1 sent through the same transform: inside a chunk of 8 lists the products are accumulated in the spectral
 * domain, l ascending, the weight spectrum in the digit's place and the list spectrum in the key row's -- first term a plain
 * product, every later term four explicit fused multiply-adds -- then ONE inverse transform and conversion per polynomial,
 * added as int32; the bias is added to every word of c1.  The transforms are liboracle.so's.
 * Compiled by tests/conv_oracle.py with gcc -ffp-contract=off: every fma below is written out. */
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "tfhe_oracle.h"

#define CONV_CHUNK 8

/* w: the row's weights, zero-padded to [L N] int8; lists: the vector's lists [L][2][N]; out: [2][N].
 * Only chunks [chunk_lo, chunk_hi) enter (all of them: 0, (L + 7) / 8); the bias is always added.
 * hwm (may be NULL): the largest |value| any chunk of either polynomial held before its conversion is folded into *hwm. */
void conv_ref_lists(const int8_t *w, int L, const int32_t *lists, int32_t bias, int chunk_lo, int chunk_hi, int32_t *out,
                    double *hwm)
{
    uint32_t P[2][ORC_N];
    memset(P, 0, sizeof P);
    for (int c = chunk_lo; c < chunk_hi; c++) {
        static _Thread_local double S[2][ORC_N], X[ORC_N], B[ORC_N], raw[ORC_N];
        const int l_end = (c + 1) * CONV_CHUNK < L ? (c + 1) * CONV_CHUNK : L;
        for (int l = c * CONV_CHUNK; l < l_end; l++) {
            int32_t V[ORC_N];
            V[0] = w[(size_t)l * ORC_N];
            for (int k = 1; k < ORC_N; k++) V[ORC_N - k] = -(int32_t)w[(size_t)l * ORC_N + k];
            orc_fft_fwd(V, X);
            for (int p = 0; p < 2; p++) {
                orc_fft_fwd(lists + ((size_t)l * 2 + p) * ORC_N, B);
                for (int e = 0; e < ORC_NH; e++) {
                    const double dr = X[2 * e], di = X[2 * e + 1], br = B[2 * e], bi = B[2 * e + 1];
                    if (l == c * CONV_CHUNK) {
                        S[p][2 * e] = fma(-di, bi, dr * br);
                        S[p][2 * e + 1] = fma(di, br, dr * bi);
                    } else {
                        S[p][2 * e] = fma(-di, bi, fma(dr, br, S[p][2 * e]));
                        S[p][2 * e + 1] = fma(di, br, fma(dr, bi, S[p][2 * e + 1]));
                    }
                }
            }
        }
        for (int p = 0; p < 2; p++) {
            int32_t r[ORC_N];
            orc_fft_inv(S[p], r);
            for (int i = 0; i < ORC_N; i++) P[p][i] += (uint32_t)r[i];
            if (hwm) {
                orc_fft_inv_raw(S[p], raw);
                for (int i = 0; i < ORC_N; i++)
                    if (fabs(raw[i]) > *hwm) *hwm = fabs(raw[i]);
            }
        }
    }
    uint32_t *o = (uint32_t *)out;
    for (int i = 0; i < ORC_N; i++) {
        o[i] = P[0][i];
        o[ORC_N + i] = P[1][i] + (uint32_t)bias;
    }
}
