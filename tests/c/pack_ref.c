/* pack_ref.c -- test-side reference of the packing key switch behind eoc_pack_device.
 *
 * One output list: out = (0, B) - sum over chunks of 16 key indices of the chunk's converted sum.  Inside a chunk the
 * spectra of the rows (m, j), m ascending then j = 1 .. 4 ascending, are accumulated per output polynomial -- first term a
 * plain product, every later term four explicit fused multiply-adds (cmux_ref.c's nesting) -- then ONE inverse transform
 * and conversion per output polynomial, subtracted as int32.  The digits are the signed base-16 digits of
 * a + 2^15 + sum_p 8 2^(32 - 4p): a rounding decomposition.  The transforms are liboracle.so's.
 * Compiled by tests/pack_oracle.py with gcc -ffp-contract=off: every fma below is written out. */
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "tfhe_oracle.h"

#define PACK_T 4
#define PACK_BASEBIT 4
#define PACK_CHUNK 16

/* rows [npoly][N] int32 -> [npoly][N doubles], unscaled (the device image carries an exact 2^-9) */
void pack_ref_key_fft(const int32_t *rows, size_t npoly, double *out)
{
    for (size_t k = 0; k < npoly; k++) orc_fft_fwd(rows + k * ORC_N, out + k * ORC_N);
}

/* digit polynomial j (1 .. 4) of key index m of `filled` samples in [filled][n+1] */
static void digits(const int32_t *in, int n, int filled, int m, int j, int32_t *dec)
{
    uint32_t off = 1u << (31 - PACK_T * PACK_BASEBIT);
    for (int p = 1; p <= PACK_T; p++) off += 8u << (32 - PACK_BASEBIT * p);
    for (int i = 0; i < ORC_N; i++) {
        const uint32_t a = i < filled ? (uint32_t)in[(size_t)i * (n + 1) + m] : 0u;
        dec[i] = (int32_t)(((a + off) >> (32 - PACK_BASEBIT * j)) & 15u) - 8;
    }
}

/* key_fft: [n][4][2][N doubles]; in: [filled][n+1], filled <= N; out: [2][N]; only chunks [chunk_lo, chunk_hi) are
 * subtracted from (0, B) (all of them: 0, (n + 15) / 16) */
void pack_ref_list(int n, const double *key_fft, const int32_t *in, int filled, int chunk_lo, int chunk_hi, int32_t *out)
{
    uint32_t *o = (uint32_t *)out;
    memset(out, 0, 2 * ORC_N * sizeof(int32_t));
    for (int i = 0; i < filled; i++) o[ORC_N + i] = (uint32_t)in[(size_t)i * (n + 1) + n];
    for (int c = chunk_lo; c < chunk_hi; c++) {
        static _Thread_local double S[2][ORC_N], X[ORC_N];
        int first = 1;
        const int m_end = (c + 1) * PACK_CHUNK < n ? (c + 1) * PACK_CHUNK : n;
        for (int m = c * PACK_CHUNK; m < m_end; m++)
            for (int j = 1; j <= PACK_T; j++) {
                int32_t dec[ORC_N];
                digits(in, n, filled, m, j, dec);
                orc_fft_fwd(dec, X);
                for (int q = 0; q < 2; q++) {
                    const double *B = key_fft + (((size_t)m * PACK_T + (j - 1)) * 2 + q) * ORC_N;
                    double *s = S[q];
                    for (int e = 0; e < ORC_NH; e++) {
                        const double dr = X[2 * e], di = X[2 * e + 1], br = B[2 * e], bi = B[2 * e + 1];
                        if (first) {
                            s[2 * e] = fma(-di, bi, dr * br);
                            s[2 * e + 1] = fma(di, br, dr * bi);
                        } else {
                            s[2 * e] = fma(-di, bi, fma(dr, br, s[2 * e]));
                            s[2 * e + 1] = fma(di, br, fma(dr, bi, s[2 * e + 1]));
                        }
                    }
                }
                first = 0;
            }
        for (int q = 0; q < 2; q++) {
            int32_t r[ORC_N];
            orc_fft_inv(S[q], r);
            for (int i = 0; i < ORC_N; i++) o[q * ORC_N + i] -= (uint32_t)r[i];
        }
    }
}
