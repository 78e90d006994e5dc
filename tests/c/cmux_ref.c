/* cmux_ref.c -- test-side reference of the external product behind eoc_cmux_device.
 *
 * One function: r = C (x) D for an ARBITRARY TLWE difference D, restating the FFT path of orc_blind_rotate_step
 * (oracle/tfhe_oracle.c) -- truncating gadget decomposition with the offset, 2l forward transforms, for output polynomial
 * c ONE chain over the 2l terms (the digits of the other input polynomial first, then the own ones; first term a plain
 * product, every later term four explicit fused multiply-adds), one inverse transform.  The transforms are liboracle.so's.
 * tests/test_cmux_cpu.py pins it to orc_blind_rotate_step itself for D = (X^a - 1) acc.
 * Compiled by tests/cmux_oracle.py with gcc -ffp-contract=off: every fma below is written out. */
#include <math.h>
#include <stdint.h>

#include "tfhe_oracle.h"

/* sel_fft: [2l][2][N doubles] = orc_fft_fwd of every polynomial of the selector (unscaled, as orc_bk_to_fft);
 * D, r: [2][N] */
void cmux_ref_extprod(const orc_params *p, const double *sel_fft, const int32_t *D, int32_t *r)
{
    const int l = p->l, Bgbit = p->Bgbit;
    const uint32_t Bg = 1u << Bgbit;
    static _Thread_local double X[2][4][ORC_N];
    uint32_t off = 0;
    for (int pp = 1; pp <= l; pp++) off += (Bg >> 1) << (32 - pp * Bgbit);
    for (int q = 0; q < 2; q++)
        for (int pp = 1; pp <= l; pp++) {
            int32_t dec[ORC_N];
            for (int j = 0; j < ORC_N; j++) {
                const uint32_t u = (uint32_t)D[q * ORC_N + j] + off;
                dec[j] = (int32_t)((u >> (32 - pp * Bgbit)) & (Bg - 1)) - (int32_t)(Bg >> 1);
            }
            orc_fft_fwd(dec, X[q][pp - 1]);
        }
    for (int c = 0; c < 2; c++) {
        double S[ORC_N];
        int first = 1;
        for (int qq = 0; qq < 2; qq++) {
            const int q = qq == 0 ? 1 - c : c;
            for (int pp = 1; pp <= l; pp++) {
                const double *B = sel_fft + ((size_t)(q * l + (pp - 1)) * 2 + c) * ORC_N;
                const double *x = X[q][pp - 1];
                for (int e = 0; e < ORC_NH; e++) {
                    const double dr = x[2 * e], di = x[2 * e + 1], br = B[2 * e], bi = B[2 * e + 1];
                    if (first) {
                        S[2 * e] = fma(-di, bi, dr * br);
                        S[2 * e + 1] = fma(di, br, dr * bi);
                    } else {
                        S[2 * e] = fma(-di, bi, fma(dr, br, S[2 * e]));
                        S[2 * e + 1] = fma(di, br, fma(dr, bi, S[2 * e + 1]));
                    }
                }
                first = 0;
            }
        }
        orc_fft_inv(S, r + c * ORC_N);
    }
}
