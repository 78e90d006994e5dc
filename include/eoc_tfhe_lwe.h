/* eoc_tfhe_lwe.h -- dense layers on LWE samples: a public int8 matrix applied to batches of samples, an exact integer matrix
 * product on the matrix cores.  Plain C; includes eoc_tfhe_gpu.h, whose types and error codes it uses.  The unit
 * has a header of its own because its kernel lives in a code object of its own (csrc/lwe_matmul.hip); folding these entries
 * into eoc_tfhe_gpu.h belongs to the change that also enters them in the test-side kernel ledger and interleave cases. */
#ifndef EOC_TFHE_LWE_H
#define EOC_TFHE_LWE_H

#include "eoc_tfhe_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- dense layers on LWE samples ----------------------------------------------------------------------------
 * A weighted sum of many encrypted values with PUBLIC weights on the samples the engine itself produces and consumes -- gate
 * outputs, LUT outputs, the samples eoc_seeded_expand_device regenerates --, with no list, no packing key and no key switch:
 * FHE-DiNN's dense layer in its original form.  The output is a sample under the same key and of the same dimension.
 *   weights     w[rows][cols] int8, every value in [-127, 127] (-128: EOC_ERR_ARG).  bias[rows] Torus32, optional.
 *               rows in [1, 2^20], cols in [1, 2^16] (2^16 * 127 * 128 < 2^31: every limb accumulator stays inside int32).
 *   inputs      d_cts [batch][cols][width] int32: `batch` vectors of `cols` samples of `width` words each, width in [1, 4096]:
 *               n + 1 for ordinary samples, N + 1 for samples in front of a key switch; any other width is taken too -- the rule
 *               is per word and does not know what a word means.
 *   output      d_out [batch][rows][width] int32.
 *   rule        wrapping 32-bit arithmetic, word by word:  out[b][r][j] = sum_k w[r][k] cts[b][k][j]  (mod 2^32)  for every j;
 *               bias[r] is added to the BODY word, j = width - 1 (a sample is its mask words, then its body, as every [n+1]
 *               sample of eoc_tfhe_gpu.h).  The result is an integer: the kernel's words are those of the four-line reference
 *               (w as int64) @ (cts as uint32 as int64) & 0xffffffff, whatever the order of the terms.
 *               On the device: k_lwe_matmul, v_mfma_i32_32x32x32_i8.  Every ciphertext word v is split into four signed bytes
 *               in registers by the carry-free rule  v == sum_j t_j 2^(8 j) + 0x80808080,  t_j the signed byte j of
 *               v ^ 0x80808080; four int32 accumulator tiles per (row tile, column tile) are recombined in-lane as
 *               acc0 + (acc1 << 8) + (acc2 << 16) + (acc3 << 24), and 0x80808080 sum_k w[r][k] is added per row.  (The carry
 *               rule l_0 = ((v + 128) & 255) - 128, v <- (v - l_0) >> 8, ... of the key-switch limb image gives the same words.)
 *   alignment   every buffer needs 4-byte alignment only.
 *   image       eoc_lwe_weights_to_device builds the model's device image once, on the host: the A operand's fragments
 *               [ceil(rows / 32)][ceil(cols / 32)][64 lanes][16 B] -- lane (h = lane >> 5, r = lane & 31) of fragment (rt, ks)
 *               holds w[32 rt + r][32 ks + 16 h + i] in byte i, ZERO past rows and cols --, then the per-row corrections
 *               [32 ceil(rows / 32)] int32, 0x80808080 sum_k w[r][k] mod 2^32.  eoc_lwe_weights_image_bytes(rows, cols) =
 *               ceil(rows / 32) (1024 ceil(cols / 32) + 128) bytes (0 for a shape that is refused).  A model load, as
 *               eoc_weights_to_device: checked on the host, no key, drains `hip_stream` (EOC_ERR_STATE under capture).
 *   noise       the error of an output is exactly sum_k w_k e_k: noise.lwe_linear_var = |w|^2 x the inputs' variance, nothing
 *               else -- no packing error on the inputs, no key-switch error on the output (Network.check(hidden="lwe")).
 *   security    nothing new: a public linear map of ciphertexts.
 *   engine      eoc_lwe_matmul_device needs NO key and NO workspace, takes its arguments as kernel arguments (no descriptor ring
 *               slot) and is legal under capture.  batch x rows = 0 is a no-op; EOC_ERR_ARG for a null pointer (d_bias may be
 *               NULL), a shape out of range, an output that overlaps the samples, the image or the bias: the output is then
 *               untouched.  eoc_engine_lwe_matmul_launches counts one per launch (one per 65 535 vectors);
 *               eoc_engine_kernel_times books the kernel under the key switch.
 *   host        eoc_lwe_matmul: host buffers on the global context (no key needed), synchronous; WHOLE input vectors are cut
 *               into eoc_shard_range blocks, one per engine; every engine builds the image itself. */
size_t eoc_lwe_weights_image_bytes(size_t rows, size_t cols);
int eoc_lwe_weights_to_device(eoc_engine *e, const int8_t *h_w, size_t rows, size_t cols, void *d_image, void *hip_stream);
int eoc_lwe_matmul_device(eoc_engine *e, const void *d_image, size_t rows, size_t cols, const int32_t *d_cts, size_t width,
                          size_t batch, const int32_t *d_bias /* may be NULL */, int32_t *d_out, void *hip_stream);
uint64_t eoc_engine_lwe_matmul_launches(eoc_engine *e);
int eoc_lwe_matmul(const int8_t *h_w, size_t rows, size_t cols, const int32_t *h_cts, size_t width, size_t batch,
                   const int32_t *h_bias /* may be NULL */, int32_t *h_out);

#ifdef __cplusplus
}
#endif
#endif /* EOC_TFHE_LWE_H */
