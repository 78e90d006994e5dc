// lwe_matmul.h -- what engine.hip sees of the library's third code object, lwe_matmul.hip (include/eoc_tfhe_lwe.h,
// DESIGN.md 25): the shape rule, the weight image's size and host-side builder, and the launcher of k_lwe_matmul.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace eoc {

constexpr size_t kLweMaxRows = (size_t)1 << 20;  // grid y stays below 65 536 row-tile pairs
constexpr size_t kLweMaxCols = (size_t)1 << 16;  // 2^16 * 127 * 128 < 2^31: every limb accumulator stays inside int32
constexpr size_t kLweMaxWidth = 4096;            // words per sample

static inline bool lwe_shape_ok(size_t rows, size_t cols)
{
    return rows >= 1 && cols >= 1 && rows <= kLweMaxRows && cols <= kLweMaxCols;
}
// bytes of the image of a rows x cols model: the operand fragments [ceil(rows / 32)][ceil(cols / 32)][64 lanes][16 B], then
// the per-row corrections [32 ceil(rows / 32)] int32; 0 for a refused shape
size_t lwe_image_bytes(size_t rows, size_t cols);
// the image of w[rows][cols] (every value in [-127, 127], checked by the caller) into lwe_image_bytes(rows, cols) host bytes
void lwe_image_build(const int8_t *w, size_t rows, size_t cols, void *h_image);
// out[b][r][j] = sum_k w[r][k] cts[b][k][j] (+ bias[r] on the body word j = width - 1), mod 2^32; shapes checked by the
// caller, batch * rows > 0.  *launches is raised by the kernel launches made (one per 65 535 vectors)
hipError_t lwe_matmul_launch(const void *d_image, size_t rows, size_t cols, const int32_t *d_cts, size_t width, size_t batch,
                             const int32_t *d_bias, int32_t *d_out, hipStream_t st, uint64_t *launches);

} // namespace eoc
