// lwe_matmul.hip -- the library's third code object (include/eoc_tfhe_lwe.h): a public int8 matrix applied to
// batches of LWE samples on the matrix cores,
//     out[b][r][j] = sum_k w[r][k] cts[b][k][j]   (mod 2^32)   for every word j of a sample,
// an exact integer matrix product per vector b: M = rows, N = width (the words of a sample), K = cols.  engine.hip holds the
// entry points and calls in here through lwe_matmul.h; nothing of kernels.hip.h is included, so this object's kernel set is
// what this file defines.
//
// The exact signed-byte-limb recipe of k_keyswitch_mfma (kernels.hip.h), with the int32 operand -- there a key, split once at
// install -- split in registers: the CARRY-FREE rule.  With t_j the SIGNED byte j of v ^ 0x80808080,
//     v == t_0 + t_1 2^8 + t_2 2^16 + t_3 2^24 + 0x80808080   (mod 2^32):
// flipping the top bit of a byte subtracts 128 from its unsigned value, and 128 (1 + 2^8 + 2^16 + 2^24) is the constant.  So
//     out = acc_0 + (acc_1 << 8) + (acc_2 << 16) + (acc_3 << 24) + 0x80808080 sum_k w[r][k],   acc_j = sum_k w[r][k] t_j(k),
// four int8 products with int32 accumulators (|acc_j| <= 2^16 * 127 * 128 < 2^31 for cols <= 2^16) and a per-row constant the
// image carries.  The carry rule of k_ksk_limbs gives the same words: the result is an integer, whichever way it is split.
//
//   * A operand = the weights' fragment image [row tile][K step][lane][16 B]: lane (h = lane >> 5, r = lane & 31) holds
//     w[32 rt + r][32 ks + 16 h + i] in byte i, zero past `rows` and `cols`: one 16-byte load per lane, 1 KiB per wave.
//   * B operand: lane (h, c = lane & 31) loads the 16 words cts[b][32 ks + 16 h + i][32 ct + c], i = 0 .. 15 -- sixteen rows of
//     cts at one column, 128 contiguous bytes per half-wave and row --, flips the top bits (one XOR per word) and transposes
//     the 16 x 4 bytes with v_perm_b32 into four fragments, byte i of fragment j = t_j of word i.  The instruction pairs A's and
//     B's bytes of equal (h, byte), which both operands call k = 32 ks + 16 h + i.
//   * C/D: col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 h: the four limbs of an output word sit at the same lane and
//     register of four accumulator tiles, so the recombination is in-lane.
//   * Tails: a row index past `cols` or a column past `width` is held to the last one -- every load is inside the buffer --;
//     the image's zero padding takes the repeated rows out of the sum, and the store mask (row < rows, col < width) takes the
//     repeated columns out of the result.
// A wave owns one column tile of 32 words and kLmmRowTiles row tiles (8 accumulator tiles, 128 registers); a workgroup is
// kLmmWaves waves on consecutive column tiles.  No LDS, no barrier, no atomics: a wave's words are its own.
// grid: x = ceil(ceil(width / 32) / kLmmWaves), y = ceil(ceil(rows / 32) / kLmmRowTiles), z = vectors; block = 64 kLmmWaves.
#include "lwe_matmul.h"

#include <algorithm>
#include <cstring>

namespace eoc {

typedef int lmm_i4 __attribute__((ext_vector_type(4)));
typedef int lmm_i16 __attribute__((ext_vector_type(16)));
typedef lmm_i4 lmm_i4_a4 __attribute__((aligned(4))); // a fragment of the image: the image needs 4-byte alignment only

constexpr int kLmmWaves = 4;    // waves (column tiles) per workgroup
constexpr int kLmmRowTiles = 2; // row tiles per wave
constexpr uint32_t kLmmFlip = 0x80808080u;

__global__ __launch_bounds__(64 * kLmmWaves, 2) void k_lwe_matmul(const lmm_i4_a4 *__restrict__ frags,
                                                                  const int32_t *__restrict__ corr, const int32_t *__restrict__ cts,
                                                                  const int32_t *__restrict__ bias, int32_t *__restrict__ out,
                                                                  uint32_t rows, uint32_t cols, uint32_t width)
{
    const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
    const uint32_t wv = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t ct = blockIdx.x * kLmmWaves + wv;
    if (ct * 32u >= width) return; // the whole wave: nothing waits for it
    const uint32_t nks = (cols + 31u) / 32u, nrt = (rows + 31u) / 32u;
    const uint32_t rt0 = blockIdx.y * kLmmRowTiles, b = blockIdx.z;
    const uint32_t col = ct * 32u + (uint32_t)r;
    const uint32_t colc = col < width ? col : width - 1u;
    const int32_t *src = cts + (size_t)b * cols * width + colc;

    // the 16 words of K step ks: rows 32 ks + 16 h + i of the vector, held to the last row
    auto load_step = [&](uint32_t ks, uint32_t (&v)[16]) {
        const uint32_t k0 = ks * 32u + 16u * (uint32_t)h;
        if (ks * 32u + 32u <= cols) {
            const int32_t *p = src + (size_t)k0 * width;
#pragma unroll
            for (int i = 0; i < 16; i++) v[i] = (uint32_t)p[(size_t)i * width];
        } else {
#pragma unroll
            for (int i = 0; i < 16; i++) {
                const uint32_t k = k0 + (uint32_t)i;
                v[i] = (uint32_t)src[(size_t)(k < cols ? k : cols - 1u) * width];
            }
        }
    };

    lmm_i16 acc[kLmmRowTiles][4];
#pragma unroll
    for (int m = 0; m < kLmmRowTiles; m++)
#pragma unroll
        for (int j = 0; j < 4; j++)
#pragma unroll
            for (int q = 0; q < 16; q++) acc[m][j][q] = 0;

    uint32_t cur[16], nxt[16];
    load_step(0, cur);
#pragma unroll 1
    for (uint32_t ks = 0; ks < nks; ks++) {
#pragma unroll
        for (int i = 0; i < 16; i++) nxt[i] = cur[i];
        if (ks + 1u < nks) load_step(ks + 1u, nxt); // in flight during this step's products
        // bytes (word 4 q + i, limb j) -> fragment j, dword q, byte i
        lmm_i4 bl[4];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const uint32_t a = cur[4 * q] ^ kLmmFlip, bb = cur[4 * q + 1] ^ kLmmFlip, c = cur[4 * q + 2] ^ kLmmFlip,
                           d = cur[4 * q + 3] ^ kLmmFlip;
            // v_perm_b32 (s0, s1, sel): selector byte 0 .. 3 takes that byte of s1, 4 .. 7 that byte of s0
            const uint32_t ab_lo = __builtin_amdgcn_perm(bb, a, 0x05010400u), ab_hi = __builtin_amdgcn_perm(bb, a, 0x07030602u);
            const uint32_t cd_lo = __builtin_amdgcn_perm(d, c, 0x05010400u), cd_hi = __builtin_amdgcn_perm(d, c, 0x07030602u);
            bl[0][q] = (int)__builtin_amdgcn_perm(cd_lo, ab_lo, 0x05040100u);
            bl[1][q] = (int)__builtin_amdgcn_perm(cd_lo, ab_lo, 0x07060302u);
            bl[2][q] = (int)__builtin_amdgcn_perm(cd_hi, ab_hi, 0x05040100u);
            bl[3][q] = (int)__builtin_amdgcn_perm(cd_hi, ab_hi, 0x07060302u);
        }
#pragma unroll
        for (int m = 0; m < kLmmRowTiles; m++) {
            if (rt0 + (uint32_t)m < nrt) { // the wave's row tiles that exist
                const lmm_i4 a = frags[((size_t)(rt0 + (uint32_t)m) * nks + ks) * 64 + lane];
#pragma unroll
                for (int j = 0; j < 4; j++) acc[m][j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, bl[j], acc[m][j], 0, 0, 0);
            }
        }
#pragma unroll
        for (int i = 0; i < 16; i++) cur[i] = nxt[i];
    }

    if (col >= width) return;
    const bool body = bias != nullptr && col == width - 1u; // the body is the last word of a sample
#pragma unroll
    for (int m = 0; m < kLmmRowTiles; m++)
#pragma unroll
        for (int q = 0; q < 16; q++) {
            const uint32_t row = (rt0 + (uint32_t)m) * 32u + (uint32_t)((q & 3) + 8 * (q >> 2) + 4 * h);
            if (row < rows) {
                uint32_t v = (uint32_t)acc[m][0][q] + ((uint32_t)acc[m][1][q] << 8) + ((uint32_t)acc[m][2][q] << 16) +
                             ((uint32_t)acc[m][3][q] << 24) + (uint32_t)corr[row];
                if (body) v += (uint32_t)bias[row];
                out[((size_t)b * rows + row) * width + col] = (int32_t)v;
            }
        }
}

size_t lwe_image_bytes(size_t rows, size_t cols)
{
    if (!lwe_shape_ok(rows, cols)) return 0;
    const size_t nrt = (rows + 31) / 32, nks = (cols + 31) / 32;
    return nrt * nks * 1024 + nrt * 32 * sizeof(int32_t);
}

void lwe_image_build(const int8_t *w, size_t rows, size_t cols, void *h_image)
{
    const size_t nrt = (rows + 31) / 32, nks = (cols + 31) / 32;
    std::memset(h_image, 0, lwe_image_bytes(rows, cols));
    int8_t *frag = static_cast<int8_t *>(h_image);
    uint32_t *corr = reinterpret_cast<uint32_t *>(frag + nrt * nks * 1024);
    for (size_t row = 0; row < rows; row++) {
        const size_t rt = row / 32, r = row % 32;
        uint32_t sum = 0;
        for (size_t k = 0; k < cols; k++) {
            const size_t ks = k / 32, h = (k % 32) / 16, i = k % 16;
            frag[((rt * nks + ks) * 64 + h * 32 + r) * 16 + i] = w[row * cols + k];
            sum += (uint32_t)(int32_t)w[row * cols + k];
        }
        corr[row] = kLmmFlip * sum;
    }
}

hipError_t lwe_matmul_launch(const void *d_image, size_t rows, size_t cols, const int32_t *d_cts, size_t width, size_t batch,
                             const int32_t *d_bias, int32_t *d_out, hipStream_t st, uint64_t *launches)
{
    const size_t nrt = (rows + 31) / 32, nks = (cols + 31) / 32, nct = (width + 31) / 32;
    const lmm_i4_a4 *frags = static_cast<const lmm_i4_a4 *>(d_image);
    const int32_t *corr = reinterpret_cast<const int32_t *>(static_cast<const char *>(d_image) + nrt * nks * 1024);
    const size_t zmax = 65535;
    for (size_t b0 = 0; b0 < batch; b0 += zmax) {
        const size_t nb = std::min(zmax, batch - b0);
        const dim3 grid((unsigned)((nct + kLmmWaves - 1) / kLmmWaves), (unsigned)((nrt + kLmmRowTiles - 1) / kLmmRowTiles), (unsigned)nb);
        hipLaunchKernelGGL(k_lwe_matmul, grid, dim3(64 * kLmmWaves), 0, st, frags, corr, d_cts + b0 * cols * width, d_bias,
                           d_out + b0 * rows * width, (uint32_t)rows, (uint32_t)cols, (uint32_t)width);
        if (hipError_t err = hipGetLastError()) return err;
        ++*launches;
    }
    return hipSuccess;
}

} // namespace eoc
