// The text of the three leveled kernels (kernels.hip.h describes each above the place it is included): k_cmux, k_demux and
// k_automaton_step, and from the SAME lines their rounding twins k_rcmux, k_rdemux and k_rstep (DESIGN.md 21).  The includer
// sets EOC_LEVELED_KERNEL (1 the CMux, 2 the demultiplexer, 3 the automaton step) and EOC_LEVELED_ROUND (0 the oracle's
// truncating gadget, 1 the rounding one); the one line in which a twin differs is in part 2 of the frame (leveled_pair.inc),
// which reads EOC_LEVELED_ROUND.  Included text and not a template parameter or a shared device function: the twins need
// names of their own (the ISA guards count kernels by name), a bool parameter would rename the shipped instances, and a
// force-inlined body is what changed the shipped code before (kernels.hip.h, above k_blind_rotate).  tools/isa_diff.py: the
// eighteen truncating instances compile to the instructions they had as texts of kernels.hip.h.
#if EOC_LEVELED_ROUND
#define EOC_LEVELED_NAME(trunc, round) round
#else
#define EOC_LEVELED_NAME(trunc, round) trunc
#endif

#if EOC_LEVELED_KERNEL == 1
template <int L, int BGBIT = 0>
__global__ __launch_bounds__(128 * kCmuxItemsPerWG, 2) void EOC_LEVELED_NAME(k_cmux, k_rcmux)(CmuxArgs A, const d2 *__restrict__ g_tw,
                                                                                              const d2 *__restrict__ g_twist)
{
#define EOC_LEVELED_PART 1
#include "leveled_pair.inc"
    const int32_t *pa = A.in0 + ix * A.in0_x + iy * A.in0_y + (size_t)h * kN;
    const int32_t *pb = A.in1 + ix * A.in1_x + iy * A.in1_y + (size_t)h * kN;
    const d2 *sel = A.sel + ix * A.sel_x + iy * A.sel_y;
#define EOC_LEVELED_PART 2
#include "leveled_pair.inc"
    // offset + (X^rot B_h - A_h).  The rotation is index arithmetic on B's loads (X^N = -1: the upper half of the 2N-period
    // is negated)
#pragma unroll
    for (int r = 0; r < 16; r++) {
        const int j = lane + 64 * (r & 7) + (r >> 3) * kNH;
        const int idx = (j - A.rot) & (2 * kN - 1);
        const uint32_t b = (uint32_t)pb[idx & (kN - 1)];
        const uint32_t v = offset + EOC_NEGACYCLIC(idx, b) - (uint32_t)pa[j];
        if (r < 8) dlo[r] = v;
        else dhi[r - 8] = v;
    }
#define EOC_LEVELED_PART 3
#include "leveled_pair.inc"
    int32_t *po = A.out + ix * A.out_x + iy * A.out_y + (size_t)h * kN;
#pragma unroll
    for (int r = 0; r < 8; r++) {
        const int j = lane + 64 * r;
        const uint2 e = leveled_words(S[r], ut[r]);
        po[j] = (int32_t)((uint32_t)pa[j] + e.x);
        po[j + kNH] = (int32_t)((uint32_t)pa[j + kNH] + e.y);
    }
}

#elif EOC_LEVELED_KERNEL == 2
template <int L, int BGBIT = 0>
__global__ __launch_bounds__(128 * kCmuxItemsPerWG, 2) void EOC_LEVELED_NAME(k_demux, k_rdemux)(DemuxArgs A, const d2 *__restrict__ g_tw,
                                                                                                const d2 *__restrict__ g_twist)
{
#define EOC_LEVELED_PART 1
#include "leveled_pair.inc"
    const int32_t *px = A.in + ix * A.in_x + iy * A.in_y + (size_t)h * kN;
    const d2 *sel = A.sel + ix * A.sel_x + iy * A.sel_y;
#define EOC_LEVELED_PART 2
#include "leveled_pair.inc"
    // offset + x_h
#pragma unroll
    for (int r = 0; r < 8; r++) {
        dlo[r] = offset + (uint32_t)px[lane + 64 * r];
        dhi[r] = offset + (uint32_t)px[lane + 64 * r + kNH];
    }
#define EOC_LEVELED_PART 3
#include "leveled_pair.inc"
    const size_t oo = ix * A.out_x + iy * A.out_y + (size_t)h * kN;
    int32_t *p0 = A.out0 + oo, *p1 = A.out1 + oo;
    if (A.accumulate) {
#pragma unroll
        for (int r = 0; r < 8; r++) {
            const int j = lane + 64 * r;
            const uint2 e = leveled_words(S[r], ut[r]);
            atomicAdd(p1 + j, (int)e.x);
            atomicAdd(p1 + j + kNH, (int)e.y);
            atomicAdd(p0 + j, (int)((uint32_t)px[j] - e.x));
            atomicAdd(p0 + j + kNH, (int)((uint32_t)px[j + kNH] - e.y));
        }
    } else {
#pragma unroll
        for (int r = 0; r < 8; r++) {
            const int j = lane + 64 * r;
            const uint2 e = leveled_words(S[r], ut[r]);
            p1[j] = (int32_t)e.x;
            p1[j + kNH] = (int32_t)e.y;
            p0[j] = (int32_t)((uint32_t)px[j] - e.x);
            p0[j + kNH] = (int32_t)((uint32_t)px[j + kNH] - e.y);
        }
    }
}

#elif EOC_LEVELED_KERNEL == 3
template <int L, int BGBIT = 0>
__global__ __launch_bounds__(128 * kCmuxItemsPerWG, 2) void EOC_LEVELED_NAME(k_automaton_step, k_rstep)(AutoStepArgs A,
                                                                                                        const d2 *__restrict__ g_tw,
                                                                                                        const d2 *__restrict__ g_twist)
{
#define EOC_LEVELED_PART 1
#include "leveled_pair.inc"
    const AutoTrans tr = A.trans[ix]; // uniform: one record per wave pair
    const int32_t *pv = A.prev + iy * A.prev_y + (size_t)h * kN;
    const int32_t *pa = pv + (size_t)tr.next0 * (2 * kN);
    const int32_t *pb = pv + (size_t)tr.next1 * (2 * kN);
    const int w0 = tr.w0 & (2 * kN - 1), w1 = tr.w1 & (2 * kN - 1);
    const d2 *sel = A.sel + iy * A.sel_y;
#define EOC_LEVELED_PART 2
#include "leveled_pair.inc"
    // offset + (X^(-w1) B_h - X^(-w0) A_h)
#pragma unroll
    for (int r = 0; r < 16; r++) {
        const int j = lane + 64 * (r & 7) + (r >> 3) * kNH;
        const int ia = (j + w0) & (2 * kN - 1), ib = (j + w1) & (2 * kN - 1);
        const uint32_t a = (uint32_t)pa[ia & (kN - 1)], b = (uint32_t)pb[ib & (kN - 1)];
        const uint32_t v = offset + EOC_NEGACYCLIC(ib, b) - EOC_NEGACYCLIC(ia, a);
        if (r < 8) dlo[r] = v;
        else dhi[r - 8] = v;
    }
#define EOC_LEVELED_PART 3
#include "leveled_pair.inc"
    int32_t *po = A.next + ix * (size_t)(2 * kN) + iy * A.next_y + (size_t)h * kN;
    // the gather indices are formed again from a value the compiler cannot match with the load phase's: carried across the
    // product, those sixteen registers are what spills <3,7>
    int w0s = w0;
    asm volatile("" : "+s"(w0s));
#pragma unroll
    for (int r = 0; r < 8; r++) {
        const int j = lane + 64 * r;
        const uint2 e = leveled_words(S[r], ut[r]);
        const int i0 = (j + w0s) & (2 * kN - 1), i1 = (j + kNH + w0s) & (2 * kN - 1);
        const uint32_t a0 = (uint32_t)pa[i0 & (kN - 1)], a1 = (uint32_t)pa[i1 & (kN - 1)];
        po[j] = (int32_t)(EOC_NEGACYCLIC(i0, a0) + e.x);
        po[j + kNH] = (int32_t)(EOC_NEGACYCLIC(i1, a1) + e.y);
    }
}

#else
#error "leveled_kernels.inc: define EOC_LEVELED_KERNEL as 1 (the CMux), 2 (the demultiplexer) or 3 (the automaton step)"
#endif
#undef EOC_LEVELED_NAME
#undef EOC_LEVELED_KERNEL
#undef EOC_LEVELED_ROUND
