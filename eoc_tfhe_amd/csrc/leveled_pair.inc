// The frame of a LEVELED kernel: one external product of a converted selector with a TLWE sample, run by one wave pair per
// item.  k_cmux, k_demux and k_automaton_step (and their rounding twins: leveled_kernels.inc) include this one text, a part at a time (EOC_LEVELED_PART), around the three
// things in which they differ, so the mapping, the LDS plan, the dead pair's rule and the product are the same by construction:
//     part 1;  the operand pointers and `sel`, formed from ix, iy, h;  part 2;  dlo / dhi filled;  part 3;  the store phase.
// A text and not a function: the frame as a struct returned by a force-inlined function (the row loader a function template)
// compiled every k_demux instance to different code, and so did these same lines in another order -- the gadget's sum ahead
// of the kernel's pointers changed all eighteen instances (kernels.hip.h, above k_blind_rotate).
//
// Part 1, the item.  In scope: A (the args struct: nx), g_tw, g_twist.
//   Out: s_tw, s_twist, scr, scr_partner (the LDS carve: the tables, then one transpose scratch per wave); tid, lane, wv, h;
//   the table load, issued (part 3 waits for it); live, ix, iy: a pair past the end of the grid computes the last item again
//   and stores nothing, so every barrier is reached by all waves.
// Part 2, the gadget.  In scope: L, BGBIT, A (Bgbit); EOC_LEVELED_ROUND of the includer (leveled_kernels.inc).
//   Out: offset (Bg/2 at every digit position; in a rounding twin 2^(31 - L Bgbit) more, where L Bgbit < 32), gd; dlo[8], dhi[8], declared: the kernel leaves coefficient lane + 64 r of
//   offset + its operand in dlo[r], coefficient lane + 64 r + 512 in dhi[r].
// Part 3, the product and the dead pair's exit.  In scope: all of the above, and sel (the item's converted selector).
//   Out: S[8], ut[8] as ext_product_pair.inc leaves them: cmulc(S[r], ut[r]) holds coefficients lane + 64 r (x) and
//   lane + 64 r + 512 (y) of output polynomial h before truncation; 1/512 is in the selector's image.  Only live pairs go on.
#if EOC_LEVELED_PART == 1
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    d2 *s_tw = reinterpret_cast<d2 *>(smem);
    d2 *s_twist = s_tw + kTwEntries;
    d2 *s_scr_all = s_twist + kNH;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int h = wv & 1;
    d2 *scr = s_scr_all + wv * kScr;
    d2 *scr_partner = s_scr_all + (wv ^ 1) * kScr;
    load_tables(s_tw, s_twist, g_tw, g_twist, tid, 128 * kCmuxItemsPerWG);

    const uint32_t x_raw = blockIdx.x * kCmuxItemsPerWG + (uint32_t)(wv >> 1);
    const bool live = x_raw < A.nx;
    const size_t ix = live ? x_raw : A.nx - 1, iy = blockIdx.y;
#elif EOC_LEVELED_PART == 2
    const int Bgbit = BGBIT > 0 ? BGBIT : A.Bgbit;
    uint32_t offset = 0;
#pragma unroll
    for (int p = 1; p <= L; p++) offset += ((1u << Bgbit) >> 1) << (32 - p * Bgbit);
#if EOC_LEVELED_ROUND
    if (L * Bgbit < 32) offset += 1u << (31 - L * Bgbit); // half of what the gadget drops: the rounding twins (DESIGN.md 21)
#endif
    const Gadget<BGBIT> gd = make_gadget<BGBIT>(Bgbit);
    uint32_t dlo[8], dhi[8];
#elif EOC_LEVELED_PART == 3
    __syncthreads(); // the tables

    auto load_row = [&](int p, int c, d2 (&b)[8]) __attribute__((always_inline)) { load_selector_row<L>(sel, h, lane, p, c, b); };
    d2 S[8], ut[8];
    {
        const d2 (*const xp_t2)[4] = nullptr, (*const xp_t1)[4] = nullptr; // nothing is loop-invariant here: tables from LDS
#define EOC_XP_STAMP(k) do { } while (0)
#include "ext_product_pair.inc"
#undef EOC_XP_STAMP
    }
    if (!live) return;
#else
#error "leveled_pair.inc: define EOC_LEVELED_PART as 1 (the item), 2 (the gadget) or 3 (the product and the exit)"
#endif
#undef EOC_LEVELED_PART
