// Body of k_blind_rotate / k_blind_rotate_tv / k_lut_many (kernels.hip.h), included into each.  In scope: template
// parameters L, BGBIT, SABAR; kernel arguments A, g_tw, g_twist; constexpr bool TV; tv, tv_rows (the test polynomials, used
// when TV); constexpr bool MANY; n_tables (interleaved tables per test polynomial, extracted when MANY); constexpr bool
// TLDS (gadget length 2 in its earlier form: tables read from LDS in the step loop, whole key rows requested per step);
// constexpr bool ENC (with TV: tv holds TLWE lists [lists][2][N], wave h seeds ACC_h from polynomial h of the job's list).
// From kernels.hip.h: Gadget / digit_pass (the digit pass), cmul0 / cmac1 (the chains' arithmetic), rot_digits.  The step's
// external product is written out here only for gadget length 2 (key rows streamed, the tuned part); every other
// instance includes ext_product_pair.inc, the text k_cmux includes too.
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    d2 *s_tw = reinterpret_cast<d2 *>(smem);
    d2 *s_twist = s_tw + kTwEntries;
    d2 *s_scr_all = s_twist + kNH;

    const int tid = threadIdx.x, lane = tid & 63;
    const int h = __builtin_amdgcn_readfirstlane(tid >> 6);
    d2 *scr = s_scr_all + h * kScr;
    d2 *scr_partner = s_scr_all + (h ^ 1) * kScr;
    int32_t *ext = reinterpret_cast<int32_t *>(scr); // [2N] signed periodic image of ACC_h (between steps)

    const uint32_t job = blockIdx.x; // grid = number of jobs
    // the rotation amounts of this job are wave-uniform and constant during the kernel: read as dwords (rows are 64-byte
    // aligned: bara_stride is a multiple of 32 entries) by vector loads of a uniform address, or (SABAR) by scalar loads
    // through the constant address space
    typedef const __attribute__((address_space(4))) uint32_t *cu32p;
    unsigned long long bara_addr = (unsigned long long)(uintptr_t)(A.bara + (size_t)job * A.bara_stride);

    // gadget length 2 keeps every loop-invariant table value in registers (below) and needs no table in LDS; TLDS selects
    // the earlier form, which reads three of the five sets from LDS in every step (EOC_TFHE_BR_TABLES_LDS=1)
    constexpr bool kResAll = L == 2 && !TLDS;
    if constexpr (!kResAll) load_tables(s_tw, s_twist, g_tw, g_twist, tid, 128);
    if (A.prep && A.step_begin == 0) { // folded k_prepare: this workgroup's row of rotation amounts
        const uint32_t gjob = A.job0 + job, g = gjob / A.ks_S;
        prepare_row(A.inline_desc ? A.desc0 : A.ks_descs[g], gjob - g * A.ks_S, A.n, A.bara + (size_t)job * A.bara_stride, tid, 128);
        if constexpr (SABAR) eoc_row_stores_to_l2();
        __syncthreads();
        if constexpr (SABAR) eoc_scalar_cache_acquire();
    }
    // loads through the constant address space may be moved freely by the compiler (the memory is assumed invariant): the
    // row's address is made opaque HERE, behind the prologue that may just have written the row, so that no load of it can
    // be scheduled above this point
    asm volatile("" : "+s"(bara_addr));
    const cu32p bara32 = (cu32p)bara_addr;
    // shipped form: the row is copied into LDS once (vector loads behind the barrier above: the workgroup's own stores,
    // or an earlier kernel's) and every step reads its amount from there
    uint16_t *s_abar = reinterpret_cast<uint16_t *>(s_scr_all + 2 * kScr);
    if constexpr (!SABAR) {
        const uint32_t *bara_v = reinterpret_cast<const uint32_t *>(A.bara + (size_t)job * A.bara_stride);
        for (int m = tid; m < (A.n + 2) / 2; m += 128) reinterpret_cast<uint32_t *>(s_abar)[m] = bara_v[m];
        __syncthreads();
    }
    auto load_abar = [&](int idx) __attribute__((always_inline)) {
        if constexpr (SABAR) return (int)((bara32[idx >> 1] >> ((idx & 1) * 16)) & 0xffffu);
        else return (int)s_abar[idx];
    };

    // ACC = (0, X^(2N - barb) * testvect), testvect = (mu, ..., mu), or (TV) the job's test polynomial
    uint32_t racc[16]; // register copy of ACC_h: coefficient lane + 64 r in racc[r] (r < 8), lane + 64 r + 512 in racc[8 + r]
    {
        const int barb = load_abar(A.n);
        const int rot = (2 * kN - barb) & (2 * kN - 1);
        const int32_t *st = A.acc_state + ((size_t)job * 2 + h) * kN;
        const int32_t *tvj = TV ? tv + (size_t)((A.job0 + job) / tv_rows) * kN : nullptr; // jobs are [table][row]
        if constexpr (ENC) tvj = tv + ((size_t)((A.job0 + job) / tv_rows) * 2 + h) * kN; // an encrypted list: (c0, c1)
#pragma unroll
        for (int r = 0; r < 16; r++) {
            int j = lane + 64 * (r & 7) + (r >> 3) * kNH;
            int idx = (j - rot) & (2 * kN - 1);
            int32_t v;
            if constexpr (TV) {
                const uint32_t c = (uint32_t)tvj[idx & (kN - 1)]; // X^N = -1: the upper half of the period is negated
                v = (int32_t)((idx & kN) ? 0u - c : c);
            } else {
                v = (idx & kN) ? -A.mu : A.mu;
            }
            if constexpr (!ENC) v = h ? v : 0;
            if (A.step_begin > 0) v = st[j]; // continue a blind rotation started by an earlier launch
            racc[r] = (uint32_t)v;
        }
    }
    __syncthreads();

    const int Bgbit = BGBIT > 0 ? BGBIT : A.Bgbit;
    uint32_t offset = 0;
#pragma unroll
    for (int p = 1; p <= L; p++) offset += ((1u << Bgbit) >> 1) << (32 - p * Bgbit);
    const Gadget<BGBIT> gd = make_gadget<BGBIT>(Bgbit);
    constexpr int KPL = 2 * L;
    const __amdgpu_buffer_rsrc_t bk_rsrc =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<double *>(A.bkfft), 0, (int)((size_t)A.n * KPL * 2 * kNH * 16), 0x00020000);

#ifdef EOC_STAMPS
    unsigned long long st_acc[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    unsigned long long st_prev = __builtin_amdgcn_s_memtime();
    st_acc[12] = st_prev;                                          // loop entry time
    st_acc[14] = __builtin_amdgcn_s_getreg((4) | (0 << 6) | (31 << 11));  // HW_REG_HW_ID: CU / SE / SIMD / wave slot
    st_acc[13] = __builtin_amdgcn_s_getreg((20) | (0 << 6) | (31 << 11)); // HW_REG_XCC_ID
#endif
    const int prio_slot = __builtin_amdgcn_s_getreg((4) | (0 << 6) | (3 << 11)); // HW_ID.WAVE_ID: slot on the SIMD
    // gadget length 2 has registers to spare: the forward transform's last four twiddles stay resident
    constexpr bool kResT2 = L == 2;
    d2 res_t2[4];
    if constexpr (kResAll) tw_load(res_t2, g_tw + kTwF2 + lane, 64);
    else if constexpr (kResT2) tw_load(res_t2, s_tw + kTwF2 + lane, 64);
    constexpr bool kResT1 = L == 2; // ... and the inverse transform's first table pass
    d2 res_t1[4];
    if constexpr (kResAll) tw_load(res_t1, g_tw + kTwI1 + (lane & 7), 8);
    else if constexpr (kResT1) tw_load(res_t1, s_tw + kTwI1 + (lane & 7), 8);
    // kResAll: the forward pair's first table pass, the inverse's last one and the eight un-twist factors as well
    d2 res_f1[4], res_i0[4], ut[8];
    if constexpr (kResAll) {
        tw_load(res_f1, g_tw + kTwF1 + (lane >> 3), 8);
        tw_load(res_i0, g_tw + kTwI0 + lane, 64);
#pragma unroll
        for (int r = 0; r < 8; r++) ut[r] = g_twist[lane + 64 * r];
    }
    int abar_next = load_abar(A.step_begin);
    for (int i = A.step_begin; i < A.step_end; i++) {
        EOC_STAMP(15);
        // The two waves that share a SIMD belong to different workgroups, and the issue arbiter favours the older
        // one: in a launch that exactly fills the chip (1024 gates = 512 workgroups) the first half of the grid
        // finishes at 0.82x and the second half at 1.19x of the mean, and the launch lasts as long as its slowest
        // workgroup.  The two waves occupy different wave slots, so the slot parity tells them apart: the
        // later-placed (odd) one holds the high priority A.prio_duty sixteenths of the steps, the other one the
        // rest.  12/16 makes both halves finish together (-10 % on the launch).  Launches of several rounds are
        // faster WITHOUT it (the arbiter's run-to-completion bias suits them: +4 %), so the host passes a
        // negative duty there.
        if (A.prio_duty >= 0) {
            const bool first_part = (i & 15) < A.prio_duty;
            if (first_part == ((prio_slot & 1) != 0))
                __builtin_amdgcn_s_setprio(1);
            else
                __builtin_amdgcn_s_setprio(0);
        } else if (A.prio_duty <= -2) {
            // launches of several rounds: the co-resident waves are at unrelated steps, so the alternation is taken
            // from the shader clock both of them read (phase length 2^(-prio_duty) cycles), even shares
            const unsigned long long now = __builtin_amdgcn_s_memtime();
            if ((int)((now >> (-A.prio_duty)) & 1) == (prio_slot & 1))
                __builtin_amdgcn_s_setprio(1);
            else
                __builtin_amdgcn_s_setprio(0);
        }
        const int abar = __builtin_amdgcn_readfirstlane(abar_next);
        // one step ahead (entry n is barb: always in bounds): an LDS read that retires with the rotation's ds_bpermutes, or
        // (SABAR) an s_load that retires with the key rows
        abar_next = load_abar(i + 1);
        // (X^abar - 1) * ACC_h.  abar == 0 gives an all-zero polynomial, all-zero digits and an exact
        // zero update, which is what skipping the step (as libtfhe does) amounts to.
        // rows (h, p), p = 1..L, of BK_i by buffer loads: the row's byte offset is wave-uniform (SGPR), the lane part one
        // loop-invariant VGPR
        auto load_row = [&](int p, int c, d2 (&b)[8]) __attribute__((always_inline)) {
            const uint32_t row_off = (uint32_t)((((size_t)i * KPL + h * L) * 2 + (size_t)(p - 1) * 2 + c) * kNH * 16);
#pragma unroll
            for (int r = 0; r < 8; r++)
                b[r] = __builtin_bit_cast(d2, __builtin_amdgcn_raw_buffer_load_b128(bk_rsrc, lane * 16, (int)(row_off + r * 1024), 0));
        };
        uint32_t dlo[8], dhi[8];
        {
            const int s = abar & 63;
            const int src = ((lane - s) & 63) << 2;
            uint32_t t[16], d[16];
#pragma unroll
            for (int r = 0; r < 16; r++) t[r] = (uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)racc[r]);
            const bool borrow = lane < s;
#define EOC_RQ(q) case q: rot_digits<q>(t, racc, borrow, offset, d); break;
            switch (abar >> 6) {
                EOC_RQ(0) EOC_RQ(1) EOC_RQ(2) EOC_RQ(3) EOC_RQ(4) EOC_RQ(5) EOC_RQ(6) EOC_RQ(7)
                EOC_RQ(8) EOC_RQ(9) EOC_RQ(10) EOC_RQ(11) EOC_RQ(12) EOC_RQ(13) EOC_RQ(14) EOC_RQ(15)
                EOC_RQ(16) EOC_RQ(17) EOC_RQ(18) EOC_RQ(19) EOC_RQ(20) EOC_RQ(21) EOC_RQ(22) EOC_RQ(23)
                EOC_RQ(24) EOC_RQ(25) EOC_RQ(26) EOC_RQ(27) EOC_RQ(28) EOC_RQ(29) EOC_RQ(30)
                default: rot_digits<31>(t, racc, borrow, offset, d); break;
            }
#undef EOC_RQ
#pragma unroll
            for (int r = 0; r < 8; r++) {
                dlo[r] = d[r];
                dhi[r] = d[8 + r];
            }
        }
        EOC_STAMP(0);
        // the external product: S = the spectrum-side update of ACC_h, before the un-twist
        d2 S[8];
        if constexpr (kResAll) {
            // the two forward transforms as one skewed pair; the spectra stay in registers for both chains
            d2 xs[2][8];
            auto make_x0 = [&](int p, d2 (&x)[8]) __attribute__((always_inline)) { digit_pass(dlo, dhi, gd.shift(p), gd, x); };
            // The key rows are streamed through the two chains bin block by bin block (block b < 8: rows (p = 1, 2) of the
            // partner's output polynomial at bins r = b; b >= 8: the own ones at r = b - 8), kRowAhead blocks requested ahead
            // of the one in use, so that no whole row is ever live next to both spectra and the resident tables.  Per bin
            // the terms arrive in the canonical order and in cmac1's nesting.  The scheduling barriers pin the requests: the
            // scheduler otherwise hoists all of them to the top.
            constexpr int kRowAhead = 3;
            const uint32_t step_off = (uint32_t)((((size_t)i * KPL + h * L) * 2) * kNH * 16);
            d2 q[16][2];
            auto issue = [&](int b) __attribute__((always_inline)) {
                const uint32_t off = step_off + (uint32_t)((b < 8 ? 1 - h : h) * kNH * 16 + (b & 7) * 1024);
                q[b][0] = __builtin_bit_cast(d2, __builtin_amdgcn_raw_buffer_load_b128(bk_rsrc, lane * 16, (int)off, 0));
                q[b][1] = __builtin_bit_cast(d2, __builtin_amdgcn_raw_buffer_load_b128(bk_rsrc, lane * 16, (int)(off + 2 * kNH * 16), 0));
            };
            make_x0(1, xs[0]);
            EOC_STAMP(1);
            fft_fwd_rest_x2(xs[0], xs[1], [&]() __attribute__((always_inline)) { make_x0(2, xs[1]); }, s_tw, scr, lane, &res_t2,
                            &res_f1, [&]() __attribute__((always_inline)) {
#pragma unroll
                                for (int b = 0; b < kRowAhead; b++) issue(b);
                            });
            EOC_STAMP(2);
            EOC_SB();
#pragma unroll
            for (int r = 0; r < 8; r++) { // the partner's chain: each bin block leaves for the scratch as it completes
                scr[r * 64 + lane] = cmac1(xs[1][r], q[r][1], cmul0(xs[0][r], q[r][0]));
                EOC_SB();
                issue(r + kRowAhead); // from r = 8 - kRowAhead on: own rows, in flight across the barrier
                EOC_SB();
            }
            EOC_STAMP(4);
            __syncthreads();
            EOC_STAMP(5);
            constexpr int kChainAhead = 2; // blocks of the partner's chain read ahead of the one in use
#pragma unroll
            for (int r = 0; r < kChainAhead; r++) S[r] = scr_partner[r * 64 + lane];
            EOC_SB();
#pragma unroll
            for (int r = 0; r < 8; r++) { // the chain of the other input polynomial, continued with the own digits
                S[r] = cmac1(xs[0][r], q[8 + r][0], S[r]);
                S[r] = cmac1(xs[1][r], q[8 + r][1], S[r]);
                EOC_SB();
                if (r + kChainAhead < 8) S[r + kChainAhead] = scr_partner[(r + kChainAhead) * 64 + lane];
                if (8 + r + kRowAhead < 16) issue(8 + r + kRowAhead);
                EOC_SB();
            }
            EOC_STAMP(6);
            __syncthreads(); // the partner has read this wave's scratch before the inverse transform overwrites it
            EOC_STAMP(7);
            fft_inv_wave<true>(S, ut, s_tw, s_twist, scr, lane, &res_t1, &res_i0);
        } else { // every other gadget length, and TLDS: whole key rows, the code k_cmux runs too
            const d2 (*const xp_t2)[4] = kResT2 ? &res_t2 : nullptr, (*const xp_t1)[4] = kResT1 ? &res_t1 : nullptr;
#define EOC_XP_STAMP(k) EOC_STAMP(k)
#include "ext_product_pair.inc"
#undef EOC_XP_STAMP
        }
        EOC_STAMP(8);
#pragma unroll
        for (int r = 0; r < 8; r++) {
            d2 y = cmulc(S[r], ut[r]); // 1/512 is in the key image
            racc[r] += wrap_trunc(y.x);
            racc[8 + r] += wrap_trunc(y.y);
        }
        wave_lds_fence();
        EOC_STAMP(9);
    }
    if (A.step_end >= A.n) { // the sample extraction below reads the image: written once, after the last step
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int j = lane + 64 * r;
            ext[j] = (int32_t)racc[r];
            ext[j + kN] = (int32_t)(0u - racc[r]);
        }
        wave_lds_fence();
    }
#ifdef EOC_STAMPS
    st_acc[11] = __builtin_amdgcn_s_memtime(); // loop exit time
    if (A.stamps && lane == 0)
        for (int k = 0; k < 16; k++) A.stamps[((size_t)blockIdx.x * 2 + h) * 16 + k] = st_acc[k];
#endif

    // the lane index again, from the hardware (not from threadIdx): nothing lane-derived then has to stay live across
    // the step loop just for these stores
    const int lane_e = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    if (A.step_end < A.n) { // not the last part: park the accumulator for the next launch
        int32_t *st = A.acc_state + ((size_t)job * 2 + h) * kN;
#pragma unroll
        for (int r = 0; r < 16; r++) st[lane_e + 64 * (r & 7) + (r >> 3) * kNH] = (int32_t)racc[r];
        return;
    }
    // tLweExtractLweSample, index 0: u_0 = ACC_0[0], u_j = -ACC_0[N - j] = ext[2N - j]; b = ACC_1[0]
    // MANY: index j = 0 .. n_tables - 1, u_i = ext[(2N + j - i) mod 2N], b = ACC_1[j].  The engine passes no ks_descs to
    // these kernels; the test of it stays a run-time one on purpose: with the folded branch discarded at compile time, the
    // Set B instance (<3, 7>) is allocated differently and spills ~90 VGPRs.
    if (MANY && !A.ks_descs) {
        // slot j of job (table g, row s) goes to workspace row (g T + j) S + s, S = tv_rows; A.u is this launch's job0
        const uint32_t gjob = A.job0 + job, g = gjob / tv_rows, si = gjob - g * tv_rows;
        int32_t *u0 = A.u - (size_t)A.job0 * (kN + 1) + ((size_t)g * n_tables * tv_rows + si) * (kN + 1);
        const size_t slot_stride = (size_t)tv_rows * (kN + 1);
        if (h == 0) {
            for (uint32_t jt = 0; jt < n_tables; jt++) {
                int32_t *u = u0 + jt * slot_stride;
#pragma unroll
                for (int r = 0; r < 16; r++) {
                    const int j = lane_e + 64 * r;
                    u[j] = ext[(2 * kN + (int)jt - j) & (2 * kN - 1)];
                }
            }
        } else if ((uint32_t)lane_e < n_tables) {
            u0[lane_e * slot_stride + kN] = ext[lane_e];
        }
    } else if (A.ks_descs) { // + lweKeySwitch set-up: ubar_j = u_j + 2^(31 - t basebit), out = (0, ..., 0, b)
        const uint32_t gjob = A.job0 + job;
        if (h == 0) {
#pragma unroll
            for (int r = 0; r < 16; r++) {
                int j = lane + 64 * r;
                A.ubar[(size_t)gjob * kN + j] = (uint32_t)ext[(2 * kN - j) & (2 * kN - 1)] + A.ks_prec_offset;
            }
        } else {
            const uint32_t g = gjob / A.ks_S, si = gjob - g * A.ks_S;
            int32_t *o = (A.inline_desc ? A.desc0.out : A.ks_descs[g].out) + (size_t)si * (A.n + 1);
            for (int m = lane; m < A.n; m += 64) o[m] = 0;
            if (lane == 0) o[A.n] = ext[0];
        }
    } else {
        int32_t *u = A.u + (size_t)job * (kN + 1);
        if (h == 0) {
#pragma unroll
            for (int r = 0; r < 16; r++) {
                int j = lane + 64 * r;
                u[j] = ext[(2 * kN - j) & (2 * kN - 1)];
            }
        } else if (lane == 0) {
            u[kN] = ext[0];
        }
    }
