// Body of k_blind_rotate_wide / k_blind_rotate_wide_tv / k_lut_many_wide (kernels.hip.h), included into each.  In scope:
// template parameters BGBIT, SABAR; kernel arguments A, g_tw, g_twist; constexpr bool TV; tv, tv_rows (the test
// polynomials, used when TV); constexpr bool MANY; n_tables (tables per test polynomial, extracted when MANY); constexpr
// bool ENC (with TV: tv holds TLWE lists [lists][2][N] and the wave seeds both accumulators from the job's list).
// From kernels.hip.h: Gadget / digit_pass (the digit pass), cmul0 / cmac1 (the chains' arithmetic), rot_digits.
    constexpr int L = 2, KPL = 4;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    d2 *s_tw = reinterpret_cast<d2 *>(smem);
    d2 *s_twist = s_tw + kTwEntries;
    d2 *s_scr_all = s_twist + kNH;

    const int tid = threadIdx.x, lane = tid & 63;
    const int h = __builtin_amdgcn_readfirstlane(tid >> 6);
    d2 *scr = s_scr_all + h * kScr;
    int32_t *ext = reinterpret_cast<int32_t *>(scr);

    const uint32_t job = blockIdx.x * kBRWideJobsPerWG + (uint32_t)h; // grid = ceil(jobs / waves per workgroup)
    load_tables(s_tw, s_twist, g_tw, g_twist, tid, 64 * kBRWideJobsPerWG);
    if (A.prep && A.step_begin == 0 && job < A.njobs) { // folded k_prepare: this wave's row of rotation amounts
        const uint32_t gjob = A.job0 + job, g = gjob / A.ks_S;
        prepare_row(A.inline_desc ? A.desc0 : A.ks_descs[g], gjob - g * A.ks_S, A.n, A.bara + (size_t)job * A.bara_stride, lane, 64);
        if constexpr (SABAR) eoc_row_stores_to_l2();
    }
    __syncthreads();
    if constexpr (SABAR) eoc_scalar_cache_acquire();
    if (job >= A.njobs) return; // the idle wave of an odd last workgroup (the only barrier is behind it)

    typedef const __attribute__((address_space(4))) uint32_t *cu32p;
    unsigned long long bara_addr = (unsigned long long)(uintptr_t)(A.bara + (size_t)job * A.bara_stride);
    asm volatile("" : "+s"(bara_addr)); // opaque behind the prologue: see k_blind_rotate
    const cu32p bara32 = (cu32p)bara_addr;
    // shipped form: the wave copies its row into LDS once and every step reads its amount from there (a wave's LDS
    // operations execute in order: no barrier between the copy and the reads)
    uint16_t *s_abar = reinterpret_cast<uint16_t *>(s_scr_all + kBRWideJobsPerWG * kScr) + h * (kAbarLds / 2);
    if constexpr (!SABAR) {
        const uint32_t *bara_v = reinterpret_cast<const uint32_t *>(A.bara + (size_t)job * A.bara_stride);
        for (int m = lane; m < (A.n + 2) / 2; m += 64) reinterpret_cast<uint32_t *>(s_abar)[m] = bara_v[m];
        wave_lds_fence();
    }
    auto load_abar = [&](int idx) __attribute__((always_inline)) {
        if constexpr (SABAR) return (int)((bara32[idx >> 1] >> ((idx & 1) * 16)) & 0xffffu);
        else return (int)s_abar[idx];
    };

    // ACC = (0, X^(2N - barb) * testvect): coefficient lane + 64 r of polynomial q in racc_q[r] (r < 8), + 512 in racc_q[8 + r]
    uint32_t racc0[16], racc1[16];
    {
        const int barb = load_abar(A.n);
        const int rot = (2 * kN - barb) & (2 * kN - 1);
        const int32_t *st = A.acc_state + (size_t)job * 2 * kN;
        const int32_t *tvj = TV ? tv + (size_t)((A.job0 + job) / tv_rows) * kN : nullptr; // jobs are [table][row]
        if constexpr (ENC) tvj = tv + (size_t)((A.job0 + job) / tv_rows) * 2 * kN; // an encrypted list: (c0, c1)
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int j = lane + 64 * (r & 7) + (r >> 3) * kNH;
            const int idx = (j - rot) & (2 * kN - 1);
            int32_t v0 = 0, v1;
            if constexpr (ENC) {
                const uint32_t c0 = (uint32_t)tvj[idx & (kN - 1)], c1 = (uint32_t)tvj[kN + (idx & (kN - 1))];
                v0 = (int32_t)((idx & kN) ? 0u - c0 : c0);
                v1 = (int32_t)((idx & kN) ? 0u - c1 : c1);
            } else if constexpr (TV) {
                const uint32_t c = (uint32_t)tvj[idx & (kN - 1)];
                v1 = (int32_t)((idx & kN) ? 0u - c : c);
            } else {
                v1 = (idx & kN) ? -A.mu : A.mu;
            }
            if (A.step_begin > 0) { // continue a blind rotation started by an earlier launch
                v0 = st[j];
                v1 = st[kN + j];
            }
            racc0[r] = (uint32_t)v0;
            racc1[r] = (uint32_t)v1;
        }
    }

    const int Bgbit = BGBIT > 0 ? BGBIT : A.Bgbit;
    uint32_t offset = 0;
#pragma unroll
    for (int p = 1; p <= L; p++) offset += ((1u << Bgbit) >> 1) << (32 - p * Bgbit);
    const Gadget<BGBIT> gd = make_gadget<BGBIT>(Bgbit);
    const __amdgpu_buffer_rsrc_t bk_rsrc =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<double *>(A.bkfft), 0, (int)((size_t)A.n * KPL * 2 * kNH * 16), 0x00020000);
    const int prio_slot = __builtin_amdgcn_s_getreg((4) | (0 << 6) | (3 << 11)); // HW_ID.WAVE_ID: slot on the SIMD

#ifdef EOC_STAMPS
    unsigned long long st_acc[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    unsigned long long st_prev = __builtin_amdgcn_s_memtime();
    st_acc[12] = st_prev;
    st_acc[14] = __builtin_amdgcn_s_getreg((4) | (0 << 6) | (31 << 11));
    st_acc[13] = __builtin_amdgcn_s_getreg((20) | (0 << 6) | (31 << 11));
#endif
    int abar_next = load_abar(A.step_begin);
    for (int i = A.step_begin; i < A.step_end; i++) {
        EOC_STAMP(15);
        if (A.prio_duty >= 0) { // see k_blind_rotate: the two waves of a SIMD alternate the issue priority
            const bool first_part = (i & 15) < A.prio_duty;
            if (first_part == ((prio_slot & 1) != 0))
                __builtin_amdgcn_s_setprio(1);
            else
                __builtin_amdgcn_s_setprio(0);
        }
        const int abar = __builtin_amdgcn_readfirstlane(abar_next);
        abar_next = load_abar(i + 1); // one step ahead: an LDS read, or (SABAR) an s_load
        // (X^abar - 1) * ACC_q, q = 0, 1, as biased digit words (see k_blind_rotate)
        uint32_t d0[16], d1[16];
        {
            const int s = abar & 63;
            const int src = ((lane - s) & 63) << 2;
            uint32_t t0[16], t1[16];
#pragma unroll
            for (int r = 0; r < 16; r++) t0[r] = (uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)racc0[r]);
#pragma unroll
            for (int r = 0; r < 16; r++) t1[r] = (uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)racc1[r]);
            const bool borrow = lane < s;
#define EOC_RQ(q) case q: rot_digits<q>(t0, racc0, borrow, offset, d0); rot_digits<q>(t1, racc1, borrow, offset, d1); break;
            switch (abar >> 6) {
                EOC_RQ(0) EOC_RQ(1) EOC_RQ(2) EOC_RQ(3) EOC_RQ(4) EOC_RQ(5) EOC_RQ(6) EOC_RQ(7)
                EOC_RQ(8) EOC_RQ(9) EOC_RQ(10) EOC_RQ(11) EOC_RQ(12) EOC_RQ(13) EOC_RQ(14) EOC_RQ(15)
                EOC_RQ(16) EOC_RQ(17) EOC_RQ(18) EOC_RQ(19) EOC_RQ(20) EOC_RQ(21) EOC_RQ(22) EOC_RQ(23)
                EOC_RQ(24) EOC_RQ(25) EOC_RQ(26) EOC_RQ(27) EOC_RQ(28) EOC_RQ(29) EOC_RQ(30)
                default: rot_digits<31>(t0, racc0, borrow, offset, d0); rot_digits<31>(t1, racc1, borrow, offset, d1); break;
            }
#undef EOC_RQ
        }
        // digit p of the 16 coefficients of this lane (digit words d[0..7] = low half, d[8..15] = high half), first pass
        auto make_x0 = [&](const uint32_t (&d)[16], int p, d2 (&x)[8]) __attribute__((always_inline)) {
            digit_pass(d, d + 8, gd.shift(p), gd, x);
        };
        EOC_STAMP(0);
        d2 xs0[2][8], xs1[2][8];
        make_x0(d0, 1, xs0[0]);
        fft_fwd_rest_x2(xs0[0], xs0[1], [&]() __attribute__((always_inline)) { make_x0(d0, 2, xs0[1]); }, s_tw, scr, lane);
        EOC_STAMP(1);
        make_x0(d1, 1, xs1[0]);
        fft_fwd_rest_x2(xs1[0], xs1[1], [&]() __attribute__((always_inline)) { make_x0(d1, 2, xs1[1]); }, s_tw, scr, lane);
        EOC_STAMP(2);

        // the two chains, bin block by bin block; row (q, p, c) of BK_i sits at ((i KPL + q L + p - 1) 2 + c) * 8 KiB
        d2 S0[8], S1[8];
        const uint32_t step_off = (uint32_t)((size_t)i * KPL * 2 * kNH * 16);
        auto ld = [&](int q, int p, int c, int r) __attribute__((always_inline)) {
            const uint32_t off = step_off + (uint32_t)((((q * L) + (p - 1)) * 2 + c) * kNH * 16 + r * 1024);
            return __builtin_bit_cast(d2, __builtin_amdgcn_raw_buffer_load_b128(bk_rsrc, lane * 16, (int)off, 0));
        };
#pragma unroll
        for (int r = 0; r < 8; r++) {
            const d2 b110 = ld(1, 1, 0, r), b120 = ld(1, 2, 0, r), b010 = ld(0, 1, 0, r), b020 = ld(0, 2, 0, r);
            const d2 b011 = ld(0, 1, 1, r), b021 = ld(0, 2, 1, r), b111 = ld(1, 1, 1, r), b121 = ld(1, 2, 1, r);
            d2 a0 = cmul0(xs1[0][r], b110);
            a0 = cmac1(xs1[1][r], b120, a0);
            a0 = cmac1(xs0[0][r], b010, a0);
            a0 = cmac1(xs0[1][r], b020, a0);
            d2 a1 = cmul0(xs0[0][r], b011);
            a1 = cmac1(xs0[1][r], b021, a1);
            a1 = cmac1(xs1[0][r], b111, a1);
            a1 = cmac1(xs1[1][r], b121, a1);
            S0[r] = a0;
            S1[r] = a1;
        }
        EOC_STAMP(3);
        d2 ut[8];
        fft_inv_x2(S0, S1, ut, s_tw, s_twist, scr, lane);
        EOC_STAMP(8);
#pragma unroll
        for (int r = 0; r < 8; r++) {
            const d2 y0 = cmulc(S0[r], ut[r]), y1 = cmulc(S1[r], ut[r]); // 1/512 is in the key image
            racc0[r] += wrap_trunc(y0.x);
            racc0[8 + r] += wrap_trunc(y0.y);
            racc1[r] += wrap_trunc(y1.x);
            racc1[8 + r] += wrap_trunc(y1.y);
        }
        wave_lds_fence();
        EOC_STAMP(9);
    }
#ifdef EOC_STAMPS
    st_acc[11] = __builtin_amdgcn_s_memtime();
    if (A.stamps && lane == 0)
        for (int k = 0; k < 16; k++) A.stamps[((size_t)blockIdx.x * kBRWideJobsPerWG + h) * 16 + k] = st_acc[k];
#endif

    const int lane_e = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    if (A.step_end < A.n) { // not the last part: park the accumulators for the next launch
        int32_t *st = A.acc_state + (size_t)job * 2 * kN;
#pragma unroll
        for (int r = 0; r < 16; r++) {
            st[lane_e + 64 * (r & 7) + (r >> 3) * kNH] = (int32_t)racc0[r];
            st[kN + lane_e + 64 * (r & 7) + (r >> 3) * kNH] = (int32_t)racc1[r];
        }
        return;
    }
    // tLweExtractLweSample, index 0: u_0 = ACC_0[0], u_j = -ACC_0[N - j]; b = ACC_1[0].  The signed periodic image of
    // ACC_0 goes through the scratch once (read by index); register r holds coefficient lane + 64 (r & 7) + 512 (r >> 3)
#pragma unroll
    for (int r = 0; r < 16; r++) {
        const int j = lane_e + 64 * r;
        ext[j] = (int32_t)racc0[r];
        ext[j + kN] = (int32_t)(0u - racc0[r]);
    }
    wave_lds_fence();
    if constexpr (MANY) { // index j = 0 .. n_tables - 1 into slot rows (g T + j) S + s (see k_lut_many); b = ACC_1[j] is
                          // coefficient j of lane j's register 0
        const uint32_t gjob = A.job0 + job, g = gjob / tv_rows, si = gjob - g * tv_rows;
        int32_t *u0 = A.u - (size_t)A.job0 * (kN + 1) + ((size_t)g * n_tables * tv_rows + si) * (kN + 1);
        const size_t slot_stride = (size_t)tv_rows * (kN + 1);
        for (uint32_t jt = 0; jt < n_tables; jt++) {
            int32_t *u = u0 + jt * slot_stride;
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int j = lane_e + 64 * r;
                u[j] = ext[(2 * kN + (int)jt - j) & (2 * kN - 1)];
            }
        }
        if ((uint32_t)lane_e < n_tables) u0[lane_e * slot_stride + kN] = (int32_t)racc1[0];
        return;
    }
    const int32_t bval = (int32_t)__builtin_amdgcn_readfirstlane((int)racc1[0]); // ACC_1[0]: lane 0, register 0
    if (A.ks_descs) { // + lweKeySwitch set-up: ubar_j = u_j + 2^(31 - t basebit), out = (0, ..., 0, b)
        const uint32_t gjob = A.job0 + job;
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int j = lane_e + 64 * r;
            A.ubar[(size_t)gjob * kN + j] = (uint32_t)ext[(2 * kN - j) & (2 * kN - 1)] + A.ks_prec_offset;
        }
        const uint32_t g = gjob / A.ks_S, si = gjob - g * A.ks_S;
        int32_t *o = (A.inline_desc ? A.desc0.out : A.ks_descs[g].out) + (size_t)si * (A.n + 1);
        for (int m = lane_e; m < A.n; m += 64) o[m] = 0;
        if (lane_e == 0) o[A.n] = bval;
    } else {
        int32_t *u = A.u + (size_t)job * (kN + 1);
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int j = lane_e + 64 * r;
            u[j] = ext[(2 * kN - j) & (2 * kN - 1)];
        }
        if (lane_e == 0) u[kN] = bval;
    }
