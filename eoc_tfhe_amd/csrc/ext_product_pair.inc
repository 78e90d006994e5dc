// The external product of a WAVE PAIR, any gadget length: k_blind_rotate's step where the key rows are not streamed
// (blind_rotate_pair.inc) and the leveled kernels' frame (leveled_pair.inc: k_cmux, k_demux, k_automaton_step) include this
// one text, inside a scope of their own, so they agree bit for bit by construction.  A text and not a function: as a function template, force-inlined, it compiled every instance that uses it
// to different code (kernels.hip.h, above k_blind_rotate).
// Wave h holds the digit words of input polynomial h.  It runs the l forward transforms (two at a time, skewed on the one
// scratch; an odd last one alone), multiplies the spectra, which stay in registers, by rows (h, p) for the OTHER output
// polynomial, hands that chain to its partner through `scr`, continues the chain it finds in `scr_partner` with rows
// (h, p) for output polynomial h, and runs the inverse transform.  All waves of the workgroup pass here together: two
// workgroup barriers.
// In scope: L, h, lane; load_row(p, c, b): row (h, p), p = 1..L, for output polynomial c; dlo, dhi, gd (the digit words
// and their Gadget); s_tw, s_twist, scr, scr_partner; xp_t2, xp_t1 (twiddles resident in registers, or nullptr: see
// fft_fwd_rest_x2 / fft_inv_wave); EOC_XP_STAMP(k) (segment k in the diagnostic build, else empty).
// Out: S[8], the spectrum-side result before the un-twist, and ut[8], the un-twist factors -- declared by the includer.
        d2 xs[L][8], ra[8], rb[8];
#pragma unroll
        for (int p0 = 0; p0 + 1 < L; p0 += 2) {
            load_row(p0 + 1, 1 - h, ra);
            load_row(p0 + 2, 1 - h, rb);
            digit_pass(dlo, dhi, gd.shift(p0 + 1), gd, xs[p0]);
            EOC_XP_STAMP(1);
            fft_fwd_rest_x2(xs[p0], xs[p0 + 1],
                            [&]() __attribute__((always_inline)) { digit_pass(dlo, dhi, gd.shift(p0 + 2), gd, xs[p0 + 1]); },
                            s_tw, scr, lane, xp_t2);
            EOC_XP_STAMP(2);
            cmac8(p0 == 0, xs[p0], ra, S);
            cmac8(false, xs[p0 + 1], rb, S);
            EOC_XP_STAMP(3);
        }
        if constexpr ((L & 1) != 0) {
            load_row(L, 1 - h, ra);
            digit_pass(dlo, dhi, gd.shift(L), gd, xs[L - 1]);
            EOC_XP_STAMP(1);
            fft_fwd_rest(xs[L - 1], s_tw, scr, lane);
            EOC_XP_STAMP(2);
            cmac8(L == 1, xs[L - 1], ra, S);
            EOC_XP_STAMP(3);
        }
        // own rows: the first two are requested before the exchange (requesting the first one a register pass
        // earlier into a third buffer, or the second one only after the exchange, changes nothing: measured)
        load_row(1, h, ra);
        if constexpr (L >= 2) load_row(2, h, rb);
#pragma unroll
        for (int r = 0; r < 8; r++) scr[r * 64 + lane] = S[r];
        EOC_XP_STAMP(4);
        __syncthreads();
        EOC_XP_STAMP(5);
#pragma unroll
        for (int r = 0; r < 8; r++) S[r] = scr_partner[r * 64 + lane]; // the chain of the other input polynomial
        cmac8(false, xs[0], ra, S);
        if constexpr (L >= 3) load_row(3, h, ra);
        if constexpr (L >= 2) cmac8(false, xs[1], rb, S);
        if constexpr (L >= 4) load_row(4, h, rb);
        if constexpr (L >= 3) cmac8(false, xs[2], ra, S);
        if constexpr (L >= 4) cmac8(false, xs[3], rb, S);
        EOC_XP_STAMP(6);
        __syncthreads(); // the partner has read this wave's scratch before the inverse transform overwrites it
        EOC_XP_STAMP(7);
        fft_inv_wave(S, ut, s_tw, s_twist, scr, lane, xp_t1);
