// stage_iir.h - IIRFilterBlock and AGC / PowerSquelch stages (scan kernels)
// (part of liblrhip.so; included by lrhip.hip in this order, one translation unit)
#pragma once

// =====================================================================================================
// IIRFilterBlock
// =====================================================================================================
struct IirStage : lrhip_stage {
    int S = 1, nb = 0, na = 0, P = 0;
    bool scan = false;
    IirCoeffs co;
    DeviceBuf d_tpow, d_ttile, d_tseg;    // A^(LC*2^k), k = 0..8 (9 PxP matrices, float up to order 4, double above); A^TILE in double; per-launch carry powers
    IirSeqCoeffs seq;
    std::vector<double> Ttile;            // A^TILE in double (row-major PxP) for the per-launch carry powers
    int warm_tiles = 0;                   // > 0: A^(warm_tiles*TILE) underflows Float32 -> single-launch iir_stream_kernel
    int warm_chunks = 0;                  // > 0 (first order): |p|^(16 warm_chunks) < 1e-12 with at most half a tile -> one-shot launch, a workgroup per tile
    TwoSlots xhist, state;                // the last inputs and the recurrence state of the scan forms: each its own pair, flipped together
    DeviceBuf tile_end, tile_start, seq_xs, seq_ys;
    unsigned long D = 1, index = 0;       // fused DownsamplerBlock behind the filter (chains)
    const char *kind() const override { return "iir"; }
    unsigned long max_output(unsigned long n) const override { return D == 1 ? n : n / D + 1; }
    int seek(unsigned long long n0, unsigned long long *n0_out) override
    {
        if (reset()) return -1;
        index = (unsigned long)((D - n0 % D) % D);
        *n0_out = (n0 + D - 1) / D;
        return 0;
    }
    // a recurrence forgets its start only if it decays: the single-launch form already requires A^(warm_tiles * TILE) to underflow Float32
    long memory() const override { return warm_tiles > 0 ? (long)warm_tiles * IIR_TILE + nb : -1; }
    void rate(unsigned long *num, unsigned long *den) const override { *num = D; *den = 1; }
    unsigned long align() const override { return scan ? (unsigned long)IIR_TILE : 1UL; }
    int reset() override
    {
        index = 0;
        if (xhist.reset(sizeof(float) * S * IIR_MAX_NB) || state.reset(sizeof(float) * S * (IIR_MAX_P + 1))) return -1;
        if (zero_fill(seq_xs, sizeof(float) * S * IIR_SEQ_MAX) || zero_fill(seq_ys, sizeof(float) * S * IIR_SEQ_MAX)) return -1;
        return 0;
    }
    template <int SS, int PP, int NBT>
    int run_scan_nb(const float *x, float *y, long n)
    {
        using ST = typename IirScanT<PP>::T;
        long ntiles = (n + IIR_TILE - 1) / IIR_TILE;
        const float *xh = xhist.in<float>(), *st = state.in<float>();
        float *st_out = state.out<float>();
        const ST *tp = (const ST *)d_tpow.p;
        if (warm_tiles > 0) {
            // tiles per workgroup: enough workgroups to fill the chip a few times over, at most 8 tiles each
            long slots = (long)ctx().num_cus * 8;
            int run = (int)(ntiles / slots);
            run = run < 1 ? 1 : run > 8 ? 8 : run;
            if (run < 2 * warm_tiles && ntiles > 4 * warm_tiles) run = 2 * warm_tiles;      // bound the re-read overhead
            int wc = 0;
            static const bool no_oneshot = getenv("LRHIP_IIR_NO_ONESHOT") != nullptr;      // A/B knob: whole warm-up tiles (round 2)
            static const bool no_coal = getenv("LRHIP_IIR_NO_COAL") != nullptr;            // A/B knob: per-thread chunk loads / stores (round 2)
            // A/B knob: ordinary stores instead of non-temporal ones (measured, 2^26 samples: Float32 first order 0.100 -> 0.082 ms and two poles 0.117 -> 0.091 with
            // them; the ComplexFloat32 kernels do not move - 155 registers = 3 workgroups per CU hold them at 4.8 TB/s; forcing 4 spills 80 bytes and loses 40 %)
            static const bool plain_st = getenv("LRHIP_IIR_PLAIN_STORES") != nullptr;
            static const int run_knob = getenv("LRHIP_IIR_RUN") ? atoi(getenv("LRHIP_IIR_RUN")) : 0;       // A/B knob: tiles per workgroup
            if (warm_chunks > 0 && !no_oneshot) {
                // partial warm-up tile: only its last warm_chunks chunks are read.  Tiles per workgroup by measurement (2^26 samples, one box, ms):
                //   first order Float32        1: 0.104   2: 0.098   4: 0.109   8: 0.112
                //   2 poles, 5 taps, Complex   1: 0.267   2: 0.226   4: 0.219   8: 0.213   16: 0.247      (whole warm-up tile, 8: 0.232)
                wc = warm_chunks;
                if (PP == 1) run = ntiles >= 8L * ctx().num_cus ? 2 : 1;
                if (run_knob > 0) run = run_knob;
            }
            unsigned grid = (unsigned)((ntiles + run - 1) / run);
            hipLaunchKernelGGL((iir_stream_kernel<SS, PP, NBT>), dim3(grid), dim3(256), 0, ctx().stream, x, y, n, xh, st, st_out, (long)D, (long)index, run,
                               wc ? 1 : warm_tiles, wc, co, xhist.out<float>(), tp, (no_coal ? 1 : 0) | (plain_st ? 2 : 0));
            LR_LAUNCH_CHECK();
            return 0;
        }
        if (tile_end.reserve(sizeof(ST) * ntiles * SS * PP) || tile_start.reserve(sizeof(ST) * ntiles * SS * PP) ||
            d_tseg.reserve(sizeof(ST) * 8 * PP * PP)) return -1;
        if (ntiles > 1) {
            hipLaunchKernelGGL((iir_scan_kernel<SS, PP, false, NBT>), dim3((unsigned)ntiles), dim3(256), 0, ctx().stream, x, (float *)nullptr, n, xh,
                               (const ST *)nullptr, (ST *)tile_end.p, st, st_out, 1L, 0L, co, tp);
            LR_LAUNCH_CHECK();
        }
        // carry scan: 256 segments of `seg` tiles; the powers A^(TILE*seg*2^k) are computed on the device in double
        long nt = ntiles > 1 ? ntiles : 1, seg = (nt + 255) / 256;
        hipLaunchKernelGGL((iir_tseg_kernel<PP, ST>), dim3(1), dim3(1), 0, ctx().stream, (const double *)d_ttile.p, seg, (ST *)d_tseg.p);
        hipLaunchKernelGGL((iir_carry_kernel<SS, PP>), dim3(1), dim3(256), 0, ctx().stream, (const ST *)tile_end.p, (ST *)tile_start.p,
                           nt, seg, st, (const ST *)d_tseg.p, tp);
        LR_LAUNCH_CHECK();
        hipLaunchKernelGGL((iir_scan_kernel<SS, PP, true, NBT>), dim3((unsigned)ntiles), dim3(256), 0, ctx().stream, x, y, n, xh,
                           (const ST *)tile_start.p, (ST *)nullptr, st, st_out, (long)D, (long)index, co, tp);
        LR_LAUNCH_CHECK();
        if (nb > 1) {
            hipLaunchKernelGGL(iir_state_kernel<SS>, dim3(1), dim3(64), 0, ctx().stream, x, n, nb, xh, xhist.out<float>());
            LR_LAUNCH_CHECK();
        }
        return 0;
    }
    template <int SS, int PP>
    int run_scan(const float *x, float *y, long n)
    {
        // the feed-forward loop is unrolled to NBT taps (terms beyond nb are predicated off, not free): 2 = single-pole filters, 4 = biquads and the
        // reference suite's 4-ff-tap entry, 16 = the rest
        // (8 = the reference suite's "5 ff 3 fb" entry on orders up to 4: 0.373 -> measured below with half the predicated terms and 8 fewer staged samples)
        if (nb <= 2) return run_scan_nb<SS, PP, 2>(x, y, n);
        if (nb <= 4) return run_scan_nb<SS, PP, 4>(x, y, n);
        if constexpr (PP <= 4) {
            if (nb <= 8) return run_scan_nb<SS, PP, 8>(x, y, n);
        }
        return run_scan_nb<SS, PP, 16>(x, y, n);
    }
    long run(const void *in_dev, unsigned long n, void *out_dev, unsigned long cap) override
    {
        if (!n) return 0;
        unsigned long n_out = D == 1 ? n : (n > index ? (n - index + D - 1) / D : 0);
        if (n_out > cap) return set_error("iir: output capacity %lu < %lu", cap, n_out);
        const float *x = (const float *)in_dev;
        float *y = (float *)out_dev;
        int rc = 0;
        if (scan) {
            // with a single tile the carry kernel just seeds tile_start[0] from the carried state
#define LR_IIR_P(SS, PP) case PP: rc = run_scan<SS, PP>(x, y, (long)n); break
            if (S == 1) switch (P) { LR_IIR_P(1, 1); LR_IIR_P(1, 2); LR_IIR_P(1, 3); LR_IIR_P(1, 4); LR_IIR_P(1, 5); LR_IIR_P(1, 6); LR_IIR_P(1, 7); default: rc = run_scan<1, 8>(x, y, (long)n); }
            else switch (P) { LR_IIR_P(2, 1); LR_IIR_P(2, 2); LR_IIR_P(2, 3); LR_IIR_P(2, 4); LR_IIR_P(2, 5); LR_IIR_P(2, 6); LR_IIR_P(2, 7); default: rc = run_scan<2, 8>(x, y, (long)n); }
#undef LR_IIR_P
            if (rc) return rc;
            // the one commit of the scan forms, whichever ran (with nb <= 1 the three-pass form leaves xhist.out() unwritten: nothing reads it)
            xhist.flip();
            state.flip();
        } else {
            if (S == 1) hipLaunchKernelGGL(iir_seq_kernel<1>, dim3(1), dim3(64), 0, ctx().stream, x, y, (long)n, seq, (float *)seq_xs.p, (float *)seq_ys.p);
            else hipLaunchKernelGGL(iir_seq_kernel<2>, dim3(1), dim3(64), 0, ctx().stream, x, y, (long)n, seq, (float *)seq_xs.p, (float *)seq_ys.p);
            LR_LAUNCH_CHECK();
        }
        if (D > 1) index = index + n_out * D - n;       // downsampler.lua:53
        return (long)n_out;
    }
};

// The stage behind lrhip_iir_create, which has checked the taps: the sequential form's coefficients and, for the scan forms (orders 1 .. IIR_MAX_P),
// the normalised coefficients and the powers of the recurrence's companion matrix that the kernels step by.
static IirStage *iir_build(const float *b, unsigned nb, const float *a, unsigned na, int input_complex)
{
    auto q = new_stage<IirStage>();
    if (!q) return nullptr;
    q->S = input_complex ? 2 : 1;
    q->in_size = q->out_size = 4 * q->S;
    q->nb = (int)nb; q->na = (int)na; q->P = (int)na - 1;
    q->seq.nb = (int)nb; q->seq.na = (int)na;
    for (unsigned i = 0; i < nb; i++) q->seq.b[i] = b[i];
    for (unsigned i = 0; i < na; i++) q->seq.a[i] = a[i];
    q->scan = q->P >= 1 && q->P <= IIR_MAX_P && nb <= IIR_MAX_NB;
    if (q->scan) {
        int P = q->P;
        IirCoeffs &co = q->co;
        memset(&co, 0, sizeof(co));
        co.nb = (int)nb; co.P = P;
        for (unsigned i = 0; i < nb; i++) co.b[i] = (float)((double)b[i] / (double)a[0]);
        for (int i = 0; i < P; i++) co.a[i] = (float)((double)a[i + 1] / (double)a[0]);
        // companion matrix of the homogeneous recurrence for the state (y[n-1], ..., y[n-P])
        std::vector<double> A((size_t)P * P, 0.0), T;
        for (int k = 0; k < P; k++) A[k] = -(double)co.a[k];
        for (int r = 1; r < P; r++) A[r * P + r - 1] = 1.0;
        T = A;
        for (int s = 1; s < IIR_LC; s <<= 1) matmul(T, T, T, P);      // A^LC (LC is a power of two)
        std::vector<float> tpow((size_t)9 * P * P);
        std::vector<double> tpow64((size_t)9 * P * P);
        const double p16 = P == 1 ? T[0] : 0.0;                     // first order: A^LC is the scalar p^16
        for (int k = 0; k <= 8; k++) {
            for (int i = 0; i < P * P; i++) { tpow[(size_t)k * P * P + i] = (float)T[i]; tpow64[(size_t)k * P * P + i] = T[i]; }
            if (k == 8) q->Ttile = T;
            matmul(T, T, T, P);
        }
        if (P == 1 && std::fabs(p16) < 1.0 && p16 != 0.0) {
            // chunks of 16 samples after which a zero start has decayed to 1e-12: the partial warm-up of the one-shot launch
            const int wc = (int)std::ceil(std::log(1e-12) / std::log(std::fabs(p16)));
            if (wc >= 1 && wc <= 128) q->warm_chunks = wc;
        } else if (P == 1 && p16 == 0.0) {
            q->warm_chunks = 1;
        }
        // (orders 2-4 were given the same one-shot launch in round 3 - 4 chunks of warm-up instead of a whole tile per 8 - and lost: 0.417 against 0.372 ms
        // for the suite's 3-feedback-tap entry on ComplexFloat32, same box: every workgroup then runs the 18-barrier block scan twice per emitted tile)
        // Round 3, on top of the two-barrier wave scan: a workgroup per tile still loses (0.267 against 0.232 ms), but the partial warm-up tile itself pays
        // at the old 8 tiles per workgroup - 0.213 (run_scan_nb above has the table).
        if (P >= 2 && P <= 4) {
            std::vector<double> A16(tpow64.begin(), tpow64.begin() + P * P), M = A16;
            for (int wc = 1; wc <= 128 && !q->warm_chunks; wc++) {
                double mx = 0.0;
                for (double v : M) mx = std::fabs(v) > mx ? std::fabs(v) : mx;
                if (std::isfinite(mx) && mx < 1e-12) q->warm_chunks = wc;
                matmul(M, A16, M, P);
            }
        }
        if (P == 1) {                                               // p^(16 (l + 1)), l < 64: the per-lane powers of the single-launch kernel's wave scan
            double acc = 1.0;
            for (int l = 0; l < 64; l++) { acc *= p16; tpow.push_back((float)acc); }
        } else if (P <= 4) {                                        // the same for orders 2-4: the matrices A^(16 (l + 1))
            std::vector<double> A16(tpow64.begin(), tpow64.begin() + P * P), M = A16;
            for (int l = 0; l < 64; l++) {
                for (int i = 0; i < P * P; i++) tpow.push_back((float)M[i]);
                matmul(M, A16, M, P);
            }
        }
        if (P > 4 ? upload(q->d_tpow, tpow64.data(), tpow64.size() * sizeof(double)) : upload(q->d_tpow, tpow.data(), tpow.size() * sizeof(float))) return nullptr;
        if (upload(q->d_ttile, q->Ttile.data(), q->Ttile.size() * sizeof(double))) return nullptr;
        // memory shorter than `w` tiles in Float32 terms?  (every entry of A^(w*TILE) underflows)  -> single-launch kernel
        static const bool force_3pass = getenv("LRHIP_IIR_3PASS") != nullptr;       // A/B knob
        std::vector<double> W = q->Ttile;
        for (int w = 1; w <= 4 && !force_3pass && !q->warm_tiles; w *= 2) {
            double mx = 0.0;
            bool finite = true;
            for (double v : W) { finite = finite && std::isfinite(v); mx = std::fabs(v) > mx ? std::fabs(v) : mx; }
            if (finite && mx < 1e-46) q->warm_tiles = w;
            matmul(W, W, W, P);
        }
    }
    if (q->reset()) return nullptr;
    return q.release();
}

// =====================================================================================================
// AGCBlock
// =====================================================================================================
struct AgcStage : lrhip_stage {
    AgcParams p;
    int S = 1;
    bool squelch = false;                              // PowerSquelchBlock: power scan + gate only
    Carried<double[2]> state;                          // (P, G): the power estimate and the gain
    DeviceBuf mapsP, mapsG, startP, startG;
    const char *kind() const override { return "agc"; }
    long memory() const override { return -1; }
    int reset() override { return state.reset(); }
    template <int SS>
    int go(const float *x, float *y, unsigned long n)
    {
        unsigned long nt = (n + AGC_TILE - 1) / AGC_TILE;
        if (mapsP.reserve(nt * 2 * sizeof(double)) || mapsG.reserve(nt * 2 * sizeof(double)) || startP.reserve(nt * sizeof(double)) ||
            startG.reserve(nt * sizeof(double))) return -1;
        const double *st = *state.in();
        double *st_out = *state.out();
        double *mp = (double *)mapsP.p, *mg = (double *)mapsG.p, *sp = (double *)startP.p, *sg = (double *)startG.p;
        dim3 g((unsigned)nt), b(256);
        hipLaunchKernelGGL((agc_pass_kernel<SS, 0>), g, b, 0, ctx().stream, x, y, n, p, mp, mg, (const double *)sp, (const double *)sg, st_out);
        hipLaunchKernelGGL(agc_carry_kernel, dim3(1), b, 0, ctx().stream, (const double *)mp, nt, st, sp);
        if (squelch) {
            hipLaunchKernelGGL((agc_pass_kernel<SS, 3>), g, b, 0, ctx().stream, x, y, n, p, mp, mg, (const double *)sp, (const double *)sg, st_out);
        } else {
            hipLaunchKernelGGL((agc_pass_kernel<SS, 1>), g, b, 0, ctx().stream, x, y, n, p, mp, mg, (const double *)sp, (const double *)sg, st_out);
            hipLaunchKernelGGL(agc_carry_kernel, dim3(1), b, 0, ctx().stream, (const double *)mg, nt, st + 1, sg);
            hipLaunchKernelGGL((agc_pass_kernel<SS, 2>), g, b, 0, ctx().stream, x, y, n, p, mp, mg, (const double *)sp, (const double *)sg, st_out);
        }
        LR_LAUNCH_CHECK();
        state.flip();
        return 0;
    }
    long run(const void *in_dev, unsigned long n, void *out_dev, unsigned long cap) override
    {
        if (n > cap) return set_error("agc: output capacity %lu < %lu", cap, n);
        if (!n) return 0;
        int rc = S == 2 ? go<2>((const float *)in_dev, (float *)out_dev, n) : go<1>((const float *)in_dev, (float *)out_dev, n);
        return rc ? rc : (long)n;
    }
};
