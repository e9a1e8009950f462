// stage_fir.h - FIRFilterBlock stage: direct Toeplitz-MFMA / overlap-save FFT / decimating kernels, fused rotator, downsampler, discriminator; fir_build()
// (part of liblrhip.so; included by lrhip.hip in this order, one translation unit)
#pragma once
#include "fir_form.h"
#include "fir_plan.h"
#include "fir_tables.h"
#include "launch_prep.h"

// the kernel instantiation for a raw record format (RX_FMT_U8 / S8 / S16LE; kernels_fir.h): fn(std::integral_constant<int, RX_FMT_*>{}).  ComplexFloat32
// samples are no record format: the callers that take them too name that instantiation themselves
template <typename Fn>
static int with_record_format(int fmt, Fn fn)
{
    switch (fmt) {
        case RX_FMT_U8: return fn(std::integral_constant<int, RX_FMT_U8>{});
        case RX_FMT_S8: return fn(std::integral_constant<int, RX_FMT_S8>{});
        default: return fn(std::integral_constant<int, RX_FMT_S16LE>{});
    }
}

// =====================================================================================================
// FIRFilterBlock (+ fused FrequencyTranslatorBlock in front, + fused DownsamplerBlock behind)
// =====================================================================================================
struct FirStage : lrhip_stage, FirShape {      // (FirShape, fir_form.h: M, S, D, taps, the fused neighbours - what the choice of kernel depends on)
    // rotator + discriminator epilogue on the persistent Toeplitz kernel: window-relative phasors (kernels_fir.h, REL) unless the environment asks for the stand-alone rotator's
    // phasors bit for bit; A/B knob: one-wave workgroups for that kernel (every wave stages its own window, no barriers: measured equal).  Read per stage, not per process
    FirStage() { rel_rot = !LRHIP_DISC_EPI_LDS && getenv("LRHIP_TUNER_EXACT") == nullptr;
                 rel_nw1 = getenv("LRHIP_TUNER_NW1") != nullptr; }
    std::vector<float> taps_rev;          // host copy, reversed (firfilter.lua:234-238)
    // the taps in natural order again (what fir_build was given): M taps of 1 (real) or 2 (complex) floats
    std::vector<float> natural_taps() const
    {
        const int ts = taps_complex ? 2 : 1;
        std::vector<float> h((size_t)M * ts);
        for (int t = 0; t < M; t++)
            for (int c = 0; c < ts; c++) h[(size_t)t * ts + c] = taps_rev[(size_t)(M - 1 - t) * ts + c];
        return h;
    }
    DeviceBuf d_taps, d_atab, d_ctaps4;
    // ---- carried from call to call: the history, the discriminator's previous sample, the fused recurrence's state, the decimation index and the absolute
    // sample count.  A launch reads the *_in() slots and writes the *_out() ones; commit() alone advances any of it (reset() and seek() set it)
    int hist_pad = 0;                     // leading pad floats in the history buffers (1 for complex taps, see launch_mfma_cc)
    TwoSlots hist, disc, iir;             // (M - 1) S floats behind the pad; one float2; four floats
    unsigned long index = 0;              // carried downsampler index (downsampler.lua:53)
    uint64_t rot_step = 0, count = 0;     // absolute index of the next input sample
    const float *h_in() const { return (const float *)hist.in() + hist_pad; }
    float *h_out() const { return M > 1 ? (float *)hist.out() + hist_pad : nullptr; }      // (one tap: nothing to carry)
    const float2 *disc_in() const { return (const float2 *)disc.in(); }
    float2 *disc_out() const { return (float2 *)disc.out(); }
    const float *iir_in() const { return (const float *)iir.in(); }
    float *iir_out() const { return (float *)iir.out(); }
    // what a launch_* / dispatch_* returns: -1 with the message set, or which of the next slots its launches wrote
    enum : int { WROTE_HIST = 1, WROTE_DISC = 2, WROTE_IIR = 4 };
    static int wrote_hist(const float *ho) { return ho ? WROTE_HIST : 0; }
    // overlap-save emission framing (firfilter.lua:451-485)
    long L = 0, fill = 0;
    DeviceBuf pending, work;
    static constexpr int FFT_PART = FIR_FFT_PART;
    // round 3: IQFileSource's format stage (u8 / s8 / s16le records, in_fmt) in front of a fused Tuner is folded into it: the persistent kernel converts the records
    // on the way into LDS (kernels_fir.h FMT); the stage itself (not owned) converts for every other launch form
    lrhip_stage *fmt_stage = nullptr;
    DeviceBuf converted;
    bool raw_now = false;                 // set around core() while x holds raw records
    DeviceBuf d_fft_tables;
    DeviceBuf d_fft4k_tables;             // 513 .. 1281 taps on a ComplexFloat32 stream: the 4096-point kernel (kernels_firfft4k.h)
    DeviceBuf d_fft64_tables;             // ... and its one-wave-per-block form (kernels_firfft64.h)
    int mode_req = 0;                     // use_fft as the caller passed it (0..3), before 3 = automatic was resolved
    DeviceBuf d_dec_tables;
    double rot_omega = 0.0;
    int post_unary = 0;      // 1 + UN_CMAG / UN_CPHASE / UN_CREAL / UN_CIMAG folded into the LDS-staged decimator's store (chains: tuner -> ComplexMagnitude ...), Float32 out
    DeviceBuf edge;
    // fix-up of the wave-first discriminator outputs (disc_epilogue): done by fir_disc_fixup_kernel, or - defer_fixup - left to the next
    // stage of the chain, a pair-mode window filter that patches the samples as it stages them (FwcParams::fix_edge): one launch less
    bool defer_fixup = false, fix_ready = false;
    long fix_nunits = 0; int fix_unit = 0;  // the deferred fix-up as fir_disc_fixup_kernel would have been launched (consumer chunks that emit nothing)
    int fix_shift = 8;                     // log2 of the outputs per edge record pair
    const float2 *fix_prev_ptr = nullptr;
    FirStage *fix_src = nullptr;           // consumer side: the stage whose edge records are to be applied
    double disc_gain = 1.0;

    const char *kind() const override { return "fir"; }
    unsigned long max_output(unsigned long n) const override
    {
        if (use_fft) return (unsigned long)(((fill + (long)n) / L) * L);
        return D == 1 ? n : n / D + 1;
    }
    int reset() override
    {
        index = 0; count = 0; fill = 0;
        if (iir_fused && iir.reset(4 * sizeof(float))) return -1;
        if ((pre_disc || post_disc) && disc.reset(sizeof(float2))) return -1;
        return hist.reset(((size_t)(M > 1 ? M - 1 : 1) * S + hist_pad) * sizeof(float));
    }

    int seek(unsigned long long n0, unsigned long long *n0_out) override
    {
        if (use_fft && n0 % (unsigned long long)L) return set_error("fir(fft framing): a partition must start on a block boundary (multiple of %ld samples)", L);
        if (reset()) return -1;
        count = n0;                                                     // fused rotator: phase = step * absolute index
        index = (unsigned long)((D - n0 % D) % D);                      // fused downsampler: kept outputs are the absolute indices 0 mod D
        *n0_out = (n0 + D - 1) / D;
        return 0;
    }
    long memory() const override
    {
        long m = M - 1 + (pre_disc ? 1 : 0);
        if (post_disc) m += D;                                          // one filter output earlier
        if (iir_fused) m += (long)D * 320 * iir_warm;                   // the low-rate recurrence's in-launch warm-up length, in outputs
        return m;
    }
    void rate(unsigned long *num, unsigned long *den) const override { *num = D; *den = 1; }
    unsigned long align() const override { return fir_align(*this, fir_knobs()); }
    // the form a launch from a sample-aligned / unaligned input pointer takes
    const FirShape &shape() const { return *this; }
    FirForm form(bool aligned) const { return fir_form(*this, fir_knobs(), aligned); }
    static bool decfft_supported(unsigned d, int m, int s) { return fir_decfft_supported(d, m, s); }
    bool hilbert_ok() const { return fir_hilbert_ok(*this); }
    bool can_post_unary() const { return fir_can_post_unary(*this); }
    bool can_post_disc() const { return fir_can_post_disc(*this, fir_knobs()); }
    static bool mfma_supported_decim(unsigned d) { return fir_mfma_supported_decim(d); }
    bool direct_io_ok() const override { return !fix_src && fir_direct_io_ok(*this, fir_knobs()); }
    // the instantiation of the Toeplitz kernel: persistent and fully unrolled (fir_mfma_persistent names the shapes), or generic
    template <int SS, int DD, int NACC>
    int launch_mfma(bool persistent, const float *x, long n, float *y, long n_out)
    {
        if (!persistent) return launch_mfma_ks<SS, DD, NACC, 0>(x, n, y, n_out);
        if constexpr (DD == 1) return ksteps == 36 ? launch_mfma_ks<SS, DD, NACC, 36>(x, n, y, n_out) : launch_mfma_ks<SS, DD, NACC, 37>(x, n, y, n_out);
        else if constexpr (DD == 5) return launch_mfma_ks<SS, DD, NACC, 51>(x, n, y, n_out);
        else if constexpr (SS == 2 && (DD == 4 || DD == 8 || DD == 10)) return launch_mfma_ks<SS, DD, NACC, fir_disc_ksteps(DD)>(x, n, y, n_out);
        else return set_error("internal: no persistent Toeplitz kernel at decimation %d", DD);
    }

    template <int SS, int DD, int NACC, int KS, int NW = 4>
    int launch_mfma_ks(const float *x, long n, float *y, long n_out)
    {
        using G = FirMfmaGeom<SS, DD>;
        constexpr int TILE_OUT = G::tile_out(NACC, NW);
        if constexpr (NW == 4 && SS == 2 && DD == 5 && KS == 51) {
            // tuner + discriminator with window-relative phasors: one-wave workgroups (every wave stages its own window, no barriers)
            if (rot && post_disc && rel_rot && rel_nw1) return launch_mfma_ks<SS, DD, NACC, KS, 1>(x, n, y, n_out);
        }
        // alignment slack so that the tile's first staged sample is 16-B aligned in global memory (raw records: the 4- / 8-byte word of two samples)
        const unsigned esz = raw_now ? (in_fmt == RX_FMT_S16LE ? 4u : 2u) : (unsigned)(4 * SS);
        if (((uintptr_t)x % esz) != 0) return set_error("fir: fused rotator / discriminator needs a sample-aligned input pointer");      // (without them: the direct kernel, fir_form)
        long sample_addr = (long)((uintptr_t)x / esz);
        int q = 4 / SS;
        long v = sample_addr + (long)index - (M - 1);
        int e = (int)(((v % q) + q) % q);
        int span = G::span(NACC, ksteps, NW);
        size_t lds_floats = (size_t)fir_taps_len(DD, ksteps) + (size_t)G::phys(SS * span) + G::PAD + 8;
        size_t lds_bytes = lds_floats * sizeof(float);
        long ntiles = (n_out + TILE_OUT - 1) / TILE_OUT;
        const float *atab = (const float *)d_atab.p;          // zero-padded reversed taps
        const float *h = h_in();
        int out_aligned = ((uintptr_t)y % 16) == 0;
        uint64_t rs = rot ? rot_step : 0, rc = rot ? count : 0;
        float *ho = KS > 0 ? h_out() : nullptr;      // the persistent kernels write the next history, the generic one leaves it to commit()
        if constexpr (KS > 0) {
            auto launch = [&](auto kern) -> int {
                const long slots = chip_slots(kern, 64 * NW, lds_bytes);
                if (slots < 0) return -1;
                const int rounds = persistent_rounds(ntiles, slots, fir_knobs().fir_rounds);      // tile order (LRHIP_FIR_ROUNDS)
                const unsigned grid = persistent_grid(ntiles, slots, rounds);
                if (post_disc && edge.reserve((size_t)ntiles * 2 * NW * sizeof(float2))) return -1;
                hipLaunchKernelGGL(kern, dim3(grid), dim3(64 * NW), lds_bytes, ctx().stream, h, x, atab, y, M, n, n_out, (long)index, e,
                                   ntiles, out_aligned, rs, rc, (float2 *)edge.p, post_disc ? disc_out() : nullptr, 1.0 / disc_gain, ho, rounds);
                return 0;
            };
            int rc2;
            if constexpr (SS == 2 && (DD == 4 || DD == 8 || DD == 10)) {
                // only the Tuner + discriminator form is instantiated at these decimations (launch_mfma)
                if (!(post_disc && rot)) return set_error("internal: decimation %d has a persistent kernel for tuner + discriminator only", DD);
            }
            if constexpr (SS == 2 && (DD == 1 || DD == 5 || DD == 4 || DD == 8 || DD == 10)) {
                if (post_disc) {
                    if constexpr (DD == 4 || DD == 8 || DD == 10)
                        rc2 = rel_rot ? launch(fir_mfma_persistent_kernel<2, DD, NACC, true, KS, 1, true>) : launch(fir_mfma_persistent_kernel<2, DD, NACC, true, KS, 1, false>);
                    else if constexpr (NW == 1) rc2 = launch(fir_mfma_persistent_kernel<2, DD, NACC, true, KS, 1, true, 1>);
                    else if constexpr (LRHIP_DISC_EPI_LDS) rc2 = rot ? launch(fir_mfma_persistent_kernel<2, DD, NACC, true, KS, 1>) : launch(fir_mfma_persistent_kernel<2, DD, NACC, false, KS, 1>);
                    else rc2 = !rot ? launch(fir_mfma_persistent_kernel<2, DD, NACC, false, KS, 1>)
                             : rel_rot ? launch(fir_mfma_persistent_kernel<2, DD, NACC, true, KS, 1, true>) : launch(fir_mfma_persistent_kernel<2, DD, NACC, true, KS, 1, false>);
                    if (rc2) return rc2;
                    LR_LAUNCH_CHECK();
                    // records per unit of FIX_UNIT outputs: a wave's range in the in-register epilogue, a whole tile in the LDS one
                    constexpr int FIX_UNIT = LRHIP_DISC_EPI_LDS ? TILE_OUT : TILE_OUT / NW;
                    const long nunits = LRHIP_DISC_EPI_LDS ? ntiles : NW * ntiles;
                    // (the consumer patches at most 32 samples per half window: a record pair per >= 256 outputs)
                    if (defer_fixup && (FIX_UNIT & (FIX_UNIT - 1)) == 0 && FIX_UNIT >= 256) {
                        fix_ready = true;
                        fix_nunits = nunits; fix_unit = FIX_UNIT;
                        fix_prev_ptr = disc_in();
                        fix_shift = 0;
                        while ((1 << fix_shift) < FIX_UNIT) fix_shift++;
                    } else {
                        hipLaunchKernelGGL(fir_disc_fixup_kernel, dim3((unsigned)((nunits + 255) / 256)), dim3(256), 0, ctx().stream, (const float2 *)edge.p,
                                           nunits, FIX_UNIT, y, n_out, disc_in(), 1.0 / disc_gain);
                        LR_LAUNCH_CHECK();
                    }
                    return wrote_hist(ho) | WROTE_DISC;
                }
            }
            if (post_disc) return set_error("internal: discriminator epilogue without a persistent kernel variant");
            if constexpr (SS == 2 && DD == 5 && KS == 51 && NW == 4) {
                if (raw_now) {
                    auto raw = [&](auto r) {
                        return with_record_format(in_fmt, [&](auto fmt) { return launch(fir_mfma_persistent_kernel<2, DD, NACC, decltype(r)::value, KS, 0, false, 4, decltype(fmt)::value>); });
                    };
                    rc2 = rot ? raw(std::true_type{}) : raw(std::false_type{});
                    if (rc2) return rc2;
                    LR_LAUNCH_CHECK();
                    return wrote_hist(ho);
                }
            }
            if (raw_now) return set_error("internal: raw records reached a kernel without a record instantiation");
            if constexpr (DD == 4 || DD == 8 || DD == 10) return set_error("internal: no plain persistent kernel at decimation %d", DD);
            else {
                if constexpr (SS == 2) rc2 = rot ? launch(fir_mfma_persistent_kernel<2, DD, NACC, true, KS>) : launch(fir_mfma_persistent_kernel<2, DD, NACC, false, KS>);
                else rc2 = rot ? set_error("rotator fusion needs complex input") : launch(fir_mfma_persistent_kernel<1, DD, NACC, false, KS>);
                if (rc2) return rc2;
            }
        } else {
            if (post_disc) return set_error("internal: discriminator epilogue without a persistent kernel variant");
            auto launch = [&](auto kern) -> int {
                if (kernel_allow_lds(kern, lds_bytes)) return -1;
                hipLaunchKernelGGL(kern, dim3((unsigned)ntiles), dim3(256), lds_bytes, ctx().stream, h, x, atab, y, M, n, n_out, (long)index, e,
                                   ksteps, out_aligned, rs, rc);
                return 0;
            };
            int rc2;
            if constexpr (SS == 2) rc2 = rot ? launch(fir_mfma_kernel<2, DD, NACC, true, 1>) : launch(fir_mfma_kernel<2, DD, NACC, false, 1>);
            else rc2 = rot ? set_error("rotator fusion needs complex input") : launch(fir_mfma_kernel<1, DD, NACC, false, 1>);
            if (rc2) return rc2;
        }
        LR_LAUNCH_CHECK();
        return wrote_hist(ho);
    }

    // HilbertTransformBlock in one launch (hilbert_ok; hilbert() below).  y2 receives n ComplexFloat32 samples (delayed input, filtered input)
    // the window form (kernels_firwin.h hilbert_win_kernel): the reference's tap counts, taps at even distance from the centre exactly zero
    int hilb_sparse = -1;
    template <int MM>
    int launch_hilbert_win(const float *x, long n, float *y2)
    {
        using G = FwhGeom<MM>;
        const size_t lds_bytes = (size_t)G::LDS_FLOATS * sizeof(float);
        auto kern = hilbert_win_kernel<MM>;
        const long ntiles = (n + FWR_TILE - 1) / FWR_TILE, slots = chip_slots(kern, 256, lds_bytes);
        if (slots < 0) return -1;
        long run = (ntiles + 4 * slots - 1) / (4 * slots);
        if (fir_knobs().hilbert_run > 0) run = fir_knobs().hilbert_run;      // A/B knob: tiles per workgroup
        const unsigned grid = (unsigned)((ntiles + run - 1) / run);
        hipLaunchKernelGGL(kern, dim3(grid), dim3(256), lds_bytes, ctx().stream, h_in(), x, (const float *)d_taps.p, y2, n, run, h_out());
        LR_LAUNCH_CHECK();
        return WROTE_HIST;
    }
    // the generic Float32 Toeplitz kernel with the pair epilogue (kernels_fir.h, HILB); the history is left to commit()
    int launch_hilbert_mfma(const float *x, long n, float *y2)
    {
        constexpr int NACC = 4;
        using G = FirMfmaGeom<1, 1>;
        constexpr int TILE_OUT = G::tile_out(NACC);
        if (((uintptr_t)x % 4) != 0) return set_error("hilbert: unaligned input pointer");
        const long v = (long)((uintptr_t)x / 4) + (long)index - (M - 1);
        const int e = (int)(((v % 4) + 4) % 4);
        const int span = G::span(NACC, ksteps);
        const size_t lds_bytes = ((size_t)fir_taps_len(1, ksteps) + (size_t)G::phys(span) + G::PAD + 8) * sizeof(float);
        const long ntiles = (n + TILE_OUT - 1) / TILE_OUT;
        auto kern = fir_mfma_kernel<1, 1, NACC, false, 1, true>;
        if (kernel_allow_lds(kern, lds_bytes)) return -1;
        hipLaunchKernelGGL(kern, dim3((unsigned)ntiles), dim3(256), lds_bytes, ctx().stream, h_in(), x, (const float *)d_atab.p, y2, M, n, n,
                           (long)index, e, ksteps, (int)(((uintptr_t)y2 % 16) == 0), (uint64_t)0, (uint64_t)0);
        LR_LAUNCH_CHECK();
        return 0;
    }

    // complex taps: two real Toeplitz filters (re / im) of 2M taps over the interleaved float stream, decimation 2D,
    // sharing every B fragment.  Stream position of output k in float units is 2*q_k + 1 once the float stream is
    // given one leading pad float (so the history is the 2M-1 floats the S = 1 kernel expects).
    template <int DD2, int NACC>
    int launch_mfma_cc(const float *x, long n, float *y, long n_out)
    {
        using G = FirMfmaGeom<1, DD2>;
        constexpr int TILE_OUT = G::tile_out(NACC);
        if (((uintptr_t)x % 8) != 0) return set_error("internal: unaligned input reached the complex-taps Toeplitz kernel");      // (the direct kernel's: fir_form)
        const int M2 = 2 * M;
        const long first2 = 2 * (long)index + 1, n2 = 2 * n;
        long v = (long)((uintptr_t)x / 4) + first2 - (M2 - 1);
        int e = (int)(((v % 4) + 4) % 4);
        int span = G::span(NACC, ksteps);
        size_t lds_bytes = ((size_t)2 * fir_taps_len(DD2, ksteps) + (size_t)G::phys(span) + G::PAD + 8) * sizeof(float);
        long ntiles = (n_out + TILE_OUT - 1) / TILE_OUT;
        const float *atab = (const float *)d_atab.p;          // [re taps | im taps], each zero-padded
        const float *h = h_in() - hist_pad;                   // includes the pad float
        int out_aligned = ((uintptr_t)y % 16) == 0;
        auto kern = fir_mfma_kernel<1, DD2, NACC, false, 2>;
        if (kernel_allow_lds(kern, lds_bytes)) return -1;
        hipLaunchKernelGGL(kern, dim3((unsigned)ntiles), dim3(256), lds_bytes, ctx().stream, h, x, atab, y, M2, n2, n_out, first2, e,
                           ksteps, out_aligned, (uint64_t)0, (uint64_t)0);
        LR_LAUNCH_CHECK();
        return 0;
    }

    int dispatch_mfma_cc(const float *x, long n, float *y, long n_out)
    {
        switch (D) {
            case 1: return launch_mfma_cc<2, 4>(x, n, y, n_out);
            case 2: return launch_mfma_cc<4, 2>(x, n, y, n_out);
            case 3: return launch_mfma_cc<6, 1>(x, n, y, n_out);
            case 4: return launch_mfma_cc<8, 1>(x, n, y, n_out);
            case 5: return launch_mfma_cc<10, 1>(x, n, y, n_out);
            default: return set_error("internal: no complex-taps Toeplitz kernel at decimation %u", D);
        }
    }

    template <int VV, int NG>
    int launch_fft4k_ng(const float *x, long n, float *y, long n_out)
    {
        constexpr long Lf = F4K_N - VV;
        const size_t lds_bytes = (size_t)f4k_lds_elems(NG) * sizeof(float2);
        auto kern = fir_fft4k_kernel<VV, NG>;
        const long nblocks = (n_out + Lf - 1) / Lf, nslots = (nblocks + NG - 1) / NG, slots = chip_slots(kern, 256 * NG, lds_bytes);
        if (slots < 0) return -1;
        const unsigned grid = persistent_grid(nslots, slots, 0);
        hipLaunchKernelGGL(kern, dim3(grid), dim3(256 * NG), lds_bytes, ctx().stream, h_in(), x, (const float2 *)d_fft4k_tables.p, y, M, n,
                           n_out, nblocks, h_out(), fir_knobs().f4k_xcd_map);      // (XCD-major block order)
        LR_LAUNCH_CHECK();
        return WROTE_HIST;
    }
    // one WAVE per 4096-point block as 64 x 64 (kernels_firfft64.h): eight waves per CU with the conjugate-symmetric H of real taps, four with complex taps
    template <int VV, int WAVES, int SS = 2, bool HG = false>
    int launch_fft64(const float *x, long n, float *y, long n_out)
    {
        constexpr long Lf = F4K_N - VV;
        const size_t lds_bytes = (size_t)f64_lds_elems(WAVES) * sizeof(float2);
        auto kern = fir_fft64_kernel<VV, WAVES, 1, SS, HG>;
        if (kernel_allow_lds(kern, lds_bytes)) return -1;
        // (Float32 stream: two stream blocks per transform - the kernel's block count is the number of transforms)
        const long nblocks = ((n_out + Lf - 1) / Lf + (2 - SS)) / (3 - SS), nslots = (nblocks + WAVES - 1) / WAVES;
        const unsigned grid = (unsigned)(nslots < ctx().num_cus ? nslots : ctx().num_cus);      // 108 / 158 KB of LDS: one workgroup per CU
        hipLaunchKernelGGL(kern, dim3(grid), dim3(64 * WAVES), lds_bytes, ctx().stream, h_in(), x, (const float2 *)d_fft64_tables.p, y, M, n,
                           n_out, nblocks, h_out(), fir_knobs().f4k_xcd_map, 0L, 0);
        LR_LAUNCH_CHECK();
        return WROTE_HIST;
    }
    // round 5: V = 2 048, one partition (eight waves on real taps, four on complex ones) or two (four waves, a run of consecutive blocks per wave)
    template <int NP, int SS = 2>
    int launch_fft64_long(const float *x, long n, float *y, long n_out)
    {
        constexpr int VV = 2048, WAVES = 4;
        constexpr long Lf = F4K_N - VV;
        const size_t lds_bytes = (size_t)f64_lds_elems(WAVES, NP) * sizeof(float2);
        auto kern = fir_fft64_kernel<VV, WAVES, NP, SS>;
        if (kernel_allow_lds(kern, lds_bytes)) return -1;
        const long nblocks = (n_out + Lf - 1) / Lf, nslots = (nblocks + WAVES - 1) / WAVES;
        const unsigned grid = (unsigned)(nslots < ctx().num_cus ? nslots : ctx().num_cus);
        // round 6: 4 098 .. 8 193 taps (fft64_np = 3, 4) = a second launch with partitions 2 and 3 on the stream delayed by 4 096 samples, adding to y
        const int launches = NP == 2 && fft64_np > 2 ? 2 : 1;
        int wrote = 0;
        for (int l = 0; l < launches; l++) {
            float *ho = l == 0 ? h_out() : nullptr;
            hipLaunchKernelGGL(kern, dim3(grid), dim3(64 * WAVES), lds_bytes, ctx().stream, h_in(), x,
                               (const float2 *)d_fft64_tables.p + (size_t)l * F64_TABLE_ELEMS2, y, M, n, n_out, nblocks, ho, 0, (long)l * F4K_N, l);
            LR_LAUNCH_CHECK();
            wrote |= wrote_hist(ho);
        }
        return wrote;
    }
    template <int VV>
    int launch_fft64_v(const float *x, long n, float *y, long n_out)
    {
        if (S == 1) return launch_fft64<VV, 8, 1>(x, n, y, n_out);
        if (taps_complex) return fir_knobs().f64_hg ? launch_fft64<VV, 8, 2, true>(x, n, y, n_out) : launch_fft64<VV, 4>(x, n, y, n_out);
        return launch_fft64<VV, 8>(x, n, y, n_out);
    }
    template <int VV>
    int launch_fft4k(const float *x, long n, float *y, long n_out)
    {
        return fir_knobs().f4k_ng == 2 ? launch_fft4k_ng<VV, 2>(x, n, y, n_out) : launch_fft4k_ng<VV, 1>(x, n, y, n_out);
    }
    // ---- partitioned overlap-save (kernels_firpols.h, round 4): 513 taps and more in one launch per 1 536 taps, ComplexFloat32 or Float32 stream
    template <int SS, int PP>
    int launch_pols_p(const float *x, long n, float *y, long n_out, int part0)
    {
        const size_t lds_bytes = (size_t)pols_lds_elems(SS, PP) * sizeof(float2);
        constexpr int POLS_WPB = pols_wpb(SS, PP);
        auto kern = fir_pols_kernel<SS, PP>;
        if (kernel_allow_lds(kern, lds_bytes)) return -1;
        // a wave owns a run of consecutive blocks (its spectra delay line); runs of ~40 blocks keep the P - 1 warm-up blocks of a run under 5 %,
        // and the number of runs is a whole number of rounds of (CUs x waves) where the launch is long enough
        constexpr long RPW = SS == 2 ? 1 : 2;
        const long nblocks = (n_out + POLS_HOP - 1) / POLS_HOP, per_round = (long)ctx().num_cus * POLS_WPB * RPW;
        long rounds = (nblocks + per_round * 20) / (per_round * 40);
        if (rounds < 1) rounds = 1;
        long run = fir_knobs().pols_run > 0 ? fir_knobs().pols_run : (nblocks + per_round * rounds - 1) / (per_round * rounds);
        if (run < 4 * (PP - 1) + 4) run = 4 * (PP - 1) + 4;
        const long nruns = (nblocks + run - 1) / run, nslots = (nruns + POLS_WPB * RPW - 1) / (POLS_WPB * RPW);
        const unsigned grid = (unsigned)(nslots < ctx().num_cus ? nslots : ctx().num_cus);
        float *ho = part0 == 0 ? h_out() : nullptr;
        hipLaunchKernelGGL(kern, dim3(grid), dim3(64 * POLS_WPB), lds_bytes, ctx().stream, h_in(), x, (const float2 *)d_fft_tables.p, y, M, n,
                           n_out, nblocks, run, part0, part0 > 0 ? 1 : 0, ho);
        LR_LAUNCH_CHECK();
        return wrote_hist(ho);
    }
    template <int SS>
    int launch_pols(const float *x, long n, float *y, long n_out)
    {
        const int nparts = (M + FFT_PART - 1) / FFT_PART;
        int wrote = 0;
        // partitions per launch: up to 3 at twelve waves per CU (a delay line of two spectra in registers, 168 registers per lane).  Round 5: a ComplexFloat32 filter of
        // four partitions and more (1 537 taps up) takes FOUR per launch at eight waves per CU (three spectra, 256 registers): 4 096 taps in two launches instead
        // of three - same box, three alternations (profiles/r05_ab_pols_p4.txt): 1.4846 / 1.4822 / 1.4842 -> 1.1281 / 1.1296 / 1.1158 ms on 2^26 samples.
        // LRHIP_POLS_P=3 is the round-4 split (A/B knob).
        const int PMAX = (fir_knobs().pols_p == 4 && SS == 2 && nparts >= 4) ? 4 : 3;
        for (int p0 = 0; p0 < nparts; p0 += PMAX) {
            const int P = nparts - p0 < PMAX ? nparts - p0 : PMAX;
            int rc;
            if constexpr (SS == 2) rc = P == 4 ? launch_pols_p<SS, 4>(x, n, y, n_out, p0) : P == 3 ? launch_pols_p<SS, 3>(x, n, y, n_out, p0) : P == 2 ? launch_pols_p<SS, 2>(x, n, y, n_out, p0) : launch_pols_p<SS, 1>(x, n, y, n_out, p0);
            else rc = P == 3 ? launch_pols_p<SS, 3>(x, n, y, n_out, p0) : P == 2 ? launch_pols_p<SS, 2>(x, n, y, n_out, p0) : launch_pols_p<SS, 1>(x, n, y, n_out, p0);
            if (rc < 0) return rc;
            wrote |= rc;
        }
        return wrote;
    }

    int launch_fft(const float *x, long n, float *y, long n_out)
    {
        switch (fir_fft_form(*this, fir_knobs(), n_out, ctx().num_cus)) {
            case FirFftForm::Long64: return fft64_np == 1 ? launch_fft64_v<2048>(x, n, y, n_out) : S == 1 ? launch_fft64_long<2, 1>(x, n, y, n_out) : launch_fft64_long<2>(x, n, y, n_out);      // (np = 2, 3, 4: two partitions per launch)
            case FirFftForm::Pols: return S == 2 ? launch_pols<2>(x, n, y, n_out) : launch_pols<1>(x, n, y, n_out);
            case FirFftForm::Wave64: return fft4k_V == 768 ? launch_fft64_v<768>(x, n, y, n_out) : fft4k_V == 1024 ? launch_fft64_v<1024>(x, n, y, n_out) : launch_fft64_v<1280>(x, n, y, n_out);
            case FirFftForm::Wg4k: return fft4k_V == 768 ? launch_fft4k<768>(x, n, y, n_out) : fft4k_V == 1024 ? launch_fft4k<1024>(x, n, y, n_out) : launch_fft4k<1280>(x, n, y, n_out);
            case FirFftForm::Pass1024: break;
        }
        const size_t lds_bytes = (size_t)FFT_LDS_ELEMS * sizeof(float2) + (size_t)fir_knobs().fft_lds_pad;
        const float *h = h_in();
        int wrote = 0;
        // one launch per partition of at most FFT_PART taps (a plain filter has one); partitions after the first accumulate
        const int nparts = (M + FFT_PART - 1) / FFT_PART;
        for (int part = 0; part < nparts; part++) {
            const int Mp = part + 1 < nparts ? FFT_PART : M - part * FFT_PART;
            const long Lf = FFTN - ((Mp - 1 + 63) / 64) * 64;      // block advance of the fused kernel (overlap rounded to 64)
            long nblocks = (n_out + Lf - 1) / Lf;
            long nffts = S == 2 ? nblocks : (nblocks + 1) / 2;
            const float2 *tables = (const float2 *)d_fft_tables.p + (size_t)part * FFT_TABLE_ELEMS;
            auto go = [&](auto kern) -> int {
                const long slots = chip_slots(kern, 64 * FFT_WPB, lds_bytes), want = (nffts + FFT_WPB - 1) / FFT_WPB;
                if (slots < 0) return -1;
                // one-shot order with 8 batches per workgroup once the launch exceeds the resident slots: 316 GS/s against 263-314
                // (run-to-run spread) for the persistent stride on 2^28 samples, same box, alternating
                // (only when the launch is many times the resident slots: a 2^26-sample chain's 1/5-rate audio filter, 1 873 workgroups
                // on 768 slots, keeps the persistent walk - 8 batches per workgroup would leave two thirds of the CUs idle)
                // Round 3, re-measured after the early first-block loads and the wave-uniform addressing (two boxes, alternating, HIP events): the persistent walk is
                // now the faster order at every size - 2^26 samples 0.2155 against 0.2368 ms, 2^27 0.4199 / 0.4357, 2^28 0.8359 / 0.8412 and 0.8591 / 0.8646; the
                // Float32 and complex-taps filters at 2^26 gain 9 % - a launch of 8-batch workgroups ends with a ragged last round that the one-block stride
                // does not have.  The one-shot order stays as LRHIP_FFT_ROUNDS=8.
                const int rounds = persistent_rounds(want, slots, fir_knobs().fft_rounds);
                unsigned grid = persistent_grid(want, slots, rounds);
                // input / output in HOST memory (host_execute's direct mode, chain.h): a short persistent grid, so that the reads of one block and the writes of
                // another share the link instead of every wave loading, then every wave storing
                if (host_io_grid() > 0 && rounds == 0 && grid > (unsigned)host_io_grid()) grid = (unsigned)host_io_grid();
                // tapered tail of the one-shot order (kernels_firfft.h): the last three "waves" of workgroups own rounds/2, rounds/4, rounds/8 batches
                // (measured equal on 2^28 samples, same box: 0.865-0.878 ms with, 0.860-0.867 without - the ~45 us fixed cost the size sweep shows is not
                // the tail of long workgroups; opt-in, LRHIP_FFT_TAPER=1)
                int n_full = 0, taper = 0;
                if (rounds >= 2 && fir_knobs().fft_taper) {
                    const long r1 = rounds / 2, r2 = rounds / 4 > 0 ? rounds / 4 : 1, r3 = rounds / 8 > 0 ? rounds / 8 : 1;
                    const long tail_b = slots * (r1 + r2 + r3);
                    if (want > 2 * tail_b) {
                        taper = (int)slots;
                        n_full = (int)((want - tail_b) / rounds);
                        long rem = want - (long)n_full * rounds;                         // >= tail_b
                        long k1 = slots, k2 = slots;
                        rem -= k1 * r1 + k2 * r2;
                        long k3 = rem > 0 ? (rem + r3 - 1) / r3 : 0;
                        grid = (unsigned)(n_full + k1 + k2 + k3);
                    }
                }
                const float2 *dp = pre_disc ? disc_in() : nullptr;
                float *ho = (!pre_disc && part == 0) ? h_out() : nullptr;      // (pre_disc: the history is discriminator output, commit()'s kernel writes it)
#ifdef LRHIP_FFT_TRACE
                static unsigned long long *trace = nullptr;
                static long trace_launches = 0;
                const size_t trace_n = (size_t)8 * FFT_WPB * 32 * 12;
                if (!trace) {
                    LR_HIP(hipMalloc(&trace, trace_n * 8));
                    LR_HIP(hipMemcpyToSymbol(HIP_SYMBOL(lrhip_fft_trace), &trace, sizeof(trace)));
                }
                if (++trace_launches == 12) LR_HIP(hipMemsetAsync(trace, 0, trace_n * 8, ctx().stream));
#endif
                hipLaunchKernelGGL(kern, dim3(grid), dim3(64 * FFT_WPB), lds_bytes, ctx().stream, h, x, tables, y, Mp, n, n_out, nblocks,
                                   1.0 / disc_gain, dp, ho, M, (long)part * FFT_PART, part > 0 ? 1 : 0, rounds, n_full, taper);
#ifdef LRHIP_FFT_TRACE
                if (trace_launches == 12) {
                    // stamps: 0 loop top, 1 loads issued (the first dft16 waits for them), 2 stage 1 done, 3 E1 exchanged, 4 stage 2 + inner transpose done,
                    // 5 stage 3 / H / inverse stage 3 + inner transpose done, 6 inverse stage 2 done, 7 E1 back, 8 inverse stage 1 done, 9 stores issued
                    LR_HIP(hipStreamSynchronize(ctx().stream));
                    std::vector<unsigned long long> tr(trace_n);
                    LR_HIP(hipMemcpy(tr.data(), trace, trace_n * 8, hipMemcpyDeviceToHost));
                    static const char *names[9] = {"issue", "load+st1", "E1", "st2+T", "st3 H st3 T", "ist2", "E1back", "ist1", "store"};
                    double sum[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, blk = 0;
                    int cnt = 0;
                    for (int w = 0; w < 8 * FFT_WPB; w++)
                        for (int t = 1; t < 30; t++) {
                            const unsigned long long *s = &tr[((size_t)w * 32 + t) * 12], *nx = s + 12;
                            if (!s[0] || !s[9] || !nx[0]) continue;
                            for (int i = 0; i < 9; i++) sum[i] += (double)(s[i + 1] - s[i]);
                            blk += (double)(nx[0] - s[0]);
                            cnt++;
                        }
                    if (cnt) {
                        fprintf(stderr, "fft trace (%d blocks):", cnt);
                        for (int i = 0; i < 9; i++) fprintf(stderr, "  %s %.0f", names[i], sum[i] / cnt);
                        fprintf(stderr, "  | block %.0f clocks\n", blk / cnt);
                    }
                }
#endif
                return wrote_hist(ho);
            };
            int rc = S == 2 ? go(fir_fft_kernel<2, 0>) : pre_disc ? go(fir_fft_kernel<1, 1>) : go(fir_fft_kernel<1, 0>);
            if (rc < 0) return rc;
            LR_LAUNCH_CHECK();
            wrote |= rc;
        }
        return wrote;
    }

    // decimations without a Toeplitz instantiation (and taps too long for its LDS table): LDS-staged one-output-per-thread kernel, first or second form (decim_lds2_ok)
    int launch_decim_lds(bool v2, const float *x, long n, float *y, long n_out)
    {
        // staged samples per tile: the kernel's registers allow DECIM_SPAN_MAX; LRHIP_DECIM_SPAN (A/B) asks for less = smaller tiles, more workgroups per CU
        const long span_env = fir_knobs().decim_span;
        const long span_cap = v2 ? DECIM2_SPAN_MAX : DECIM_SPAN_MAX;
        const long span_max = span_env >= 512 && span_env < span_cap && span_env >= M + 64 ? span_env : span_cap;
        const int dsc = post_disc ? 1 : 0;       // discriminator epilogue (second form only): OW counts the stored outputs, every tile computes one more in front
        if (dsc && !v2) return set_error("internal: discriminator epilogue on the first LDS-staged decimator form");
        long ow = (span_max - M) / (long)D + 1 - dsc;
        int OW = (int)(ow > 256 - 4 * dsc ? 256 - 4 * dsc : ow < 1 ? 1 : ow);
        long ntiles = (n_out + OW - 1) / OW;
        long span = (long)(OW - 1 + dsc) * D + M;
        size_t lds_bytes = v2 ? ((size_t)((M + 3) & ~3) + (size_t)2 * decim2_slots((int)span, (long)D)) * sizeof(float)
                              : ((size_t)(((taps_complex ? 2 : 1) * M + 3) & ~3) + (size_t)S * (span + (span >> 5) + 2)) * sizeof(float);
        const float *h = h_in();
        float *ho = h_out();
        // (more: what the second form's kernels take behind `rounds`)
        auto go = [&](auto kern, auto... more) -> int {
            const long slots = chip_slots(kern, 256, lds_bytes);
            if (slots < 0) return -1;
            const int rounds = persistent_rounds(ntiles, slots, fir_knobs().decim_rounds);
            hipLaunchKernelGGL(kern, dim3(persistent_grid(ntiles, slots, rounds)), dim3(256), lds_bytes, ctx().stream, h, x, (const float *)d_taps.p, y, M, n, n_out, (long)index,
                               (long)D, OW, ntiles, rot ? rot_step : (uint64_t)0, rot ? count : (uint64_t)0, ho, post_unary, rounds, more...);
            return 0;
        };
        auto go2 = [&](auto kern) -> int {
            return go(kern, 1.0 / disc_gain, dsc ? disc_in() : (const float2 *)nullptr, dsc ? disc_out() : (float2 *)nullptr,
                      rel_rot ? 0 : 1);      // an exact chain keeps one fmaf chain per output (no tap split over the half-waves)
        };
        int rc;
        if (v2) {
            auto pick = [&](auto ph) -> int {
                constexpr bool PH = decltype(ph)::value;
                if (raw_now) {
                    auto raw = [&](auto r) { return with_record_format(in_fmt, [&](auto fmt) { return go2(fir_decim_lds2_kernel<decltype(r)::value, decltype(fmt)::value, PH>); }); };
                    return rot ? raw(std::true_type{}) : raw(std::false_type{});
                }
                return rot ? go2(fir_decim_lds2_kernel<true, RX_FMT_CF32, PH>) : go2(fir_decim_lds2_kernel<false, RX_FMT_CF32, PH>);
            };
            rc = decim2_esh((long)D) ? pick(std::true_type{}) : pick(std::false_type{});
        } else if (raw_now) {
            if (taps_complex || S != 2) return set_error("internal: raw records reached a kernel without a record instantiation");
            auto raw = [&](auto r) { return with_record_format(in_fmt, [&](auto fmt) { return go(fir_decim_lds_kernel<2, decltype(r)::value, false, decltype(fmt)::value>); }); };
            rc = rot ? raw(std::true_type{}) : raw(std::false_type{});
        } else
        rc = taps_complex ? go(fir_decim_lds_kernel<2, false, true>)
                 : S == 2 ? (rot ? go(fir_decim_lds_kernel<2, true>) : go(fir_decim_lds_kernel<2, false>))
                        : (rot ? set_error("rotator fusion needs complex input") : go(fir_decim_lds_kernel<1, false>));
        if (rc) return rc;
        LR_LAUNCH_CHECK();
        return wrote_hist(ho) | (dsc ? WROTE_DISC : 0);
    }

    template <int DD>
    int launch_decfft_d(const float *x, long n, float *y, long n_out)
    {
        const size_t lds_bytes = (size_t)df_lds_elems(DD) * sizeof(float2);
        DfParams pr;
        pr.M = M; pr.n = n; pr.n_out = n_out; pr.first = (long)index;
        pr.nblocks = (n_out + DF_LO - 1) / DF_LO;
        pr.rot_step_fx = rot ? rot_step : 0; pr.rot_count0 = rot ? count : 0;
        const double wD = rot ? rot_omega * (double)DD : 0.0;
        pr.cD = make_float2((float)std::cos(wD), (float)std::sin(wD));
        pr.inv_gain = 1.0 / disc_gain;
        pr.taps_rev = (const float *)d_taps.p; pr.taps_complex = taps_complex;
        pr.dbg = ablation_bits("LRHIP_DECFFT_DBG");      // ablation knob (tools/ab_decfft.py): 0 unless the library was built with -DLRHIP_ABLATION
        const float *h = h_in();
        float *ho = h_out();
        auto go = [&](auto kern) -> int {
            const long nquads = (pr.nblocks + 3) / 4, slots = chip_slots(kern, 256, lds_bytes);
            if (slots < 0) return -1;
            // one-shot order (common.h grid_for): workgroups of 4 waves x `rounds` consecutive quads, handed out in address order.  More
            // quads per wave amortise the table load and the first (unhidden) window request; same-box A/B at 2^26 samples:
            // rounds 1 / 2 / 4 = 0.171 / 0.167 / 0.164 ms
            int rounds = fir_knobs().decfft_rounds > 0 ? fir_knobs().decfft_rounds : (nquads >= 16 * slots ? 4 : nquads >= 8 * slots ? 2 : 1);
            pr.rounds = rounds;
            const long wgs = (nquads + 4L * rounds - 1) / (4L * rounds);
            hipLaunchKernelGGL(kern, dim3((unsigned)wgs), dim3(256), lds_bytes, ctx().stream, h, x, (const float2 *)d_dec_tables.p, y, pr,
                               post_disc ? disc_in() : nullptr, post_disc ? disc_out() : nullptr, ho);
            return 0;
        };
        int rc = post_disc ? go(fir_decfft_kernel<DD, 1>) : go(fir_decfft_kernel<DD, 0>);
        if (rc) return rc;
        LR_LAUNCH_CHECK();
        return wrote_hist(ho) | (post_disc ? WROTE_DISC : 0);
    }

    int launch_direct(const float *x, long n, float *y, long n_out)
    {
        if (rot) return set_error("internal: direct FIR kernel has no fused rotator");
        unsigned grid = grid_for((unsigned long)n_out, 256);
        const float *h = h_in(), *t = (const float *)d_taps.p;
        if (S == 1)
            hipLaunchKernelGGL(fir_direct_kernel<0>, dim3(grid), dim3(256), 0, ctx().stream, h, x, t, y, M, n, n_out, (long)index, (long)D);
        else if (!taps_complex)
            hipLaunchKernelGGL(fir_direct_kernel<1>, dim3(grid), dim3(256), 0, ctx().stream, h, x, t, y, M, n, n_out, (long)index, (long)D);
        else
            hipLaunchKernelGGL(fir_direct_kernel<2>, dim3(grid), dim3(256), 0, ctx().stream, h, x, t, y, M, n, n_out, (long)index, (long)D);
        LR_LAUNCH_CHECK();
        return 0;
    }

    template <int MM, bool ONESHOT = false>
    int launch_win_real_m(const float *x, long n, float *y)
    {
        using G = FwrGeom<MM>;
        const size_t lds_bytes = (size_t)G::LDS_FLOATS * sizeof(float);
        auto kern = fir_win_real_kernel<MM, false>;
        const long ntiles = (n + FWR_TILE - 1) / FWR_TILE, slots = chip_slots(kern, 256, lds_bytes);
        if (slots < 0) return -1;
        FwrParams pr;
        memset(&pr, 0, sizeof(pr));
        pr.hist = h_in(); pr.x = x; pr.n = n; pr.taps_rev = (const float *)d_taps.p; pr.y = y;
        pr.hist_out = h_out();
        pr.run = ONESHOT ? 1 : (ntiles + slots - 1) / slots;
        pr.dec = 1;
        hipLaunchKernelGGL(kern, dim3((unsigned)((ntiles + pr.run - 1) / pr.run)), dim3(256), lds_bytes, ctx().stream, pr);
        LR_LAUNCH_CHECK();
        return wrote_hist(pr.hist_out);
    }
    // register-window kernel of kernels_firwin2.h (fir_win_cplx_ok, fir_win_pair_ok, fir_win_short_ok) and the recurrence fused behind its pair mode
    float iir_b0 = 1.f, iir_na1 = 0.f, iir_na1_lo = 0.f;
    int iir_warm = 1;
    DeviceBuf d_iir_ptab;
    // first-order recurrence behind the pair-mode filter: needs |a1|^(320 w) < 1e-12 for the in-launch warm-up (w waves of 64 lanes x 5 outputs)
    // The pole q (a double: p^D of the polyphase identity) is carried as a Float32 pair hi + lo: rounded to one Float32 its relative error of
    // 2^-24 moves the DC gain by 2^-24 q / (1 - q), which for a slow filter is far above the 1e-6 parity bar of the recurrence it replaces.
    int fuse_iir1(double b0, double q)
    {
        if (!fir_win_pair_ok(*this, fir_knobs())) return -1;
        const double a1 = -q, p = std::fabs(q);
        int w = 0;
        for (int c = 1; c <= 4 && !w; c *= 2)
            if (p < 1.0 && std::pow(p, 320.0 * c) < 1e-12) w = c;
        if (!w) return -1;
        std::vector<float> ptab(64);
        double pR = 1.0, acc = 1.0;
        for (int k = 0; k < 5; k++) pR *= -(double)a1;
        for (int l = 0; l < 64; l++) { acc *= pR; ptab[(size_t)l] = (float)acc; }
        if (upload(d_iir_ptab, ptab.data(), ptab.size() * sizeof(float))) return -1;
        iir_fused = true; iir_b0 = (float)b0; iir_na1 = (float)q; iir_na1_lo = (float)(q - (double)iir_na1); iir_warm = w;
        return reset();
    }
    template <int MM, int MODE, int DD = 5, bool ONESHOT = false>
    int launch_win_cplx_m(const float *x, long n, float *y, long n_out)
    {
        using G = FwcGeom<DD, 5, MM, MODE>;
        const size_t lds_bytes = (size_t)G::LDS_FLOATS * sizeof(float);
        auto kern = fir_win_cplx_kernel<DD, 5, MM, MODE>;
        const long slots = chip_slots(kern, 256, lds_bytes);
        if (slots < 0) return -1;
        FwcParams pr;
        memset(&pr, 0, sizeof(pr));
        pr.hist = h_in(); pr.x = x; pr.n = n; pr.taps_rev = (const float *)(G::CTAPS ? d_ctaps4.p : d_taps.p); pr.y = y;
        pr.n_out = n_out; pr.first = (long)index;
        pr.hist_out = h_out();
        pr.ntiles = G::PAIR ? (n_out + 2L * G::TO - 1) / (2L * G::TO) : (n_out + G::TA - 1) / G::TA;
        pr.rot_step_fx = rot ? rot_step : 0; pr.rot_count0 = rot ? count : 0;
        if (G::DISC) {
            pr.prev_in = disc_in(); pr.prev_out = disc_out();
            pr.inv_gain = 1.0 / disc_gain;
        }
        unsigned grid;
        if (G::IIR) {
            pr.b0 = iir_b0; pr.na1 = iir_na1; pr.na1_lo = iir_na1_lo; pr.ptab = (const float *)d_iir_ptab.p; pr.warm_waves = iir_warm;
            pr.state_in = iir_in(); pr.state_out = iir_out();
            pr.fix_edge = pr.fix_prev = (const float2 *)d_iir_ptab.p;          // readable dummies (64 floats): the kernel loads unconditionally
            pr.fix_inv_gain = 1.0;
            if (fix_src && fix_src->fix_ready) {
                pr.fix_edge = (const float2 *)fix_src->edge.p; pr.fix_prev = fix_src->fix_prev_ptr; pr.fix_inv_gain = 1.0 / fix_src->disc_gain;
                pr.fix_on = 1;
                pr.fix_shift = fix_src->fix_shift;
                fix_src->fix_ready = false;
            }
            pr.run = (pr.ntiles + slots - 1) / slots;
            if (fir_knobs().tail_run > 0) pr.run = fir_knobs().tail_run;
            grid = (unsigned)((pr.ntiles + pr.run - 1) / pr.run);
        } else {
            pr.warm_waves = 4; pr.run = 1;
            // pair mode without the recurrence (a 136-tap decimate-by-5 Float32 filter on its own): the kernel's prefetch loads from fix_edge / fix_prev
            // unconditionally on every interior tile - readable dummies here as well (the taps: 136 floats), not the null pointers of the memset above
            if (G::PAIR) { pr.fix_edge = pr.fix_prev = (const float2 *)d_taps.p; pr.fix_inv_gain = 1.0; }
            // ONESHOT: a workgroup per tile, handed out in address order (short filters are a streaming problem: common.h grid_for)
            grid = (unsigned)((ONESHOT || fir_knobs().win_oneshot || pr.ntiles < slots) ? pr.ntiles : slots);
        }
        hipLaunchKernelGGL(kern, dim3(grid), dim3(256), lds_bytes, ctx().stream, pr);
        LR_LAUNCH_CHECK();
        return wrote_hist(pr.hist_out) | (G::DISC ? WROTE_DISC : 0) | (G::IIR ? WROTE_IIR : 0);
    }
    int launch_win_cplx(const float *x, long n, float *y, long n_out)
    {
        if (post_disc) return rot ? launch_win_cplx_m<128, FWC_ROT | FWC_DISC>(x, n, y, n_out) : launch_win_cplx_m<128, FWC_DISC>(x, n, y, n_out);
        return rot ? launch_win_cplx_m<128, FWC_ROT>(x, n, y, n_out) : launch_win_cplx_m<128, 0>(x, n, y, n_out);
    }
    int launch_short_real(const float *x, long n, float *y)
    {
        const float *h = h_in(), *t = (const float *)d_taps.p;
        float *ho = h_out();
        const unsigned grid = grid_for((unsigned long)((n + 3) / 4), 256);
        if (M == 16) hipLaunchKernelGGL(fir_short_real_kernel<16>, dim3(grid), dim3(256), 0, ctx().stream, h, x, t, y, n, ho);
        else hipLaunchKernelGGL(fir_short_real_kernel<32>, dim3(grid), dim3(256), 0, ctx().stream, h, x, t, y, n, ho);
        LR_LAUNCH_CHECK();
        return wrote_hist(ho);
    }

    template <int SS>
    int dispatch_mfma(bool persistent, const float *x, long n, float *y, long n_out)
    {
        switch (D) {
            case 1: return launch_mfma<SS, 1, LRHIP_FIR_D1_NACC>(persistent, x, n, y, n_out);
            case 2: return launch_mfma<SS, 2, 4>(persistent, x, n, y, n_out);
            case 3: return launch_mfma<SS, 3, 2>(persistent, x, n, y, n_out);
            case 4: return launch_mfma<SS, 4, 2>(persistent, x, n, y, n_out);
            case 5: return fir_knobs().d5_nacc == 1 ? launch_mfma<SS, 5, 1>(persistent, x, n, y, n_out) : launch_mfma<SS, 5, 2>(persistent, x, n, y, n_out);
            case 6: return launch_mfma<SS, 6, 1>(persistent, x, n, y, n_out);
            case 7: return launch_mfma<SS, 7, 1>(persistent, x, n, y, n_out);
            case 8: return launch_mfma<SS, 8, 1>(persistent, x, n, y, n_out);
            case 10: return launch_mfma<SS, 10, 1>(persistent, x, n, y, n_out);
            default: return set_error("internal: no Toeplitz kernel at decimation %u", D);
        }
    }

    // The one place where the carried state advances, behind a call's launches.  wrote: what they wrote into the next slots (WROTE_*).  The history is
    // carried here where no launch did - a call that emits nothing launches no filter and still carries it; x is read for that alone - and exactly the
    // slots that were written become current
    int commit(long n, long n_out, int wrote, const float *x = nullptr)
    {
        if (pre_disc) {
            // (the history is discriminator output: real taps, no pad, M >= 32 - plan_disc_fir)
            unsigned grid = grid_for((unsigned long)(M > 1 ? M - 1 : 1), 256);
            hipLaunchKernelGGL(fir_fft_pre_history_kernel, dim3(grid), dim3(256), 0, ctx().stream, h_in(), x, h_out(), M, n, 1.0 / disc_gain, disc_in(), disc_out());
            LR_LAUNCH_CHECK();
            wrote |= WROTE_HIST | WROTE_DISC;
        } else if (!(wrote & WROTE_HIST) && M > 1) {
            unsigned grid = grid_for((unsigned long)(M - 1) * S, 256);
            if (S == 1)
                hipLaunchKernelGGL(fir_history_kernel<1>, dim3(grid), dim3(256), 0, ctx().stream, h_in(), x, h_out(), M, n);
            else
                hipLaunchKernelGGL(fir_history_kernel<2>, dim3(grid), dim3(256), 0, ctx().stream, h_in(), x, h_out(), M, n);
            LR_LAUNCH_CHECK();
        }
        hist.flip();
        if (wrote & WROTE_DISC) disc.flip();
        if (wrote & WROTE_IIR) iir.flip();
        index = index + (unsigned long)n_out * D - (unsigned long)n;
        count += (uint64_t)n;
        return 0;
    }

    // HilbertTransformBlock in one launch (hilbert_ok): 0, or -1 with the message set.  D = 1: the index stays 0
    int hilbert(const float *x, long n, float *y2)
    {
        if (hilb_sparse < 0) {
            hilb_sparse = (M == 65 || M == 129) ? 1 : 0;
            for (int j = 0; j < M && hilb_sparse; j += 2)
                if (taps_rev[(size_t)j] != 0.0f) hilb_sparse = 0;
        }
        const bool win = hilb_sparse && !fir_knobs().hilbert_mfma && index == 0;
        const int wrote = !win ? launch_hilbert_mfma(x, n, y2) : M == 65 ? launch_hilbert_win<65>(x, n, y2) : launch_hilbert_win<129>(x, n, y2);
        return wrote < 0 ? -1 : commit(n, n, wrote, x);
    }

    // filter n inputs (device), emit the retained outputs; commit() advances history / index / count
    long core(const float *x, long n, float *y, unsigned long cap)
    {
        if (n <= 0) return 0;
        fix_ready = false;
        long n_out = (unsigned long)n > index ? (long)((n - index + D - 1) / D) : 0;
        if ((unsigned long)n_out > cap) return set_error("fir: output capacity %lu < %ld", cap, n_out);
        if (fix_src && fix_src->fix_ready && n_out == 0) {
            // the producer left its wave-first discriminator outputs to this stage's staging, but this chunk launches no window kernel
            // (fewer inputs than the decimation index): patch them in place before they enter the history
            hipLaunchKernelGGL(fir_disc_fixup_kernel, dim3((unsigned)((fix_src->fix_nunits + 255) / 256)), dim3(256), 0, ctx().stream,
                               (const float2 *)fix_src->edge.p, fix_src->fix_nunits, fix_src->fix_unit, const_cast<float *>(x), n, fix_src->fix_prev_ptr,
                               1.0 / fix_src->disc_gain);
            LR_LAUNCH_CHECK();
            fix_src->fix_ready = false;
        }
        int wrote = 0;
        if (n_out > 0) {
            const FirForm f = form((uintptr_t)x % (raw_now ? (in_fmt == RX_FMT_S16LE ? 4u : 2u) : 4u * (unsigned)S) == 0);      // (aligned to the sample - raw records: the record - size?)
            int rc = -1;
            switch (f) {
                case FirForm::DecFft: rc = D == 2 ? launch_decfft_d<2>(x, n, y, n_out) : D == 4 ? launch_decfft_d<4>(x, n, y, n_out) : D == 5 ? launch_decfft_d<5>(x, n, y, n_out) : launch_decfft_d<8>(x, n, y, n_out); break;
                case FirForm::OverlapSave: rc = launch_fft(x, n, y, n_out); break;
                case FirForm::WinReal: rc = M == 32 ? launch_win_real_m<32>(x, n, y) : M == 64 ? launch_win_real_m<64>(x, n, y) : launch_win_real_m<128>(x, n, y); break;
                case FirForm::WinCplx: rc = launch_win_cplx(x, n, y, n_out); break;
                case FirForm::WinShort: rc = M == 16 ? launch_win_cplx_m<16, 0, 1, true>(x, n, y, n_out) : M == 32 ? launch_win_cplx_m<32, 0, 1, true>(x, n, y, n_out) : launch_win_cplx_m<64, 0, 1, true>(x, n, y, n_out); break;
                case FirForm::WinShortC: rc = M == 16 ? launch_win_cplx_m<16, FWC_CTAPS, 1, true>(x, n, y, n_out) : launch_win_cplx_m<32, FWC_CTAPS, 1, true>(x, n, y, n_out); break;
                case FirForm::ShortReal: rc = launch_short_real(x, n, y); break;
                case FirForm::WinPair: rc = iir_fused ? launch_win_cplx_m<136, FWC_PAIR | FWC_IIR>(x, n, y, n_out) : launch_win_cplx_m<136, FWC_PAIR>(x, n, y, n_out); break;
                case FirForm::DecimLds1: case FirForm::DecimLds2: rc = launch_decim_lds(f == FirForm::DecimLds2, x, n, y, n_out); break;
                case FirForm::Direct: rc = launch_direct(x, n, y, n_out); break;
                case FirForm::MfmaCc: rc = dispatch_mfma_cc(x, n, y, n_out); break;
                case FirForm::MfmaPersistent: case FirForm::MfmaGeneric: rc = S == 1 ? dispatch_mfma<1>(f == FirForm::MfmaPersistent, x, n, y, n_out) : dispatch_mfma<2>(f == FirForm::MfmaPersistent, x, n, y, n_out); break;
            }
            if (rc < 0) return rc;
            wrote = rc;
        }
        return commit(n, n_out, wrote, x) ? -1 : n_out;
    }

    // does this chunk reach the persistent Tuner kernel, the one with a record instantiation?  (core()'s dispatch, the D = 5 / 128-tap shape)
    bool raw_path_ok(const void *in_dev, unsigned long n_in) const
    {
        if (!in_fmt || !fir_raw_records_ok(*this, fir_knobs()) || n_in <= index) return false;      // (no output: nothing launches, the history kernel would read x)
        return ((uintptr_t)in_dev % (in_fmt == RX_FMT_S16LE ? 4u : 2u)) == 0;
    }
    long run(const void *in_dev, unsigned long n_in, void *out_dev, unsigned long cap) override
    {
        const float *x = (const float *)in_dev;
        float *y = (float *)out_dev;
        if (in_fmt) {
            if (!n_in) return 0;
            if (!fir_knobs().tuner_no_raw && raw_path_ok(in_dev, n_in)) {
                raw_now = true;
                const long rc = core(x, (long)n_in, y, cap);
                raw_now = false;
                return rc;
            }
            if (converted.reserve((size_t)n_in * 8 + 16)) return -1;
            const long m = fmt_stage->run(in_dev, n_in, converted.p, n_in);
            if (m < 0) return m;
            x = (const float *)converted.p;
        }
        if (!use_fft) return core(x, (long)n_in, y, cap);
        // overlap-save framing: emit only whole L-blocks, keep the tail pending (firfilter.lua:451-485)
        long total = fill + (long)n_in, emit = (total / L) * L;
        size_t ss = (size_t)S * sizeof(float);
        if (emit == 0) {
            if (n_in) LR_HIP(hipMemcpyAsync((char *)pending.p + fill * ss, x, n_in * ss, hipMemcpyDeviceToDevice, ctx().stream));
            fill = total;
            return 0;
        }
        if ((unsigned long)emit > cap) return set_error("fir(fft framing): output capacity %lu < %ld", cap, emit);
        if (work.reserve((size_t)((long)n_in + L) * ss)) return -1;      // the largest total this chunk size can see: no regrowth as `fill` moves
        if (fill) LR_HIP(hipMemcpyAsync(work.p, pending.p, fill * ss, hipMemcpyDeviceToDevice, ctx().stream));
        LR_HIP(hipMemcpyAsync((char *)work.p + fill * ss, x, n_in * ss, hipMemcpyDeviceToDevice, ctx().stream));
        long rc = core((const float *)work.p, emit, y, cap);
        if (rc < 0) return rc;
        fill = total - emit;
        if (fill) LR_HIP(hipMemcpyAsync(pending.p, (char *)work.p + emit * ss, fill * ss, hipMemcpyDeviceToDevice, ctx().stream));
        return emit;
    }
};

static uint64_t turns_fixed(double omega);      // (stage_elem.h: a rotator's omega as 64-bit fixed-point turns per sample)
// FIRFilterBlock as a stage: the request resolved into a shape (fir_plan.h) - refused there, before the device is touched - and the tables that shape
// calls for built (fir_tables.h) and uploaded
static FirStage *fir_build(const float *taps, unsigned ntaps, int taps_complex, int input_complex, unsigned decim, int use_fft, bool rot, double omega)
{
    const FirPlan p = fir_resolve({taps ? ntaps : 0, taps_complex, input_complex, decim, use_fft, rot});
    if (p.refusal) { set_error("%s", p.refusal); return nullptr; }
    std::unique_ptr<FirStage> q = new_stage<FirStage>();
    if (!q) return nullptr;
    q->M = (int)ntaps; q->S = input_complex ? 2 : 1; q->taps_complex = taps_complex; q->D = decim; q->rot = rot; q->in_size = q->out_size = 4 * q->S;
    q->mode_req = p.mode_req; q->use_fft = p.use_fft; q->fft_arith = p.fft_arith; q->decfft = p.decfft; q->ctaps4 = p.ctaps4;
    q->ksteps = p.ksteps; q->fft4k_V = p.fft4k_V; q->fft64_np = p.fft64_np; q->hist_pad = p.hist_pad; q->L = p.L;
    if (rot) { q->rot_step = turns_fixed(omega); if (p.decfft) q->rot_omega = omega; }
    q->taps_rev = fir_reversed_taps(taps, ntaps, taps_complex);
    const auto up = [](DeviceBuf &b, const std::vector<float> &t) { return upload(b, t.data(), t.size() * sizeof(float)); };
    const unsigned T = p.tables;      // (FIR_TAB_*; the uploads in the order they always had)
    if (up(q->d_taps, q->taps_rev)) return nullptr;
    if ((T & FIR_TAB_TOEPLITZ) && up(q->d_atab, fir_toeplitz_taps(q->taps_rev, q->M, (int)decim, p.ksteps))) return nullptr;
    if ((T & FIR_TAB_CTAPS4) && up(q->d_ctaps4, fir_ctaps4_table(q->taps_rev, q->M))) return nullptr;
    if ((T & FIR_TAB_TOEPLITZ_CC) && up(q->d_atab, fir_toeplitz_cc_taps(q->taps_rev, q->M, (int)decim, p.ksteps))) return nullptr;
    if ((T & FIR_TAB_DECFFT) && up(q->d_dec_tables, fir_decfft_tables(taps, q->M, taps_complex, (int)decim, q->rot_omega))) return nullptr;
    if ((T & FIR_TAB_FFT1024) && up(q->d_fft_tables, fir_fft1024_tables(taps, ntaps, taps_complex))) return nullptr;
    if (T & FIR_TAB_FFT64) {      // 513 .. 1 281 taps: both 4096-point kernels read the one spectrum of all taps
        std::vector<double> Hr, Hi;
        taps_spectrum(taps, taps_complex, 0, ntaps, F4K_N, Hr, Hi);
        if ((T & FIR_TAB_FFT4K) && up(q->d_fft4k_tables, fir_fft4k_tables(Hr, Hi))) return nullptr;
        if (up(q->d_fft64_tables, fir_fft64_tables(Hr, Hi))) return nullptr;
    }
    if ((T & FIR_TAB_FFT64_LONG) && up(q->d_fft64_tables, fir_fft64_long_tables(taps, ntaps, taps_complex, p.fft64_np))) return nullptr;
    if (q->use_fft && q->pending.reserve((size_t)q->L * q->S * sizeof(float))) return nullptr;      // the framing's tail of less than a block
    if (q->reset()) return nullptr;
    return q.release();
}
