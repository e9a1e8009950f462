// chain_plan.h - lrhip_chain_create_ex's planner: one rule per fused form over the caller's stages, then the passes over the planned ops
// (part of liblrhip.so; included by lrhip.hip in this order, one translation unit)
#pragma once

// the chain's flags (lrhip_chain_create_ex), read once
struct PlanFlags {
    bool fusion;          // not LRHIP_CHAIN_NO_FUSION: every block runs its own kernels; edges stay on the device
    bool exact_rotator;   // LRHIP_CHAIN_EXACT_ROTATOR
    bool own_arith;       // LRHIP_CHAIN_NO_POLYPHASE_TAIL: "keep every block's own arithmetic" (polyphase tail and FIR cascade alike)
    bool single_launch;   // not LRHIP_CHAIN_NO_SINGLE_LAUNCH
};
// what a rule sees: the caller's stages (borrowed), the flags, and the ops planned so far.  A rule at stage i appends the op(s) it built and returns
// how many stages it consumed, returns 0 (does not apply) or -1 (error, set_error).  The environment knobs are A/B switches, read once per process.
struct Plan {
    lrhip_stage_t **st;
    unsigned n;
    PlanFlags f;
    std::vector<lrhip_chain::Op> &ops;
    template <typename T> T *at(unsigned k) const { return k < n ? dynamic_cast<T *>(st[k]) : nullptr; }
    void add(std::unique_ptr<lrhip_stage> built) { ops.emplace_back(std::move(built)); }
};
// a FrequencyDiscriminatorBlock folded in front of (pre) or behind a freshly built filter: ComplexFloat32 in, Float32 out
static int fold_discriminator(FirStage *f, bool pre, const FmDiscrimStage *d)
{
    (pre ? f->pre_disc : f->post_disc) = true;
    f->disc_gain = d->gain;
    f->in_size = 8;
    f->out_size = 4;
    return f->reset();
}
// fir fir ... (ComplexFloat32 stream, every one of them on the overlap-save arithmetic: "fast", or left to the library)  ->  ONE filter with the convolved taps
// while they fit the 4096-point kernel (kernels_firfft4k.h: 1 281 taps).  A chain of filters is a filter; overlap-save promises 1e-6 of the exact
// result, not the bits of a particular block size, and the merged filter rounds once where the chain rounds per stage.  The reference suite's first
// entry (five 256-tap filters back to back, luaradio_benchmark.lua:17-37) = 1 276 taps = one launch instead of five.
static int plan_fir_cascade(Plan &p, unsigned i)
{
    static const bool no_cascade = getenv("LRHIP_NO_FIR_CASCADE") != nullptr;      // A/B knob
    auto mergeable = [&p](unsigned k) -> FirStage * {
        FirStage *f = p.at<FirStage>(k);
        return (f && f->S == 2 && f->D == 1 && !f->rot && !f->pre_disc && !f->post_disc && !f->use_fft && f->fft_arith && (f->mode_req == 2 || f->mode_req == 3)) ? f : nullptr;
    };
    // (LRHIP_CHAIN_NO_POLYPHASE_TAIL = "keep every block's own arithmetic": the same kind of identity, the same switch)
    if (no_cascade || p.f.own_arith || !mergeable(i) || !mergeable(i + 1)) return 0;
    // taps in natural order, double, complex (real taps: zero imaginary parts)
    auto natural = [](const FirStage *f) {
        const std::vector<float> t = f->natural_taps();
        const int ts = f->taps_complex ? 2 : 1;
        std::vector<double> h((size_t)2 * f->M, 0.0);
        for (int k = 0; k < f->M; k++)
            for (int c = 0; c < ts; c++) h[2 * k + c] = t[(size_t)k * ts + c];
        return h;
    };
    std::vector<double> acc = natural(mergeable(i));
    bool cplx = mergeable(i)->taps_complex;
    unsigned k = i + 1;
    for (FirStage *fk; (fk = mergeable(k)) && acc.size() / 2 + (size_t)fk->M - 1 <= 1281; k++) {
        const std::vector<double> h = natural(fk);
        std::vector<double> out(acc.size() + h.size() - 2, 0.0);
        for (size_t a = 0; a < acc.size() / 2; a++)
            for (size_t b = 0; b < h.size() / 2; b++) {
                out[2 * (a + b)] += acc[2 * a] * h[2 * b] - acc[2 * a + 1] * h[2 * b + 1];
                out[2 * (a + b) + 1] += acc[2 * a] * h[2 * b + 1] + acc[2 * a + 1] * h[2 * b];
            }
        acc.swap(out);
        cplx = cplx || fk->taps_complex;
    }
    if (k == i + 1) return 0;
    const unsigned Mm = (unsigned)(acc.size() / 2);
    std::vector<float> taps((size_t)Mm * (cplx ? 2 : 1));
    for (unsigned t = 0; t < Mm; t++)
        for (int c = 0; c < (cplx ? 2 : 1); c++) taps[(cplx ? 2 * t : t) + c] = (float)acc[2 * t + c];
    std::unique_ptr<FirStage> merged(fir_build(taps.data(), Mm, cplx ? 1 : 0, 1, 1, 2, false, 0.0));
    if (!merged) return -1;
    p.add(std::move(merged));
    return (int)(k - i);
}
// [multiplyconstant(real)] upsampler fir(real taps, plain) [downsampler]  ->  one polyphase resampling launch
static int plan_resample(Plan &p, unsigned i)
{
    static const bool no_resample_fusion = getenv("LRHIP_NO_RESAMPLE_FUSION") != nullptr;      // A/B knob
    static const bool no_interp_win = getenv("LRHIP_NO_INTERP_WIN") != nullptr;      // A/B knob: one output per thread (fir_resample_kernel)
    unsigned k = i;
    MulConstStage *mc = p.at<MulConstStage>(k);
    if (mc && mc->mode <= 1) k++; else mc = nullptr;
    UpsamplerStage *up = p.at<UpsamplerStage>(k);
    FirStage *rf = up ? p.at<FirStage>(k + 1) : nullptr;
    // (a filter whose arithmetic was left to the library - use_fft nil, mode 3 - may have picked overlap-save for itself: the polyphase form wins)
    if (no_resample_fusion || !rf || rf->taps_complex || rf->use_fft || (rf->fft_arith && rf->mode_req != 3) || rf->D != 1 || rf->rot || rf->pre_disc) return 0;
    DownsamplerStage *rd = p.at<DownsamplerStage>(k + 2);
    const unsigned long D = rd ? rd->factor : 1;
    const int L = (int)up->factor;
    if (!ResampleStage::fits(rf->M, L, D)) return 0;
    std::unique_ptr<ResampleStage> q(new (std::nothrow) ResampleStage());
    if (!q) return set_error("out of memory");
    q->S = rf->S; q->M = rf->M; q->L = L; q->D = D;
    q->HQ = (rf->M - 1) / L + 1;
    q->c = mc ? mc->cr : 1.f;
    q->in_size = q->out_size = rf->S * 4;
    const std::vector<float> taps = rf->natural_taps();
    if (upload(q->d_taps, taps.data(), taps.size() * sizeof(float)) || q->reset()) return -1;
    if (!no_interp_win && q->S == 2 && q->M == 128 && ((D == 1 && L >= 2 && L <= 5) || ResampleStage::rational_supported(L, D))) {
        // tap table of fir_interp_kernel: ttab[s * LP + p] = h[p + (J - 1 - s) L], step 0 = the oldest sample
        const int J = (q->M + L - 1) / L, LP = (L + 3) & ~3;
        std::vector<float> tt((size_t)J * LP, 0.f);
        for (int st = 0; st < J; st++)
            for (int ph = 0; ph < L; ph++) {
                const int t = ph + (J - 1 - st) * L;
                if (t < q->M) tt[(size_t)st * LP + ph] = taps[t];
            }
        if (upload(q->d_ttab, tt.data(), tt.size() * sizeof(float))) return -1;
        q->interp_J = J;
    }
    p.add(std::move(q));
    return (int)(k + 2 + (rd ? 1 : 0) - i);
}
// [rotator] fir(real taps, plain) [downsampler] [discriminator | complex -> real element-wise block]  ->  one decimating Toeplitz-MFMA launch
static int plan_tuner(Plan &p, unsigned i)
{
    static const bool rot_fir_d1 = getenv("LRHIP_ROT_FIR_FUSE_D1") != nullptr;      // A/B knob: fuse a rotator in front of a D = 1 filter all the same
    static const bool no_disc_fusion = getenv("LRHIP_NO_DISC_FUSION") != nullptr;      // A/B knob
    static const bool no_auto_decfft = getenv("LRHIP_NO_AUTO_DECFFT") != nullptr;      // A/B knob
    static const bool no_unary_fold = getenv("LRHIP_NO_UNARY_FOLD") != nullptr;      // A/B knob
    RotatorStage *rot = p.at<RotatorStage>(i);
    const unsigned j = rot ? i + 1 : i;
    FirStage *fir = p.at<FirStage>(j);
    if (!fir || fir->use_fft || fir->D != 1 || fir->rot) return 0;
    if (rot && fir->taps_complex) return 0;      // rotator folding is implemented for real taps only
    DownsamplerStage *ds = p.at<DownsamplerStage>(j + 1);
    // a rotator in front of a filter that does NOT decimate stays a launch of its own: the rotating Toeplitz kernel at D = 1 has no register room left
    // (112-296 bytes of scratch) and runs 2^26 samples in 0.62 ms, against 0.17 (rotator) + 0.21 (overlap-save) / 0.39 (direct form) for the pair
    if (rot && !ds && !rot_fir_d1) return 0;
    // ... [discriminator]: runs as the epilogue of the persistent kernel (ComplexFloat32 outputs never reach HBM)
    const unsigned after = j + 1 + (ds ? 1 : 0);
    // a filter that asked for overlap-save arithmetic keeps it when fused with a downsampler (polyphase FFT form, kernels_firdecfft.h)
    // (only when the caller asked for it explicitly, mode 2: an automatic filter takes the direct form when it decimates - faster here)
    const bool want_fft = fir->fft_arith && fir->mode_req == 2 && ds && FirStage::decfft_supported((unsigned)ds->factor, fir->M, fir->S);
    // overlap-save arithmetic the caller pinned (mode 2) stays; an automatic filter (mode 3) that gets a rotator or a downsampler
    // fused takes the direct form, and then also the discriminator epilogue
    const bool fft_pinned = fir->fft_arith && !(fir->mode_req == 3 && (rot || ds));
    FmDiscrimStage *dsc_after = (!no_disc_fusion && fir->S == 2 && !fir->taps_complex && (!fft_pinned || want_fft)) ? p.at<FmDiscrimStage>(after) : nullptr;
    if (!rot && !ds && !dsc_after) return 0;
    const unsigned D = ds ? (unsigned)ds->factor : 1;
    const std::vector<float> taps = fir->natural_taps();
    const bool want_rot = rot && fir->S == 2;
    const double omega = want_rot ? rot->omega : 0.0;
    std::unique_ptr<FirStage> fused;
    if (want_fft || FirStage::mfma_supported_decim(D) || !rot || (fir->S == 2 && !fir->taps_complex && fir->M + 255 <= DECIM_SPAN_MAX))
        fused.reset(fir_build(taps.data(), (unsigned)fir->M, fir->taps_complex, fir->S == 2, D, want_fft ? 2 : 0, want_rot, omega));
    if (rot && !want_rot) fused.reset();
    bool with_disc = fused && dsc_after && fused->can_post_disc();
    // Round 5 (the receivers OFF the stock shape): the Toeplitz kernel has its discriminator epilogue at decimation 5 / 128 taps only, so
    // an FM receiver at another input rate (Tuner /4, /8) ran its tuner, the discriminator and their fix-ups as separate launches.  The polyphase-FFT
    // decimator has the epilogue at every decimation it supports: an AUTOMATIC filter (use_fft nil / "auto": the caller left the arithmetic to the
    // library) that would otherwise lose the epilogue takes that form - tuner + discriminator stay one launch.  Pinned direct-form filters
    // (use_fft = false), exact chains and unsupported decimations keep what they had.
    // Measured on 2^26 RF samples, one box (profiles/r05_receiver_shapes.txt): Tuner /4 0.385 -> 0.236 ms (5 -> 2 launches); Tuner /8 0.291 -> 0.367 ms, the
    // polyphase-FFT form with eight branches is the slower tuner there - so decimation 4 only (2 is unmeasured and stays as it was).
    if (!no_auto_decfft && fused && dsc_after && !with_disc && !want_fft && fir->mode_req == 3 && ds && D == 4 && !p.f.exact_rotator && fir->S == 2 && !fir->taps_complex &&
        FirStage::decfft_supported(D, fir->M, fir->S)) {
        std::unique_ptr<FirStage> alt(fir_build(taps.data(), (unsigned)fir->M, fir->taps_complex, true, D, 2, want_rot, omega));
        if (alt && alt->decfft && alt->can_post_disc()) { fused = std::move(alt); with_disc = true; }
    }
    if (!fused || (!rot && !ds && !with_disc)) return 0;      // nothing was fused
    if (p.f.exact_rotator) fused->rel_rot = false;     // block-of-8 staging with the stand-alone rotator's phasors: fused == unfused bit for bit
    if (with_disc && fold_discriminator(fused.get(), false, dsc_after)) return -1;
    // ... [complex -> real element-wise block] behind an LDS-staged decimator (decimations without a Toeplitz instantiation: the AM / SSB / NBFM
    // receivers' Tuner(…, 50)): ComplexMagnitude / ComplexPhase / ComplexToReal / ComplexToImag run on the accumulators, one launch less and the
    // ComplexFloat32 tuner output never reaches HBM; the same Float32 operation on the same Float32 filter outputs = the unfused bits
    UnaryStage *un = (!no_unary_fold && !with_disc) ? p.at<UnaryStage>(after) : nullptr;
    const bool with_unary = un && fused->can_post_unary() && (un->op == UN_CMAG || un->op == UN_CPHASE || un->op == UN_CREAL || un->op == UN_CIMAG);
    if (with_unary) { fused->post_unary = 1 + un->op; fused->out_size = 4; }
    p.add(std::move(fused));
    return (int)(after + (with_disc || with_unary ? 1 : 0) - i);
}
// fir(Float32 stream, real taps) -> first-order iir: the shape of the two rules below (their iir, or null).  A filter pinned to overlap-save (use_fft 1 / 2)
// keeps it.
static IirStage *fir_iir_pair(const Plan &p, unsigned i)
{
    static const bool no_fir_iir_fusion = getenv("LRHIP_NO_FIR_IIR_FUSION") != nullptr;      // A/B knob
    FirStage *f1 = p.at<FirStage>(i);
    IirStage *ii = f1 ? p.at<IirStage>(i + 1) : nullptr;
    const bool ok = !no_fir_iir_fusion && ii && f1->S == 1 && !f1->taps_complex && f1->D == 1 && !f1->rot && !f1->pre_disc && !f1->post_disc && !f1->use_fft &&
                    (f1->mode_req == 0 || f1->mode_req == 3) && FirWinRealStage::supported_taps(f1->M) && ii->S == 1 && ii->scan && ii->P == 1 && ii->nb <= 2 &&
                    ii->D == 1 && FirWinRealStage::warm_waves_for((double)ii->seq.a[1] / (double)ii->seq.a[0]) > 0;
    return ok ? ii : nullptr;
}
// fir -> first-order iir -> downsampler(2 .. 16).  Only every D-th output of the recurrence is kept, and
//     y[n] = u[n] + p y[n-1]   =>   y[n] = sum_{k<D} p^k u[n-k]  +  p^D y[n-D]           (exact identity, p = -a1/a0)
// so the kept samples are a DECIMATING filter  g = h * b * (1, p, .., p^(D-1))  followed by the first-order recurrence with
// pole p^D at the LOW rate: 1/D of the multiply-adds, and the high-rate audio is never computed.  Same transfer function,
// different rounding: <= 1e-6 of the reference's arithmetic (the bar of the IIR blocks), not bit-identical to it.
static int plan_polyphase_tail(Plan &p, unsigned i)
{
    static const bool no_polyphase_tail = getenv("LRHIP_NO_POLYPHASE_TAIL") != nullptr;      // A/B knob
    IirStage *ii = fir_iir_pair(p, i);
    DownsamplerStage *ds = ii ? p.at<DownsamplerStage>(i + 2) : nullptr;
    if (no_polyphase_tail || p.f.own_arith || !ds || ds->factor < 2 || ds->factor > 16) return 0;
    const FirStage *f1 = p.at<FirStage>(i);
    const std::vector<float> taps = f1->natural_taps();
    const int D = (int)ds->factor, nbb = ii->nb;
    const double a0 = (double)ii->seq.a[0];
    const double pp = -(double)(float)((double)ii->seq.a[1] / a0);      // the pole as the IIR kernels round it (IirCoeffs)
    std::vector<double> cpoly((size_t)(nbb + D - 1), 0.0);
    double pk = 1.0;
    for (int k = 0; k < D; k++, pk *= pp)
        for (int jb = 0; jb < nbb; jb++) cpoly[(size_t)(k + jb)] += pk * (double)(float)((double)ii->seq.b[jb] / a0);
    const int Mg0 = f1->M + nbb + D - 2, Mg = (Mg0 + 3) & ~3;            // zero taps at the far end: a multiple of four for the window kernel
    std::vector<float> g((size_t)Mg, 0.f);
    for (int t = 0; t < Mg0; t++) {
        double acc = 0.0;
        for (int c2 = 0; c2 < (int)cpoly.size(); c2++)
            if (t - c2 >= 0 && t - c2 < f1->M) acc += (double)taps[(size_t)(t - c2)] * cpoly[(size_t)c2];
        g[(size_t)t] = (float)acc;
    }
    std::unique_ptr<FirStage> fd(fir_build(g.data(), (unsigned)Mg, 0, 0, (unsigned)D, 0, false, 0.0));
    if (!fd) return 0;
    // the low-rate recurrence runs on the filter's accumulators when the window kernel takes this shape ...
    if (fd->fuse_iir1(1.0, pk) == 0) { p.add(std::move(fd)); return 3; }
    // ... and as its own launch otherwise - if the pole p^D survives rounding to ONE Float32: that moves the DC gain by
    // 2^-24 q / (1 - q), held below 3e-7 here (the fused form above carries the pole as a Float32 pair instead)
    const bool pole_ok = std::fabs(pk) * 5.96e-8 <= 3e-7 * (1.0 - std::fabs(pk));
    const float b2[1] = {1.0f}, a2[2] = {1.0f, (float)(-pk)};          // pk = p^D after the loop
    std::unique_ptr<lrhip_stage> i2(pole_ok ? lrhip_iir_create(b2, 1, a2, 2, 0) : nullptr);
    if (!i2) return 0;
    p.add(std::move(fd)); p.add(std::move(i2));
    return 3;
}
// fir -> first-order iir -> [downsampler] without the polyphase tail: the recurrence can run on the accumulators of the D = 1 window kernel (kernels_firwin.h),
// one launch, but slower on MI355X than overlap-save filter + scan (0.068 against 0.060 ms on the WBFM audio tail) - opt-in, LRHIP_FIR_IIR_WIN=1
static int plan_fir_iir_win(Plan &p, unsigned i)
{
    static const bool fir_iir_win = getenv("LRHIP_FIR_IIR_WIN") != nullptr;
    IirStage *ii = fir_iir_win ? fir_iir_pair(p, i) : nullptr;
    if (!ii) return 0;
    DownsamplerStage *ds = p.at<DownsamplerStage>(i + 2);
    const FirStage *f1 = p.at<FirStage>(i);
    std::unique_ptr<FirWinRealStage> fw(firwin_real_build(f1->natural_taps().data(), f1->M, ii->seq.b, ii->nb, ii->seq.a, ii->na, ds ? ds->factor : 1));
    if (!fw) return 0;
    p.add(std::move(fw));
    return ds ? 3 : 2;
}
// discriminator -> overlap-save FIR on the real stream: the discriminator runs in the FFT kernel's load stage
static int plan_disc_fir(Plan &p, unsigned i)
{
    static const bool no_disc_fusion = getenv("LRHIP_NO_DISC_FUSION") != nullptr;      // A/B knob
    FmDiscrimStage *dsc = p.at<FmDiscrimStage>(i);
    FirStage *f1 = dsc ? p.at<FirStage>(i + 1) : nullptr;
    if (no_disc_fusion || !f1 || !f1->fft_arith || f1->M > FirStage::FFT_PART || f1->use_fft || f1->S != 1 || f1->D != 1 || f1->rot || f1->pre_disc) return 0;
    std::unique_ptr<FirStage> fused(fir_build(f1->natural_taps().data(), (unsigned)f1->M, 0, 0, 1, 2, false, 0.0));
    if (!fused) return 0;
    if (fold_discriminator(fused.get(), true, dsc)) return -1;
    p.add(std::move(fused));
    return 2;
}
// iir (scan path) -> downsampler: the final scan pass stores only the kept samples
static int plan_iir_downsample(Plan &p, unsigned i)
{
    IirStage *iir = p.at<IirStage>(i);
    DownsamplerStage *ds = (iir && iir->scan && iir->D == 1) ? p.at<DownsamplerStage>(i + 1) : nullptr;
    if (!ds || ds->factor <= 1) return 0;
    std::unique_ptr<IirStage> f(static_cast<IirStage *>(lrhip_iir_create(iir->seq.b, (unsigned)iir->nb, iir->seq.a, (unsigned)iir->na, iir->S == 2)));
    if (!f) return 0;
    f->D = ds->factor;
    p.add(std::move(f));
    return 2;
}
// binaryphasecorrector -> complextoreal  ->  one phase corrector whose rotation pass stores the real part only (Float32): the same once-rounded
// component, so exact, in default and EXACT chains alike.  The fused stage takes over the caller's corrector's carried state (window, ring,
// next measurement, rotation, NaN flag), as digital_fuse_tail does.
static int plan_phasecorr_real(Plan &p, unsigned i)
{
    PhaseCorrStage *pc = p.at<PhaseCorrStage>(i);
    UnaryStage *un = pc && !pc->real_out ? p.at<UnaryStage>(i + 1) : nullptr;
    if (!un || un->op != UN_CREAL) return 0;
    std::unique_ptr<PhaseCorrStage> f(new (std::nothrow) PhaseCorrStage());
    if (!f) return set_error("out of memory");
    f->p = pc->p;
    f->real_out = true;
    f->in_size = 8; f->out_size = 4;
    if (f->reset()) return -1;
    LR_HIP(hipMemcpyAsync((PcState *)f->state.in(), pc->state.in(), sizeof(PcState), hipMemcpyDeviceToDevice, ctx().stream));
    LR_HIP(hipMemcpyAsync(f->ring.p, pc->ring.p, (size_t)pc->p.N * sizeof(unsigned long long), hipMemcpyDeviceToDevice, ctx().stream));
    f->off = pc->off;
    p.add(std::move(f));
    return 2;
}
// the rules in the order they are tried at each stage (the first that applies wins: the cascade must see filters before the tuner rule does)
static int (*const kPlanRules[])(Plan &, unsigned) = {plan_fir_cascade, plan_resample, plan_tuner, plan_polyphase_tail, plan_fir_iir_win, plan_disc_fir,
                                                      plan_iir_downsample, plan_phasecorr_real};
// ---- passes over the planned ops ----------------------------------------------------------------------------------------------------------------
// the RX_FMT_* of IQFileSource records a kernel can read in place (u8 / s8 / s16le I/Q), from a caller's format stage; 0: none
static int raw_record_fmt(const lrhip_chain::Op &o)
{
    const FormatStage *fs = o.built() ? nullptr : dynamic_cast<const FormatStage *>(o.stage);
    if (!fs || fs->pack || fs->scalars != 2 || kFormats[fs->fmt].swap) return 0;
    const int cls = kFormats[fs->fmt].cls;
    return cls == 0 ? RX_FMT_U8 : cls == 1 ? RX_FMT_S8 : cls == 3 ? RX_FMT_S16LE : 0;
}
// a Toeplitz tuner + discriminator stage directly in front of the pair-mode window filter hands its wave-boundary fix-up to that filter's
// staging (kernels_firwin2.h FwcParams::fix_edge): the WBFM receiver is then two launches
static void fold_fixups(std::vector<lrhip_chain::Op> &ops)
{
    static const bool no_fixup_fold = getenv("LRHIP_NO_FIXUP_FOLD") != nullptr;      // A/B knob
    for (size_t k = 0; k + 1 < ops.size() && !no_fixup_fold; k++) {
        FirStage *prod = ops[k].built() ? dynamic_cast<FirStage *>(ops[k].stage) : nullptr;
        FirStage *cons = ops[k + 1].built() ? dynamic_cast<FirStage *>(ops[k + 1].stage) : nullptr;
        if (prod && cons && prod->post_disc && prod->form(true) == FirForm::MfmaPersistent && cons->iir_fused && cons->form(true) == FirForm::WinPair) {
            prod->defer_fixup = true;
            cons->fix_src = prod;
        }
    }
}
// ... and the two become ONE stage whose run() is a single launch (kernels_rx.h): the discriminator stream stays in LDS.  The stage keeps
// both FirStages and their state formats, so the two-launch form remains its fallback (and what LRHIP_CHAIN_NO_SINGLE_LAUNCH selects)
static int merge_receivers(std::vector<lrhip_chain::Op> &ops, const PlanFlags &f)
{
    static const bool no_u8_fold = getenv("LRHIP_RX_NO_U8_FOLD") != nullptr;      // A/B knob
    for (size_t k = 0; k + 1 < ops.size(); k++) {
        FirStage *prod = ops[k].built() ? dynamic_cast<FirStage *>(ops[k].stage) : nullptr;
        FirStage *cons = ops[k + 1].built() ? dynamic_cast<FirStage *>(ops[k + 1].stage) : nullptr;
        if (!RxStage::shapes_ok(prod, cons)) continue;
        std::unique_ptr<RxStage> rx(new (std::nothrow) RxStage());
        if (!rx) return set_error("out of memory");
        rx->A.reset(static_cast<FirStage *>(ops[k].own.release()));
        rx->B.reset(static_cast<FirStage *>(ops[k + 1].own.release()));
        rx->single_launch = f.single_launch;
        // IQFileSource's u8 / s8 / s16le records directly in front of it: the receiver reads them itself (2 or 4 bytes per RF sample instead of a
        // conversion pass and an 8-byte read); every other format keeps its conversion launch
        const int raw = (k > 0 && !no_u8_fold) ? raw_record_fmt(ops[k - 1]) : 0;
        if (raw) { rx->in_u8 = true; rx->fmt = ops[k - 1].stage; rx->in_fmt = raw; }
        if (rx->prepare()) return -1;
        ops[k] = lrhip_chain::Op(std::move(rx));
        ops.erase(ops.begin() + (long)k + 1);
        if (raw) { ops.erase(ops.begin() + (long)k - 1); k--; }
    }
    return 0;
}
// ... and the same records in front of a plain fused Tuner or Decimator ([rotator +] 128-tap filter + decimation 5, no discriminator: the branch of a
// fan-out, TunerBlock / DecimatorBlock on its own; or the LDS-staged decimators of the AM / SSB / NBFM receivers, decimation 9 .. 50): folded into the
// kernel's staging (kernels_fir.h FMT)
static void fold_tuner_records(std::vector<lrhip_chain::Op> &ops)
{
    static const bool no_tuner_fold = getenv("LRHIP_TUNER_NO_RAW_FOLD") != nullptr;      // A/B knob
    for (size_t k = 0; k + 1 < ops.size() && !no_tuner_fold; k++) {
        const int raw = raw_record_fmt(ops[k]);
        FirStage *tf = ops[k + 1].built() ? dynamic_cast<FirStage *>(ops[k + 1].stage) : nullptr;
        if (!raw || !tf) continue;
        // (narrower than the stage's own predicate on purpose: a filter that does not decimate is no Tuner / Decimator and keeps its conversion launch)
        if (!fir_raw_records_ok(*tf, fir_knobs()) || tf->D == 1) continue;
        tf->in_fmt = raw;
        tf->fmt_stage = ops[k].stage;
        tf->in_size = ops[k].stage->in_size;
        ops.erase(ops.begin() + (long)k);
    }
}
// clocksampler -> slicer [-> differentialdecoder] becomes ONE clocksampler whose final pass writes the (decoded) bits.  All exact, so in default and EXACT
// chains alike.  The fused stage takes over the carried state of the caller's clocksampler and differential decoder (the slicer has none), so a chain
// built from stages that have already run continues their streams.
static int digital_fuse_tail(std::vector<lrhip_chain::Op> &ops)
{
    for (size_t k = 0; k + 1 < ops.size(); k++) {
        ZcStage *cs = dynamic_cast<ZcStage *>(ops[k].stage);
        SlicerStage *sl = dynamic_cast<SlicerStage *>(ops[k + 1].stage);
        if (!cs || !cs->sampler || cs->tail.out != DG_OUT_FLOAT || !sl) continue;
        DiffDecStage *dd = k + 2 < ops.size() ? dynamic_cast<DiffDecStage *>(ops[k + 2].stage) : nullptr;
        std::unique_ptr<ZcStage> f(new (std::nothrow) ZcStage());
        if (!f) return set_error("out of memory");
        f->p = cs->p;
        f->sampler = true;
        f->tail.out = dd ? DG_OUT_DECODE : DG_OUT_SLICE;
        f->tail.slice_t = sl->t;
        f->tail.invert = dd ? dd->invert : 0;
        f->in_size = 4; f->out_size = 1;
        if (f->reset()) return -1;
        // carried state: the clocksampler's, plus the decoder's previous input bit
        DgState *fs = (DgState *)f->st.in();                 // what the fused stage's first call reads
        LR_HIP(hipMemcpyAsync(fs, cs->st.in(), sizeof(DgState), hipMemcpyDeviceToDevice, ctx().stream));
        if (dd) LR_HIP(hipMemcpyAsync(&fs->bit, dd->state.in(), 1, hipMemcpyDeviceToDevice, ctx().stream));
        if (dd) LR_HIP(hipMemsetAsync((char *)&fs->bit + 1, 0, sizeof(int) - 1, ctx().stream));
        ops.erase(ops.begin() + (long)k + 1, ops.begin() + (long)k + (dd ? 3 : 2));
        ops[k] = lrhip_chain::Op(std::move(f));
    }
    return 0;
}
