// stage_pfbsynth.h - the polyphase + FFT synthesis filterbank (kernels_pfbsynth.h), created through lrhip_unary_create
// ("pfbsynthesizer:channels=K:oversample=R:taps=v,v,...")
// (part of liblrhip.so; included by lrhip.hip after stage_modulator.h, one translation unit)
#pragma once

// Input: the frame stream of PfbChannelizerStage, K ComplexFloat32 values per frame, counted in VALUES; output: D = K / R samples per completed frame.
// Carried: the values of an incomplete frame (`pend`, npend < K of them), the V frames of the last Q - 1 frames (the first Q - 1 rows of `scratch`,
// zero at the start of the stream) and the number of frames emitted so far modulo R, which fixes the column of a frame's first output.
struct PfbSynthesizerStage : lrhip_stage {
    int seek(unsigned long long, unsigned long long *) override { return set_error("seek: not supported by the synthesizer stage"); }
    long memory() const override { return -1; }
    int M = 0, K = 0, log2k = 0, Q = 0, R = 1, D = 0;
    DeviceBuf taps, tw, pend, scratch, moved;        // scratch: [Q - 1 carried V frames | this call's V frames]; moved: Q - 1 frames in transit
    unsigned long npend = 0;
    unsigned phase = 0;                              // frames emitted so far modulo R
    const char *kind() const override { return "pfb_synthesizer"; }
    unsigned long max_output(unsigned long n) const override { return ((n + K - 1) / K) * D; }
    void rate(unsigned long *num, unsigned long *den) const override { *num = (unsigned long)R; *den = 1; }
    // the accepted domain, that of PfbChannelizerStage: K a power of two in [8, 4096], K <= M <= min(64 K, 65536), R in {1, 2, 4}
    static const char *refusal(unsigned ntaps, unsigned nchannels, unsigned oversample)
    {
        if (oversample != 1 && oversample != 2 && oversample != 4) return "pfb_synthesizer: oversample must be 1, 2 or 4";
        if (nchannels < 8 || nchannels > 4096 || (nchannels & (nchannels - 1))) return "pfb_synthesizer: nchannels must be a power of two in [8, 4096]";
        const unsigned hi = 64 * nchannels < 65536 ? 64 * nchannels : 65536;
        if (ntaps < nchannels || ntaps > hi) return "pfb_synthesizer: ntaps must be in [nchannels, min(64 * nchannels, 65536)]";
        return nullptr;
    }
    size_t row_bytes() const { return (size_t)K * sizeof(float2); }
    size_t carried_bytes() const { return (size_t)(Q - 1) * row_bytes(); }
    // tilings by K, the one copy in code of the table in kernels_pfbsynth.h.  The transform: frames per workgroup and per fft_lds group (the R = 1
    // table of the analysis kernel); the sums: frames per register block and per workgroup
    int ifft_tile() const { return K <= 256 ? PFB_TILE_SMALL / K : K == 512 ? 8 : K == 1024 ? 4 : PFB_TILE_LARGE / K; }
    int ifft_group() const { return K <= 1024 ? ifft_tile() : PFB_SCRATCH / K; }
    int sums_block() const { return R == 1 ? 8 : 4; }
    int sums_tile() const { return R * sums_block() * (K >= 512 ? 1 : 512 / K); }
    int reset() override
    {
        npend = 0; phase = 0;
        if (pend.reserve(row_bytes()) || moved.reserve(carried_bytes() ? carried_bytes() : 4)) return -1;
        return zero_fill(scratch, carried_bytes());
    }
    // room for `bytes` of scratch; the carried rows at its front survive a move to a larger allocation
    int reserve_scratch(size_t bytes)
    {
        if (bytes <= scratch.cap) return 0;
        DeviceBuf grown;
        if (grown.reserve(bytes)) return -1;
        if (carried_bytes()) LR_HIP(hipMemcpyAsync(grown.p, scratch.p, carried_bytes(), hipMemcpyDeviceToDevice, ctx().stream));
        LR_HIP(hipStreamSynchronize(ctx().stream));          // the old allocation may still be in use by queued kernels
        std::swap(grown.p, scratch.p);
        std::swap(grown.cap, scratch.cap);
        return 0;
    }
    template <int NT>
    int launch_ifft(const float2 *x, long nframes)
    {
        const int T = ifft_tile(), G = ifft_group();
        size_t lds_bytes = ((size_t)(T + G) * K + K / 2) * sizeof(float2);
        auto kern = pfb_synth_ifft_kernel<NT>;
        if (kernel_allow_lds(kern, lds_bytes)) return -1;
        unsigned grid = (unsigned)((nframes + T - 1) / T);
        hipLaunchKernelGGL(kern, dim3(grid), dim3(NT), lds_bytes, ctx().stream, (const float2 *)pend.p, x, (const float2 *)tw.p,
                           (float2 *)scratch.p + (size_t)(Q - 1) * K, log2k, T, G, (long)npend, nframes);
        LR_LAUNCH_CHECK();
        return 0;
    }
    template <int RR, int F>
    int launch_sums(float2 *y, long nframes)
    {
        const int TS = sums_tile();
        unsigned grid = (unsigned)((nframes + TS - 1) / TS);
        hipLaunchKernelGGL((pfb_synth_sums_kernel<RR, F>), dim3(grid), dim3(256), 0, ctx().stream, (const float2 *)scratch.p, (const float *)taps.p, y,
                           M, log2k, Q, TS, nframes, (int)phase);
        LR_LAUNCH_CHECK();
        return 0;
    }
    int copy_rows(const void *src, void *dst)
    {
        const long n4 = (long)(carried_bytes() / sizeof(float4));
        hipLaunchKernelGGL(pfb_synth_copy_kernel, dim3(grid_for((unsigned long)n4, 256)), dim3(256), 0, ctx().stream, (const float4 *)src, (float4 *)dst, n4);
        LR_LAUNCH_CHECK();
        return 0;
    }
    long run(const void *in_dev, unsigned long n_in, void *out_dev, unsigned long cap) override
    {
        if (!n_in) return 0;
        const unsigned long total = npend + n_in;
        const long nframes = (long)(total / (unsigned long)K);
        const unsigned long n_out = (unsigned long)nframes * D;
        if (n_out > cap) return set_error("pfb_synthesizer: output capacity %lu < %lu", cap, n_out);
        const float2 *x = (const float2 *)in_dev;
        if (nframes > 0) {
            if (reserve_scratch((size_t)(Q - 1 + nframes) * row_bytes())) return -1;
            int rc = K <= 256 ? launch_ifft<256>(x, nframes) : K == 1024 ? launch_ifft<512>(x, nframes) : launch_ifft<1024>(x, nframes);
            if (rc) return rc;
            float2 *y = (float2 *)out_dev;
            rc = R == 1 ? launch_sums<1, 8>(y, nframes) : R == 2 ? launch_sums<2, 4>(y, nframes) : launch_sums<4, 4>(y, nframes);
            if (rc) return rc;
            // the last Q - 1 rows move to the front; where they overlap their new place (fewer than Q - 1 new frames) they go through `moved`
            if (Q > 1) {
                const char *tail = (const char *)scratch.p + (size_t)nframes * row_bytes();
                if (nframes >= Q - 1) {
                    if (copy_rows(tail, scratch.p)) return -1;
                } else if (copy_rows(tail, moved.p) || copy_rows(moved.p, scratch.p)) return -1;
            }
        }
        // what is left of the stream after the completed frames: all of it from x once a frame was completed, appended to the pending values otherwise
        const unsigned long left = total - (unsigned long)nframes * K;
        const int start = nframes > 0 ? 0 : (int)npend;
        if ((int)left > start) {
            hipLaunchKernelGGL(pfb_synth_pending_kernel, dim3(grid_for(left - start, 256)), dim3(256), 0, ctx().stream, x, (float2 *)pend.p,
                               (long)((unsigned long)nframes * K) - (long)npend, start, (int)left);
            LR_LAUNCH_CHECK();
        }
        npend = left;
        phase = (unsigned)((phase + nframes) % R);
        return (long)n_out;
    }
};

static PfbSynthesizerStage *pfb_synthesizer_build(const std::vector<float> &g, unsigned nchannels, unsigned oversample)
{
    auto q = new_stage<PfbSynthesizerStage>();
    if (!q) return nullptr;
    const int M = (int)g.size(), K = (int)nchannels;
    q->M = M; q->K = K; q->R = (int)oversample; q->D = K / q->R;
    q->Q = (M + q->D - 1) / q->D;
    while ((1 << q->log2k) < K) q->log2k++;
    q->in_size = q->out_size = 8;
    std::vector<float> tw((size_t)K);      // W_K^m = exp(-2 pi i m / K), m < K / 2 (kernels_fft.h), computed in double
    for (int m = 0; m < K / 2; m++) {
        double ang = -2.0 * 3.14159265358979323846 * m / K;
        tw[2 * m] = (float)std::cos(ang);
        tw[2 * m + 1] = (float)std::sin(ang);
    }
    if (upload(q->taps, g.data(), (size_t)M * sizeof(float)) || upload(q->tw, tw.data(), tw.size() * sizeof(float))) return nullptr;
    if (q->reset()) return nullptr;
    return q.release();
}

// "pfbsynthesizer:channels=K:oversample=R:taps=v,v,...": K, R integers; the taps Float32 values as decimal (%.9g) or hexadecimal floating-point
// text, each read with strtod and rounded to Float32 (the modulators' table convention, stage_modulator.h).  The domain is refused before the device
// is looked at.
static lrhip_stage_t *pfb_synthesizer_create(const char *op)
{
    OpFields f;
    long K = 0, R = 0;
    std::vector<float> g;
    // (a list of more than 65536 taps is refused below by its count: no need to read on)
    if (!f.split(op, "pfb_synthesizer", {{"channels", nullptr}, {"oversample", nullptr}, {"taps", nullptr}}, false) || !f.integer("channels", 0, 1000000, K) ||
        !f.integer("oversample", 0, 1000000, R) || !f.floats("taps", g, 65536, "tap", " (a number)", "the taps end")) return nullptr;
    if (const char *why = PfbSynthesizerStage::refusal((unsigned)g.size(), (unsigned)K, (unsigned)R)) { set_error("%s (got %zu taps, %ld channels)", why, g.size(), K); return nullptr; }
    return pfb_synthesizer_build(g, (unsigned)K, (unsigned)R);
}
