// stage_pfb.h - the polyphase + FFT channelizer (kernels_pfb.h)
// (part of liblrhip.so; included by lrhip.hip in this order, one translation unit)
#pragma once

// Same block, same emission rule and same carried state as ChannelizerStage (stage_resample.h): a frame as soon as sample mK has arrived,
// `index` = position of the next frame's newest sample inside the next call, the last M - 1 samples in a ping-pong history.
// Oversampled by R (lrhip_pfb_oversampled_create): the hop is D = K / R, a frame as soon as sample mD has arrived, and the number of frames emitted so
// far modulo R is carried too - it is the class of the next frame, which fixes its rotation (kernels_pfb.h).  R = 1 is the critically sampled stage.
struct PfbChannelizerStage : lrhip_stage {
    int seek(unsigned long long, unsigned long long *) override { return set_error("seek: not supported by the channelizer stage"); }
    long memory() const override { return -1; }
    int M = 0, K = 0, log2k = 0, P = 0, R = 1, D = 0;
    DeviceBuf taps, tw;
    TwoSlots hist;                   // the last M - 1 input samples
    unsigned long index = 0;
    unsigned phase = 0;              // frames emitted so far modulo R
    const char *kind() const override { return "pfb_channelizer"; }
    unsigned long max_output(unsigned long n) const override { return (n / D + 1) * K; }
    // the accepted domain (lrhip_pfb_channelizer_create): K a power of two in [8, 4096], K <= M <= min(64 K, 65536)
    static const char *refusal(unsigned ntaps, unsigned nchannels)
    {
        if (nchannels < 8 || nchannels > 4096 || (nchannels & (nchannels - 1))) return "pfb_channelizer: nchannels must be a power of two in [8, 4096]";
        const unsigned hi = 64 * nchannels < 65536 ? 64 * nchannels : 65536;
        if (ntaps < nchannels || ntaps > hi) return "pfb_channelizer: ntaps must be in [nchannels, min(64 * nchannels, 65536)]";
        return nullptr;
    }
    static const char *refusal(unsigned ntaps, unsigned nchannels, unsigned oversample)
    {
        if (oversample != 1 && oversample != 2 && oversample != 4) return "pfb_channelizer: oversample must be 1, 2 or 4";
        return refusal(ntaps, nchannels);
    }
    // tilings by K (kernels_pfb.h): frames per workgroup, frames per fft_lds group
    int frames_per_tile() const { return K <= 256 ? PFB_TILE_SMALL / K : K == 512 ? 8 : K == 1024 ? 4 : PFB_TILE_LARGE / K; }
    int frames_per_group() const { return K <= 1024 ? frames_per_tile() : PFB_SCRATCH / K; }
    int reset() override
    {
        index = 0; phase = 0;
        return hist.reset((size_t)(M - 1) * 2 * sizeof(float));
    }
    template <int F, int NT>
    int launch(const float *x, long n, float *y, long nframes)
    {
        const int T = frames_per_tile(), G = frames_per_group();
        size_t lds_bytes = ((size_t)(T + G) * K + K / 2) * sizeof(float2);
        auto kern = pfb_channelizer_kernel<F, NT>;
        if (kernel_allow_lds(kern, lds_bytes)) return -1;
        unsigned grid = (unsigned)((nframes + T - 1) / T);
        hipLaunchKernelGGL(kern, dim3(grid), dim3(NT), lds_bytes, ctx().stream, hist.in<float>(), x, (const float *)taps.p,
                           (const float2 *)tw.p, y, M, log2k, P, T, G, n, nframes, (long)index);
        LR_LAUNCH_CHECK();
        return 0;
    }
    template <int RR, int F, int NT>
    int launch_oversampled(int T, int G, const float *x, long n, float *y, long nframes)
    {
        if (F > 1 && T % (RR * F)) return set_error("pfb_channelizer: a tile of %d frames does not hold blocks of %d frames in %d classes", T, F, RR);
        size_t lds_bytes = ((size_t)(T + G) * K + K / 2) * sizeof(float2);
        auto kern = pfb_oversampled_kernel<RR, F, NT>;
        if (kernel_allow_lds(kern, lds_bytes)) return -1;
        unsigned grid = (unsigned)((nframes + T - 1) / T);
        hipLaunchKernelGGL(kern, dim3(grid), dim3(NT), lds_bytes, ctx().stream, hist.in<float>(), x, (const float *)taps.p,
                           (const float2 *)tw.p, y, M, log2k, P, T, G, n, nframes, (long)index, (int)phase);
        LR_LAUNCH_CHECK();
        return 0;
    }
    // the oversampled tilings, the one copy in code of the table in kernels_pfb.h: <R, F, threads>(T, G)
    int launch_oversampled_by_k(const float *x, long n, float *y, long nframes)
    {
        const int Ts = PFB_TILE_SMALL / K;
        if (R == 2) switch (log2k) {
            case 7: return launch_oversampled<2, 8, 256>(16, 16, x, n, y, nframes);
            case 8: return launch_oversampled<2, 4, 256>(8, 8, x, n, y, nframes);
            case 9: return launch_oversampled<2, 4, 1024>(8, 8, x, n, y, nframes);
            case 10: return launch_oversampled<2, 2, 512>(4, 4, x, n, y, nframes);
            case 11: return launch_oversampled<2, 4, 1024>(8, 1, x, n, y, nframes);
            case 12: return launch_oversampled<2, 1, 1024>(2, 1, x, n, y, nframes);
            default: return launch_oversampled<2, 8, 256>(Ts, Ts, x, n, y, nframes);          // K <= 64
        }
        switch (log2k) {
            case 7: return launch_oversampled<4, 4, 256>(16, 16, x, n, y, nframes);
            case 8: return launch_oversampled<4, 2, 256>(8, 8, x, n, y, nframes);
            case 9: return launch_oversampled<4, 4, 1024>(16, 4, x, n, y, nframes);
            case 10: return launch_oversampled<4, 2, 512>(8, 1, x, n, y, nframes);
            case 11: return launch_oversampled<4, 2, 1024>(8, 1, x, n, y, nframes);
            case 12: return launch_oversampled<4, 1, 1024>(2, 1, x, n, y, nframes);
            default: return launch_oversampled<4, 8, 256>(Ts, Ts, x, n, y, nframes);          // K <= 64
        }
    }
    long run(const void *in_dev, unsigned long n_in, void *out_dev, unsigned long cap) override
    {
        long n = (long)n_in;
        if (n <= 0) return 0;
        long nframes = n_in > index ? (long)((n_in - index + D - 1) / D) : 0;
        if ((unsigned long)(nframes * K) > cap) return set_error("pfb_channelizer: output capacity %lu < %ld", cap, nframes * K);
        const float *x = (const float *)in_dev;
        if (nframes > 0) {
            // frames per register block and threads per workgroup (kernels_pfb.h)
            float *y = (float *)out_dev;
            int rc = R > 1 ? launch_oversampled_by_k(x, n, y, nframes)
                   : K <= 256 ? launch<8, 256>(x, n, y, nframes) : K == 512 ? launch<8, 1024>(x, n, y, nframes) : K == 1024 ? launch<4, 512>(x, n, y, nframes)
                   : K == 2048 ? launch<4, 1024>(x, n, y, nframes) : launch<2, 1024>(x, n, y, nframes);
            if (rc) return rc;
        }
        unsigned grid = grid_for((unsigned long)(M - 1) * 2, 256);
        hipLaunchKernelGGL(fir_history_kernel<2>, dim3(grid), dim3(256), 0, ctx().stream, hist.in<float>(), x, hist.out<float>(), M, n);
        LR_LAUNCH_CHECK();
        hist.flip();
        index = index + (unsigned long)nframes * D - n_in;
        phase = (unsigned)((phase + nframes) % R);
        return nframes * K;
    }
};

// The matrix-core channelizer behind lrhip_channelizer_create (ChannelizerStage, stage_resample.h), which has checked the shape: its W operand
static ChannelizerStage *channelizer_build(const float *taps, unsigned ntaps, unsigned nchannels)
{
    auto q = new_stage<ChannelizerStage>();
    if (!q) return nullptr;
    int M = (int)ntaps, K = (int)nchannels, K2 = 2 * K;
    q->M = M; q->K = K;
    q->in_size = q->out_size = 8;
    // W[2i][2c] = Re g, W[2i+1][2c] = -Im g, W[2i][2c+1] = Im g, W[2i+1][2c+1] = Re g,
    // g_c[i] = h[M-1-i] * exp(+j*2*pi*c*(M-1-i)/K)   (kernels_channelizer.h)
    std::vector<float> W((size_t)2 * M * K2);
    const double PI2 = 6.283185307179586476925286766559;
    for (int i = 0; i < M; i++)
        for (int c = 0; c < K; c++) {
            int j = M - 1 - i;
            double a = PI2 * (double)(((long)c * j) % K) / K, h = taps[j];
            float gr = (float)(h * std::cos(a)), gi = (float)(h * std::sin(a));
            W[(size_t)(2 * i) * K2 + 2 * c] = gr;
            W[(size_t)(2 * i + 1) * K2 + 2 * c] = -gi;
            W[(size_t)(2 * i) * K2 + 2 * c + 1] = gi;
            W[(size_t)(2 * i + 1) * K2 + 2 * c + 1] = gr;
        }
    if (upload(q->W, W.data(), W.size() * sizeof(float))) return nullptr;
    if (q->reset()) return nullptr;
    return q.release();
}
