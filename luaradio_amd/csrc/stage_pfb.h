// stage_pfb.h - the polyphase + FFT channelizer (kernels_pfb.h)
// (part of liblrhip.so; included by lrhip.hip in this order, one translation unit)
#pragma once

// Same block, same emission rule and same carried state as ChannelizerStage (stage_resample.h): a frame as soon as sample mK has arrived,
// `index` = position of the next frame's newest sample inside the next call, the last M - 1 samples in a ping-pong history.
struct PfbChannelizerStage : lrhip_stage {
    int seek(unsigned long long, unsigned long long *) override { return set_error("seek: not supported by the channelizer stage"); }
    long memory() const override { return -1; }
    int M = 0, K = 0, log2k = 0, P = 0;
    DeviceBuf taps, tw, hist[2];
    int cur = 0;
    unsigned long index = 0;
    const char *kind() const override { return "pfb_channelizer"; }
    unsigned long max_output(unsigned long n) const override { return (n / K + 1) * K; }
    // the accepted domain (lrhip_pfb_channelizer_create): K a power of two in [8, 4096], K <= M <= min(64 K, 65536)
    static const char *refusal(unsigned ntaps, unsigned nchannels)
    {
        if (nchannels < 8 || nchannels > 4096 || (nchannels & (nchannels - 1))) return "pfb_channelizer: nchannels must be a power of two in [8, 4096]";
        const unsigned hi = 64 * nchannels < 65536 ? 64 * nchannels : 65536;
        if (ntaps < nchannels || ntaps > hi) return "pfb_channelizer: ntaps must be in [nchannels, min(64 * nchannels, 65536)]";
        return nullptr;
    }
    // tilings by K (kernels_pfb.h): frames per workgroup, frames per fft_lds group
    int frames_per_tile() const { return K <= 256 ? PFB_TILE_SMALL / K : K == 512 ? 8 : K == 1024 ? 4 : PFB_TILE_LARGE / K; }
    int frames_per_group() const { return K <= 1024 ? frames_per_tile() : PFB_SCRATCH / K; }
    int reset() override
    {
        cur = 0; index = 0;
        size_t hb = (size_t)(M - 1) * 2 * sizeof(float);
        return (zero_fill(hist[0], hb) || zero_fill(hist[1], hb)) ? -1 : 0;
    }
    template <int F, int NT>
    int launch(const float *x, long n, float *y, long nframes)
    {
        const int T = frames_per_tile(), G = frames_per_group();
        size_t lds_bytes = ((size_t)(T + G) * K + K / 2) * sizeof(float2);
        auto kern = pfb_channelizer_kernel<F, NT>;
        if (lds_bytes > 48 * 1024) LR_HIP(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
        unsigned grid = (unsigned)((nframes + T - 1) / T);
        hipLaunchKernelGGL(kern, dim3(grid), dim3(NT), lds_bytes, ctx().stream, (const float *)hist[cur].p, x, (const float *)taps.p,
                           (const float2 *)tw.p, y, M, log2k, P, T, G, n, nframes, (long)index);
        LR_LAUNCH_CHECK();
        return 0;
    }
    long run(const void *in_dev, unsigned long n_in, void *out_dev, unsigned long cap) override
    {
        long n = (long)n_in;
        if (n <= 0) return 0;
        long nframes = n_in > index ? (long)((n_in - index + K - 1) / K) : 0;
        if ((unsigned long)(nframes * K) > cap) return set_error("pfb_channelizer: output capacity %lu < %ld", cap, nframes * K);
        const float *x = (const float *)in_dev;
        if (nframes > 0) {
            // frames per register block and threads per workgroup (kernels_pfb.h)
            float *y = (float *)out_dev;
            int rc = K <= 256 ? launch<8, 256>(x, n, y, nframes) : K == 512 ? launch<8, 1024>(x, n, y, nframes) : K == 1024 ? launch<4, 512>(x, n, y, nframes)
                   : K == 2048 ? launch<4, 1024>(x, n, y, nframes) : launch<2, 1024>(x, n, y, nframes);
            if (rc) return rc;
        }
        unsigned grid = grid_for((unsigned long)(M - 1) * 2, 256);
        hipLaunchKernelGGL(fir_history_kernel<2>, dim3(grid), dim3(256), 0, ctx().stream, (const float *)hist[cur].p, x, (float *)hist[cur ^ 1].p, M, n);
        LR_LAUNCH_CHECK();
        cur ^= 1;
        index = index + (unsigned long)nframes * K - n_in;
        return nframes * K;
    }
};
