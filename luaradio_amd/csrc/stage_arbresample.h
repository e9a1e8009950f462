// stage_arbresample.h - the arbitrary-ratio resampler (kernels_arbresample.h, arbresample_plan.h), created through lrhip_unary_create
// ("arbresampler:type=cf32|f32:phases=P:step=<decimal uint64>:taps=<P*T Float32 values>")
// (part of liblrhip.so; included by lrhip.hip after stage_source.h, one translation unit)
#pragma once

// Carried: the T - 1 input samples in front of the next call (ping-pong, written by the kernel), the absolute counts Q0 of inputs consumed and m0 of
// outputs emitted.  Output m is emitted as soon as input i(m) has arrived: after Q inputs ceil(Q * 2^48 / step) outputs exist, a call returns the
// difference to m0 - from the lengths alone, nothing is read back - and may return 0.
struct ArbResampleStage : lrhip_stage {
    int S = 2, P = 0, log2p = 0, T = 0;
    uint64_t step = arbplan::ONE;
    TwoSlots hist;                    // the T - 1 input samples in front of the next call
    DeviceBuf d_tab;                  // d_tab: {G[p][k], D[p][k]} pairs at a row stride of T + 1 pairs, as the kernel keeps them in LDS
    uint64_t Q0 = 0, m0 = 0;
    const char *kind() const override { return "arbresampler"; }
    unsigned long max_output(unsigned long n) const override { return (unsigned long)arbplan::max_output(n, step); }
    long memory() const override { return T - 1; }
    // input samples per output sample, step / 2^48 in lowest terms
    void rate(unsigned long *num, unsigned long *den) const override
    {
        const int z = __builtin_ctzll(step | arbplan::ONE);
        *num = (unsigned long)(step >> z);
        *den = (unsigned long)(arbplan::ONE >> z);
    }
    int reset() override
    {
        Q0 = 0; m0 = 0;
        return hist.reset((size_t)(T - 1) * S * sizeof(float));
    }
    int seek(unsigned long long n0, unsigned long long *n0_out) override
    {
        const arbplan::Count c = arbplan::seek_output(n0, step);
        if (c.hi) return set_error("arbresampler: seek to input %llu lies behind output 2^64", n0);
        if (reset()) return -1;
        Q0 = n0;
        m0 = c.lo;
        *n0_out = m0;
        return 0;
    }
    long run(const void *in_dev, unsigned long n, void *out_dev, unsigned long cap) override
    {
        if (!n) return 0;
        if (Q0 + n < Q0) return set_error("arbresampler: more than 2^64 input samples");
        const arbplan::Count c = arbplan::output_count(Q0 + n, step);
        if (c.hi || c.lo - m0 > (uint64_t)LONG_MAX) return set_error("arbresampler: more than 2^64 output samples");
        const long n_out = (long)(c.lo - m0);
        if ((unsigned long)n_out > cap) return set_error("arbresampler: output capacity %lu < %ld", cap, n_out);
        if (!in_dev) return set_error("arbresampler: null input buffer");
        if (n_out && !out_dev) return set_error("arbresampler: null output buffer");
        const size_t lds_bytes = arb_lds_bytes(P, T, step, S);
        auto go = [&](auto kern) -> int {
            const long ntiles = (n_out + ARB_TILE - 1) / ARB_TILE, slots = chip_slots(kern, ARB_NT, lds_bytes);
            if (slots < 0) return -1;
            const unsigned grid = persistent_grid(ntiles, slots, 0);           // a workgroup stages the tables once and strides through the tiles
            hipLaunchKernelGGL(kern, dim3(grid ? grid : 1), dim3(ARB_NT), lds_bytes, ctx().stream, hist.in<float>(), (const float *)in_dev,
                               (const float2 *)d_tab.p, (float *)out_dev, T, log2p, step, (long)n, n_out, m0, Q0, arb_span_cap(step, T),
                               (int)(((uintptr_t)out_dev & 7) == 0), hist.out<float>());
            return 0;
        };
        const int rc = S == 2 ? go(arb_resample_kernel<2>) : go(arb_resample_kernel<1>);
        if (rc) return rc;
        LR_LAUNCH_CHECK();
        hist.flip();
        Q0 += n;
        m0 = c.lo;
        return n_out;
    }
};

// The checks need no device and run in front of it.  The stage derives G and D from the prototype h itself: G[p][k] = h[k P + p], row P = row 0 one
// tap later (G[P][k] = G[0][k + 1], G[P][T - 1] = 0), D[p][k] = fl32(G[p + 1][k] - G[p][k]).
static lrhip_stage_t *arbresampler_create(const char *op)
{
    OpFields f;
    long P = 0;
    uint64_t step = 0;
    std::vector<float> h;
    if (!f.split(op, "arbresampler", {{"type", nullptr}, {"phases", nullptr}, {"step", nullptr}, {"taps", nullptr}}, false)) return nullptr;
    const int type = f.word("type", {"cf32", "f32"}, "arbresampler: unsupported type \"", "\" (cf32 or f32)");
    if (type < 0) return nullptr;
    // (a list of more than 8192 taps is refused below by its count: no need to read on)
    if (!f.integer("phases", 0, 1000000, P) || !f.u64("step", step) || !f.floats("taps", h, arbplan::TABLE_MAX, "tap", " (a number)", "the taps end")) return nullptr;
    if (step < arbplan::STEP_MIN || step > arbplan::STEP_MAX) {
        set_error("arbresampler: step must be in [2^44, 2^52] (a ratio of 16 .. 1/16), got %llu", (unsigned long long)step);
        return nullptr;
    }
    if (P < (1 << arbplan::LOG2P_MIN) || P > (1 << arbplan::LOG2P_MAX) || (P & (P - 1))) { set_error("arbresampler: phases must be a power of two in [16, 256], got %ld", P); return nullptr; }
    if (h.size() > (size_t)arbplan::TABLE_MAX) { set_error("arbresampler: phases * taps per phase must not exceed 8192 (got more than 8192 taps): use fewer phases"); return nullptr; }
    if (h.empty() || h.size() % (size_t)P) { set_error("arbresampler: the number of taps must be a multiple of phases (got %zu taps, %ld phases)", h.size(), P); return nullptr; }
    const long T = (long)(h.size() / (size_t)P);
    if (T < arbplan::T_MIN || T > arbplan::T_MAX) { set_error("arbresampler: taps per phase must be in [4, 512], got %ld", T); return nullptr; }
    auto q = new_stage<ArbResampleStage>();
    if (!q) return nullptr;
    q->S = type == 0 ? 2 : 1;
    q->in_size = q->out_size = 4 * q->S;
    q->P = (int)P; q->T = (int)T; q->step = step;
    while ((1 << q->log2p) < P) q->log2p++;
    auto G = [&](long p, long k) -> float { return p < P ? h[(size_t)(k * P + p)] : k + 1 < T ? h[(size_t)((k + 1) * P)] : 0.f; };
    std::vector<float> tab((size_t)2 * P * (T + 1), 0.f);
    for (long p = 0; p < P; p++)
        for (long k = 0; k < T; k++) {
            const float g = G(p, k), d = G(p + 1, k) - g;
            tab[(size_t)2 * (p * (T + 1) + k)] = g;
            tab[(size_t)2 * (p * (T + 1) + k) + 1] = d;
        }
    if (upload(q->d_tab, tab.data(), tab.size() * sizeof(float)) || q->reset()) return nullptr;
    return q.release();
}
