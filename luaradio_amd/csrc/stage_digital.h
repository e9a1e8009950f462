// stage_digital.h - ZeroCrossingClockRecoveryBlock, SamplerBlock, SlicerBlock, DifferentialDecoderBlock and the fused "clocksampler"
// (kernels_digital.h).  The sampler and the clocksampler are the first stages whose output count depends on the data: run() / run2() return the
// exact count, read back from the device after the final pass (one small synchronous copy per call).
// (part of liblrhip.so; included by lrhip.hip after stage_elem2.h, one translation unit)
#pragma once

// The clock recovery's closed form (kernels_digital.h) for symbol period P: decided here, and only where it is proven.
//   P >= 2, 2^e <= P < 2^(e+1) with P + 1 <= 2^(e+1), and P < 2^40.
//   From each kind of reset the literal loop runs (exactly: an offset >= 1 loses integers without rounding) to its first pulse ks, whose add gives
//   o1 = fl(o' + P), o' in [0, 1).  If o1 < P + 1 then o1 = A ulp(P) with r0 = A - Pi in [0, U), and by induction every later offset after
//   an add is Pi + r (r in [0, U)) units of ulp(P): the integer part goes in exact "- 1" steps, the fraction o' in [0, 1) is a multiple of ulp(P),
//   and o' + P < P + 1 <= 2^(e+1) stays on P's grid - no rounding ever again.  The j-th later pulse is at ks + floor((j Pi + r0) / U), i.e.
//   sample k >= ks pulses iff ((k - ks + 1) U - r0 - 1) mod Pi < U.
static void zc_prepare(double P, double T, ZcParams &p)
{
    memset(&p, 0, sizeof(p));
    p.P = P; p.T = T;
    if (!(P >= 2.0) || !(P < 1099511627776.0)) return;
    int ex = 0;
    (void)frexp(P, &ex);
    const int e = ex - 1;
    if (P + 1.0 > ldexp(1.0, e + 1)) return;
    const double u = ldexp(1.0, e - 52);
    const unsigned long long U = 1ull << (52 - e), Pi = (unsigned long long)(P / u);
    for (int kind = 0; kind < 2; kind++) {
        double o = kind ? P * 0.5 : P;
        long long k = 0;
        while (o >= 2.0) { const double s = floor(o) - 1.0; o -= s; k += (long long)s; }
        o = o - 1.0;                                          // o was in [1, 2): this sample pulses
        const double o1 = o + P;
        if (!(o >= 0.0) || !(o1 < P + 1.0)) return;
        const unsigned long long A = (unsigned long long)(o1 / u);
        if ((double)A * u != o1 || A < Pi || A - Pi >= U) return;
        const long long r0 = (long long)(A - Pi);
        __int128 c = (__int128)(1 - k) * (__int128)U - r0 - 1;
        c %= (__int128)Pi;
        if (c < 0) c += (__int128)Pi;
        p.ks[kind] = k;
        p.c0[kind] = (unsigned long long)c;
    }
    p.U = U; p.Pi = Pi;
    p.closed = 1;
}

static DgState dg_state_init(double P = 0.0)
{
    DgState s;
    memset(&s, 0, sizeof(s));
    s.h = -1;                                                // hysteresis false / clock LOW
    s.o = P;                                                 // zerocrossingclockrecovery.lua:37: the offset starts at one symbol period
    return s;
}

// =====================================================================================================
// ZeroCrossingClockRecoveryBlock, and the fused clocksampler (+ slicer + differential decoder)
// =====================================================================================================
struct ZcStage : lrhip_stage {
    ZcParams p;
    bool sampler = false;                    // clocksampler: emits x[i] where the recovered clock rises
    DgTail tail{DG_OUT_FLOAT, 0.0, 0};
    DeviceBuf scratch, staging;
    Carried<DgState> st;
    const char *kind() const override { return sampler ? "clocksampler" : "zerocrossingclockrecovery"; }
    long memory() const override { return -1; }
    int reset() override { return st.reset(dg_state_init(p.P)); }
    unsigned long max_output(unsigned long n) const override { return sampler ? (n + 1) / 2 + 1 : n; }
    long run(const void *in_dev, unsigned long n, void *out_dev, unsigned long cap) override
    {
        if (!sampler && n > cap) return set_error("%s: output capacity %lu < %lu", kind(), cap, n);
        if (!n) return 0;
        const unsigned long nt = (n + DG_TILE - 1) / DG_TILE;
        const ZcScratch sc(nt);
        if (scratch.reserve(sc.total)) return -1;
        HSum *tiles = sc.tiles.in(scratch);
        int *t_h = sc.t_h.in(scratch), *t_kind = sc.t_kind.in(scratch), *t_prev = sc.t_prev.in(scratch), *t_bit = sc.t_bit.in(scratch);
        long long *t_rpos = sc.t_rpos.in(scratch);
        double *t_o = sc.t_o.in(scratch);
        unsigned *t_cnt = sc.t_cnt.in(scratch);
        const DgState *si = st.in();
        DgState *so = st.out();
        const float *x = (const float *)in_dev;
        hipLaunchKernelGGL(zc_summary_kernel, dim3((unsigned)nt), dim3(256), 0, ctx().stream, x, n, p.T, tiles);
        LR_LAUNCH_CHECK();
        hipLaunchKernelGGL(zc_carry_kernel, dim3(1), dim3(256), 0, ctx().stream, (const HSum *)tiles, nt, n, p, si, so, t_h, t_rpos, t_kind, t_o, t_prev);
        LR_LAUNCH_CHECK();
        if (!sampler) {
            hipLaunchKernelGGL((zc_emit_kernel<0>), dim3((unsigned)nt), dim3(256), 0, ctx().stream, x, n, p, tail, out_dev, si, so,
                               (const int *)t_h, (const long long *)t_rpos, (const int *)t_kind, (const double *)t_o, (const int *)t_prev, t_cnt, t_bit);
            LR_LAUNCH_CHECK();
            st.flip();
            return (long)n;
        }
        const unsigned long bound = max_output(n);
        if (cap < bound) return set_error("%s: output capacity %lu < bound %lu", kind(), cap, bound);
        // each tile's emitted samples / sliced bits in a slot of DG_TILE / 2 entries (a rising clock edge needs a sample without pulse before it)
        const size_t esz = tail.out == DG_OUT_FLOAT ? 4 : 1;
        if (staging.reserve(nt * (DG_TILE / 2) * esz)) return -1;
        hipLaunchKernelGGL((zc_emit_kernel<1>), dim3((unsigned)nt), dim3(256), 0, ctx().stream, x, n, p, tail, staging.p, si, so,
                           (const int *)t_h, (const long long *)t_rpos, (const int *)t_kind, (const double *)t_o, (const int *)t_prev, t_cnt, t_bit);
        LR_LAUNCH_CHECK();
        // packing: up to 256 workgroups, each a run of `per` tiles
        const unsigned long per = (nt + 255) / 256, groups = (nt + per - 1) / per;
        if (tail.out == DG_OUT_FLOAT)
            hipLaunchKernelGGL((dg_compact_kernel<DG_OUT_FLOAT>), dim3((unsigned)groups), dim3(256), 0, ctx().stream, (const void *)staging.p, (const unsigned *)t_cnt,
                               (const int *)t_bit, nt, per, tail, out_dev, cap, si, so);
        else if (tail.out == DG_OUT_SLICE)
            hipLaunchKernelGGL((dg_compact_kernel<DG_OUT_SLICE>), dim3((unsigned)groups), dim3(256), 0, ctx().stream, (const void *)staging.p, (const unsigned *)t_cnt,
                               (const int *)t_bit, nt, per, tail, out_dev, cap, si, so);
        else
            hipLaunchKernelGGL((dg_compact_kernel<DG_OUT_DECODE>), dim3((unsigned)groups), dim3(256), 0, ctx().stream, (const void *)staging.p, (const unsigned *)t_cnt,
                               (const int *)t_bit, nt, per, tail, out_dev, cap, si, so);
        LR_LAUNCH_CHECK();
        st.flip();
        DgState got;
        if (st.fetch(got)) return -1;
        if (got.count > bound) return set_error("%s: %llu outputs exceed the bound %lu", kind(), got.count, bound);
        return (long)got.count;
    }
};

// =====================================================================================================
// SamplerBlock: data (Float32 or ComplexFloat32) and clock (Float32) -> the data type, data-dependent count
// =====================================================================================================
struct SamplerStage : BinaryStage {
    DeviceBuf scratch;
    Carried<DgState> st;
    const char *kind() const override { return "sampler"; }
    long memory() const override { return -1; }
    int reset() override { return st.reset(dg_state_init()); }
    unsigned long max_output(unsigned long n) const override { return (n + 1) / 2 + 1; }
    long run2(const void *data, const void *clk, unsigned long n, void *y, unsigned long cap) override
    {
        if (!n) return 0;
        const unsigned long bound = max_output(n);
        if (cap < bound) return set_error("sampler: output capacity %lu < bound %lu", cap, bound);
        const unsigned long nt = (n + DG_TILE - 1) / DG_TILE;
        const SamplerScratch sc(nt);
        if (scratch.reserve(sc.total)) return -1;
        SSum *tiles = sc.tiles.in(scratch);
        int *t_h = sc.t_h.in(scratch);
        unsigned long long *t_off = sc.t_off.in(scratch);
        const DgState *si = st.in();
        DgState *so = st.out();
        hipLaunchKernelGGL(sampler_summary_kernel, dim3((unsigned)nt), dim3(256), 0, ctx().stream, (const float *)clk, n, tiles);
        LR_LAUNCH_CHECK();
        hipLaunchKernelGGL(sampler_carry_kernel, dim3(1), dim3(256), 0, ctx().stream, (const SSum *)tiles, nt, si, so, t_h, t_off);
        LR_LAUNCH_CHECK();
        if (in_size == 8)
            hipLaunchKernelGGL(sampler_final_kernel<2>, dim3((unsigned)nt), dim3(256), 0, ctx().stream, (const float *)data, (const float *)clk, n, (float *)y, cap,
                               (const int *)t_h, (const unsigned long long *)t_off);
        else
            hipLaunchKernelGGL(sampler_final_kernel<1>, dim3((unsigned)nt), dim3(256), 0, ctx().stream, (const float *)data, (const float *)clk, n, (float *)y, cap,
                               (const int *)t_h, (const unsigned long long *)t_off);
        LR_LAUNCH_CHECK();
        st.flip();
        DgState got;
        if (st.fetch(got)) return -1;
        if (got.count > bound) return set_error("sampler: %llu outputs exceed the bound %lu", got.count, bound);
        return (long)got.count;
    }
};

// =====================================================================================================
// SlicerBlock: Float32 -> Bit (1 B), x > threshold in double
// =====================================================================================================
struct SlicerStage : lrhip_stage {
    double t = 0.0;
    const char *kind() const override { return "slicer"; }
    int reset() override { return 0; }
    long run(const void *in_dev, unsigned long n, void *out_dev, unsigned long cap) override
    {
        if (n > cap) return set_error("slicer: output capacity %lu < %lu", cap, n);
        if (!n) return 0;
        hipLaunchKernelGGL(slicer_kernel, dim3(grid_for(n, 256)), dim3(256), 0, ctx().stream, (const float *)in_dev, (uint8_t *)out_dev, n, t);
        LR_LAUNCH_CHECK();
        return (long)n;
    }
};

// =====================================================================================================
// DifferentialDecoderBlock: Bit -> Bit, out = prev ^ x (inverted: (prev ^ x + 1) % 2), prev = the previous input byte
// =====================================================================================================
struct DiffDecStage : lrhip_stage {
    int invert = 0;
    Carried<uint8_t> state;                  // the last input byte of the previous call
    const char *kind() const override { return "differentialdecoder"; }
    long memory() const override { return 1; }
    int reset() override { return state.reset(); }
    long run(const void *in_dev, unsigned long n, void *out_dev, unsigned long cap) override
    {
        if (n > cap) return set_error("differentialdecoder: output capacity %lu < %lu", cap, n);
        if (!n) return 0;
        hipLaunchKernelGGL(diffdec_kernel, dim3(grid_for(n, 256)), dim3(256), 0, ctx().stream, (const uint8_t *)in_dev, (uint8_t *)out_dev, n, invert,
                           state.in(), state.out());
        LR_LAUNCH_CHECK();
        state.flip();
        return (long)n;
    }
};

// ---- constructors behind lrhip_unary_create (op strings, op_string.h)
// "zerocrossingclockrecovery:period=P:threshold=T" and "clocksampler:period=P:threshold=T"
static lrhip_stage_t *zc_create(const char *op)
{
    OpFields f;
    double P = 0.0, T = 0.0;
    if (!f.split(op, nullptr, {{"period", nullptr}, {"threshold", nullptr}}, true) || !f.number("period", P) || !f.number("threshold", T)) return nullptr;
    if (!(P > 0.0) || !std::isfinite(P)) { set_error("%s: period must be finite and > 0", f.name.c_str()); return nullptr; }
    if (!std::isfinite(T)) { set_error("%s: threshold must be finite", f.name.c_str()); return nullptr; }
    auto q = new_stage<ZcStage>();
    if (!q) return nullptr;
    zc_prepare(P, T, q->p);
    q->sampler = f.name == "clocksampler";
    q->in_size = q->out_size = 4;
    if (q->reset()) return nullptr;
    return q.release();
}

// "slicer:threshold=T"
static lrhip_stage_t *slicer_create(const char *op)
{
    OpFields f;
    double T = 0.0;
    if (!f.split(op, "slicer", {{"threshold", nullptr}}, true) || !f.number("threshold", T)) return nullptr;
    auto q = new_stage<SlicerStage>();
    if (!q) return nullptr;
    q->t = T;
    q->in_size = 4; q->out_size = 1;
    return q.release();
}

// "differentialdecoder:invert=0|1"
static lrhip_stage_t *diffdec_create(const char *op)
{
    OpFields f;
    bool invert = false;
    if (!f.split(op, "differentialdecoder", {{"invert", nullptr}}, true) || !f.flag("invert", invert)) return nullptr;
    auto q = new_stage<DiffDecStage>();
    if (!q) return nullptr;
    q->invert = invert;
    q->in_size = q->out_size = 1;
    if (q->reset()) return nullptr;
    return q.release();
}
