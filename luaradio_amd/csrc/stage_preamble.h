// stage_preamble.h - PreambleSamplerBlock and ManchesterDecoderBlock (kernels_preamble.h) and VaricodeDecoderBlock (kernels_varicode.h), created
// through lrhip_unary_create ("preamblesampler:period=T:num_samples=N:preamble=0101...", "manchesterdecoder:invert=0|1" and "varicodedecoder").
// All three have a data-dependent output count: run() returns the exact count, read back from the device after the last pass (one small
// synchronous copy per call), and memory() = -1.
// (part of liblrhip.so; included by lrhip.hip after stage_digital.h, one translation unit)
#pragma once

// The largest circular buffer B = 2^ceil_log2(T L + 1) a preamblesampler accepts: 2^21 samples (8 MiB of history, twice for the ping-pong),
// which admits every T L <= 2^20.
constexpr long long PS_MAX_B = 1ll << 21;

// =====================================================================================================
// PreambleSamplerBlock: Float32 -> Float32, data-dependent count
// =====================================================================================================
struct PsStage : lrhip_stage {
    PsParams p{0, 0, 0, 0};
    std::vector<uint32_t> pre_bits;          // the preamble, bit k of word k / 32
    DeviceBuf pre, scratch;
    TwoSlots hist;                           // the history of B samples, flipped together with st
    Carried<PsState> st;                     // SEARCHING, preamblesampler.lua:56-59
    const char *kind() const override { return "preamblesampler"; }
    long memory() const override { return -1; }
    int reset() override
    {
        if (upload(pre, pre_bits.data(), pre_bits.size() * sizeof(uint32_t)) || st.reset()) return -1;
        return hist.reset((size_t)p.B * sizeof(float));               // the reference's buffer starts as zeros (:52)
    }
    // Output 0 of a frame is emitted at sample j*, output m >= 1 at j* + m T - 1: inside a frame consecutive emissions are T - 1 (m = 0 -> 1) or
    // T samples apart.  The last one is at s' - 1; the next frame's i* >= s' and its j* > i*, so its first emission is at s' + 1 or later: 2
    // samples apart.  Every sample carries at most one emission, whatever the carried state, so n bounds every T >= 2; for T >= 3 emissions
    // are at least 2 samples apart and n samples hold at most ceil(n / 2) of them (the + 1 as for the sampler).
    unsigned long max_output(unsigned long n) const override { return p.T >= 3 ? (n + 1) / 2 + 1 : n; }
    long run(const void *in_dev, unsigned long n, void *out_dev, unsigned long cap) override
    {
        if (!n) return 0;
        const unsigned long bound = max_output(n);
        if (cap < bound) return set_error("preamblesampler: output capacity %lu < bound %lu", cap, bound);
        const unsigned long nt = (n + PS_TILE - 1) / PS_TILE;
        // frames with an output inside one call: the j* of consecutive frames are at least (N - 1) T + 2 samples apart, so at most
        // n / ((N - 1) T) + 1 of them lie inside the call, plus the frame in progress at its start
        const unsigned long max_frames = n / ((unsigned long)(p.N - 1) * (unsigned long)p.T) + 2;
        const PsScratch sc(nt, max_frames);
        if (scratch.reserve(sc.total)) return -1;
        unsigned long long *mask_m = sc.mask_m.in(scratch), *mask_d = sc.mask_d.in(scratch);
        int *tile_m = sc.tile_m.in(scratch), *tile_d = sc.tile_d.in(scratch);
        PsFrame *frames = sc.frames.in(scratch);
        const PsState *si = st.in();
        PsState *so = st.out();
        const float *hi = hist.in<float>();
        float *ho = hist.out<float>();
        const float *x = (const float *)in_dev;
        hipLaunchKernelGGL(ps_match_kernel, dim3((unsigned)nt), dim3(256), 0, ctx().stream, x, hi, n, p, (const uint32_t *)pre.p, mask_m, mask_d, tile_m, tile_d);
        LR_LAUNCH_CHECK();
        hipLaunchKernelGGL(ps_walk_kernel, dim3(1), dim3(256), 0, ctx().stream, (const unsigned long long *)mask_m, (const unsigned long long *)mask_d,
                           (const int *)tile_m, (const int *)tile_d, nt, n, p, si, so, frames, max_frames, cap);
        LR_LAUNCH_CHECK();
        unsigned long grid = (unsigned long)(p.B / 64) > max_frames ? (unsigned long)(p.B / 64) : max_frames;
        grid = grid > 2048 ? 2048 : (grid < 1 ? 1 : grid);
        hipLaunchKernelGGL(ps_emit_kernel, dim3((unsigned)grid), dim3(64), 0, ctx().stream, x, hi, ho, n, p, (const PsState *)so, (const PsFrame *)frames,
                           (float *)out_dev, cap);
        LR_LAUNCH_CHECK();
        st.flip();
        hist.flip();
        PsState got;
        if (st.fetch(got)) return -1;
        if (got.overflow || got.count > bound) return set_error("preamblesampler: %llu outputs in %llu frames exceed the bound %lu (%lu frames)", got.count, got.frames, bound, max_frames);
        return (long)got.count;
    }
};

// "preamblesampler:period=T:num_samples=N:preamble=0101...": T and N integers, preamble a string of 0 / 1 characters
static lrhip_stage_t *preamblesampler_create(const char *op)
{
    OpFields f;
    long T = 0, N = 0;
    std::string bits;
    if (!f.split(op, "preamblesampler", {{"period", nullptr}, {"num_samples", nullptr}, {"preamble", nullptr}}, true) ||
        !f.integer("period", -0x7fffffffl, 0x7fffffffl, T) || !f.integer("num_samples", -0x7fffffffl, 0x7fffffffl, N) || !f.bits("preamble", bits)) return nullptr;
    // preamblesampler.lua:108-121: with a period of 1 the offset becomes 0 and is decremented before it is tested, with one sample per frame
    // the bit count is past num_samples before it is compared - either way the reference never leaves SAMPLING
    if (T < 2) { set_error("preamblesampler: period must be >= 2 samples per symbol (got %ld)", T); return nullptr; }
    if (N < 2) { set_error("preamblesampler: num_samples must be >= 2 (got %ld)", N); return nullptr; }
    if (bits.empty()) { set_error("preamblesampler: the preamble is empty"); return nullptr; }
    const long long TL = (long long)T * (long long)bits.size();
    long long B = 1;
    while (B < TL + 1 && B <= PS_MAX_B) B *= 2;                  // 2^ceil_log2(T L + 1), preamblesampler.lua:52
    if (B > PS_MAX_B) { set_error("preamblesampler: period * preamble length = %lld needs a buffer above the limit of %lld samples", TL, PS_MAX_B); return nullptr; }
    auto q = new_stage<PsStage>();
    if (!q) return nullptr;
    q->p = PsParams{(int)T, (int)bits.size(), (int)N, B};
    q->pre_bits.assign((bits.size() + 31) / 32, 0u);
    for (size_t k = 0; k < bits.size(); k++)
        if (bits[k] == '1') q->pre_bits[k >> 5] |= 1u << (k & 31);
    q->in_size = q->out_size = 4;
    if (q->reset()) return nullptr;
    return q.release();
}

// =====================================================================================================
// ManchesterDecoderBlock: Bit -> Bit, data-dependent count (at most one output per two inputs, plus the pending bit: (n + 1) / 2)
// =====================================================================================================
struct MdStage : lrhip_stage {
    int invert = 0;
    DeviceBuf scratch;
    Carried<MdState> st;                     // nothing pending, manchesterdecoder.lua:27
    const char *kind() const override { return "manchesterdecoder"; }
    long memory() const override { return -1; }
    int reset() override { return st.reset(); }
    // an output consumes two inputs of its own (the pending bit and the one that completes the pair); the first may be carried: (n + 1) / 2
    unsigned long max_output(unsigned long n) const override { return (n + 1) / 2; }
    long run(const void *in_dev, unsigned long n, void *out_dev, unsigned long cap) override
    {
        if (!n) return 0;
        const unsigned long bound = max_output(n);
        if (cap < bound) return set_error("manchesterdecoder: output capacity %lu < bound %lu", cap, bound);
        const unsigned long nt = (n + DG_TILE - 1) / DG_TILE;
        const MdScratch sc(nt);
        if (scratch.reserve(sc.total)) return -1;
        MSum *tiles = sc.tiles.in(scratch);
        int *t_state = sc.t_state.in(scratch);
        unsigned long long *t_off = sc.t_off.in(scratch);
        const MdState *si = st.in();
        MdState *so = st.out();
        const uint8_t *x = (const uint8_t *)in_dev;
        hipLaunchKernelGGL(md_summary_kernel, dim3((unsigned)nt), dim3(256), 0, ctx().stream, x, n, tiles);
        LR_LAUNCH_CHECK();
        hipLaunchKernelGGL(md_carry_kernel, dim3(1), dim3(256), 0, ctx().stream, (const MSum *)tiles, nt, si, so, t_state, t_off);
        LR_LAUNCH_CHECK();
        hipLaunchKernelGGL(md_final_kernel, dim3((unsigned)nt), dim3(256), 0, ctx().stream, x, n, invert, (uint8_t *)out_dev, cap, (const int *)t_state,
                           (const unsigned long long *)t_off);
        LR_LAUNCH_CHECK();
        st.flip();
        MdState got;
        if (st.fetch(got)) return -1;
        if (got.count > bound) return set_error("manchesterdecoder: %llu outputs exceed the bound %lu", got.count, bound);
        return (long)got.count;
    }
};

// "manchesterdecoder:invert=0|1"
static lrhip_stage_t *manchesterdecoder_create(const char *op)
{
    OpFields f;
    bool invert = false;
    if (!f.split(op, "manchesterdecoder", {{"invert", nullptr}}, true) || !f.flag("invert", invert)) return nullptr;
    auto q = new_stage<MdStage>();
    if (!q) return nullptr;
    q->invert = invert;
    q->in_size = q->out_size = 1;
    if (q->reset()) return nullptr;
    return q.release();
}

// =====================================================================================================
// VaricodeDecoderBlock: Bit -> Byte, data-dependent count (the Manchester decoder's shape: tile summaries of state maps, one carry workgroup,
// a final pass that stores packed - with the characters counted from the true entry states in between, kernels_varicode.h)
// =====================================================================================================
struct VcStage : lrhip_stage {
    DeviceBuf scratch;
    Carried<VcState, VC_MAX_LEN> st;         // an empty state, varicodedecoder.lua:22
    const char *kind() const override { return "varicodedecoder"; }
    long memory() const override { return -1; }
    int reset() override { return st.reset(); }
    unsigned long max_output(unsigned long n) const override { return vc_max_output(n); }
    long run(const void *in_dev, unsigned long n, void *out_dev, unsigned long cap) override
    {
        if (!n) return 0;
        const unsigned long bound = max_output(n);
        if (cap < bound) return set_error("varicodedecoder: output capacity %lu < bound %lu", cap, bound);
        const unsigned long nt = (n + DG_TILE - 1) / DG_TILE;
        const VcScratch sc(nt);
        if (scratch.reserve(sc.total)) return -1;
        VcMap *tiles = sc.tiles.in(scratch);
        unsigned long long *t_off = sc.t_off.in(scratch);
        int *t_state = sc.t_state.in(scratch);
        unsigned *t_cnt = sc.t_cnt.in(scratch), *t_thread = sc.t_thread.in(scratch);
        const VcState *si = st.in();
        VcState *so = st.out();
        const uint8_t *ci = st.ci(), *x = (const uint8_t *)in_dev;
        hipLaunchKernelGGL(vc_summary_kernel, dim3((unsigned)nt), dim3(256), 0, ctx().stream, x, n, tiles);
        LR_LAUNCH_CHECK();
        hipLaunchKernelGGL(vc_carry_kernel, dim3(1), dim3(256), 0, ctx().stream, (const VcMap *)tiles, nt, x, n, si, ci, so, st.co(), t_state);
        LR_LAUNCH_CHECK();
        hipLaunchKernelGGL(vc_count_kernel, dim3((unsigned)nt), dim3(256), 0, ctx().stream, x, n, si, ci, (const int *)t_state, t_cnt, t_thread);
        LR_LAUNCH_CHECK();
        hipLaunchKernelGGL(vc_offsets_kernel, dim3(1), dim3(256), 0, ctx().stream, (const unsigned *)t_cnt, nt, t_off, so);
        LR_LAUNCH_CHECK();
        hipLaunchKernelGGL(vc_final_kernel, dim3((unsigned)nt), dim3(256), 0, ctx().stream, x, n, si, ci, (const unsigned *)t_thread,
                           (const unsigned long long *)t_off, (uint8_t *)out_dev, cap);
        LR_LAUNCH_CHECK();
        st.flip();
        VcState got;
        if (st.fetch(got)) return -1;
        if (got.count > bound) return set_error("varicodedecoder: %llu outputs exceed the bound %lu", got.count, bound);
        return (long)got.count;
    }
};
