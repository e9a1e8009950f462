// stage_fecglue.h - PunctureBlock, DepunctureBlock, ConvolutionalInterleaverBlock, ConvolutionalDeinterleaverBlock and AdditiveScramblerBlock
// (kernels_fecglue.h, fecglue_plan.h), created through lrhip_unary_create ("puncture:pattern=B", "depuncture:pattern=B:input=llr|bit",
// "convinterleave:branches=I:step=M", "convdeinterleave:branches=I:step=M", "scrambler:table=HEX:offset=K").  Every stage is a function of the
// absolute stream index alone, checks its domain before the device is looked at, and fuses with nothing.
// (part of liblrhip.so; included by lrhip.hip after stage_reedsolomon.h, one translation unit)
#pragma once

// PunctureBlock (Bit -> Bit) and DepunctureBlock (Float32 or Bit -> Float32): FramedStage with frames in elements
struct PunctureStage : FramedStage {
    bool depuncture = false, bit_input = false;
    DeviceBuf map;
    int launch(const uint8_t *carried, const uint8_t *in_dev, uint8_t *out_dev, uint32_t c, long nf) override
    {
        if ((uintptr_t)in_dev % (unsigned)in_size || (uintptr_t)out_dev % (unsigned)out_size) return set_error("%s: a buffer is not aligned to its elements", who);
        const unsigned long n_out = (unsigned long)nf * frame.fo;
        const int small = n_out < (1ul << 32);
        const uint8_t *m = (const uint8_t *)map.p;
        if (!depuncture)
            hipLaunchKernelGGL(puncture_kernel, dim3(grid_for((n_out + 15) / 16 + 1, FG_NT)), dim3(FG_NT), 0, ctx().stream, carried, in_dev, out_dev, m, c, frame.fi,
                               frame.fo, n_out, small);
        else if (bit_input)
            hipLaunchKernelGGL(depuncture_kernel<true>, dim3(grid_for(n_out, FG_NT)), dim3(FG_NT), 0, ctx().stream, (const void *)carried, (const void *)in_dev,
                               (uint32_t *)out_dev, m, c, frame.fi, frame.fo, n_out, small);
        else
            hipLaunchKernelGGL(depuncture_kernel<false>, dim3(grid_for(n_out, FG_NT)), dim3(FG_NT), 0, ctx().stream, (const void *)carried, (const void *)in_dev,
                               (uint32_t *)out_dev, m, c, frame.fi, frame.fo, n_out, small);
        LR_LAUNCH_CHECK();
        return 0;
    }
};

static lrhip_stage_t *puncture_create(const char *op)
{
    OpFields f;
    const bool depuncture = !strncmp(op, "depuncture", 10);
    const char *who = depuncture ? "depuncture" : "puncture";
    std::vector<OpKey> keys = {{"pattern", nullptr}};
    if (depuncture) keys.push_back({"input", nullptr});
    std::string pattern;
    if (!f.split(op, who, keys, false) || !f.bits("pattern", pattern)) return nullptr;
    switch (fgplan::check_pattern(pattern.c_str(), pattern.size())) {
    case 0: break;
    case 1: set_error("%s: pattern must be %d .. %d characters (got %zu)", who, fgplan::PATTERN_MIN, fgplan::PATTERN_MAX, pattern.size()); return nullptr;
    default: set_error("%s: pattern must not be all 0 (got \"%s\")", who, pattern.c_str()); return nullptr;
    }
    int input = 1;
    if (depuncture && (input = f.word("input", {"llr", "bit"}, "depuncture: unsupported input \"", "\" (llr or bit)")) < 0) return nullptr;
    auto q = new_stage<PunctureStage>();
    if (!q) return nullptr;
    const uint32_t len = (uint32_t)pattern.size();
    uint8_t host[fgplan::PATTERN_MAX] = {0};
    q->who = who;
    q->depuncture = depuncture;
    q->bit_input = input == 1;
    if (depuncture) {
        q->frame = fgplan::depuncture_frame(pattern.c_str(), len);
        fgplan::depuncture_map(pattern.c_str(), len, host);
        q->in_size = q->bit_input ? 1 : 4; q->out_size = 4;
    } else {
        q->frame = fgplan::puncture_frame(pattern.c_str(), len);
        fgplan::puncture_map(pattern.c_str(), len, host);
        q->in_size = q->out_size = 1;
    }
    if (upload(q->map, host, sizeof host) || q->reset()) return nullptr;
    return q.release();
}

// ConvolutionalInterleaverBlock / ConvolutionalDeinterleaverBlock, Byte -> Byte, 1 : 1.  Carried: the last D = (I - 1) M I input bytes (two buffers,
// ping-pong, as DelayStage carries its own; zeros wherever the stream begins or continues) and the branch q = Q mod I of the next input
struct ConvInterleaveStage : lrhip_stage {
    uint32_t I = 2, M = 1, D = 2, q = 0;
    bool deinterleave = false;
    TwoSlots carry;
    const char *kind() const override { return deinterleave ? "convdeinterleave" : "convinterleave"; }
    long memory() const override { return (long)D; }
    int seek_to(uint64_t n0)
    {
        q = (uint32_t)(n0 % I);
        return carry.reset(D);
    }
    int reset() override { return seek_to(0); }
    int seek(unsigned long long n0, unsigned long long *n0_out) override
    {
        if (seek_to(n0)) return -1;
        *n0_out = n0;
        return 0;
    }
    long run(const void *in_dev, unsigned long n, void *out_dev, unsigned long cap) override
    {
        if (n > cap) return set_error("%s: output capacity %lu < %lu", kind(), cap, n);
        if (!n) return 0;
        if (n > (unsigned long)LONG_MAX) return set_error("%s: more than 2^63 bytes in one call", kind());
        if (!in_dev) return set_error("%s: null input buffer", kind());
        if (!out_dev) return set_error("%s: null output buffer", kind());
        // a tile of T outputs reads T + D inputs: T no smaller than D keeps that below twice, 16 KiB keeps the shallow shapes at several workgroups per CU
        const uint32_t T = D > 32768 ? 32768 : 16384;
        const size_t lds_bytes = ((size_t)T + D + 32 + 15) & ~(size_t)15;
        if (kernel_allow_lds(convinterleave_kernel, lds_bytes)) return -1;
        const unsigned long tiles = (n + 15 + T - 1) / T;
        const uint8_t *carried = carry.in<uint8_t>();
        hipLaunchKernelGGL(convinterleave_kernel, dim3(grid_for(tiles, 1)), dim3(FG_NT), lds_bytes, ctx().stream, carried, (const uint8_t *)in_dev, (uint8_t *)out_dev,
                           I, M, D, (int)deinterleave, q, n, T, (int)(n < (1ul << 32)));
        LR_LAUNCH_CHECK();
        hipLaunchKernelGGL(frame_carry_kernel, dim3(grid_for(D, 256)), dim3(256), 0, ctx().stream, carried, (const uint8_t *)in_dev, carry.out<uint8_t>(), D,
                           (uint64_t)n, D);
        LR_LAUNCH_CHECK();
        carry.flip();
        q = (uint32_t)((q + n % I) % I);
        return (long)n;
    }
};

static lrhip_stage_t *convinterleave_create(const char *op)
{
    OpFields f;
    const bool deinterleave = !strncmp(op, "convdeinterleave", 16);
    const char *who = deinterleave ? "convdeinterleave" : "convinterleave";
    long I = 0, M = 0;
    if (!f.split(op, who, {{"branches", nullptr}, {"step", nullptr}}, false) || !f.integer("branches", LONG_MIN, LONG_MAX, I) ||
        !f.integer("step", LONG_MIN, LONG_MAX, M)) return nullptr;
    switch (fgplan::check_interleaver(I, M)) {
    case 0: break;
    case 1: set_error("%s: branches must be %d .. %d (got %ld)", who, fgplan::BRANCHES_MIN, fgplan::BRANCHES_MAX, I); return nullptr;
    case 2: set_error("%s: step must be %d .. %d (got %ld)", who, fgplan::STEP_MIN, fgplan::STEP_MAX, M); return nullptr;
    default: set_error("%s: the depth (branches - 1) * step * branches = %ld must be at most %u", who, (I - 1) * M * I, fgplan::DEPTH_MAX); return nullptr;
    }
    auto q = new_stage<ConvInterleaveStage>();
    if (!q) return nullptr;
    q->I = (uint32_t)I; q->M = (uint32_t)M; q->D = fgplan::depth((uint32_t)I, (uint32_t)M);
    q->deinterleave = deinterleave;
    q->in_size = q->out_size = 1;
    if (q->reset()) return nullptr;
    return q.release();
}

// AdditiveScramblerBlock, Byte -> Byte, 1 : 1, stateless but for the table index of the next byte
struct ScramblerStage : lrhip_stage {
    uint32_t P = 1, K = 0, index = 0;
    DeviceBuf ext;                             // the table and its first 15 bytes again
    const char *kind() const override { return "scrambler"; }
    int reset() override { index = K; return 0; }
    int seek(unsigned long long n0, unsigned long long *n0_out) override
    {
        index = fgplan::table_index(n0, K, P);
        *n0_out = n0;
        return 0;
    }
    long run(const void *in_dev, unsigned long n, void *out_dev, unsigned long cap) override
    {
        if (n > cap) return set_error("scrambler: output capacity %lu < %lu", cap, n);
        if (!n) return 0;
        if (n > (unsigned long)LONG_MAX) return set_error("scrambler: more than 2^63 bytes in one call");
        if (!in_dev) return set_error("scrambler: null input buffer");
        if (!out_dev) return set_error("scrambler: null output buffer");
        hipLaunchKernelGGL(scrambler_kernel, dim3(grid_for((n + 15) / 16 + 1, FG_NT)), dim3(FG_NT), 0, ctx().stream, (const uint8_t *)in_dev, (uint8_t *)out_dev,
                           (const uint8_t *)ext.p, index, P, n, (int)(n < (1ul << 32)));
        LR_LAUNCH_CHECK();
        index = fgplan::table_advance(index, n, P);
        return (long)n;
    }
};

static lrhip_stage_t *scrambler_create(const char *op)
{
    OpFields f;
    std::vector<uint8_t> table;
    long K = 0;
    if (!f.split(op, "scrambler", {{"table", nullptr}, {"offset", nullptr}}, false) || !f.hex("table", table)) return nullptr;
    if (table.size() > (size_t)fgplan::TABLE_MAX) { set_error("scrambler: the table has %zu bytes, it must be 1 .. %d", table.size(), fgplan::TABLE_MAX); return nullptr; }
    if (!f.integer("offset", LONG_MIN, LONG_MAX, K)) return nullptr;
    if (K < 0 || K >= (long)table.size()) { set_error("scrambler: offset must be 0 .. %zu, the table's length less one (got %ld)", table.size() - 1, K); return nullptr; }
    auto q = new_stage<ScramblerStage>();
    if (!q) return nullptr;
    q->P = (uint32_t)table.size(); q->K = (uint32_t)K;
    std::vector<uint8_t> ext(table.size() + 15);
    for (size_t i = 0; i < ext.size(); i++) ext[i] = table[i % table.size()];
    q->in_size = q->out_size = 1;
    if (upload(q->ext, ext.data(), ext.size()) || q->reset()) return nullptr;
    return q.release();
}
