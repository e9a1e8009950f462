// stage_rdsframer.h - RDSFramerBlock (kernels_rdsframer.h), created through lrhip_unary_create ("rdsframer", no parameters).  Bit in, one 8-byte
// record (uint16_t blocks[4]) per frame out.  The output count depends on the data: run() returns the exact count, read back from the device after
// the last pass (one small synchronous copy per call), and memory() = -1.
// (part of liblrhip.so; included by lrhip.hip after stage_preamble.h, one translation unit)
#pragma once

struct RfStage : lrhip_stage {
    DeviceBuf table, state, carried, scratch;    // state: two RfState; carried: two slots of RF_CARRY bytes (ping-pong with `cur`)
    PinnedBuf h_state;
    int cur = 0;
    const char *kind() const override { return "rdsframer"; }
    long memory() const override { return -1; }
    int reset() override
    {
        cur = 0;
        uint8_t flags[1024];
        rf_flag_table(flags);
        RfState s[2];
        memset(s, 0, sizeof(s));                             // an empty frame buffer, rdsframer.lua:96-98
        if (upload(table, flags, sizeof(flags)) || upload(state, s, sizeof(s))) return -1;
        return zero_fill(carried, 2 * RF_CARRY);
    }
    // accepted frames are disjoint windows of 104 bits inside "carried bits, then the call": at most (103 + n) / 104 of them
    unsigned long max_output(unsigned long n) const override { return (n + (RF_FRAME - 1)) / RF_FRAME; }
    long run(const void *in_dev, unsigned long n, void *out_dev, unsigned long cap) override
    {
        if (!n) return 0;
        const unsigned long bound = max_output(n);
        if (cap < bound) return set_error("rdsframer: output capacity %lu < bound %lu", cap, bound);
        // tiles of window starts over the carried bits (at most 103) and the call
        const unsigned long nt = (n + (RF_FRAME - 1) + PS_TILE - 1) / PS_TILE;
        const size_t o_tv = (size_t)nt * PS_WORDS * 8, o_st = (o_tv + (size_t)nt * 4 + 7) / 8 * 8, total = o_st + (size_t)bound * 8;
        if (scratch.reserve(total) || h_state.reserve(sizeof(RfState))) return -1;
        char *sp = (char *)scratch.p;
        unsigned long long *mask_v = (unsigned long long *)sp;
        int *tile_v = (int *)(sp + o_tv);
        long long *starts = (long long *)(sp + o_st);
        const RfState *si = (const RfState *)state.p + cur;
        RfState *so = (RfState *)state.p + (cur ^ 1);
        const uint8_t *ci = (const uint8_t *)carried.p + (size_t)cur * RF_CARRY;
        uint8_t *co = (uint8_t *)carried.p + (size_t)(cur ^ 1) * RF_CARRY;
        const uint8_t *x = (const uint8_t *)in_dev;
        hipLaunchKernelGGL(rf_match_kernel, dim3((unsigned)nt), dim3(256), 0, ctx().stream, x, ci, n, si, (const uint8_t *)table.p, mask_v, tile_v);
        LR_LAUNCH_CHECK();
        hipLaunchKernelGGL(rf_walk_kernel, dim3(1), dim3(256), 0, ctx().stream, (const unsigned long long *)mask_v, (const int *)tile_v, nt, n, si, so, starts,
                           bound);
        LR_LAUNCH_CHECK();
        hipLaunchKernelGGL(rf_emit_kernel, dim3((unsigned)((bound + 255) / 256)), dim3(256), 0, ctx().stream, x, ci, co, n, si, (const RfState *)so,
                           (const long long *)starts, (unsigned long long *)out_dev, cap);
        LR_LAUNCH_CHECK();
        cur ^= 1;
        // the data-dependent count: the one small read-back of this stage
        LR_HIP(hipMemcpyAsync(h_state.p, so, sizeof(RfState), hipMemcpyDeviceToHost, ctx().stream));
        LR_HIP(hipStreamSynchronize(ctx().stream));
        const RfState got = *(const RfState *)h_state.p;
        if (got.overflow || got.count > bound) return set_error("rdsframer: %llu frames exceed the bound %lu", got.count, bound);
        return (long)got.count;
    }
};

static lrhip_stage_t *rdsframer_create(const char *op)
{
    if (strchr(op, ':')) { set_error("rdsframer: takes no parameters, got \"%s\"", op); return nullptr; }
    if (ensure_init()) return nullptr;
    std::unique_ptr<RfStage> q(new (std::nothrow) RfStage());
    if (!q) { set_error("out of memory"); return nullptr; }
    q->in_size = 1; q->out_size = 8;
    if (q->reset()) return nullptr;
    return q.release();
}
