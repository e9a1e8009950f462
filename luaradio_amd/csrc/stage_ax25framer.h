// stage_ax25framer.h - AX25FramerBlock (kernels_ax25framer.h), created through lrhip_unary_create ("ax25framer", no parameters).  Bit in, one
// struct lrhip_ax25_frame (416 bytes, include/lrhip.h) per frame out.  The output count depends on the data: run() returns the exact count, read
// back from the device after the last pass (one small synchronous copy per call), and memory() = -1.
// (part of liblrhip.so; included by lrhip.hip after stage_ertframer.h, one translation unit)
#pragma once

struct AxStage : lrhip_stage {
    DeviceBuf rows, state, carried, scratch;     // state: two AxState; carried: two slots of AX_CARRY bytes (ping-pong with `cur`)
    PinnedBuf h_state;
    int cur = 0;
    const char *kind() const override { return "ax25framer"; }
    long memory() const override { return -1; }
    int reset() override
    {
        cur = 0;
        std::vector<uint16_t> r(AX_CRC_ROWS);
        ax_crc_rows(r.data());
        AxState s[2];
        memset(s, 0, sizeof(s));                             // IDLE with an empty byte buffer, ax25framer.lua:85-90
        if (upload(rows, r.data(), r.size() * sizeof(uint16_t)) || upload(state, s, sizeof(s))) return -1;
        return zero_fill(carried, 2 * AX_CARRY);
    }
    // An emitted frame owns its opening flag (the flag that closes an emitted frame opens none), at least 120 unstuffed bits and its closing
    // flag: 136 bits of its own, of which only the last has to lie in the call: at most (n + 135) / 136 frames.
    unsigned long max_output(unsigned long n) const override { return (n + 135) / 136; }
    long run(const void *in_dev, unsigned long n, void *out_dev, unsigned long cap) override
    {
        if (!n) return 0;
        const unsigned long bound = max_output(n);
        if (cap < bound) return set_error("ax25framer: output capacity %lu < bound %lu", cap, bound);
        // tiles of positions over the carried bytes (at most AX_RAW_MAX + 7) and the call; consumed flags lie 8 or more apart
        const unsigned long most = n + AX_RAW_MAX + 7, nt = (most + PS_TILE - 1) / PS_TILE, max_flags = most / 8 + 1;
        const size_t o_tf = (size_t)nt * PS_WORDS * 8, o_fl = (o_tf + (size_t)nt * 4 + 7) / 8 * 8, o_sg = o_fl + (size_t)max_flags * 8,
                     o_va = o_sg + (size_t)bound * 8, total = o_va + max_flags;
        if (scratch.reserve(total) || h_state.reserve(sizeof(AxState))) return -1;
        char *sp = (char *)scratch.p;
        unsigned long long *mask_f = (unsigned long long *)sp, *segs = (unsigned long long *)(sp + o_sg);
        int *tile_f = (int *)(sp + o_tf);
        long long *flags = (long long *)(sp + o_fl);
        uint8_t *valid = (uint8_t *)(sp + o_va);
        const AxState *si = (const AxState *)state.p + cur;
        AxState *so = (AxState *)state.p + (cur ^ 1);
        const uint8_t *ci = (const uint8_t *)carried.p + (size_t)cur * AX_CARRY;
        uint8_t *co = (uint8_t *)carried.p + (size_t)(cur ^ 1) * AX_CARRY;
        const uint8_t *x = (const uint8_t *)in_dev;
        const uint16_t *rw = (const uint16_t *)rows.p;
        hipLaunchKernelGGL(ax_match_kernel, dim3((unsigned)nt), dim3(256), 0, ctx().stream, x, ci, n, si, mask_f, tile_f);
        LR_LAUNCH_CHECK();
        hipLaunchKernelGGL(ax_walk_kernel, dim3(1), dim3(256), 0, ctx().stream, (const unsigned long long *)mask_f, (const int *)tile_f, nt, n, si, so, flags,
                           max_flags);
        LR_LAUNCH_CHECK();
        // one wave per segment / per frame, grid-stride
        const unsigned long eval_grid = max_flags < 4096 ? max_flags : 4096, emit_grid = bound < 4096 ? bound : 4096;
        hipLaunchKernelGGL(ax_eval_kernel, dim3((unsigned)eval_grid), dim3(64), 0, ctx().stream, x, ci, si, (const AxState *)so, rw, (const long long *)flags,
                           valid);
        LR_LAUNCH_CHECK();
        hipLaunchKernelGGL(ax_select_kernel, dim3(1), dim3(256), 0, ctx().stream, x, ci, co, n, si, so, (const long long *)flags, (const uint8_t *)valid, segs,
                           bound);
        LR_LAUNCH_CHECK();
        hipLaunchKernelGGL(ax_emit_kernel, dim3((unsigned)emit_grid), dim3(64), 0, ctx().stream, x, ci, si, (const AxState *)so, rw, (const long long *)flags,
                           (const unsigned long long *)segs, (uint32_t *)out_dev, cap);
        LR_LAUNCH_CHECK();
        cur ^= 1;
        // the data-dependent count: the one small read-back of this stage
        LR_HIP(hipMemcpyAsync(h_state.p, so, sizeof(AxState), hipMemcpyDeviceToHost, ctx().stream));
        LR_HIP(hipStreamSynchronize(ctx().stream));
        const AxState got = *(const AxState *)h_state.p;
        if (got.overflow || got.count > bound) return set_error("ax25framer: %llu frames exceed the bound %lu", got.count, bound);
        return (long)got.count;
    }
};

static lrhip_stage_t *ax25framer_create(const char *op)
{
    if (strchr(op, ':')) { set_error("ax25framer: takes no parameters, got \"%s\"", op); return nullptr; }
    if (ensure_init()) return nullptr;
    std::unique_ptr<AxStage> q(new (std::nothrow) AxStage());
    if (!q) { set_error("out of memory"); return nullptr; }
    q->in_size = 1; q->out_size = AX_REC;
    if (q->reset()) return nullptr;
    return q.release();
}
