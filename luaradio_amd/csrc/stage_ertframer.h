// stage_ertframer.h - SCMFramerBlock, SCMPlusFramerBlock and IDMFramerBlock (kernels_ertframer.h), created through lrhip_unary_create
// ("scmframer", "scmplusframer", "idmframer"; no parameters).  Bit in, one record per frame out: 16, 16 and 88 bytes (include/lrhip.h).  The
// output count depends on the data: run() returns the exact count, read back from the device after the last pass (one small synchronous copy
// per call), and memory() = -1.
// (part of liblrhip.so; included by lrhip.hip after stage_rdsframer.h, one translation unit)
#pragma once

template <int K> struct EfStage : lrhip_stage {
    typedef EfProto<K> P;
    DeviceBuf rows, state, carried, scratch;     // state: two EfState; carried: two slots of EF_CARRY bytes (ping-pong with `cur`)
    PinnedBuf h_state;
    int cur = 0;
    static const char *name() { return K == EF_SCM ? "scmframer" : K == EF_SCMPLUS ? "scmplusframer" : "idmframer"; }
    const char *kind() const override { return name(); }
    long memory() const override { return -1; }
    int reset() override
    {
        cur = 0;
        uint16_t r[P::CW];
        ef_rows(K, r);
        EfState s[2];
        memset(s, 0, sizeof(s));                             // an empty frame buffer
        if (upload(rows, r, sizeof(r)) || upload(state, s, sizeof(s))) return -1;
        return zero_fill(carried, 2 * EF_CARRY);
    }
    // accepted frames are disjoint windows of L bits inside "carried bits, then the call": at most (L - 1 + n) / L of them
    unsigned long max_output(unsigned long n) const override { return (n + (P::L - 1)) / P::L; }
    long run(const void *in_dev, unsigned long n, void *out_dev, unsigned long cap) override
    {
        if (!n) return 0;
        const unsigned long bound = max_output(n);
        if (cap < bound) return set_error("%s: output capacity %lu < bound %lu", name(), cap, bound);
        // tiles of window starts over the carried bytes (at most L - 1) and the call
        const unsigned long nt = (n + (P::L - 1) + PS_TILE - 1) / PS_TILE;
        const size_t o_ma = (size_t)nt * PS_WORDS * 8, o_te = 2 * o_ma, o_st = (o_te + (size_t)nt * 4 + 7) / 8 * 8, total = o_st + (size_t)bound * 8;
        if (scratch.reserve(total) || h_state.reserve(sizeof(EfState))) return -1;
        char *sp = (char *)scratch.p;
        unsigned long long *mask_e = (unsigned long long *)sp, *mask_a = (unsigned long long *)(sp + o_ma);
        int *tile_e = (int *)(sp + o_te);
        long long *starts = (long long *)(sp + o_st);
        const EfState *si = (const EfState *)state.p + cur;
        EfState *so = (EfState *)state.p + (cur ^ 1);
        const uint8_t *ci = (const uint8_t *)carried.p + (size_t)cur * EF_CARRY;
        uint8_t *co = (uint8_t *)carried.p + (size_t)(cur ^ 1) * EF_CARRY;
        const uint8_t *x = (const uint8_t *)in_dev;
        const uint16_t *rw = (const uint16_t *)rows.p;
        unsigned long long *y = (unsigned long long *)out_dev;
        hipLaunchKernelGGL(ef_match_kernel<K>, dim3((unsigned)nt), dim3(256), 0, ctx().stream, x, ci, n, si, rw, mask_e, mask_a, tile_e);
        LR_LAUNCH_CHECK();
        hipLaunchKernelGGL(ef_walk_kernel<K>, dim3(1), dim3(256), 0, ctx().stream, x, ci, co, n, si, so, rw, (const unsigned long long *)mask_e,
                           (const unsigned long long *)mask_a, (const int *)tile_e, nt, starts, y, bound);
        LR_LAUNCH_CHECK();
        // one wave per frame, four to a workgroup
        hipLaunchKernelGGL(ef_emit_kernel<K>, dim3((unsigned)((bound + 3) / 4)), dim3(256), 0, ctx().stream, x, ci, n, si, (const EfState *)so, rw,
                           (const long long *)starts, y, cap);
        LR_LAUNCH_CHECK();
        cur ^= 1;
        // the data-dependent count: the one small read-back of this stage
        LR_HIP(hipMemcpyAsync(h_state.p, so, sizeof(EfState), hipMemcpyDeviceToHost, ctx().stream));
        LR_HIP(hipStreamSynchronize(ctx().stream));
        const EfState got = *(const EfState *)h_state.p;
        if (got.overflow || got.count > bound) return set_error("%s: %llu frames exceed the bound %lu", name(), got.count, bound);
        return (long)got.count;
    }
};

template <int K> static lrhip_stage_t *ertframer_create(const char *op)
{
    if (strchr(op, ':')) { set_error("%s: takes no parameters, got \"%s\"", EfStage<K>::name(), op); return nullptr; }
    if (ensure_init()) return nullptr;
    std::unique_ptr<EfStage<K>> q(new (std::nothrow) EfStage<K>());
    if (!q) { set_error("out of memory"); return nullptr; }
    q->in_size = 1; q->out_size = EfProto<K>::REC;
    if (q->reset()) return nullptr;
    return q.release();
}
