// stage_pocsagframer.h - POCSAGFramerBlock (kernels_pocsagframer.h), created through lrhip_unary_create ("pocsagframer", no parameters).  Bit in,
// one struct lrhip_pocsag_frame (256 bytes, include/lrhip.h) per record out.  The stage is eager (kernels_pocsagframer.h): its output does not
// depend on how the stream is cut into calls.  The output count depends on the data: run() returns the exact count, read back from the device
// after the last pass (one small synchronous copy per call), and memory() = -1.  reset() drops the pending frame and the buffered bytes.
// (part of liblrhip.so; included by lrhip.hip after stage_ax25framer.h, one translation unit)
#pragma once

struct PgStage : lrhip_stage {
    DeviceBuf state, carried, scratch;           // state: two PgState; carried: two slots of PG_CARRY bytes (ping-pong with `cur`)
    PinnedBuf h_state;
    int cur = 0;
    const char *kind() const override { return "pocsagframer"; }
    long memory() const override { return -1; }
    int reset() override
    {
        cur = 0;
        PgState s[2];
        memset(s, 0, sizeof(s));                             // FRAME_SYNC, an empty buffer, no frame: pocsagframer.lua:104-111
        if (upload(state, s, sizeof(s))) return -1;
        return zero_fill(carried, 2 * PG_CARRY);
    }
    // A record is written only while a batch is processed: at most one per codeword slot (the pending frame at an uncorrectable, idle or address
    // codeword or at a failed sync word, or the full record at a data word), and every slot visited is consumed, 32 bytes each, in the same
    // step.  A call consumes at most the carried bytes (at most 543) and its own n: at most (n + 543) / 32 records.
    unsigned long max_output(unsigned long n) const override { return (n + (PG_BATCH_LEN - 1)) / PG_CODEWORD; }
    long run(const void *in_dev, unsigned long n, void *out_dev, unsigned long cap) override
    {
        if (!n) return 0;
        const unsigned long bound = max_output(n);
        if (cap < bound) return set_error("pocsagframer: output capacity %lu < bound %lu", cap, bound);
        // tiles of positions over the carried bytes (at most 543) and the call
        const unsigned long nt = (n + (PG_BATCH_LEN - 1) + PS_TILE - 1) / PS_TILE;
        const size_t o_ts = (size_t)nt * PS_WORDS * 8, total = o_ts + (size_t)nt * 4;
        if (scratch.reserve(total) || h_state.reserve(sizeof(PgState))) return -1;
        char *sp = (char *)scratch.p;
        unsigned long long *mask_s = (unsigned long long *)sp;
        int *tile_s = (int *)(sp + o_ts);
        const PgState *si = (const PgState *)state.p + cur;
        PgState *so = (PgState *)state.p + (cur ^ 1);
        const uint8_t *ci = (const uint8_t *)carried.p + (size_t)cur * PG_CARRY;
        uint8_t *co = (uint8_t *)carried.p + (size_t)(cur ^ 1) * PG_CARRY;
        const uint8_t *x = (const uint8_t *)in_dev;
        hipLaunchKernelGGL(pg_match_kernel, dim3((unsigned)nt), dim3(256), 0, ctx().stream, x, ci, n, si, mask_s, tile_s);
        LR_LAUNCH_CHECK();
        hipLaunchKernelGGL(pg_walk_kernel, dim3(1), dim3(256), 0, ctx().stream, x, ci, co, n, si, so, (const unsigned long long *)mask_s, (const int *)tile_s,
                           nt, (uint32_t *)out_dev, bound);
        LR_LAUNCH_CHECK();
        cur ^= 1;
        // the data-dependent count: the one small read-back of this stage
        LR_HIP(hipMemcpyAsync(h_state.p, so, sizeof(PgState), hipMemcpyDeviceToHost, ctx().stream));
        LR_HIP(hipStreamSynchronize(ctx().stream));
        const PgState got = *(const PgState *)h_state.p;
        if (got.overflow || got.nrec > bound) return set_error("pocsagframer: %llu records exceed the bound %lu", got.nrec, bound);
        return (long)got.nrec;
    }
};

static lrhip_stage_t *pocsagframer_create(const char *op)
{
    if (strchr(op, ':')) { set_error("pocsagframer: takes no parameters, got \"%s\"", op); return nullptr; }
    if (ensure_init()) return nullptr;
    std::unique_ptr<PgStage> q(new (std::nothrow) PgStage());
    if (!q) { set_error("out of memory"); return nullptr; }
    q->in_size = 1; q->out_size = PG_REC;
    if (q->reset()) return nullptr;
    return q.release();
}
