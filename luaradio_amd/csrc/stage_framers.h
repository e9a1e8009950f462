// stage_framers.h - the five framers, created through lrhip_unary_create (no parameters, plain_create of stage_counted.h): Bit in, one fixed
// record per frame out (include/lrhip.h).
//   "rdsframer"                                   RDSFramerBlock (kernels_rdsframer.h): uint16_t blocks[4], 8 bytes
//   "scmframer", "scmplusframer", "idmframer"     SCMFramerBlock, SCMPlusFramerBlock, IDMFramerBlock (kernels_ertframer.h): 16, 16 and 88 bytes
//   "ax25framer"                                  AX25FramerBlock (kernels_ax25framer.h): struct lrhip_ax25_frame, 416 bytes
//   "pocsagframer"                                POCSAGFramerBlock (kernels_pocsagframer.h): struct lrhip_pocsag_frame, 256 bytes.  The stage is
//                                                 eager: its output does not depend on how the stream is cut into calls.  reset() drops the
//                                                 pending frame and the buffered bytes.
// The output count depends on the data: run() returns the exact count, read back from the device after the last pass (one small synchronous copy
// per call), and memory() = -1.  What each stage keeps of its own is its bound, the tables of its reset() and its launches.
// (part of liblrhip.so; included by lrhip.hip after stage_preamble.h, one translation unit)
#pragma once

struct RfStage : lrhip_stage {
    DeviceBuf table, scratch;
    Carried<RfState, RF_CARRY> st;                           // an empty frame buffer, rdsframer.lua:96-98
    const char *kind() const override { return "rdsframer"; }
    long memory() const override { return -1; }
    int reset() override
    {
        uint8_t flags[1024];
        rf_flag_table(flags);
        return upload(table, flags, sizeof(flags)) ? -1 : st.reset();
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
        const RfScratch sc(nt, bound);
        if (scratch.reserve(sc.total)) return -1;
        unsigned long long *mask_v = sc.mask_v.in(scratch);
        int *tile_v = sc.tile_v.in(scratch);
        long long *starts = sc.starts.in(scratch);
        const RfState *si = st.in();
        RfState *so = st.out();
        const uint8_t *x = (const uint8_t *)in_dev;
        hipLaunchKernelGGL(rf_match_kernel, dim3((unsigned)nt), dim3(256), 0, ctx().stream, x, st.ci(), n, si, (const uint8_t *)table.p, mask_v, tile_v);
        LR_LAUNCH_CHECK();
        hipLaunchKernelGGL(rf_walk_kernel, dim3(1), dim3(256), 0, ctx().stream, (const unsigned long long *)mask_v, (const int *)tile_v, nt, n, si, so, starts,
                           bound);
        LR_LAUNCH_CHECK();
        hipLaunchKernelGGL(rf_emit_kernel, dim3((unsigned)((bound + 255) / 256)), dim3(256), 0, ctx().stream, x, st.ci(), st.co(), n, si, (const RfState *)so,
                           (const long long *)starts, (unsigned long long *)out_dev, cap);
        LR_LAUNCH_CHECK();
        st.flip();
        RfState got;
        if (st.fetch(got)) return -1;
        if (got.overflow || got.count > bound) return set_error("rdsframer: %llu frames exceed the bound %lu", got.count, bound);
        return (long)got.count;
    }
};

template <int K> struct EfStage : lrhip_stage {
    typedef EfProto<K> P;
    DeviceBuf rows, scratch;
    Carried<EfState, EF_CARRY> st;                           // an empty frame buffer
    const char *kind() const override { return K == EF_SCM ? "scmframer" : K == EF_SCMPLUS ? "scmplusframer" : "idmframer"; }
    long memory() const override { return -1; }
    int reset() override
    {
        uint16_t r[P::CW];
        ef_rows(K, r);
        return upload(rows, r, sizeof(r)) ? -1 : st.reset();
    }
    // accepted frames are disjoint windows of L bits inside "carried bits, then the call": at most (L - 1 + n) / L of them
    unsigned long max_output(unsigned long n) const override { return (n + (P::L - 1)) / P::L; }
    long run(const void *in_dev, unsigned long n, void *out_dev, unsigned long cap) override
    {
        if (!n) return 0;
        const unsigned long bound = max_output(n);
        if (cap < bound) return set_error("%s: output capacity %lu < bound %lu", kind(), cap, bound);
        // tiles of window starts over the carried bytes (at most L - 1) and the call
        const unsigned long nt = (n + (P::L - 1) + PS_TILE - 1) / PS_TILE;
        const EfScratch sc(nt, bound);
        if (scratch.reserve(sc.total)) return -1;
        unsigned long long *mask_e = sc.mask_e.in(scratch), *mask_a = sc.mask_a.in(scratch);
        int *tile_e = sc.tile_e.in(scratch);
        long long *starts = sc.starts.in(scratch);
        const EfState *si = st.in();
        EfState *so = st.out();
        const uint8_t *x = (const uint8_t *)in_dev;
        const uint16_t *rw = (const uint16_t *)rows.p;
        unsigned long long *y = (unsigned long long *)out_dev;
        hipLaunchKernelGGL(ef_match_kernel<K>, dim3((unsigned)nt), dim3(256), 0, ctx().stream, x, st.ci(), n, si, rw, mask_e, mask_a, tile_e);
        LR_LAUNCH_CHECK();
        hipLaunchKernelGGL(ef_walk_kernel<K>, dim3(1), dim3(256), 0, ctx().stream, x, st.ci(), st.co(), n, si, so, rw, (const unsigned long long *)mask_e,
                           (const unsigned long long *)mask_a, (const int *)tile_e, nt, starts, y, bound);
        LR_LAUNCH_CHECK();
        // one wave per frame, four to a workgroup
        hipLaunchKernelGGL(ef_emit_kernel<K>, dim3((unsigned)((bound + 3) / 4)), dim3(256), 0, ctx().stream, x, st.ci(), n, si, (const EfState *)so, rw,
                           (const long long *)starts, y, cap);
        LR_LAUNCH_CHECK();
        st.flip();
        EfState got;
        if (st.fetch(got)) return -1;
        if (got.overflow || got.count > bound) return set_error("%s: %llu frames exceed the bound %lu", kind(), got.count, bound);
        return (long)got.count;
    }
};

struct AxStage : lrhip_stage {
    DeviceBuf rows, scratch;
    Carried<AxState, AX_CARRY> st;                           // IDLE with an empty byte buffer, ax25framer.lua:85-90
    const char *kind() const override { return "ax25framer"; }
    long memory() const override { return -1; }
    int reset() override
    {
        std::vector<uint16_t> r(AX_CRC_ROWS);
        ax_crc_rows(r.data());
        return upload(rows, r.data(), r.size() * sizeof(uint16_t)) ? -1 : st.reset();
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
        const AxScratch sc(nt, max_flags, bound);
        if (scratch.reserve(sc.total)) return -1;
        unsigned long long *mask_f = sc.mask_f.in(scratch), *segs = sc.segs.in(scratch);
        int *tile_f = sc.tile_f.in(scratch);
        long long *flags = sc.flags.in(scratch);
        uint8_t *valid = sc.valid.in(scratch);
        const AxState *si = st.in();
        AxState *so = st.out();
        const uint8_t *x = (const uint8_t *)in_dev;
        const uint16_t *rw = (const uint16_t *)rows.p;
        hipLaunchKernelGGL(ax_match_kernel, dim3((unsigned)nt), dim3(256), 0, ctx().stream, x, st.ci(), n, si, mask_f, tile_f);
        LR_LAUNCH_CHECK();
        hipLaunchKernelGGL(ax_walk_kernel, dim3(1), dim3(256), 0, ctx().stream, (const unsigned long long *)mask_f, (const int *)tile_f, nt, n, si, so, flags,
                           max_flags);
        LR_LAUNCH_CHECK();
        // one wave per segment / per frame, grid-stride
        const unsigned long eval_grid = max_flags < 4096 ? max_flags : 4096, emit_grid = bound < 4096 ? bound : 4096;
        hipLaunchKernelGGL(ax_eval_kernel, dim3((unsigned)eval_grid), dim3(64), 0, ctx().stream, x, st.ci(), si, (const AxState *)so, rw, (const long long *)flags,
                           valid);
        LR_LAUNCH_CHECK();
        hipLaunchKernelGGL(ax_select_kernel, dim3(1), dim3(256), 0, ctx().stream, x, st.ci(), st.co(), n, si, so, (const long long *)flags, (const uint8_t *)valid,
                           segs, bound);
        LR_LAUNCH_CHECK();
        hipLaunchKernelGGL(ax_emit_kernel, dim3((unsigned)emit_grid), dim3(64), 0, ctx().stream, x, st.ci(), si, (const AxState *)so, rw, (const long long *)flags,
                           (const unsigned long long *)segs, (uint32_t *)out_dev, cap);
        LR_LAUNCH_CHECK();
        st.flip();
        AxState got;
        if (st.fetch(got)) return -1;
        if (got.overflow || got.count > bound) return set_error("ax25framer: %llu frames exceed the bound %lu", got.count, bound);
        return (long)got.count;
    }
};

struct PgStage : lrhip_stage {
    DeviceBuf scratch;
    Carried<PgState, PG_CARRY> st;                           // FRAME_SYNC, an empty buffer, no frame: pocsagframer.lua:104-111
    const char *kind() const override { return "pocsagframer"; }
    long memory() const override { return -1; }
    int reset() override { return st.reset(); }
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
        const PgScratch sc(nt);
        if (scratch.reserve(sc.total)) return -1;
        unsigned long long *mask_s = sc.mask_s.in(scratch);
        int *tile_s = sc.tile_s.in(scratch);
        const PgState *si = st.in();
        PgState *so = st.out();
        const uint8_t *x = (const uint8_t *)in_dev;
        hipLaunchKernelGGL(pg_match_kernel, dim3((unsigned)nt), dim3(256), 0, ctx().stream, x, st.ci(), n, si, mask_s, tile_s);
        LR_LAUNCH_CHECK();
        hipLaunchKernelGGL(pg_walk_kernel, dim3(1), dim3(256), 0, ctx().stream, x, st.ci(), st.co(), n, si, so, (const unsigned long long *)mask_s,
                           (const int *)tile_s, nt, (uint32_t *)out_dev, bound);
        LR_LAUNCH_CHECK();
        st.flip();
        PgState got;
        if (st.fetch(got)) return -1;
        if (got.overflow || got.nrec > bound) return set_error("pocsagframer: %llu records exceed the bound %lu", got.nrec, bound);
        return (long)got.nrec;
    }
};
