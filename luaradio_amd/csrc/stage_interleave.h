// stage_interleave.h - the four many-ported stages (kernels_interleave.h), created through lrhip_unary_create:
//   "interleave:channels=N:size=4|8"     N inputs -> one output, out[N i + k] = in_k[i]; returns N n elements
//   "deinterleave:channels=N:size=4|8"   one input -> N outputs, out_j[i] = in[N i + j]; port j receives ceil((n - j) / N), returns port 0's count
//   "wavpack:channels=N:bits=8|16|32"    N Float32 inputs -> records of N raw samples (u8 / s16le / s32le); returns n records
//   "wavunpack:channels=N:bits=8|16|32"  records of N raw samples -> N Float32 outputs; returns n
// They run through lrhip_stage_execute_device alone.  The many-ported side of the call is a PORT TABLE in HOST memory (include/lrhip.h):
// { uint32 magic; uint32 count; void *ptr[count]; }, read and checked here on the host; the pointers travel to the kernel by value in its argument
// block, so nothing is copied to the device and no device-side table exists.  All four are stateless (DeinterleaveBlock's carried index lives in its
// Python block, which rotates the table), memory() = 0, and they fuse with nothing: lrhip_chain_create* and the host-buffer entry points refuse them.
// (part of liblrhip.so; included by lrhip.hip after stage_digital.h, one translation unit)
#pragma once

constexpr uint32_t LRHIP_PORT_TABLE_MAGIC = 0x5450524cu;      // "LRPT" in memory

// Interleave of two channels with every pointer 16-byte aligned: the register-only kernel against the LDS transpose, MI355X, 2^24 frames,
// tools/bench_interleave.py (profiles/interleave_table.jsonl, rows "interleave2-reg" / "interleave2-lds", each in a process of its own):
//   Float32 0.0401 against 0.0436 ms, ComplexFloat32 0.0964 against 0.0970 ms (a copy of the same bytes: 0.0375 / 0.108 ms)
// so the register form is the default there; LRHIP_INTERLEAVE2_REG=0 is the A/B knob.  Any other alignment takes the LDS transpose.
static bool interleave2_reg_default() { return true; }

struct PortStage : lrhip_stage {
    enum Kind { INTERLEAVE, DEINTERLEAVE, WAVPACK, WAVUNPACK } what = INTERLEAVE;
    unsigned N = 2;
    int form = IL_COPY4;          // IL_* of kernels_interleave.h
    const char *kind() const override { return what == INTERLEAVE ? "interleave" : what == DEINTERLEAVE ? "deinterleave" : what == WAVPACK ? "wavpack" : "wavunpack"; }
    bool many_in() const { return what == INTERLEAVE || what == WAVPACK; }
    int reset() override { return 0; }
    unsigned long max_output(unsigned long n) const override { return what == INTERLEAVE ? n * N : what == DEINTERLEAVE ? (n + N - 1) / N : n; }
    void rate(unsigned long *num, unsigned long *den) const override
    {
        *num = what == DEINTERLEAVE ? N : 1;
        *den = what == INTERLEAVE ? N : 1;
    }
    unsigned words() const { return form == IL_COPY8 ? 2u : 1u; }
    double offset() const { return form == IL_U8 ? 127.5 : 0.0; }                                   // format_utils.lua:82-97: u8, s16le, s32le
    double scale() const { return form == IL_U8 ? 127.5 : form == IL_S16 ? 32767.5 : 2147483647.5; }

    // the table, read on the host: false + lrhip_strerror unless it is one of this stage's
    bool read_table(const void *table, IlPorts &ports, unsigned &aligned) const
    {
        uint32_t head[2];
        memcpy(head, table, sizeof head);
        if (head[0] != LRHIP_PORT_TABLE_MAGIC) { set_error("%s: the %s buffer is not a port table (magic 0x%08x, expected 0x%08x)", kind(), many_in() ? "input" : "output", head[0], LRHIP_PORT_TABLE_MAGIC); return false; }
        if (head[1] != N) { set_error("%s: the port table has %u ports, the stage has %u channels", kind(), head[1], N); return false; }
        aligned = 0;
        for (unsigned k = 0; k < (unsigned)IL_MAX_CH; k++) ports.p[k] = nullptr;
        for (unsigned k = 0; k < N; k++) {
            void *p;
            memcpy(&p, (const char *)table + 8 + k * sizeof(void *), sizeof p);
            if (!p) { set_error("%s: port %u of the port table is null", kind(), k); return false; }
            ports.p[k] = p;
            if ((uintptr_t)p % 16 == 0) aligned |= 1u << k;
        }
        return true;
    }

    long run(const void *in_dev, unsigned long n, void *out_dev, unsigned long cap) override
    {
        const void *table = many_in() ? in_dev : out_dev;
        if (!table) return n ? set_error("null buffer") : 0;
        IlPorts ports;
        unsigned aligned = 0;
        if (!read_table(table, ports, aligned)) return -1;
        const unsigned long n_out = what == INTERLEAVE ? n * N : what == DEINTERLEAVE ? (n + N - 1) / N : n;
        if (n_out > cap) return set_error("%s: output capacity %lu < %lu", kind(), cap, n_out);
        if (!n) return 0;
        if (many_in() ? !out_dev : !in_dev) return set_error("null buffer");
        const unsigned F = il_tile_frames(N, words());
        const unsigned long frames = what == DEINTERLEAVE ? (n + N - 1) / N : n;
        const unsigned long tiles = (frames + F - 1) / F;
        if (tiles > 0x7fffffffUL) return set_error("%s: %lu frames exceed one launch", kind(), frames);
        const dim3 grid((unsigned)tiles), block(IL_THREADS);
        const double off = offset(), sc = scale();
        if (many_in()) {
            const unsigned a_out = (uintptr_t)out_dev % 16 == 0;
            static const char *knob = getenv("LRHIP_INTERLEAVE2_REG");      // A/B knob
            const bool reg2 = knob ? atoi(knob) != 0 : interleave2_reg_default();
            if (reg2 && what == INTERLEAVE && N == 2 && aligned == 3u && a_out) {
                const unsigned long nitems = n / (4 / words());
                const dim3 g2(grid_for(nitems + 1, IL_THREADS));
                if (form == IL_COPY8) hipLaunchKernelGGL(interleave2_reg_kernel<2>, g2, block, 0, ctx().stream, (const uint32_t *)ports.p[0], (const uint32_t *)ports.p[1], (uint32_t *)out_dev, nitems, n);
                else hipLaunchKernelGGL(interleave2_reg_kernel<1>, g2, block, 0, ctx().stream, (const uint32_t *)ports.p[0], (const uint32_t *)ports.p[1], (uint32_t *)out_dev, nitems, n);
                LR_LAUNCH_CHECK();
                return (long)n_out;
            }
#define LR_IL(M) hipLaunchKernelGGL(interleave_kernel<M>, grid, block, 0, ctx().stream, ports, out_dev, n, N, aligned, a_out, off, sc)
            switch (form) {
                case IL_COPY4: LR_IL(IL_COPY4); break;
                case IL_COPY8: LR_IL(IL_COPY8); break;
                case IL_U8: LR_IL(IL_U8); break;
                case IL_S16: LR_IL(IL_S16); break;
                default: LR_IL(IL_S32); break;
            }
#undef LR_IL
        } else {
            const unsigned a_in = (uintptr_t)in_dev % 16 == 0;
            const unsigned long elems = what == DEINTERLEAVE ? n : n * N;      // wavunpack: n whole records
#define LR_DL(M) hipLaunchKernelGGL(deinterleave_kernel<M>, grid, block, 0, ctx().stream, in_dev, ports, elems, N, a_in, aligned, off, sc)
            switch (form) {
                case IL_COPY4: LR_DL(IL_COPY4); break;
                case IL_COPY8: LR_DL(IL_COPY8); break;
                case IL_U8: LR_DL(IL_U8); break;
                case IL_S16: LR_DL(IL_S16); break;
                default: LR_DL(IL_S32); break;
            }
#undef LR_DL
        }
        LR_LAUNCH_CHECK();
        return (long)n_out;
    }
};

static lrhip_stage_t *port_stage_create(const char *op)
{
    OpFields f;
    const bool wav = !strncmp(op, "wav", 3);
    const char *second = wav ? "bits" : "size";
    double ch = 0.0, sz = 0.0;
    if (!f.split(op, nullptr, {{"channels", nullptr}, {second, nullptr}}, true) || !f.number("channels", ch) || !f.number(second, sz)) return nullptr;
    const std::string &name = f.name;
    const int lo = wav ? 1 : 2;
    if (!(ch >= lo && ch <= IL_MAX_CH) || ch != std::floor(ch)) { set_error("%s: channels must be an integer in %d .. %d (got %g)", name.c_str(), lo, IL_MAX_CH, ch); return nullptr; }
    if (wav ? (sz != 8 && sz != 16 && sz != 32) : (sz != 4 && sz != 8)) {
        set_error(wav ? "%s: bits must be 8, 16 or 32 (got %g)" : "%s: size must be 4 or 8 (got %g)", name.c_str(), sz);
        return nullptr;
    }
    auto q = new_stage<PortStage>();
    if (!q) return nullptr;
    q->what = name == "interleave" ? PortStage::INTERLEAVE : name == "deinterleave" ? PortStage::DEINTERLEAVE : name == "wavpack" ? PortStage::WAVPACK : PortStage::WAVUNPACK;
    q->N = (unsigned)ch;
    if (!wav) {
        q->form = sz == 8 ? IL_COPY8 : IL_COPY4;
        q->in_size = q->out_size = (int)sz;
    } else {
        q->form = sz == 8 ? IL_U8 : sz == 16 ? IL_S16 : IL_S32;
        const int record = (int)q->N * (int)sz / 8;
        q->in_size = q->what == PortStage::WAVPACK ? 4 : record;
        q->out_size = q->what == PortStage::WAVPACK ? record : 4;
    }
    return q.release();
}
