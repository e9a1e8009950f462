// stage_reedsolomon.h - ReedSolomonEncoderBlock, ReedSolomonDecoderBlock, PackBitsBlock and UnpackBitsBlock (kernels_reedsolomon.h, rs_plan.h),
// created through lrhip_unary_create ("rsenc:n=N:k=K:gfpoly=P:fcr=F:prim=R:interleave=I", "rsdec:...:status=0|1", "packbits:order=msb|lsb",
// "unpackbits:order=msb|lsb"; gfpoly is DECIMAL text, 285 = 0x11d).
// (part of liblrhip.so; included by lrhip.hip after stage_viterbi.h, one translation unit)
#pragma once

// A stage of whole frames: FI input elements give FO output elements (rs_plan.h), an element being in_size bytes in and out_size bytes out - one
// byte each for the stages of this file, four where stage_fecglue.h moves Float32.  Carried: the elements behind the last complete frame (two
// buffers, ping-pong, written by frame_carry_kernel as bytes) and the absolute count Q of inputs consumed.  A call returns the frames that its
// inputs complete - from the lengths alone, nothing is read back - and may return 0.  There is no flush
struct FramedStage : lrhip_stage {
    rsplan::Frame frame{1, 1};
    const char *who = "";
    TwoSlots carry;
    uint64_t Q = 0;
    const char *kind() const override { return who; }
    unsigned long max_output(unsigned long n) const override { return (unsigned long)rsplan::max_output(n, frame); }
    long memory() const override { return (long)rsplan::memory(frame); }
    void rate(unsigned long *num, unsigned long *den) const override
    {
        unsigned long a = frame.fi, b = frame.fo;
        while (b) { const unsigned long r = a % b; a = b; b = r; }
        *num = frame.fi / a; *den = frame.fo / a;
    }
    int reset() override { return seek_to(0); }
    // the carried bytes are zeros wherever the stream continues
    int seek_to(uint64_t n0)
    {
        Q = n0;
        return carry.reset((size_t)frame.fi * in_size);
    }
    int seek(unsigned long long n0, unsigned long long *n0_out) override
    {
        uint64_t pos = 0;
        if (!rsplan::out_position(n0, frame, &pos)) return set_error("%s: seek to input %llu lies behind output 2^64", who, n0);
        if (seek_to(n0)) return -1;
        *n0_out = pos;
        return 0;
    }
    // frames 0 .. nf - 1 of [carry | in], c elements of it carried
    virtual int launch(const uint8_t *carried, const uint8_t *in_dev, uint8_t *out_dev, uint32_t c, long nf) = 0;
    long run(const void *in_dev, unsigned long n, void *out_dev, unsigned long cap) override
    {
        if (!n) return 0;
        if (Q + n < Q) return set_error("%s: more than 2^64 input bytes", who);
        const uint32_t c = rsplan::carried(Q, frame);
        const uint64_t nf = n / frame.fi + (c + n % frame.fi) / frame.fi;
        if (nf > (uint64_t)LONG_MAX / frame.fo) return set_error("%s: more than 2^63 output bytes in one call", who);
        const unsigned long n_out = (unsigned long)(nf * frame.fo);
        if (n_out > cap) return set_error("%s: output capacity %lu < %lu", who, cap, n_out);
        if (!in_dev) return set_error("%s: null input buffer", who);
        if (n_out && !out_dev) return set_error("%s: null output buffer", who);
        const uint8_t *carried = carry.in<uint8_t>();
        if (nf && launch(carried, (const uint8_t *)in_dev, (uint8_t *)out_dev, c, (long)nf)) return -1;
        const unsigned count = rsplan::carried(Q + n, frame);
        if (count) {
            const unsigned es = (unsigned)in_size;
            hipLaunchKernelGGL(frame_carry_kernel, dim3(grid_for(count * es, 256)), dim3(256), 0, ctx().stream, carried, (const uint8_t *)in_dev,
                               carry.out<uint8_t>(), c * es, nf * frame.fi * es, count * es);
            LR_LAUNCH_CHECK();
        }
        carry.flip();
        Q += n;
        return (long)n_out;
    }
};

// "n=N:k=K:gfpoly=P:fcr=F:prim=R:interleave=I": the checks of the code, which need no device.  false with the message set
static bool rs_read_code(const OpFields &f, rsplan::Code &code)
{
    const char *who = f.name.c_str();
    long n = 0, k = 0, gfpoly = 0, fcr = 0, prim = 0, I = 0;
    if (!f.integer("n", LONG_MIN, LONG_MAX, n) || !f.integer("k", LONG_MIN, LONG_MAX, k) || !f.integer("gfpoly", LONG_MIN, LONG_MAX, gfpoly) ||
        !f.integer("fcr", LONG_MIN, LONG_MAX, fcr) || !f.integer("prim", LONG_MIN, LONG_MAX, prim) || !f.integer("interleave", LONG_MIN, LONG_MAX, I))
        return false;
    auto fits = [](long v) { return v >= -1 && v <= 65536 ? (int)v : -1; };
    code = rsplan::Code{fits(n), fits(k), fits(gfpoly), fits(fcr), fits(prim), fits(I), 0};
    switch (rsplan::check_code(code)) {
    case 0: return true;
    case 1: set_error("%s: n must be %d .. %d (got %ld)", who, rsplan::PARITY_MIN + 1, rsplan::N_MAX, n); break;
    case 2: set_error("%s: k must be 1 .. n - 2 with n - k even and %d .. %d (got n = %ld, k = %ld)", who, rsplan::PARITY_MIN, rsplan::PARITY_MAX, n, k); break;
    case 3: set_error("%s: gfpoly 0x%lx is not a primitive polynomial of degree 8", who, (unsigned long)gfpoly); break;
    case 4: set_error("%s: fcr must be 0 .. %d (got %ld)", who, rsplan::FCR_MAX, fcr); break;
    case 5: set_error("%s: prim must be 1 .. %d and coprime to 255 (got %ld)", who, rsplan::PRIM_MAX, prim); break;
    default: set_error("%s: interleave must be %d .. %d (got %ld)", who, rsplan::I_MIN, rsplan::I_MAX, I); break;
    }
    return false;
}

struct RsStage : FramedStage {
    RsParams P{};
    bool decoder = false;
    DeviceBuf tables;
    // exp, log and, for the encoder, the parity matrix as logarithms: built on the host, once
    int upload_tables(const rsplan::Code &code)
    {
        rsplan::Field field;
        rsplan::build_field(code.gfpoly, field);
        const int p = code.n - code.k, cells = decoder ? 0 : code.k * p;
        std::vector<uint8_t> host((size_t)((RS_TABLE_BYTES + 2 * cells + 15) & ~15), 0);
        memcpy(host.data(), field.exp, rsplan::EXP_SIZE);
        memcpy(host.data() + rsplan::EXP_SIZE, field.log, 512);
        if (cells) {
            std::vector<uint8_t> matrix((size_t)cells);
            rsplan::build_parity_matrix(code, field, matrix.data());
            uint16_t *logs = (uint16_t *)(host.data() + RS_TABLE_BYTES);
            for (int i = 0; i < cells; i++) logs[i] = field.log[matrix[(size_t)i]];
        }
        int w = 1;
        while ((1 << w) < p) w++;
        P = RsParams{code.n, code.k, p, p / 2, code.interleave, code.fcr, code.prim, code.status, w, (int)host.size()};
        return upload(tables, host.data(), host.size());
    }
    // a wave's LDS: the decoder's frame; the encoder's frame, the logarithms of its bytes and its parity
    int wave_bytes() const
    {
        const int fi = (int)frame.fi;
        return decoder ? (fi + 15) & ~15 : ((fi + 15) & ~15) + ((2 * fi + 15) & ~15) + ((P.I * P.p + 15) & ~15);
    }
    int launch(const uint8_t *carried, const uint8_t *in_dev, uint8_t *out_dev, uint32_t c, long nf) override
    {
        const int waves = RS_NT / 64, wb = wave_bytes();
        const size_t lds_bytes = (size_t)P.table_bytes + (size_t)waves * wb;
        auto go = [&](auto kern) -> int {
            const long slots = chip_slots(kern, RS_NT, lds_bytes);
            if (slots < 0) return -1;
            const unsigned grid = persistent_grid((nf + waves - 1) / waves, slots, 0);          // a wave strides through the frames
            hipLaunchKernelGGL(kern, dim3(grid ? grid : 1), dim3(RS_NT), lds_bytes, ctx().stream, carried, in_dev, out_dev, (const uint32_t *)tables.p, P, c, nf, wb);
            return 0;
        };
        if (decoder ? go(rsdec_kernel) : go(rsenc_kernel)) return -1;
        LR_LAUNCH_CHECK();
        return 0;
    }
};

static lrhip_stage_t *reedsolomon_create(const char *op)
{
    OpFields f;
    rsplan::Code code{};
    const bool decoder = !strncmp(op, "rsdec", 5);
    const std::vector<OpKey> enc_keys = {{"n", nullptr}, {"k", nullptr}, {"gfpoly", nullptr}, {"fcr", nullptr}, {"prim", nullptr}, {"interleave", nullptr}};
    std::vector<OpKey> dec_keys = enc_keys;
    dec_keys.push_back({"status", nullptr});
    if (!f.split(op, decoder ? "rsdec" : "rsenc", decoder ? dec_keys : enc_keys, false) || !rs_read_code(f, code)) return nullptr;
    bool status = false;
    if (decoder && !f.flag("status", status)) return nullptr;
    code.status = status;
    auto q = new_stage<RsStage>();
    if (!q) return nullptr;
    q->who = decoder ? "rsdec" : "rsenc";
    q->decoder = decoder;
    q->frame = decoder ? rsplan::decoder_frame(code) : rsplan::encoder_frame(code);
    q->in_size = q->out_size = 1;
    if (q->upload_tables(code) || q->reset()) return nullptr;
    return q.release();
}

// PackBitsBlock (frames of 8 bits, up to 7 carried) and UnpackBitsBlock (stateless, 1 : 8)
struct BitPackStage : FramedStage {
    bool pack = true, msb = true;
    int launch(const uint8_t *carried, const uint8_t *in_dev, uint8_t *out_dev, uint32_t c, long nf) override
    {
        const unsigned long n_out = (unsigned long)nf * frame.fo;
        if (pack)
            hipLaunchKernelGGL(packbits_kernel, dim3(grid_for(n_out, 256)), dim3(256), 0, ctx().stream, carried, in_dev, out_dev, c, n_out, (int)msb);
        else
            hipLaunchKernelGGL(unpackbits_kernel, dim3(grid_for(n_out, 256)), dim3(256), 0, ctx().stream, in_dev, out_dev, n_out, (int)msb);
        LR_LAUNCH_CHECK();
        return 0;
    }
};

static lrhip_stage_t *bitpack_create(const char *op)
{
    OpFields f;
    const bool pack = !strncmp(op, "packbits", 8);
    const char *who = pack ? "packbits" : "unpackbits";
    if (!f.split(op, who, {{"order", nullptr}}, false)) return nullptr;
    const std::string before = std::string(who) + ": unsupported order \"";
    const int order = f.word("order", {"msb", "lsb"}, before.c_str(), "\" (msb or lsb)");
    if (order < 0) return nullptr;
    auto q = new_stage<BitPackStage>();
    if (!q) return nullptr;
    q->who = who;
    q->pack = pack;
    q->msb = order == 0;
    q->frame = pack ? rsplan::Frame{8, 1} : rsplan::Frame{1, 8};
    q->in_size = q->out_size = 1;
    if (q->reset()) return nullptr;
    return q.release();
}
