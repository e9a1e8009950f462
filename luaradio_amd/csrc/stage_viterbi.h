// stage_viterbi.h - ConvolutionalEncoderBlock and ViterbiDecoderBlock (kernels_viterbi.h, viterbi_plan.h), created through lrhip_unary_create
// ("convenc:k=K:polys=171,133" and "viterbi:k=K:polys=171,133:input=llr|bit:scale=s:block=D:depth=L"; the polynomials are OCTAL text).
// (part of liblrhip.so; included by lrhip.hip after stage_arbresample.h, one translation unit)
#pragma once

// "k=K:polys=g0,g1,...": the checks of the code, which need no device.  false with the message set
static bool vit_read_code(const OpFields &f, VitCode &code)
{
    const char *who = f.name.c_str();
    long K = 0;
    if (!f.integer("k", LONG_MIN, LONG_MAX, K)) return false;
    if (!f.has("polys")) { set_error("%s: missing parameter \"polys\"", who); return false; }
    if (K < vitplan::K_MIN || K > vitplan::K_MAX) { set_error("%s: constraint length must be %d .. %d (got %ld)", who, vitplan::K_MIN, vitplan::K_MAX, K); return false; }
    std::vector<unsigned long> g;
    const std::string &s = f.text("polys");
    for (size_t at = 0; at <= s.size();) {
        const size_t comma = std::min(s.find(',', at), s.size());
        const std::string item = s.substr(at, comma - at);
        if (item.empty() || item.size() > 10 || item.find_first_not_of("01234567") != std::string::npos) {
            set_error("%s: bad polynomial %zu \"%.16s\" (octal digits)", who, g.size(), item.c_str());
            return false;
        }
        g.push_back(strtoul(item.c_str(), nullptr, 8));
        at = comma + 1;
    }
    if (g.size() < (size_t)vitplan::N_MIN || g.size() > (size_t)vitplan::N_MAX) {
        set_error("%s: the number of polynomials must be %d .. %d (got %zu)", who, vitplan::N_MIN, vitplan::N_MAX, g.size());
        return false;
    }
    unsigned long all = 0;
    for (unsigned long v : g) {
        if (v >> K) { set_error("%s: polynomial %lo (octal) has bits at or above the constraint length %ld", who, v, K); return false; }
        all |= v;
    }
    if (!((all >> (K - 1)) & 1)) { set_error("%s: no polynomial of %s has bit %ld set: the current input bit reaches no output", who, s.c_str(), K - 1); return false; }
    if (!(all & 1)) { set_error("%s: no polynomial of %s has bit 0 set: the constraint length is below %ld", who, s.c_str(), K); return false; }
    code.K = (int)K;
    code.n = (int)g.size();
    for (int j = 0; j < 4; j++) code.g[j] = j < code.n ? (unsigned)g[(size_t)j] : 0u;
    return true;
}

// Carried: the last K - 1 input bits (two slots of 8 bytes, ping-pong, written by the kernel).  One input bit gives n output bits
struct ConvEncStage : lrhip_stage {
    VitCode code{};
    Carried<uint8_t[8]> hist;
    const char *kind() const override { return "convenc"; }
    unsigned long max_output(unsigned long n) const override { return n > ~0ul / (unsigned long)code.n ? ~0ul : n * (unsigned long)code.n; }
    long memory() const override { return code.K - 1; }
    void rate(unsigned long *num, unsigned long *den) const override { *num = 1; *den = (unsigned long)code.n; }
    int reset() override { return hist.reset(); }
    int seek(unsigned long long n0, unsigned long long *n0_out) override
    {
        if (n0 > ~0ull / (unsigned long long)code.n) return set_error("convenc: seek to input %llu lies behind output 2^64", n0);
        if (reset()) return -1;
        *n0_out = n0 * (unsigned long long)code.n;
        return 0;
    }
    long run(const void *in_dev, unsigned long n, void *out_dev, unsigned long cap) override
    {
        if (!n) return 0;
        if (n > (unsigned long)LONG_MAX / (unsigned long)code.n) return set_error("convenc: more than 2^63 output bits in one call");
        const unsigned long n_out = n * (unsigned long)code.n;
        if (n_out > cap) return set_error("convenc: output capacity %lu < %lu", cap, n_out);
        if (!in_dev) return set_error("convenc: null input buffer");
        if (!out_dev) return set_error("convenc: null output buffer");
        hipLaunchKernelGGL(convenc_kernel, dim3(grid_for(n, 256)), dim3(256), 0, ctx().stream, (const uint8_t *)*hist.in(), (const uint8_t *)in_dev,
                           (uint8_t *)out_dev, n, code, (uint8_t *)*hist.out());
        LR_LAUNCH_CHECK();
        hist.flip();
        return (long)n_out;
    }
};

static lrhip_stage_t *convenc_create(const char *op)
{
    OpFields f;
    VitCode code{};
    if (!f.split(op, "convenc", {{"k", nullptr}, {"polys", nullptr}}, false) || !vit_read_code(f, code)) return nullptr;
    auto q = new_stage<ConvEncStage>();
    if (!q) return nullptr;
    q->code = code;
    q->in_size = q->out_size = 1;
    if (q->reset()) return nullptr;
    return q.release();
}

// Carried: the quantised inputs from the first step of the next window on (ping-pong, written by viterbi_carry_kernel), the absolute count Q of inputs
// consumed and `done` of windows emitted.  A call returns the windows that its inputs complete - from the lengths alone, nothing is read back - and
// may return 0.  The last fewer than D + L bits of a stream never leave: there is no flush
struct ViterbiStage : lrhip_stage {
    VitCode code{};
    vitplan::Shape shape{};
    bool soft = true;
    float scale = 8.0f;
    TwoSlots carry;
    uint64_t Q = 0, done = 0;
    const char *kind() const override { return "viterbi"; }
    unsigned long max_output(unsigned long n) const override { return (unsigned long)vitplan::max_output(n, shape); }
    long memory() const override { return (long)vitplan::memory(shape); }
    void rate(unsigned long *num, unsigned long *den) const override { *num = shape.n; *den = 1; }
    int reset() override { return seek_to(0); }
    // the carried inputs are erasures, q = 0, wherever the stream continues
    int seek_to(uint64_t n0)
    {
        Q = n0; done = vitplan::windows_done(n0, shape);
        return carry.reset(vitplan::carry_capacity(shape));
    }
    int seek(unsigned long long n0, unsigned long long *n0_out) override
    {
        if (seek_to(n0)) return -1;
        *n0_out = vitplan::bits_done(n0, shape);
        return 0;
    }
    template <int R>
    int decode(const void *in_dev, unsigned long n, void *out_dev, uint64_t base, long nw)
    {
        const int chunks_max = (int)((shape.D + 2 * shape.L + 63) / 64);
        const size_t per_wave = (size_t)chunks_max * R * 64 * sizeof(uint64_t);
        // four waves share a workgroup while a window takes at most 8 KiB, two up to 16 KiB per wave, above that a wave has the workgroup alone
        int waves = VIT_NT / 64;
        while (waves > 1 && waves * per_wave > 32 * 1024) waves /= 2;
        const size_t lds_bytes = per_wave * waves;
        auto go = [&](auto kern) -> int {
            const long slots = chip_slots(kern, 64 * waves, lds_bytes);
            if (slots < 0) return -1;
            const unsigned grid = persistent_grid((nw + waves - 1) / waves, slots, 0);      // a wave strides through the windows
            hipLaunchKernelGGL(kern, dim3(grid ? grid : 1), dim3(64 * waves), lds_bytes, ctx().stream, carry.in<int8_t>(), in_dev, (uint8_t *)out_dev, code,
                               shape, base, Q, (long)n, done, nw, chunks_max, scale);
            return 0;
        };
        if (soft ? go(viterbi_kernel<R, true>) : go(viterbi_kernel<R, false>)) return -1;
        LR_LAUNCH_CHECK();
        return 0;
    }
    long run(const void *in_dev, unsigned long n, void *out_dev, unsigned long cap) override
    {
        if (!n) return 0;
        if (Q + n < Q) return set_error("viterbi: more than 2^64 input values");
        const uint64_t done1 = vitplan::windows_done(Q + n, shape), nw = done1 - done;
        if (nw > (uint64_t)LONG_MAX / shape.D) return set_error("viterbi: more than 2^63 output bits in one call");
        const unsigned long n_out = (unsigned long)(nw * shape.D);
        if (n_out > cap) return set_error("viterbi: output capacity %lu < %lu", cap, n_out);
        if (!in_dev) return set_error("viterbi: null input buffer");
        if (n_out && !out_dev) return set_error("viterbi: null output buffer");
        const uint64_t base = vitplan::carry_base(done, shape), base1 = vitplan::carry_base(done1, shape);
        if (nw) {
            const int rc = code.K <= 7 ? decode<1>(in_dev, n, out_dev, base, (long)nw) : code.K == 8 ? decode<2>(in_dev, n, out_dev, base, (long)nw)
                                                                                                  : decode<4>(in_dev, n, out_dev, base, (long)nw);
            if (rc) return rc;
        }
        const unsigned count = (unsigned)(Q + n - base1);                         // below carry_capacity (viterbi_plan.h)
        auto carry_on = [&](auto kern) {
            hipLaunchKernelGGL(kern, dim3(grid_for(count, 256)), dim3(256), 0, ctx().stream, carry.in<int8_t>(), in_dev, carry.out<int8_t>(), base, Q,
                               (long)n, base1, count, scale);
        };
        if (soft) carry_on(viterbi_carry_kernel<true>); else carry_on(viterbi_carry_kernel<false>);
        LR_LAUNCH_CHECK();
        carry.flip();
        Q += n;
        done = done1;
        return (long)n_out;
    }
};

static lrhip_stage_t *viterbi_create(const char *op)
{
    OpFields f;
    VitCode code{};
    long D = 0, L = 0;
    double scale = 0.0;
    if (!f.split(op, "viterbi", {{"k", nullptr}, {"polys", nullptr}, {"input", nullptr}, {"scale", nullptr}, {"block", nullptr}, {"depth", nullptr}}, false) ||
        !vit_read_code(f, code)) return nullptr;
    const int input = f.word("input", {"llr", "bit"}, "viterbi: unsupported input \"", "\" (llr or bit)");
    if (input < 0 || !f.number("scale", scale) || !f.integer("block", LONG_MIN, LONG_MAX, D) || !f.integer("depth", LONG_MIN, LONG_MAX, L)) return nullptr;
    const float fs = (float)scale;
    if (!(fs > 0.0f) || !std::isfinite(fs)) { set_error("viterbi: scale must be a finite Float32 above 0 (got %g)", scale); return nullptr; }
    if (D < vitplan::D_MIN || D > vitplan::D_MAX) { set_error("viterbi: block must be %d .. %d decoded bits (got %ld)", vitplan::D_MIN, vitplan::D_MAX, D); return nullptr; }
    if (L < code.K - 1 || L > vitplan::L_MAX) { set_error("viterbi: depth must be %d .. %d steps (got %ld)", code.K - 1, vitplan::L_MAX, L); return nullptr; }
    const long bytes = (D + 2 * L) * (1l << (code.K - 1)) / 8;
    if (bytes > vitplan::DECISION_BYTES_MAX) {
        set_error("viterbi: the decision words of one window, (block + 2 depth) * 2^(k - 1) / 8 = %ld bytes, exceed %d: use a smaller block or depth", bytes,
                  vitplan::DECISION_BYTES_MAX);
        return nullptr;
    }
    auto q = new_stage<ViterbiStage>();
    if (!q) return nullptr;
    q->code = code;
    q->shape = vitplan::Shape{(uint32_t)code.n, (uint32_t)D, (uint32_t)L};
    q->soft = input == 0;
    q->scale = fs;
    q->in_size = q->soft ? 4 : 1; q->out_size = 1;
    if (q->reset()) return nullptr;
    return q.release();
}
