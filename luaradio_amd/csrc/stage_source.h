// stage_source.h - SignalSource and UniformRandomSource (kernels_source.h), created through lrhip_unary_create:
//   "signalsource:signal=exponential|cosine|sine|square|triangle|sawtooth|constant:frequency=F:rate=R:amplitude=A:phase=P:offset=O"  (doubles, %.17g)
//   "uniformrandomsource:type=cf32|f32|byte|bit:lo=L:hi=H:seed=S"                                                                     (S a decimal uint64)
// The first stages WITHOUT an input: in_size = 0 (lrhip_stage::is_source()), run(in, n, ...) ignores `in` and generates n samples from the stage's
// absolute index, which is all the state there is - reset() puts it back to 0, seek(n0) sets it, memory() is 0 and any cut of the stream gives the same
// bits.  A chain takes a source as its first stage only (lrhip_chain_create_ex), where it runs as a launch of its own.
// (part of liblrhip.so; included by lrhip.hip after stage_modulator.h, one translation unit)
#pragma once

struct SourceStage : lrhip_stage {
    bool random = false;
    int sig = SRC_CONSTANT;                  // SRC_* (signalsource)
    uint64_t p0 = 0, step = 0;               // phase and frequency / rate as 0.64 fixed-point turns
    double amp = 1.0, off = 0.0;
    int rtype = RND_F32;                     // RND_* (uniformrandomsource)
    RndParams rnd{};
    unsigned long long index = 0;            // absolute index of the next sample
    const char *kind() const override { return random ? "uniformrandomsource" : "signalsource"; }
    int reset() override { index = 0; return 0; }
    int seek(unsigned long long n0, unsigned long long *n0_out) override
    {
        index = n0;
        *n0_out = n0;
        return 0;
    }
    template <typename G>
    int launch(const G &g, void *out_dev, unsigned long n)
    {
        typedef typename G::T T;
        if ((uintptr_t)out_dev % 16) {
            hipLaunchKernelGGL(source_scalar_kernel<G>, dim3(grid_for(n, 256)), dim3(256), 0, ctx().stream, (T *)out_dev, g, (uint64_t)index, n);
            LR_LAUNCH_CHECK();
            return 0;
        }
        const unsigned long nitems = n / G::PER;
        hipLaunchKernelGGL(source_vec_kernel<G>, dim3(grid_for(nitems + 1, 256 * SRC_U)), dim3(256), 0, ctx().stream, (float4 *)out_dev, g, (uint64_t)index,
                           nitems, n);
        LR_LAUNCH_CHECK();
        return 0;
    }
    template <int SIG> int launch_sig(void *out_dev, unsigned long n) { return launch(SigGen<SIG>{p0, step, amp, off}, out_dev, n); }
    long run(const void *, unsigned long n, void *out_dev, unsigned long cap) override
    {
        if (!n) return 0;
        if (n > cap) return set_error("%s: output capacity %lu < %lu", kind(), cap, n);
        if (!out_dev) return set_error("%s: null output buffer", kind());
        int rc;
        if (random) {
            rc = rtype == RND_CF32 ? launch(RndCf32Gen{rnd}, out_dev, n) : rtype == RND_F32 ? launch(RndF32Gen{rnd}, out_dev, n)
               : rtype == RND_BYTE ? launch(RndSmallGen<RND_BYTE>{rnd}, out_dev, n) : launch(RndSmallGen<RND_BIT>{rnd}, out_dev, n);
        } else {
            switch (sig) {
                case SRC_EXPONENTIAL: rc = launch(ExpGen{p0, step, amp}, out_dev, n); break;
                case SRC_COSINE: rc = launch_sig<SRC_COSINE>(out_dev, n); break;
                case SRC_SINE: rc = launch_sig<SRC_SINE>(out_dev, n); break;
                case SRC_SQUARE: rc = launch_sig<SRC_SQUARE>(out_dev, n); break;
                case SRC_TRIANGLE: rc = launch_sig<SRC_TRIANGLE>(out_dev, n); break;
                case SRC_SAWTOOTH: rc = launch_sig<SRC_SAWTOOTH>(out_dev, n); break;
                default: rc = launch_sig<SRC_CONSTANT>(out_dev, n); break;
            }
        }
        if (rc) return rc;
        index += n;
        return (long)n;
    }
};

// x as a fraction of a turn in 0.64 fixed point: uint64(rint(ldexp(x - floor(x), 64))) mod 2^64
static uint64_t source_turns(double x)
{
    const double f = std::rint(std::ldexp(x - std::floor(x), 64));
    return f >= 18446744073709551616.0 ? 0ull : (uint64_t)f;
}

static lrhip_stage_t *source_create(const char *op)
{
    OpFields f;
    const bool random = !strncmp(op, "uniformrandomsource", 19);
    if (random ? !f.split(op, nullptr, {{"type", nullptr}, {"lo", nullptr}, {"hi", nullptr}, {"seed", nullptr}}, false)
               : !f.split(op, nullptr, {{"signal", nullptr}, {"frequency", nullptr}, {"rate", nullptr}, {"amplitude", nullptr}, {"phase", nullptr}, {"offset", nullptr}}, false))
        return nullptr;
    const std::string &name = f.name;
    std::unique_ptr<SourceStage> q(new (std::nothrow) SourceStage());
    if (!q) { set_error("out of memory"); return nullptr; }
    q->random = random;
    q->in_size = 0;
    if (!random) {
        const int sig = f.word("signal", {"exponential", "cosine", "sine", "square", "triangle", "sawtooth", "constant"},       // the order of SRC_*
                               "Unsupported signal (\"", "\")");                                                                 // signal.lua:50
        if (sig < 0) return nullptr;
        double frequency, rate, phase;
        if (!f.number("frequency", frequency, true) || !f.number("rate", rate, true) || !f.number("amplitude", q->amp, true) ||
            !f.number("phase", phase, true) || !f.number("offset", q->off, true)) return nullptr;
        if (!(rate > 0.0)) { set_error("%s: rate must be positive", name.c_str()); return nullptr; }
        q->sig = sig;
        q->step = source_turns(frequency / rate);
        q->p0 = source_turns(phase / 6.283185307179586);
        q->out_size = sig == SRC_EXPONENTIAL ? 8 : 4;
    } else {
        const int t = f.word("type", {"cf32", "f32", "byte", "bit"}, "uniformrandomsource: unsupported type \"", "\" (cf32, f32, byte or bit)");      // the order of RND_*
        if (t < 0) return nullptr;
        double lo, hi;
        if (!f.number("lo", lo, true) || !f.number("hi", hi, true)) return nullptr;
        if (lo > hi) { set_error("%s: lo must not exceed hi", name.c_str()); return nullptr; }
        uint64_t seed = 0;
        if (!f.u64("seed", seed)) return nullptr;
        q->rtype = t;
        q->rnd.seed = seed;
        q->rnd.lo = lo;
        q->rnd.span = hi - lo;
        if (!std::isfinite(q->rnd.span)) { set_error("%s: hi - lo must be finite", name.c_str()); return nullptr; }
        if (t == RND_BYTE) {
            if (lo < 0.0 || hi > 255.0 || lo != std::floor(lo) || hi != std::floor(hi)) { set_error("%s: a Byte range is two integers in 0 .. 255", name.c_str()); return nullptr; }
            q->rnd.blo = (uint32_t)lo;
            q->rnd.bcount = (uint32_t)(hi - lo) + 1u;
        }
        q->out_size = t == RND_CF32 ? 8 : t == RND_F32 ? 4 : 1;
    }
    if (ensure_init()) return nullptr;
    return q.release();
}
