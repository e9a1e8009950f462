// stage_phasecorr.h - BinaryPhaseCorrectorBlock (kernels_phasecorr.h), created through lrhip_unary_create("binaryphasecorrector:num_samples=N:
// sample_interval=I"); with real_out (chain_plan.h: a ComplexToRealBlock behind it) it writes the real part only, Float32.
// (part of liblrhip.so; included by lrhip.hip before stage_digital.h, one translation unit)
#pragma once

struct PhaseCorrStage : lrhip_stage {
    PcParams p;
    bool real_out = false;
    Carried<PcState> state;
    DeviceBuf ring, scratch;                 // ring: the last N q, slot = measurement index mod N
    unsigned long long off = 0;              // host mirror of PcState.off (it depends on the call lengths only): sizes the measurement passes
    const char *kind() const override { return real_out ? "binaryphasecorrector+complextoreal" : "binaryphasecorrector"; }
    // a partition seeked to s measures at the multiples of I from s on; from s + N I on every window holds measurements made after s
    long memory() const override { return (long)(p.N * p.I); }
    int start(unsigned long long first_off)
    {
        PcState s;
        memset(&s, 0, sizeof(s));
        s.off = first_off;
        s.rot[0] = (float)cos(-0.0);                        // phi_moving_average = 0.0 (binaryphasecorrector.lua:38): (1, -0)
        s.rot[1] = (float)sin(-0.0);
        off = first_off;
        if (state.reset(s)) return -1;
        return zero_fill(ring, (size_t)p.N * sizeof(unsigned long long));
    }
    int reset() override { return start(0); }
    int seek(unsigned long long n0, unsigned long long *n0_out) override
    {
        if (start((p.I - n0 % p.I) % p.I)) return -1;
        *n0_out = n0;
        return 0;
    }
    long run(const void *in_dev, unsigned long n, void *out_dev, unsigned long cap) override
    {
        if (n > cap) return set_error("%s: output capacity %lu < %lu", kind(), cap, n);
        if (!n) return 0;
        const unsigned long long M = n > off ? (n - off - 1) / p.I + 1 : 0, nt = (M + PC_TILE - 1) / PC_TILE;
        // scratch: q and rotation per measurement, tile sums and first NaNs, the call's first NaN
        const size_t o_rot = M * 8, o_sum = o_rot + M * 8, o_nan = o_sum + nt * 8, o_at = o_nan + nt * 8, total = o_at + 8;
        if (scratch.reserve(total)) return -1;
        char *sp = (char *)scratch.p;
        unsigned long long *Q = (unsigned long long *)sp, *t_sum = (unsigned long long *)(sp + o_sum), *t_nan = (unsigned long long *)(sp + o_nan),
                           *nan_at = (unsigned long long *)(sp + o_at);
        float2 *rot = (float2 *)(sp + o_rot);
        unsigned long long *rg = (unsigned long long *)ring.p;
        const PcState *si = state.in();
        PcState *so = state.out();
        const float2 *x = (const float2 *)in_dev;
        if (M) {
            hipLaunchKernelGGL(pc_measure_kernel, dim3((unsigned)nt), dim3(256), 0, ctx().stream, x, M, p, si, (const unsigned long long *)rg, Q, t_sum, t_nan);
            LR_LAUNCH_CHECK();
        }
        hipLaunchKernelGGL(pc_carry_kernel, dim3(1), dim3(256), 0, ctx().stream, t_sum, (const unsigned long long *)t_nan, nt, M, (unsigned long long)n, p, si, so,
                           nan_at);
        LR_LAUNCH_CHECK();
        if (M) {
            hipLaunchKernelGGL(pc_window_kernel, dim3((unsigned)nt), dim3(256), 0, ctx().stream, (const unsigned long long *)Q, (const unsigned long long *)rg,
                               (const unsigned long long *)t_sum, (const unsigned long long *)nan_at, M, p, si, so, rot);
            LR_LAUNCH_CHECK();
        }
        const bool vec = ((((uintptr_t)in_dev) | ((uintptr_t)out_dev)) & 15) == 0;
        const unsigned long long items = vec ? (n + 1) / 2 : n;
        const unsigned grid = grid_for(items, 256);
#define LR_PC(V, R)                                                                                                                                         \
    hipLaunchKernelGGL((pc_rotate_kernel<V, R>), dim3(grid), dim3(256), 0, ctx().stream, x, out_dev, (unsigned long long)n, items, M, p, si,                   \
                       (const float2 *)rot, (const unsigned long long *)Q, rg)
        if (vec && real_out) LR_PC(2, true);
        else if (vec) LR_PC(2, false);
        else if (real_out) LR_PC(1, true);
        else LR_PC(1, false);
#undef LR_PC
        LR_LAUNCH_CHECK();
        state.flip();
        off = off + M * p.I - n;
        return (long)n;
    }
};

// "binaryphasecorrector:num_samples=N[:sample_interval=I]" (binaryphasecorrector.lua:28-33: I defaults to 32)
static lrhip_stage_t *phasecorr_create(const char *op)
{
    OpFields f;
    double N = 0.0, I = 0.0;
    if (!f.split(op, "binaryphasecorrector", {{"num_samples", nullptr}, {"sample_interval", "32"}}, true) || !f.number("num_samples", N) ||
        !f.number("sample_interval", I)) return nullptr;
    if (!(N >= 1.0 && N <= 16777216.0) || N != floor(N)) { set_error("binaryphasecorrector: num_samples must be an integer in [1, 2^24]"); return nullptr; }
    if (!(I >= 1.0 && I <= 2147483648.0) || I != floor(I)) { set_error("binaryphasecorrector: sample_interval must be an integer in [1, 2^31]"); return nullptr; }
    auto q = new_stage<PhaseCorrStage>();
    if (!q) return nullptr;
    q->p.N = (unsigned long long)N;
    q->p.I = (unsigned long long)I;
    int c = 0;                                               // ceil(log2(2N))
    while ((1ull << c) < 2 * q->p.N) c++;
    const int s = 61 - c < 52 ? 61 - c : 52;
    q->p.scale = ldexp(1.0, s);
    q->p.den = (double)q->p.N * q->p.scale;
    q->in_size = q->out_size = 8;
    if (q->reset()) return nullptr;
    return q.release();
}
