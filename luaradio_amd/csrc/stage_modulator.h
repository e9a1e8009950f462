// stage_modulator.h - PulseAmplitudeModulatorBlock and QuadratureAmplitudeModulatorBlock (kernels_modulator.h), created through lrhip_unary_create
// ("pam:period=P:bits=b:msb=0|1:table=a0,a1,..." and "qam:...:table=re0,im0,re1,im1,...").  The output count is a function of the lengths only
// ((pending + n) / b symbols of P samples), so run() reads nothing back; the up to b - 1 pending bits stay on the device.
// (part of liblrhip.so; included by lrhip.hip after stage_preamble.h, one translation unit)
#pragma once

struct ModStage : lrhip_stage {
    unsigned P = 1;
    int b = 1, msb = 1;
    bool qam = false;
    DeviceBuf d_table;                       // 2^b entries, Float32 (pam) or interleaved ComplexFloat32 (qam)
    Carried<uint8_t[MOD_MAX_BITS]> carry;    // the pending bits, a byte each
    int pend = 0;                            // bits carried from the calls so far (< b)
    const char *kind() const override { return qam ? "qam" : "pam"; }
    int reset() override
    {
        pend = 0;
        return carry.reset();
    }
    // a call completes at most ceil(n / b) symbols whatever is pending
    unsigned long max_output(unsigned long n) const override { return ((n + (unsigned long)b - 1) / (unsigned long)b) * P; }
    void rate(unsigned long *num, unsigned long *den) const override { *num = (unsigned long)b; *den = P; }
    unsigned long align() const override { return (unsigned long)b; }
    // a partition can start only between two symbols: inside one, the bits the previous partition holds back are unknown here
    int seek(unsigned long long n0, unsigned long long *n0_out) override
    {
        if (n0 % (unsigned long long)b) return set_error("%s: seek to bit %llu is inside a symbol of %d bits", kind(), n0, b);
        if (reset()) return -1;
        *n0_out = n0 / (unsigned long long)b * P;
        return 0;
    }
    template <typename T, int PER>
    int launch(const uint8_t *x, const ModParams &p, void *out_dev, unsigned long n_out)
    {
        const uint8_t *ci = *carry.in();
        uint8_t *co = *carry.out();
        const T *tab = (const T *)d_table.p;
        if ((uintptr_t)out_dev % 16) {
            hipLaunchKernelGGL(mod_scalar_kernel<T>, dim3(grid_for(n_out, 256)), dim3(256), 0, ctx().stream, x, ci, co, tab, (T *)out_dev, p, n_out);
            LR_LAUNCH_CHECK();
            return 0;
        }
        const unsigned long nitems = n_out / PER;
        const dim3 grid(grid_for(nitems + 1, 256 * MOD_U));
        float4 *y = (float4 *)out_dev;
        if (P > 1) hipLaunchKernelGGL((mod_hold_kernel<T, PER>), grid, dim3(256), 0, ctx().stream, x, ci, co, tab, y, p, nitems, n_out);
        else hipLaunchKernelGGL((mod_map_kernel<T, PER>), grid, dim3(256), 0, ctx().stream, x, ci, co, tab, y, p, nitems, n_out);
        LR_LAUNCH_CHECK();
        return 0;
    }
    long run(const void *in_dev, unsigned long n, void *out_dev, unsigned long cap) override
    {
        if (!n) return 0;
        const unsigned long nsym = ((unsigned long)pend + n) / (unsigned long)b, n_out = nsym * P;
        if (n_out > cap) return set_error("%s: output capacity %lu < %lu", kind(), cap, n_out);
        const ModParams p{P, b, msb, pend, n, nsym};
        // (a call that completes no symbol still runs: its bits join the carried ones)
        const int rc = qam ? launch<float2, 2>((const uint8_t *)in_dev, p, out_dev, n_out) : launch<float, 4>((const uint8_t *)in_dev, p, out_dev, n_out);
        if (rc) return rc;
        pend = (int)((unsigned long)pend + n - nsym * (unsigned long)b);
        carry.flip();
        return (long)n_out;
    }
};

static ModStage *modulator_build(bool qam, unsigned P, int b, int msb, const std::vector<float> &table)
{
    auto q = new_stage<ModStage>();
    if (!q) return nullptr;
    q->qam = qam; q->P = P; q->b = b; q->msb = msb;
    q->in_size = 1; q->out_size = qam ? 8 : 4;
    if (upload(q->d_table, table.data(), table.size() * sizeof(float)) || q->reset()) return nullptr;
    return q.release();
}

// "pam:period=P:bits=b:msb=0|1:table=v,v,...": P, b integers; the table 2^b Float32 values (pam) or 2^b re,im pairs (qam) as decimal (%.9g) or
// hexadecimal floating-point text, each read with strtod and rounded to Float32 - both forms give back the Float32 they were printed from
static lrhip_stage_t *modulator_create(const char *op)
{
    OpFields f;
    long P = 0, b = 0, msb = 0;
    std::vector<float> table;
    if (!f.split(op, nullptr, {{"period", nullptr}, {"bits", nullptr}, {"msb", nullptr}, {"table", nullptr}}, false) ||
        !f.integer("period", LONG_MIN, LONG_MAX, P) || !f.integer("bits", LONG_MIN, LONG_MAX, b) || !f.integer("msb", LONG_MIN, LONG_MAX, msb) ||
        !f.floats("table", table, 0, "table entry", "", "the table ends")) return nullptr;
    const std::string &name = f.name;
    const bool qam = name == "qam";
    if (P < 1 || P >= (1l << 30)) { set_error("%s: period must be 1 .. 2^30 - 1 samples per symbol (got %ld)", name.c_str(), P); return nullptr; }
    if (b < 1 || b > MOD_MAX_BITS) { set_error("%s: bits per symbol must be 1 .. %d (got %ld)", name.c_str(), MOD_MAX_BITS, b); return nullptr; }
    if (msb != 0 && msb != 1) { set_error("%s: msb must be 0 or 1", name.c_str()); return nullptr; }
    const size_t want = ((size_t)1 << b) * (qam ? 2 : 1);
    if (table.size() != want) { set_error("%s: the table has %zu values, %d bits per symbol need %zu", name.c_str(), table.size(), (int)b, want); return nullptr; }
    return modulator_build(qam, (unsigned)P, (int)b, (int)msb, table);
}
