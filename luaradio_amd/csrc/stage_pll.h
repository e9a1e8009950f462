// stage_pll.h - PLLBlock (kernels_pll.h, pll_plan.h), created through lrhip_unary_create("pll:alpha=..:beta=..:fmin=..:fmax=..:mult=..:port=out|error").
// alpha, beta, fmin and fmax are in radians per sample, computed by the caller in double in the operation order of pll.lua:117-126; port =
// out (ComplexFloat32 cis(phi_multiplied), the default) or error (Float32).  Test knobs: segment= (C), warmup= (W), speculate=0 (serial path only).
// The stage fuses with nothing (chain_plan.h knows no rule for it) and cannot be sharded in time: no finite halo reproduces an unlocked loop.
// A call launches 1 kernel on the serial path, 4 on the speculative one, 5 when the verify pass rejected a segment (Chain.last_launches).
// (part of liblrhip.so; included by lrhip.hip before stage_digital.h, one translation unit)
#pragma once

struct PllStage : lrhip_stage {
    PllParams p;
    int port = PLL_PORT_OUT;
    unsigned long W = 0, seg_req = 0;        // warm-up length (0: none, serial only); "segment=" (0: chosen per call)
    bool allow = true;                       // "speculate=0" clears it
    Carried<PllState> state;
    DeviceBuf stats_buf, scratch;            // stats_buf: PllStats (two counters)
    PinnedBuf h_rej;
    const char *kind() const override { return port == PLL_PORT_OUT ? "pll" : "pll(error)"; }
    long memory() const override { return -1; }
    int reset() override
    {
        return (state.reset(pll_initial(p)) || zero_fill(stats_buf, sizeof(PllStats))) ? -1 : 0;
    }
    long run(const void *in_dev, unsigned long n, void *out_dev, unsigned long cap) override
    {
        if (n > cap) return set_error("%s: output capacity %lu < %lu", kind(), cap, n);
        if (!n) return 0;
        const PllPlan q = pll_make_plan(n, p, W, (unsigned long)ctx().num_cus * 512, seg_req, allow);
        const float *x = (const float *)in_dev;
        if (q.speculate) {
            if (speculated(x, n, q, out_dev)) return -1;
        } else {
            PllStats *stats = (PllStats *)stats_buf.p;
            if (port == PLL_PORT_OUT) hipLaunchKernelGGL((pll_serial_kernel<PLL_PORT_OUT>), dim3(1), dim3(64), 0, ctx().stream, x, n, p, state.in(), out_dev, state.out(), stats);
            else hipLaunchKernelGGL((pll_serial_kernel<PLL_PORT_ERROR>), dim3(1), dim3(64), 0, ctx().stream, x, n, p, state.in(), out_dev, state.out(), stats);
            LR_LAUNCH_CHECK();
        }
        state.flip();                                        // the one commit, whichever path ran
        return (long)n;
    }
    // the speculative path: 4 launches, 5 when the verify pass rejected a segment
    int speculated(const float *x, unsigned long n, const PllPlan &q, void *out_dev)
    {
        const PllState *si = state.in();
        PllState *so = state.out();
        PllStats *stats = (PllStats *)stats_buf.p;
        // scratch: entry and exit edges, phi_multiplied totals / entries, the segments' mean |err|, rejection flags
        const size_t o_exit = q.nseg * sizeof(PllEdge), o_pm = o_exit + q.nseg * sizeof(PllEdge), o_emean = o_pm + q.nseg * sizeof(double),
                     o_bad = o_emean + q.nseg * sizeof(double), total = o_bad + q.nseg;
        if (scratch.reserve(total)) return -1;
        char *sp = (char *)scratch.p;
        PllEdge *entry = (PllEdge *)sp, *exit_ = (PllEdge *)(sp + o_exit);
        double *pm = (double *)(sp + o_pm);
        double *emean = (double *)(sp + o_emean);
        unsigned char *bad = (unsigned char *)(sp + o_bad);
        const unsigned lanes_grid = (unsigned)((q.nseg + 63) / 64);
        hipLaunchKernelGGL(pll_speculate_kernel, dim3(lanes_grid), dim3(64), 0, ctx().stream, x, n, p, q.C, q.W, q.nseg, si, entry, exit_, pm, emean, stats);
        LR_LAUNCH_CHECK();
        hipLaunchKernelGGL(pll_verify_kernel, dim3((unsigned)((q.nseg + 255) / 256)), dim3(256), 0, ctx().stream, (const PllEdge *)entry, (const PllEdge *)exit_, (const double *)emean, q.nseg,
                           q.tol_phi, q.tol_f, bad, stats);
        LR_LAUNCH_CHECK();
        // did the loop hold lock?  The one small read-back of this stage: the repair walk is launched only when a segment was rejected
        if (h_rej.reserve(sizeof(unsigned long long))) return -1;
        LR_HIP(hipMemcpyAsync(h_rej.p, &stats->rejected, sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx().stream));
        LR_HIP(hipStreamSynchronize(ctx().stream));
        if (*(const unsigned long long *)h_rej.p) {
            hipLaunchKernelGGL(pll_repair_kernel, dim3(1), dim3(64), 0, ctx().stream, x, n, p, q.C, q.nseg, q.tol_phi, q.tol_f, bad, entry, exit_, pm, (const double *)emean, stats);
            LR_LAUNCH_CHECK();
        }
        hipLaunchKernelGGL(pll_prefix_kernel, dim3(1), dim3(256), 0, ctx().stream, pm, q.nseg, si);
        LR_LAUNCH_CHECK();
        if (port == PLL_PORT_OUT)
            hipLaunchKernelGGL((pll_emit_kernel<PLL_PORT_OUT>), dim3(lanes_grid), dim3(64), 0, ctx().stream, x, n, p, q.C, q.nseg, (const PllEdge *)entry, (const double *)pm,
                               out_dev, so);
        else
            hipLaunchKernelGGL((pll_emit_kernel<PLL_PORT_ERROR>), dim3(lanes_grid), dim3(64), 0, ctx().stream, x, n, p, q.C, q.nseg, (const PllEdge *)entry,
                               (const double *)pm, out_dev, so);
        LR_LAUNCH_CHECK();
        return 0;
    }
};

static lrhip_stage_t *pll_create(const char *op)
{
    OpFields f;
    if (!f.split(op, "pll", {{"alpha", nullptr}, {"beta", nullptr}, {"fmin", nullptr}, {"fmax", nullptr}, {"mult", "1"}, {"port", "out"},      // pll.lua:32: mult = 1
                             {"segment", ""}, {"warmup", ""}, {"speculate", "1"}}, true)) return nullptr;
    PllParams p;
    struct { const char *k; double *v; } nums[] = {{"alpha", &p.alpha}, {"beta", &p.beta}, {"fmin", &p.fmin}, {"fmax", &p.fmax}, {"mult", &p.mult}};
    for (auto &n : nums) {
        if (!f.number(n.k, *n.v)) return nullptr;
        if (!std::isfinite(*n.v)) { set_error("pll: %s must be finite", n.k); return nullptr; }
    }
    const int port = f.word("port", {"out", "error"}, "pll: port must be \"out\" or \"error\", not \"", "\"");
    if (port < 0) return nullptr;
    bool spec = true;
    if (!f.flag("speculate", spec)) return nullptr;
    double seg = 0.0, warm = -1.0;
    struct { const char *k; double *v; } knobs[] = {{"segment", &seg}, {"warmup", &warm}};
    for (auto &n : knobs) {
        if (!f.has(n.k)) continue;
        if (!f.number(n.k, *n.v)) return nullptr;
        if (!(*n.v >= 1.0 && *n.v <= 1073741824.0) || *n.v != floor(*n.v)) { set_error("pll: %s must be an integer in [1, 2^30]", n.k); return nullptr; }
    }
    auto q = new_stage<PllStage>();
    if (!q) return nullptr;
    q->p = p;
    q->port = port == 0 ? PLL_PORT_OUT : PLL_PORT_ERROR;
    q->seg_req = (unsigned long)seg;
    q->W = f.has("warmup") ? (unsigned long)warm : pll_warmup(p.alpha, p.beta, PLL_TOL_PHI / 256.0);
    q->allow = spec;
    q->in_size = 8;
    q->out_size = q->port == PLL_PORT_OUT ? 8 : 4;
    if (q->reset()) return nullptr;
    return q.release();
}

