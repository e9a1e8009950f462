// kernels_pll.h - PLLBlock (radio/blocks/signal/pll.lua:113-167) parallel in time while the loop is in lock: speculate, verify, repair.
//
// The loop is true feedback through a nonlinear detector, so it is no scan.  But a PLL in lock forgets its past: a lane started W samples early
// from the initial state reaches the true state at its segment (pll_plan.h: the contract, W, the tolerances and where they come from).  One
// call of n samples, segments of C:
//   speculate  one lane per segment: warm-up over [kC - W, kC) without output (lanes with kC <= W start at sample 0 from the carried state, which
//              is exact), then the segment: entry e_k, exit x_k, and the segment's phi_multiplied increment modulo 2 pi
//   verify     segment k is accepted when e_k agrees with x_(k-1) within tol and the mean |err| over it is under pi / 4 (in lock) and over PLL_LOCK_FLOOR (the input carries dither); the number of rejections is the call's one 8-byte read-back
//   repair     only when something was rejected: one thread walks the rejected segments in stream order from their predecessors' true exits
//              (out of lock: the serial recurrence at single-lane speed, which is what the reference runs)
//   prefix     phi_multiplied is never fed back: an exclusive scan of the segments' totals modulo 2 pi gives every segment's entry value
//   emit       every lane reruns its segment from its verified entry and writes the selected port; the last lane leaves the carried state
// A call too short for this (pll_make_plan) runs pll_serial_kernel: the literal loop in one thread.
//
// Lanes of a wave run the same number of steps (all but the first W / C lanes of a call), so there is no divergence; the arithmetic is a dependent
// chain of double cos / sin / atan2 per sample, ~10^2 times the cost of the 8 input bytes it consumes, which each lane fetches as 64
// contiguous bytes ahead of use (pll_run).  The input is read W / C + 2 times, after the first mostly from L2.
#pragma once
#include "common.h"
#include "pll_plan.h"

namespace lrhip {

struct PllStats { unsigned long long rejected, repaired; };

__global__ __launch_bounds__(64) void pll_speculate_kernel(const float *__restrict__ x, unsigned long n, PllParams p, unsigned long C, unsigned long W,
                                                           unsigned long nseg, const PllState *__restrict__ carried, PllEdge *__restrict__ entry,
                                                           PllEdge *__restrict__ exit_, double *__restrict__ pm_total, double *__restrict__ emean,
                                                           PllStats *__restrict__ stats)
{
    const unsigned long k = (unsigned long)blockIdx.x * 64 + threadIdx.x;
    if (k == 0) { stats->rejected = 0; stats->repaired = 0; }
    if (k >= nseg) return;
    pll_speculate_lane(x, n, p, C, W, k, *carried, entry, exit_, pm_total, emean);
}

__global__ __launch_bounds__(256) void pll_verify_kernel(const PllEdge *__restrict__ entry, const PllEdge *__restrict__ exit_, const double *__restrict__ emean,
                                                         unsigned long nseg, double tol_phi, double tol_f, unsigned char *__restrict__ bad, PllStats *__restrict__ stats)
{
    const unsigned long k = (unsigned long)blockIdx.x * 256 + threadIdx.x;
    if (k >= nseg) return;
    const bool rej = k > 0 && !pll_accept(entry[k], exit_[k - 1], emean[k], tol_phi, tol_f);
    bad[k] = rej;
    if (rej) atomicAdd(&stats->rejected, 1ull);
}

__global__ __launch_bounds__(64) void pll_repair_kernel(const float *__restrict__ x, unsigned long n, PllParams p, unsigned long C, unsigned long nseg,
                                                        double tol_phi, double tol_f, unsigned char *bad, PllEdge *entry, PllEdge *exit_, double *pm_total,
                                                        const double *emean, PllStats *stats)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) stats->repaired = pll_repair_walk(x, n, p, C, nseg, tol_phi, tol_f, bad, entry, exit_, pm_total, emean);
}

// in place: pm[k] = the segment's total on entry, phi_multiplied at the segment's first sample on return (one workgroup; every thread a run of segments)
__global__ __launch_bounds__(256) void pll_prefix_kernel(double *pm, unsigned long nseg, const PllState *__restrict__ carried)
{
    __shared__ double sh[256];
    const int tid = threadIdx.x;
    const unsigned long per = (nseg + 255) / 256, a = tid * per < nseg ? tid * per : nseg, b = a + per < nseg ? a + per : nseg;
    double sum = 0.0;
    for (unsigned long k = a; k < b; k++) sum = pll_pm_add(sum, pm[k]);
    sh[tid] = sum;
    __syncthreads();
    if (tid == 0) {
        double run = carried->pm;                    // segment 0 continues the carried value as it is
        for (int t = 0; t < 256; t++) { const double v = sh[t]; sh[t] = run; run = pll_pm_add(run, v); }
    }
    __syncthreads();
    double run = sh[tid];
    for (unsigned long k = a; k < b; k++) { const double v = pm[k]; pm[k] = run; run = pll_pm_add(run, v); }
}

template <int PORT>
__global__ __launch_bounds__(64) void pll_emit_kernel(const float *__restrict__ x, unsigned long n, PllParams p, unsigned long C, unsigned long nseg,
                                                      const PllEdge *__restrict__ entry, const double *__restrict__ pm_entry, void *__restrict__ out,
                                                      PllState *__restrict__ state_out)
{
    const unsigned long k = (unsigned long)blockIdx.x * 64 + threadIdx.x;
    if (k >= nseg) return;
    const PllState s = pll_emit_lane<PORT>(x, n, p, C, k, entry, pm_entry, out);
    if (k == nseg - 1) *state_out = s;
}

template <int PORT>
__global__ __launch_bounds__(64) void pll_serial_kernel(const float *__restrict__ x, unsigned long n, PllParams p, const PllState *__restrict__ carried,
                                                        void *__restrict__ out, PllState *__restrict__ state_out, PllStats *__restrict__ stats)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    PllState s = *carried;
    pll_run<true, PORT>(s, p, x, 0, n, out);
    *state_out = s;
    stats->rejected = 0; stats->repaired = 0;
}

}  // namespace lrhip
