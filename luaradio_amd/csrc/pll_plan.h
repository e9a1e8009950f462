// pll_plan.h - the host-checkable logic of the PLL stage (kernels_pll.h, stage_pll.h): the per-sample step of radio/blocks/signal/pll.lua:142-164,
// the warm-up length W from the loop's pole radius, the segment length C, the acceptance test and the repair walk.  Everything here compiles for
// the host as well (tools/host_pll_check.hip plays the lanes in a loop against the plain serial recurrence).
//
// THE CONTRACT.  The device trajectory is the reference's serial recurrence with state perturbations of at most `tol` at segment boundaries:
// |d phi_locked| <= tol_phi modulo 2 pi and |d freq_locked| <= tol_f where a segment starts from a speculated entry, none where it was repaired,
// none at sample 0 of a call (the carried state is exact).  phi_multiplied is never fed back; it is the prefix sum of freq * mult + alpha * err
// over that trajectory, carried modulo 2 pi.
//
// The boundary tolerances bound phi_locked and freq_locked, NOT phi_multiplied.  A perturbation (d, g) of (phi_locked, freq_locked) at an accepted
// boundary, |d| <= tol_phi, |g| <= tol_f = tol_phi beta / alpha, dies out in the fed-back state, but what it adds to phi_multiplied on the way stays:
// both differences end at 0 under the linear loop, which fixes the sums over the transient: g + beta sum(err) = 0 and d + sum(freq) + alpha
// sum(err) = 0, so sum(err) = -g / beta, sum(freq) = -d + g alpha / beta, and phi_multiplied = sum(mult freq + alpha err) moves by
// -mult d + (mult - 1) g alpha / beta: at most (|mult| + |mult - 1|) tol_phi per accepted boundary.  Its distance from the serial loop
// therefore grows with the number of accepted boundaries (the stream length) and with the multiplier; it is a random walk where the input carries
// noise and a straight line where it does not (every lane then misses the long-running trajectory by the same amount: the floor below).
// Measured on the CPU against the serial loop, unit-test loop, segments of 64: carrier + 0.1 noise, mult 20: 4e-7 after 2^15 samples, 7.8e-7
// after 2^16 and still rising (1.1e-6 with another noise seed); mult 3: 6e-8 .. 1.8e-7 throughout.  "speculate=0" gives the serial value at any length.
//
// Why this works: the phase detector is an exact atan2, so two trajectories over the same input whose wraps and clamps coincide differ by a
// quantity that evolves under the linearised loop z^2 + (alpha + beta - 2) z + (1 - alpha): it shrinks by the larger root modulus r per sample.
// A lane started W samples early from the INITIAL state therefore arrives at its segment with the true state up to 2 pi r^W - when the loop
// is in lock.  Out of lock it does not, the acceptance test says so, and the segment is rerun serially from its predecessor's true exit.
//
//   tol_phi = 2^-22 rad (2.4e-7).  Floor: err is stored as Float32, so two converged trajectories keep differing by 4e-9 .. 2e-8 rad (measured on
//             the CPU on the stereo pilot loop, the AM-synchronous loop and the unit-test loop; tools/host_pll_check.hip prints the largest entry
//             error it sees).  A tolerance at the floor would reject everything; 2^-22 is 12 x the top of the floor.  Ceiling: the golden tests hold
//             the output within 1e-6 of the f64 model; a boundary perturbation d moves cis(phi) by at most |d| while the loop pulls it back, and
//             2^-22 leaves a factor 4 for the Float32 rounding of the output (6e-8).  (phi_multiplied is not covered by this: see above.)
//   tol_f   = tol_phi * beta / alpha: the frequency error the loop filter makes of a phase error tol_phi (freq += beta err, phi += alpha err).
//   lock    = a segment is accepted only if the mean of |err| over its samples is at most pi / 4: halfway between perfect lock (0) and none (err
//             uniform over (-pi, pi], mean pi / 2; a 64-sample mean of that is 1.57 +- 0.11, seven deviations away).  The floor above is the spacing
//             of Float32 at the size of err; where err roams over the whole circle (noise, a carrier outside the clamp range) it is 2.4e-7 and
//             trajectories that have converged still differ by ~1e-7 (measured): they would pass tol_phi now and then, by chance rather than with the
//             margin it was chosen for.  Such segments are rerun serially: out of lock the stage IS the serial loop.  (A maximum of |err| instead of
//             the mean would reject 4e-4 of the samples of a locked pilot in 0.3 noise, a tenth of its 256-sample segments.)
//   floor   = a segment is accepted only if the mean of |err| over its samples is at least PLL_LOCK_FLOOR = 1e-5 rad.  Under it the input carries no
//             dither: err sits inside the Float32 rounding of the VCO sample (a dead zone of ~6e-8 rad), two trajectories that have come that close
//             see the same err and stop converging, so every lane (W .. W + C samples old) differs from the long-running trajectory by the same tiny
//             (d, g), and phi_multiplied integrates it over every boundary: on a noise-free carrier at the loop's centre, 2^16 samples, segments
//             of 64, the out port was 3.4e-6 (mult 3), 4.8e-6 (mult -2), 3.1e-5 (mult 20) from the serial loop with nothing rejected.
//             The sweep behind the value (CPU, unit-test loop at mult 3, carrier at 0.1 + sigma complex noise, 2^16 samples, no floor; largest
//             out difference from the serial loop, and the mean |err| in lock):
//               sigma 0     1e-9    1e-8    1e-7    1e-6    1e-5    1e-4    1e-3    1e-2    1e-1
//               out   3.4e-6 2.2e-6 4.0e-7  3.0e-7  2.2e-7  1.2e-7  1.2e-7  1.2e-7  1.5e-7  1.8e-7
//               |err| 1e-12  2e-10  1.1e-8  8.4e-8  8.3e-7  8.3e-6  8.3e-5  8.3e-4  8.3e-3  8.3e-2
//             The drift is under a quarter of the 1e-6 bar (2.5e-7) from sigma = 1e-6, mean |err| 8.3e-7; the floor is a decade above that.
//             Segments under it are rerun serially, so a synthetic tone without dither gets the serial loop's values at single-lane speed;
//             input with sigma = 1e-4 of noise on a unit carrier (80 dB under it) and more speculates as before.
//   tol_w   = tol_phi / 256: the warm-up ends where the linear model has shrunk the worst initial error (2 pi) to 2^-30, far under the floor, so
//             a rejection means "not in lock", not "warm-up a little short".  W = ceil(ln(tol_w / 2 pi) / ln r).
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define LR_PLL_HD __host__ __device__
#else
#define LR_PLL_HD
#endif

namespace lrhip {

constexpr double PLL_TWO_PI = 6.283185307179586476925286766559;      // 2 * math.pi
constexpr double PLL_TOL_PHI = 1.0 / 4194304.0;                       // 2^-22 rad
constexpr double PLL_LOCK_ERR = 0.78539816339744831;                  // pi / 4: the largest mean |err| of a segment in lock
constexpr double PLL_LOCK_FLOOR = 1e-5;                               // the smallest mean |err| at which a speculated entry can be verified
constexpr unsigned long PLL_MIN_SEGMENT = 64;

struct PllParams { double alpha, beta, fmin, fmax, mult; };
struct PllState { double pl, pm, fl; };                               // phi_locked, phi_multiplied, freq_locked
struct PllEdge { double pl, fl; };                                    // the fed-back part of the state at a segment boundary

// pll.lua:128-131
LR_PLL_HD inline PllState pll_initial(const PllParams &p)
{
    PllState s;
    s.pl = 0.0; s.pm = 0.0; s.fl = (p.fmin + p.fmax) / 2.0;
    return s;
}

// One sample (pll.lua:143-163), in the reference's operation order.  The VCO is a ComplexFloat32 (its cos / sin are rounded to Float32), the
// product x * conj(vco) is ComplexFloat32.__mul on the Float32 pairs (a double expression rounded to Float32 per component), err is the Float32 of
// the double atan2; cos, sin and atan2 in double, as the AGC scans compute theirs.  No contraction: the double sums round where Lua's do.
template <bool WITH_PM>
LR_PLL_HD inline float pll_step(PllState &s, const PllParams &p, float xr, float xi)
{
#pragma clang fp contract(off)
    const float vr = (float)cos(s.pl), vi = -(float)sin(s.pl);      // vco_output:conj()
    const float re = (float)((double)xr * (double)vr - (double)xi * (double)vi);
    const float im = (float)((double)xr * (double)vi + (double)xi * (double)vr);
    const float err = (float)atan2((double)im, (double)re);
    const double e = (double)err;
    s.fl = s.fl + p.beta * e;
    s.pl = s.pl + s.fl + p.alpha * e;
    if (WITH_PM) s.pm = s.pm + s.fl * p.mult + p.alpha * e;
    s.fl = (s.fl > p.fmax) ? p.fmax : s.fl;
    s.fl = (s.fl < p.fmin) ? p.fmin : s.fl;
    s.pl = (s.pl > PLL_TWO_PI) ? (s.pl - PLL_TWO_PI) : s.pl;
    s.pl = (s.pl < -PLL_TWO_PI) ? (s.pl + PLL_TWO_PI) : s.pl;
    if (WITH_PM) {
        s.pm = (s.pm > PLL_TWO_PI) ? (s.pm - PLL_TWO_PI) : s.pm;
        s.pm = (s.pm < -PLL_TWO_PI) ? (s.pm + PLL_TWO_PI) : s.pm;
    }
    return err;
}

// Segment k's speculated entry against its predecessor's exit: phi_locked modulo 2 pi, freq_locked absolutely.  A NaN on either side is a
// disagreement (every comparison with it is false), so non-finite input ends in the repair walk, which terminates.
LR_PLL_HD inline bool pll_agree(const PllEdge &entry, const PllEdge &exit_prev, double tol_phi, double tol_f)
{
    const double d = remainder(entry.pl - exit_prev.pl, PLL_TWO_PI);
    return fabs(d) <= tol_phi && fabs(entry.fl - exit_prev.fl) <= tol_f;
}

// segment k as a whole: its entry agrees with the predecessor's exit, the loop stayed in lock over it and the input carried enough dither for
// the agreement to mean something (emean: the segment's mean |err|; a NaN is rejected)
LR_PLL_HD inline bool pll_accept(const PllEdge &entry, const PllEdge &exit_prev, double emean, double tol_phi, double tol_f)
{
    return pll_agree(entry, exit_prev, tol_phi, tol_f) && emean <= PLL_LOCK_ERR && emean >= PLL_LOCK_FLOOR;
}

// the larger root modulus of z^2 + (alpha + beta - 2) z + (1 - alpha)
inline double pll_pole_radius(double alpha, double beta)
{
    const double b = alpha + beta - 2.0, c = 1.0 - alpha, disc = b * b - 4.0 * c;
    if (disc < 0.0) return sqrt(c);
    const double q = sqrt(disc), r1 = fabs((-b + q) / 2.0), r2 = fabs((-b - q) / 2.0);
    return r1 > r2 ? r1 : r2;
}

// W = ceil(ln(tol_w / 2 pi) / ln r); 0 = no finite warm-up (a loop that does not contract)
inline unsigned long pll_warmup(double alpha, double beta, double tol_w)
{
    const double r = pll_pole_radius(alpha, beta);
    if (!(r > 0.0) || !(r < 1.0) || !(tol_w > 0.0)) return 0;
    const double w = ceil(log(tol_w / PLL_TWO_PI) / log(r));
    if (!(w >= 1.0)) return 1;
    return w < 1e15 ? (unsigned long)w : 0;
}

struct PllPlan {
    unsigned long C = 0, W = 0, nseg = 0;     // segment length, warm-up length, segments of this call
    bool speculate = false;
    double tol_phi = 0.0, tol_f = 0.0;
};

// The plan of one call of n samples.  `lanes`: how many lanes the device runs at once with two waves per SIMD (compute units x 512): the
// recurrence is one dependent chain of double arithmetic per lane, which two waves per SIMD keep the pipe busy with.
//   C: with one segment per lane a call costs W + 2 C steps (speculation W + C, emission C), so C is as small as fills the device,
//      ceil(n / lanes), and at least PLL_MIN_SEGMENT, which bounds the lanes a short call starts (seg_req != 0: the "segment=" knob).
//   serial instead: no finite W, fewer than two segments, or W + 2 C > n / 2 - the speculative path would not even halve the serial n steps
//      (this covers W >= n, and loops so narrow that the warm-up is most of the call).
inline PllPlan pll_make_plan(unsigned long n, const PllParams &p, unsigned long W, unsigned long lanes, unsigned long seg_req, bool allow)
{
    PllPlan q;
    q.tol_phi = PLL_TOL_PHI;
    q.tol_f = PLL_TOL_PHI * p.beta / p.alpha;
    q.W = W;
    unsigned long C = seg_req;
    if (!C) {
        C = lanes ? (n + lanes - 1) / lanes : n;
        if (C < PLL_MIN_SEGMENT) C = PLL_MIN_SEGMENT;
    }
    q.C = C;
    q.nseg = n ? (n + C - 1) / C : 0;
    q.speculate = allow && W > 0 && q.nseg >= 2 && W + 2 * C <= n / 2;
    if (!q.speculate) { q.C = n; q.nseg = n ? 1 : 0; }
    return q;
}

// first sample of lane k's run: W samples before its segment, or sample 0 (then it starts from the carried state, which is exact)
LR_PLL_HD inline unsigned long pll_lane_start(unsigned long k, unsigned long C, unsigned long W)
{
    const unsigned long s = k * C;
    return s > W ? s - W : 0;
}

// ---- the passes over one lane / the walk, shared by the kernels and the host check ----------------------------------------------------------

enum { PLL_PORT_NONE = 0, PLL_PORT_OUT = 1, PLL_PORT_ERROR = 2 };

// samples [i0, i1) from state s; PORT selects what is written: out[i] = cis(phi_multiplied) BEFORE the update (pll.lua:145), or error[i].
// The input is fetched eight samples ahead of the arithmetic: across a wave the lanes read addresses a whole segment apart, so each lane asks for
// the 64 contiguous bytes it will consume while the previous eight are still in the dependent chain.
// Returns the sum of |err| over the run (a NaN err counts as 0: a non-finite sample is no statement about lock).
template <bool WITH_PM, int PORT>
LR_PLL_HD inline double pll_run(PllState &s, const PllParams &p, const float *x, unsigned long i0, unsigned long i1, void *out)
{
    constexpr int T = 8;
    float *of = (float *)out;
    double esum = 0.0;
    unsigned long i = i0;
    for (; i + T <= i1; i += T) {
        float v[2 * T];
#pragma unroll
        for (int j = 0; j < 2 * T; j++) v[j] = x[2 * i + j];
#pragma unroll
        for (int j = 0; j < T; j++) {
            if (PORT == PLL_PORT_OUT) { of[2 * (i + j)] = (float)cos(s.pm); of[2 * (i + j) + 1] = (float)sin(s.pm); }
            const float err = pll_step<WITH_PM>(s, p, v[2 * j], v[2 * j + 1]);
            if (PORT == PLL_PORT_ERROR) of[i + j] = err;
            esum += err == err ? (double)fabsf(err) : 0.0;
        }
    }
    for (; i < i1; i++) {
        if (PORT == PLL_PORT_OUT) { of[2 * i] = (float)cos(s.pm); of[2 * i + 1] = (float)sin(s.pm); }
        const float err = pll_step<WITH_PM>(s, p, x[2 * i], x[2 * i + 1]);
        if (PORT == PLL_PORT_ERROR) of[i] = err;
        esum += err == err ? (double)fabsf(err) : 0.0;
    }
    return esum;
}

// speculation of lane k: warm-up from the initial state (or the carried one at sample 0) without output, then the segment with phi_multiplied
// counted from 0: entry[k], exit[k] and the segment's phi_multiplied increment modulo 2 pi (the conditional single wraps keep it reduced)
LR_PLL_HD inline void pll_speculate_lane(const float *x, unsigned long n, const PllParams &p, unsigned long C, unsigned long W, unsigned long k,
                                         const PllState &carried, PllEdge *entry, PllEdge *exit_, double *pm_total, double *emean)
{
    const unsigned long s0 = k * C, s1 = s0 + C < n ? s0 + C : n, w0 = pll_lane_start(k, C, W);
    PllState s = w0 == 0 ? carried : pll_initial(p);
    pll_run<false, PLL_PORT_NONE>(s, p, x, w0, s0, nullptr);
    entry[k].pl = s.pl; entry[k].fl = s.fl;
    s.pm = 0.0;
    emean[k] = pll_run<true, PLL_PORT_NONE>(s, p, x, s0, s1, nullptr) / (double)(s1 - s0);
    exit_[k].pl = s.pl; exit_[k].fl = s.fl;
    pm_total[k] = s.pm;
}

// emission of lane k from its verified entry
template <int PORT>
LR_PLL_HD inline PllState pll_emit_lane(const float *x, unsigned long n, const PllParams &p, unsigned long C, unsigned long k, const PllEdge *entry,
                                        const double *pm_entry, void *out)
{
    const unsigned long s0 = k * C, s1 = s0 + C < n ? s0 + C : n;
    PllState s;
    s.pl = entry[k].pl; s.fl = entry[k].fl; s.pm = pm_entry[k];
    pll_run<true, PORT>(s, p, x, s0, s1, out);
    return s;
}

// The repair walk, in stream order (one thread).  bad[k] != 0: segment k was not accepted (pll_accept).  A repaired segment starts from its
// predecessor's true exit and is rerun serially; while the next segment is not acceptable behind its new exit, that one is repaired as
// well.  Out of lock this is the serial recurrence at single-lane speed.  Returns the number of segments rerun.
LR_PLL_HD inline unsigned long long pll_repair_walk(const float *x, unsigned long n, const PllParams &p, unsigned long C, unsigned long nseg,
                                                    double tol_phi, double tol_f, unsigned char *bad, PllEdge *entry, PllEdge *exit_, double *pm_total,
                                                    const double *emean)
{
    unsigned long long repaired = 0;
    for (unsigned long k = 1; k < nseg; k++) {
        if (!bad[k]) continue;
        const unsigned long s0 = k * C, s1 = s0 + C < n ? s0 + C : n;
        PllState s;
        s.pl = exit_[k - 1].pl; s.fl = exit_[k - 1].fl; s.pm = 0.0;
        entry[k] = exit_[k - 1];
        pll_run<true, PLL_PORT_NONE>(s, p, x, s0, s1, nullptr);
        exit_[k].pl = s.pl; exit_[k].fl = s.fl;
        pm_total[k] = s.pm;
        repaired++;
        if (k + 1 < nseg) bad[k + 1] = !pll_accept(entry[k + 1], exit_[k], emean[k + 1], tol_phi, tol_f);
    }
    return repaired;
}

// phi_multiplied at a segment's entry: the carried value plus the totals of the segments before it, modulo 2 pi
LR_PLL_HD inline double pll_pm_add(double a, double b) { return remainder(a + b, PLL_TWO_PI); }

}  // namespace lrhip
