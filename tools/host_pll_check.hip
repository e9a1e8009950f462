// host_pll_check.hip - the PLL stage's speculate / verify / repair logic (luaradio_amd/csrc/pll_plan.h) on the CPU: the lanes are played in a host
// loop with the very functions the kernels call, and compared with the plain serial loop of pll.lua:138-167.
//   hipcc --offload-arch=gfx950 -O1 -std=c++17 -I luaradio_amd/csrc -I include -o /tmp/host_pll_check tools/host_pll_check.hip && /tmp/host_pll_check
// Checked: W against the pole radius (2 pi r^W <= tol_w < 2 pi r^(W-1)), the plan's serial / speculative decision, that locked signals are
// accepted everywhere and stay within 1e-6 of the serial loop, that a short warm-up, pure noise and a carrier outside the clamp range end in the
// repair walk and are still consistent
// (a replay of the recurrence driven by the produced error samples reproduces out and error within 1e-6), and that a NaN terminates the walk.
// With arguments (play_file below) it plays one call over a raw ComplexFloat32 file instead: tests/test_pll_cpu.py feeds it tests/helpers/pll_signals.py.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "pll_plan.h"
using namespace lrhip;

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { failures++; printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

// pll.lua:117-126
static PllParams make_params(double bw, double fmin, double fmax, double mult, double rate)
{
    const double pi = 3.14159265358979323846;
    double loop_bw = 2 * pi * (bw / rate);
    PllParams p;
    p.fmin = 2 * pi * (fmin / rate);
    p.fmax = 2 * pi * (fmax / rate);
    const double damping = sqrt(2.0) / 2;
    loop_bw = loop_bw / (damping + 1 / (4 * damping));
    const double denom = (1 + 2 * damping * loop_bw + loop_bw * loop_bw);
    p.alpha = (4 * damping * loop_bw) / denom;
    p.beta = (4 * loop_bw * loop_bw) / denom;
    p.mult = mult;
    return p;
}

// xorshift + Box-Muller: the check needs noise, not a particular generator
struct Rng {
    uint64_t s = 0x9E3779B97F4A7C15ull;
    double uni() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return ((s >> 11) + 0.5) / 9007199254740992.0; }
    double gauss() { return sqrt(-2.0 * log(uni())) * cos(6.283185307179586 * uni()); }
};
static std::vector<float> tone(unsigned long n, double w, double ph, double sigma, Rng &g)
{
    std::vector<float> x(2 * n);
    for (unsigned long i = 0; i < n; i++) {
        x[2 * i] = (float)(cos(w * (double)i + ph) + sigma * g.gauss());
        x[2 * i + 1] = (float)(sin(w * (double)i + ph) + sigma * g.gauss());
    }
    return x;
}

struct Result { std::vector<float> out, err; std::vector<unsigned char> bad; unsigned long long rejected = 0, repaired = 0; double entry_err = 0.0; PllState last; PllPlan plan; };

// one call of the stage as the host-side run() and the kernels perform it
static Result play(const std::vector<float> &x, const PllParams &p, unsigned long W, unsigned long lanes, unsigned long seg, bool allow, PllState carried)
{
    const unsigned long n = x.size() / 2;
    Result r;
    r.out.assign(2 * n, 0.f); r.err.assign(n, 0.f);
    const PllPlan q = pll_make_plan(n, p, W, lanes, seg, allow);
    r.plan = q;
    if (!q.speculate) {
        PllState s = carried, t = carried;
        pll_run<true, PLL_PORT_OUT>(s, p, x.data(), 0, n, r.out.data());
        pll_run<true, PLL_PORT_ERROR>(t, p, x.data(), 0, n, r.err.data());
        r.last = s;
        return r;
    }
    std::vector<PllEdge> entry(q.nseg), exit_(q.nseg);
    std::vector<double> pm(q.nseg);
    std::vector<unsigned char> bad(q.nseg, 0);
    std::vector<double> emean(q.nseg);
    for (unsigned long k = 0; k < q.nseg; k++) pll_speculate_lane(x.data(), n, p, q.C, q.W, k, carried, entry.data(), exit_.data(), pm.data(), emean.data());
    for (unsigned long k = 1; k < q.nseg; k++) {
        bad[k] = !pll_accept(entry[k], exit_[k - 1], emean[k], q.tol_phi, q.tol_f);
        r.rejected += bad[k];
        const double d = fabs(remainder(entry[k].pl - exit_[k - 1].pl, PLL_TWO_PI));
        if (!bad[k] && d > r.entry_err) r.entry_err = d;
    }
    if (r.rejected) r.repaired = pll_repair_walk(x.data(), n, p, q.C, q.nseg, q.tol_phi, q.tol_f, bad.data(), entry.data(), exit_.data(), pm.data(), emean.data());
    double run = carried.pm;
    for (unsigned long k = 0; k < q.nseg; k++) { const double v = pm[k]; pm[k] = run; run = pll_pm_add(run, v); }
    for (unsigned long k = 0; k < q.nseg; k++) {
        r.last = pll_emit_lane<PLL_PORT_OUT>(x.data(), n, p, q.C, k, entry.data(), pm.data(), r.out.data());
        (void)pll_emit_lane<PLL_PORT_ERROR>(x.data(), n, p, q.C, k, entry.data(), pm.data(), r.err.data());
    }
    r.bad = bad;                                 // after the walk: the segments that were rerun serially
    return r;
}

static double max_diff(const std::vector<float> &a, const std::vector<float> &b, bool wrap = false)
{
    double m = 0.0;
    for (size_t i = 0; i < a.size(); i++) {
        double d = (double)a[i] - (double)b[i];
        if (wrap) d = remainder(d, PLL_TWO_PI);
        if (!(fabs(d) <= m)) m = fabs(d);
    }
    return m;
}

// the recurrence replayed in double, driven by the produced error samples: out must be cis(pm) and error the detector's answer at pl
static void replay(const std::vector<float> &x, const PllParams &p, const Result &r, PllState s, double *d_out, double *d_err)
{
    *d_out = *d_err = 0.0;
    for (size_t i = 0; i < r.err.size(); i++) {
        const double o0 = fabs((double)r.out[2 * i] - cos(s.pm)), o1 = fabs((double)r.out[2 * i + 1] - sin(s.pm));
        const double vr = cos(s.pl), vi = -sin(s.pl), re = x[2 * i] * vr - x[2 * i + 1] * vi, im = x[2 * i] * vi + x[2 * i + 1] * vr;
        const double de = fabs(remainder((double)r.err[i] - atan2(im, re), PLL_TWO_PI));
        if (!(o0 <= *d_out)) *d_out = o0;
        if (!(o1 <= *d_out)) *d_out = o1;
        if (!(de <= *d_err)) *d_err = de;
        const double e = (double)r.err[i];
        s.fl = s.fl + p.beta * e;
        s.pl = s.pl + s.fl + p.alpha * e;
        s.pm = s.pm + s.fl * p.mult + p.alpha * e;
        s.fl = s.fl > p.fmax ? p.fmax : s.fl;
        s.fl = s.fl < p.fmin ? p.fmin : s.fl;
        s.pl = s.pl > PLL_TWO_PI ? s.pl - PLL_TWO_PI : s.pl;
        s.pl = s.pl < -PLL_TWO_PI ? s.pl + PLL_TWO_PI : s.pl;
        s.pm = s.pm > PLL_TWO_PI ? s.pm - PLL_TWO_PI : s.pm;
        s.pm = s.pm < -PLL_TWO_PI ? s.pm + PLL_TWO_PI : s.pm;
    }
}

static void locked_case(const char *what, const PllParams &p, const std::vector<float> &x, unsigned long lanes, unsigned long seg)
{
    const unsigned long W = pll_warmup(p.alpha, p.beta, PLL_TOL_PHI / 256.0);
    const Result a = play(x, p, W, lanes, seg, true, pll_initial(p)), s = play(x, p, W, lanes, seg, false, pll_initial(p));
    const double d_out = max_diff(a.out, s.out), d_err = max_diff(a.err, s.err, true);
    printf("%-28s r %.5f W %lu C %lu: speculated %lu rejected %llu repaired %llu, entry error %.2e rad, vs serial out %.2e error %.2e\n", what,
           pll_pole_radius(p.alpha, p.beta), W, a.plan.C, a.plan.nseg, a.rejected, a.repaired, a.entry_err, d_out, d_err);
    CHECK(a.plan.speculate && !s.plan.speculate, "%s: plan", what);
    CHECK(a.rejected == 0 && a.repaired == 0, "%s: a locked loop was rejected", what);
    CHECK(d_out <= 1e-6 && d_err <= 1e-6, "%s: speculative path differs from the serial loop", what);
    CHECK(a.entry_err < PLL_TOL_PHI / 4, "%s: entry error %.2e is not well under the tolerance", what, a.entry_err);
}

// The second mode: one call of the stage over a raw ComplexFloat32 file, against the serial path of the same code.
//   host_pll_check FILE BANDWIDTH FMIN FMAX MULT RATE [SEGMENT]
// prints nseg, rejected, repaired, whether the last segment was repaired, and the largest out / error difference in each quarter of the stream
static int play_file(int argc, char **argv)
{
    if (argc < 7) { fprintf(stderr, "usage: %s FILE BANDWIDTH FMIN FMAX MULT RATE [SEGMENT]\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    std::vector<float> x;
    float buf[4096];
    for (size_t got; (got = fread(buf, sizeof(float), 4096, f)) > 0;) x.insert(x.end(), buf, buf + got);
    fclose(f);
    if (x.size() % 2) { fprintf(stderr, "%s: not a whole number of ComplexFloat32 samples\n", argv[1]); return 2; }
    const PllParams p = make_params(atof(argv[2]), atof(argv[3]), atof(argv[4]), atof(argv[5]), atof(argv[6]));
    const unsigned long seg = argc > 7 ? strtoul(argv[7], nullptr, 10) : 0, n = x.size() / 2;
    const unsigned long W = pll_warmup(p.alpha, p.beta, PLL_TOL_PHI / 256.0);
    const Result a = play(x, p, W, 131072, seg, true, pll_initial(p)), s = play(x, p, W, 131072, seg, false, pll_initial(p));
    printf("n %lu W %lu C %lu speculate %d nseg %lu rejected %llu repaired %llu last_repaired %d\n", n, W, a.plan.C, (int)a.plan.speculate, a.plan.nseg,
           a.rejected, a.repaired, (int)(a.plan.speculate && a.bad[a.plan.nseg - 1]));
    double d_out[4], d_err[4];
    for (int q = 0; q < 4; q++) {
        const unsigned long i0 = n * q / 4, i1 = n * (q + 1) / 4;
        d_out[q] = max_diff(std::vector<float>(a.out.begin() + 2 * i0, a.out.begin() + 2 * i1), std::vector<float>(s.out.begin() + 2 * i0, s.out.begin() + 2 * i1));
        d_err[q] = max_diff(std::vector<float>(a.err.begin() + i0, a.err.begin() + i1), std::vector<float>(s.err.begin() + i0, s.err.begin() + i1), true);
    }
    printf("out %.3e %.3e %.3e %.3e\n", d_out[0], d_out[1], d_out[2], d_out[3]);
    printf("error %.3e %.3e %.3e %.3e\n", d_err[0], d_err[1], d_err[2], d_err[3]);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc > 1) return play_file(argc, argv);
    Rng g;
    // ---- W against the pole radius, for the three loops the tolerances were chosen on
    const PllParams unit = make_params(0.01, 0.19, 0.21, 3.0, 2.0), pilot = make_params(100, 18950, 19050, 2.0, 220500.0), am = make_params(1000, 4900, 5100, 1.0, 44100.0);
    for (const PllParams *p : {&unit, &pilot, &am}) {
        const double r = pll_pole_radius(p->alpha, p->beta), tol_w = PLL_TOL_PHI / 256.0;
        const unsigned long W = pll_warmup(p->alpha, p->beta, tol_w);
        CHECK(r > 0.0 && r < 1.0, "pole radius %g", r);
        CHECK(W >= 1 && PLL_TWO_PI * pow(r, (double)W) <= tol_w * (1 + 1e-9) && PLL_TWO_PI * pow(r, (double)W - 1.0) > tol_w * (1 - 1e-9), "W %lu for r %g", W, r);
        // the roots really are roots: |z|^2 = 1 - alpha for a complex pair
        const double b = p->alpha + p->beta - 2.0, c = 1.0 - p->alpha;
        if (b * b < 4 * c) CHECK(fabs(r * r - c) < 1e-15, "complex pair modulus");
    }
    CHECK(fabs(pilot.alpha - 7.57e-3) < 1e-5 && fabs(pll_pole_radius(pilot.alpha, pilot.beta) - 0.99621) < 1e-5, "pilot loop alpha %.6g r %.6g", pilot.alpha,
          pll_pole_radius(pilot.alpha, pilot.beta));
    CHECK(pll_warmup(0.0, 0.0, 1e-9) == 0 && pll_warmup(0.5, 0.1, 0.0) == 0, "a loop that does not contract has no warm-up");

    // ---- the plan
    {
        const unsigned long W = pll_warmup(unit.alpha, unit.beta, PLL_TOL_PHI / 256.0);
        PllPlan q = pll_make_plan(1 << 16, unit, W, 131072, 64, true);
        CHECK(q.speculate && q.C == 64 && q.nseg == 1024, "2^16 samples in segments of 64");
        q = pll_make_plan(65, unit, W, 131072, 64, true);
        CHECK(!q.speculate && q.nseg == 1 && q.C == 65, "a call shorter than the warm-up is serial");
        q = pll_make_plan(1 << 16, unit, W, 131072, 64, false);
        CHECK(!q.speculate, "speculate=0");
        q = pll_make_plan(1 << 24, pilot, 5960, 131072, 0, true);
        CHECK(q.speculate && q.C == 128 && q.nseg == 131072, "2^24 samples fill 131072 lanes");
        q = pll_make_plan(1 << 12, pilot, 5960, 131072, 0, true);
        CHECK(!q.speculate, "W >= n is serial");
        q = pll_make_plan(0, pilot, 5960, 131072, 0, true);
        CHECK(!q.speculate && q.nseg == 0, "n = 0");
        CHECK(pll_lane_start(3, 64, 541) == 0 && pll_lane_start(9, 64, 541) == 35, "lane start");
    }

    // ---- locked loops: nothing rejected, within 1e-6 of the serial loop
    const double pi = 3.14159265358979323846;
    const unsigned long n = 1 << 16;
    const std::vector<float> x_unit = tone(n, 2 * pi * 0.1, 0.3, 0.1, g);
    locked_case("unit-test loop x3", unit, x_unit, 131072, 64);
    locked_case("unit-test loop x1/16", make_params(0.01, 0.19, 0.21, 1.0 / 16, 2.0), x_unit, 131072, 64);
    locked_case("stereo pilot loop", pilot, tone(1 << 18, 2 * pi * 19000.0 / 220500.0, 1.0, 0.3, g), 1 << 10, 0);
    locked_case("AM synchronous loop", am, tone(1 << 16, 2 * pi * 5020.0 / 44100.0, 2.0, 0.1, g), 131072, 0);

    // ---- a warm-up that is too short: rejected, repaired, and still the serial loop
    {
        const Result a = play(x_unit, unit, 8, 131072, 64, true, pll_initial(unit)), s = play(x_unit, unit, 8, 131072, 64, false, pll_initial(unit));
        const double d_out = max_diff(a.out, s.out), d_err = max_diff(a.err, s.err, true);
        printf("%-28s speculated %lu rejected %llu repaired %llu, vs serial out %.2e error %.2e\n", "warmup=8", a.plan.nseg, a.rejected, a.repaired, d_out, d_err);
        CHECK(a.rejected > 0 && a.repaired >= a.rejected, "warmup=8 must be repaired");
        CHECK(d_out <= 1e-6 && d_err <= 1e-6, "repaired output differs from the serial loop");
    }
    // ---- pure noise: no lock, mostly repaired; the output is a consistent run of the recurrence
    {
        std::vector<float> xn(2 * n);
        for (auto &v : xn) v = (float)g.gauss();
        const unsigned long W = pll_warmup(unit.alpha, unit.beta, PLL_TOL_PHI / 256.0);
        const Result a = play(xn, unit, W, 131072, 64, true, pll_initial(unit));
        double d_out, d_err;
        replay(xn, unit, a, pll_initial(unit), &d_out, &d_err);
        printf("%-28s speculated %lu rejected %llu repaired %llu, replay out %.2e error %.2e\n", "pure noise", a.plan.nseg, a.rejected, a.repaired, d_out, d_err);
        CHECK(a.repaired == a.plan.nseg - 1, "noise is out of lock: every segment is rerun serially");
        CHECK(d_out <= 1e-6 && d_err <= 1e-6, "noise: replay inconsistent");
        // carrier outside the clamp range: freq_locked sits on the clamp
        const std::vector<float> xc = tone(n, 2 * pi * 0.25 / 2.0, 0.0, 0.05, g);
        const Result c = play(xc, unit, W, 131072, 64, true, pll_initial(unit));
        replay(xc, unit, c, pll_initial(unit), &d_out, &d_err);
        printf("%-28s speculated %lu rejected %llu repaired %llu, replay out %.2e error %.2e\n", "carrier outside the clamp", c.plan.nseg, c.rejected, c.repaired, d_out, d_err);
        CHECK(d_out <= 1e-6 && d_err <= 1e-6, "clamped: replay inconsistent");
    }
    // ---- a NaN: the walk terminates, everything before it is untouched, everything after it is NaN
    {
        std::vector<float> xq = x_unit;
        const unsigned long at = 20000;
        xq[2 * at] = NAN;
        const unsigned long W = pll_warmup(unit.alpha, unit.beta, PLL_TOL_PHI / 256.0);
        const Result a = play(xq, unit, W, 131072, 64, true, pll_initial(unit)), b = play(x_unit, unit, W, 131072, 64, true, pll_initial(unit));
        bool before = true, after = true;
        for (unsigned long i = 0; i < n; i++) {
            if (i < at) before = before && a.err[i] == b.err[i] && a.out[2 * i] == b.out[2 * i] && a.out[2 * i + 1] == b.out[2 * i + 1];
            if (i == at) before = before && a.out[2 * i] == b.out[2 * i];
            if (i >= at) after = after && std::isnan(a.err[i]);
            if (i > at) after = after && std::isnan(a.out[2 * i]) && std::isnan(a.out[2 * i + 1]);
        }
        printf("%-28s rejected %llu repaired %llu\n", "NaN at 20000", a.rejected, a.repaired);
        CHECK(before && after, "NaN handling (before %d after %d)", (int)before, (int)after);
    }
    // ---- ragged calls carry the state: two calls = one call on the serial path, bit for bit
    {
        const PllParams &p = unit;
        std::vector<float> h1(x_unit.begin(), x_unit.begin() + 2 * 777), h2(x_unit.begin() + 2 * 777, x_unit.begin() + 2 * 3000), whole(x_unit.begin(), x_unit.begin() + 2 * 3000);
        const Result a = play(h1, p, 8, 131072, 64, false, pll_initial(p)), b = play(h2, p, 8, 131072, 64, false, a.last), w = play(whole, p, 8, 131072, 64, false, pll_initial(p));
        bool same = true;
        for (size_t i = 0; i < h2.size() / 2; i++) same = same && b.err[i] == w.err[777 + i] && b.out[2 * i] == w.out[2 * (777 + i)];
        CHECK(same, "carried state");
    }
    if (failures) { printf("%d FAILED\n", failures); return 1; }
    printf("OK\n");
    return 0;
}
