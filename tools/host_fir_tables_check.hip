// host_fir_tables_check.hip - what fir_build() makes of a request, on the CPU: (a) fir_resolve() (luaradio_amd/csrc/fir_plan.h) against a LITERAL table,
// (b) every table builder of luaradio_amd/csrc/fir_tables.h against its definition.  The expected values of (a) were derived by hand from the fir_build()
// that spelled the ranges out inline before fir_plan.h existed - not by running fir_resolve(): a row that fails is a change of behaviour, to be explained,
// not re-recorded.  The reference of (b) is a DFT by std::polar in long double, never a call into taps_spectrum(); the slots' bin numbers are the kernels'
// documented index maps, written out again here.  `--requests` prints the rows of (a) that are no refusal (ntaps taps_complex input_complex decim use_fft rot).
//   hipcc --offload-arch=gfx950 -O1 -std=c++17 -I luaradio_amd/csrc -I include -o /tmp/host_fir_tables_check tools/host_fir_tables_check.hip && /tmp/host_fir_tables_check
// (once with -g -Xarch_host -fsanitize=address,undefined as well: a stand-alone program, nothing of it is loaded into an interpreter)
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstring>
#include <vector>
#include "common.h"
#include "kernels_elem.h"
#include "kernels_fft.h"
#include "kernels_fir.h"
#include "kernels_firfft.h"
#include "kernels_firdecfft.h"
#include "kernels_firdecim.h"
#include "kernels_firwin.h"
#include "kernels_firfft4k.h"
#include "kernels_firfft64.h"
using namespace lrhip;
#include "fir_plan.h"
#include "fir_tables.h"

typedef std::complex<long double> cld;
static const long double PI2L = 6.283185307179586476925286766559005768L;
static int bad = 0;
static void fail(const char *what, const char *why, long a = 0, long b = 0) { if (bad++ < 40) printf("MISMATCH %s: %s (%ld, %ld)\n", what, why, a, b); }

// ---- (a) the resolve table
enum : unsigned { T = FIR_TAB_TOEPLITZ, CC = FIR_TAB_TOEPLITZ_CC, C4 = FIR_TAB_CTAPS4, DEC = FIR_TAB_DECFFT, F1K = FIR_TAB_FFT1024, F4K = FIR_TAB_FFT4K, F64 = FIR_TAB_FFT64, LONG = FIR_TAB_FFT64_LONG };
struct Row {
    const char *what;
    FirRequest r;                         // ntaps, taps_complex, input_complex, decim, use_fft, rot
    const char *refusal;                  // the whole message, or nullptr
    bool use_fft, fft_arith, decfft, ctaps4;
    int ksteps, fft4k_V, fft64_np, hist_pad;
    long L;
    unsigned tables;
};
static const char *R_TAPS = "fir: need at least one tap", *R_CPLX = "fir: complex taps require ComplexFloat32 input (firfilter.lua:69-74)", *R_DECIM = "fir: decimation must be >= 1",
                  *R_FRAMING = "fir: the reference's block-emission framing (use_fft = 1) cannot be combined with decimation",
                  *R_MODE = "fir: use_fft must be 0 (direct form), 1 (overlap-save as the reference: block emission), 2 (overlap-save arithmetic, sample-exact emission) or 3 (automatic)",
                  *R_MANY = "fir: too many taps", *R_ROT = "fir: rotator fusion unavailable for this tap count / decimation";
#define NO_PLAN false, false, false, false, 0, 0, 0, 0, 0, 0
// Toeplitz steps: real taps (e + 15 D + M + 3) / 4 with e = 1 on a ComplexFloat32 stream, 3 on a Float32 stream, where the decimation has an instantiation (1 .. 8, 10) and the tap
// array 4 * steps + 15 D + 3 rounded up to 4 floats stays within 24 KB; complex taps (2 + 30 D + 2 M + 3) / 4 at D <= 5 where two arrays of 4 * steps + 30 D + 3 floats stay within 32 KB
static const std::vector<Row> rows = {
    // ---- every refusal, and their order among themselves
    {"no taps", {0, 0, 1, 1, 0, false}, R_TAPS, NO_PLAN},
    {"no taps comes before complex taps on a Float32 stream", {0, 1, 0, 1, 0, false}, R_TAPS, NO_PLAN},
    {"complex taps on a Float32 stream", {16, 1, 0, 1, 0, false}, R_CPLX, NO_PLAN},
    {"... comes before the decimation", {16, 1, 0, 0, 0, false}, R_CPLX, NO_PLAN},
    {"decimation 0", {16, 0, 1, 0, 0, false}, R_DECIM, NO_PLAN},
    {"... comes before use_fft", {16, 0, 1, 0, 9, false}, R_DECIM, NO_PLAN},
    {"framing with decimation", {128, 0, 1, 2, 1, false}, R_FRAMING, NO_PLAN},
    {"use_fft = 7 with decimation: the framing's message comes first", {128, 0, 1, 2, 7, false}, R_FRAMING, NO_PLAN},
    {"use_fft = -1 with decimation: the same", {128, 0, 1, 2, -1, false}, R_FRAMING, NO_PLAN},
    {"use_fft = 4", {128, 0, 1, 1, 4, false}, R_MODE, NO_PLAN},
    {"use_fft = -1", {128, 0, 1, 1, -1, false}, R_MODE, NO_PLAN},
    {"... comes before too many taps", {(1u << 20) + 1, 0, 1, 1, 4, false}, R_MODE, NO_PLAN},
    {"2^20 + 1 taps", {(1u << 20) + 1, 0, 1, 1, 0, false}, R_MANY, NO_PLAN},
    {"... comes before the rotator", {(1u << 20) + 1, 0, 1, 50, 0, true}, R_MANY, NO_PLAN},
    {"2^20 taps: no table but the reversed taps", {1u << 20, 0, 1, 1, 3, false}, nullptr, false, false, false, false, 0, 0, 0, 0, 0, 0},
    {"rotator, 5 890 taps /50: 6 145 staged samples", {5890, 0, 1, 50, 0, true}, R_ROT, NO_PLAN},
    {"rotator, 5 889 taps /50: the LDS-staged decimator has it", {5889, 0, 1, 50, 0, true}, nullptr, false, false, false, false, 0, 0, 0, 0, 0, 0},
    {"rotator on a Float32 stream without a Toeplitz table", {128, 0, 0, 50, 0, true}, R_ROT, NO_PLAN},
    {"rotator, complex taps /6: no table", {64, 1, 1, 6, 0, true}, R_ROT, NO_PLAN},
    {"rotator, complex taps /2", {64, 1, 1, 2, 0, true}, nullptr, false, false, false, false, 48, 0, 0, 1, 0, CC},
    // ---- the shapes that tools/host_fir_form_check.hip names, with that file's numbers
    {"tuner shape: 128 / cf32 / D5, 207 / 4", {128, 0, 1, 5, 0, false}, nullptr, false, false, false, false, 51, 0, 0, 0, 0, T},
    {"... as a Tuner", {128, 0, 1, 5, 0, true}, nullptr, false, false, false, false, 51, 0, 0, 0, 0, T},
    {"headline: 128 / cf32 / D1, 147 / 4", {128, 0, 1, 1, 0, false}, nullptr, false, false, false, false, 36, 0, 0, 0, 0, T},
    {"128 / f32, 149 / 4", {128, 0, 0, 1, 0, false}, nullptr, false, false, false, false, 37, 0, 0, 0, 0, T},
    {"audio tail: 136 / f32 / D5, 217 / 4", {136, 0, 0, 5, 0, false}, nullptr, false, false, false, false, 54, 0, 0, 0, 0, T},
    {"128 / cf32 / D50: no instantiation", {128, 0, 1, 50, 0, false}, nullptr, false, false, false, false, 0, 0, 0, 0, 0, 0},
    {"... as a Tuner", {128, 0, 1, 50, 0, true}, nullptr, false, false, false, false, 0, 0, 0, 0, 0, 0},
    {"Hilbert 65 / f32, 86 / 4", {65, 0, 0, 1, 0, false}, nullptr, false, false, false, false, 21, 0, 0, 0, 0, T},
    {"16 real taps cf32, 35 / 4", {16, 0, 1, 1, 0, false}, nullptr, false, false, false, false, 8, 0, 0, 0, 0, T},
    // complex taps: ctaps4 only for 16 / 32 taps at D = 1; steps and hist_pad = 1 to decimation 5.  (The form check's 80-step row at D = 6 is its "with a table"
    // row, dispatch_mfma_cc's default arm: fir_build() never made that table, and the row "decim-lds v1: complex taps /6" with 0 steps is what it makes)
    {"16 complex taps, 67 / 4", {16, 1, 1, 1, 0, false}, nullptr, false, false, false, true, 16, 0, 0, 1, 0, CC | C4},
    {"... automatic: under 48 taps", {16, 1, 1, 1, 3, false}, nullptr, false, false, false, true, 16, 0, 0, 1, 0, CC | C4},
    {"17 complex taps, 69 / 4", {17, 1, 1, 1, 0, false}, nullptr, false, false, false, false, 17, 0, 0, 1, 0, CC},
    {"32 complex taps, 99 / 4", {32, 1, 1, 1, 0, false}, nullptr, false, false, false, true, 24, 0, 0, 1, 0, CC | C4},
    {"... fast: the overlap-save tables too", {32, 1, 1, 1, 2, false}, nullptr, false, true, false, true, 24, 0, 0, 1, 0, CC | C4 | F1K},
    {"16 complex taps /2, 97 / 4", {16, 1, 1, 2, 0, false}, nullptr, false, false, false, false, 24, 0, 0, 1, 0, CC},
    {"64 complex taps /2, 193 / 4", {64, 1, 1, 2, 0, false}, nullptr, false, false, false, false, 48, 0, 0, 1, 0, CC},
    {"64 complex taps /5, 283 / 4", {64, 1, 1, 5, 0, false}, nullptr, false, false, false, false, 70, 0, 0, 1, 0, CC},
    {"64 complex taps /6: no table, no pad", {64, 1, 1, 6, 0, false}, nullptr, false, false, false, false, 0, 0, 0, 0, 0, 0},
    {"1 000 complex taps, automatic, 2 035 / 4", {1000, 1, 1, 1, 3, false}, nullptr, false, true, false, false, 508, 1024, 0, 1, 0, CC | F1K | F4K | F64},
    // ---- the real-taps Toeplitz table at decimation 8 / 9 / 10 / 11
    {"/8, 252 / 4", {128, 0, 1, 8, 0, false}, nullptr, false, false, false, false, 63, 0, 0, 0, 0, T},
    {"/9", {128, 0, 1, 9, 0, false}, nullptr, false, false, false, false, 0, 0, 0, 0, 0, 0},
    {"/10, 282 / 4", {128, 0, 1, 10, 0, false}, nullptr, false, false, false, false, 70, 0, 0, 0, 0, T},
    {"/11", {128, 0, 1, 11, 0, false}, nullptr, false, false, false, false, 0, 0, 0, 0, 0, 0},
    // ---- the 24 KB bound: 4 * steps + 20 <= 6 144 floats at D = 1, steps <= 1 531
    {"6 108 taps cf32, 6 127 / 4", {6108, 0, 1, 1, 0, false}, nullptr, false, false, false, false, 1531, 0, 0, 0, 0, T},
    {"6 109 taps cf32: 1 532 steps, 6 148 floats", {6109, 0, 1, 1, 0, false}, nullptr, false, false, false, false, 0, 0, 0, 0, 0, 0},
    {"6 106 taps f32, 6 127 / 4", {6106, 0, 0, 1, 0, false}, nullptr, false, false, false, false, 1531, 0, 0, 0, 0, T},
    {"6 107 taps f32", {6107, 0, 0, 1, 0, false}, nullptr, false, false, false, false, 0, 0, 0, 0, 0, 0},
    // ---- the 32 KB bound: 2 x (4 * steps + 36) floats at D = 1, steps <= 1 015
    {"2 014 complex taps, 4 063 / 4", {2014, 1, 1, 1, 0, false}, nullptr, false, false, false, false, 1015, 0, 0, 1, 0, CC},
    {"2 015 complex taps: 1 016 steps, 2 x 4 100 floats", {2015, 1, 1, 1, 0, false}, nullptr, false, false, false, false, 0, 0, 0, 0, 0, 0},
    // ---- overlap-save arithmetic: automatic from 48 taps, the table block (fast, framing) from 32
    {"automatic 47", {47, 0, 1, 1, 3, false}, nullptr, false, false, false, false, 16, 0, 0, 0, 0, T},
    {"automatic 48", {48, 0, 1, 1, 3, false}, nullptr, false, true, false, false, 16, 0, 0, 0, 0, T | F1K},
    {"automatic 48 behind a rotator: direct form", {48, 0, 1, 1, 3, true}, nullptr, false, false, false, false, 16, 0, 0, 0, 0, T},
    {"fast 31", {31, 0, 1, 1, 2, false}, nullptr, false, false, false, false, 12, 0, 0, 0, 0, T},
    {"fast 32", {32, 0, 1, 1, 2, false}, nullptr, false, true, false, false, 12, 0, 0, 0, 0, T | F1K},
    {"fast 128 behind a rotator: no overlap-save tables", {128, 0, 1, 1, 2, true}, nullptr, false, false, false, false, 36, 0, 0, 0, 0, T},
    {"512", {512, 0, 1, 1, 2, false}, nullptr, false, true, false, false, 132, 0, 0, 0, 0, T | F1K},
    {"513: overlap 768", {513, 0, 1, 1, 2, false}, nullptr, false, true, false, false, 133, 768, 0, 0, 0, T | F1K | F4K | F64},
    {"769: 768", {769, 0, 1, 1, 2, false}, nullptr, false, true, false, false, 197, 768, 0, 0, 0, T | F1K | F4K | F64},
    {"770: 1 024", {770, 0, 1, 1, 2, false}, nullptr, false, true, false, false, 197, 1024, 0, 0, 0, T | F1K | F4K | F64},
    {"1 025: 1 024", {1025, 0, 1, 1, 2, false}, nullptr, false, true, false, false, 261, 1024, 0, 0, 0, T | F1K | F4K | F64},
    {"1 281: 1 280", {1281, 0, 1, 1, 2, false}, nullptr, false, true, false, false, 325, 1280, 0, 0, 0, T | F1K | F4K | F64},
    {"600 on a Float32 stream: the overlap is set, the workgroup-per-block tables are not built", {600, 0, 0, 1, 2, false}, nullptr, false, true, false, false, 155, 768, 0, 0, 0, T | F1K | F64},
    {"3 000 on a Float32 stream, automatic", {3000, 0, 0, 1, 3, false}, nullptr, false, true, false, false, 755, 0, 2, 0, 0, T | F1K | LONG},
    {"1 282: the long form, one partition", {1282, 0, 1, 1, 2, false}, nullptr, false, true, false, false, 325, 0, 1, 0, 0, T | F1K | LONG},
    {"2 049", {2049, 0, 1, 1, 2, false}, nullptr, false, true, false, false, 517, 0, 1, 0, 0, T | F1K | LONG},
    {"2 050: two partitions", {2050, 0, 1, 1, 2, false}, nullptr, false, true, false, false, 517, 0, 2, 0, 0, T | F1K | LONG},
    {"4 097", {4097, 0, 1, 1, 2, false}, nullptr, false, true, false, false, 1029, 0, 2, 0, 0, T | F1K | LONG},
    {"4 098: three", {4098, 0, 1, 1, 2, false}, nullptr, false, true, false, false, 1029, 0, 3, 0, 0, T | F1K | LONG},
    {"6 145 (past the 24 KB bound: no Toeplitz table)", {6145, 0, 1, 1, 2, false}, nullptr, false, true, false, false, 0, 0, 3, 0, 0, F1K | LONG},
    {"6 146: four", {6146, 0, 1, 1, 2, false}, nullptr, false, true, false, false, 0, 0, 4, 0, 0, F1K | LONG},
    {"8 192, automatic", {8192, 0, 1, 1, 3, false}, nullptr, false, true, false, false, 0, 0, 4, 0, 0, F1K | LONG},
    {"8 193: the long-form branch says <= 8 193, the block around it <= 8 192", {8193, 0, 1, 1, 2, false}, nullptr, false, false, false, false, 0, 0, 0, 0, 0, 0},
    {"8 193, automatic", {8193, 0, 1, 1, 3, false}, nullptr, false, false, false, false, 0, 0, 0, 0, 0, 0},
    // ---- the reference's framing (1): L = 2^floor(log2(8 M)) - M + 1; outside 32 .. 8 192 taps it keeps the framing without the arithmetic
    {"framing 128: 1 024 - 127", {128, 0, 1, 1, 1, false}, nullptr, true, true, false, false, 36, 0, 0, 0, 897, T | F1K},
    {"framing 100: 512 - 99", {100, 0, 0, 1, 1, false}, nullptr, true, true, false, false, 30, 0, 0, 0, 413, T | F1K},
    {"framing 31: 128 - 30", {31, 0, 1, 1, 1, false}, nullptr, true, false, false, false, 12, 0, 0, 0, 98, T},
    {"framing 9 000: 65 536 - 8 999", {9000, 0, 1, 1, 1, false}, nullptr, true, false, false, false, 0, 0, 0, 0, 56537, 0},
    {"framing 600: the long-filter tables as for fast", {600, 0, 1, 1, 1, false}, nullptr, true, true, false, false, 154, 768, 0, 0, 3497, T | F1K | F4K | F64},
    {"framing 128 behind a rotator: framing, no arithmetic", {128, 0, 1, 1, 1, true}, nullptr, true, false, false, false, 36, 0, 0, 0, 897, T},
    // ---- fast / automatic with decimation fall back to the direct form; the polyphase-FFT decimator only for fast where fir_decfft_supported
    {"fast 128 /4: ceil(128 / 4) = 32", {128, 0, 1, 4, 2, false}, nullptr, false, false, true, false, 48, 0, 0, 0, 0, T | DEC},
    {"... as a Tuner", {128, 0, 1, 4, 2, true}, nullptr, false, false, true, false, 48, 0, 0, 0, 0, T | DEC},
    {"automatic 128 /4", {128, 0, 1, 4, 3, false}, nullptr, false, false, false, false, 48, 0, 0, 0, 0, T},
    {"fast 129 /4: 33 branches taps", {129, 0, 1, 4, 2, false}, nullptr, false, false, false, false, 48, 0, 0, 0, 0, T},
    {"fast 128 /4 on a Float32 stream", {128, 0, 0, 4, 2, false}, nullptr, false, false, false, false, 48, 0, 0, 0, 0, T},
    {"fast 128 /3", {128, 0, 1, 3, 2, false}, nullptr, false, false, false, false, 44, 0, 0, 0, 0, T},
    {"fast 64 /2, 98 / 4", {64, 0, 1, 2, 2, false}, nullptr, false, false, true, false, 24, 0, 0, 0, 0, T | DEC},
    {"fast 128 /5", {128, 0, 1, 5, 2, false}, nullptr, false, false, true, false, 51, 0, 0, 0, 0, T | DEC},
    {"fast 256 /8, (1 + 120 + 259) / 4", {256, 0, 1, 8, 2, false}, nullptr, false, false, true, false, 95, 0, 0, 0, 0, T | DEC},
    {"fast 128 /50", {128, 0, 1, 50, 2, false}, nullptr, false, false, false, false, 0, 0, 0, 0, 0, 0},
};

static void check_resolve()
{
    for (const Row &w : rows) {
        const FirPlan p = fir_resolve(w.r);
        if (w.refusal || p.refusal) {
            if (!w.refusal || !p.refusal || strcmp(w.refusal, p.refusal)) { fail(w.what, p.refusal ? p.refusal : "no refusal"); }
            continue;
        }
        if (p.use_fft != w.use_fft || p.fft_arith != w.fft_arith || p.decfft != w.decfft || p.ctaps4 != w.ctaps4 || p.ksteps != w.ksteps || p.fft4k_V != w.fft4k_V ||
            p.fft64_np != w.fft64_np || p.hist_pad != w.hist_pad || p.L != w.L || p.tables != w.tables || p.mode_req != w.r.use_fft) {
            printf("MISMATCH %s: use_fft %d (want %d), fft_arith %d (%d), decfft %d (%d), ctaps4 %d (%d), ksteps %d (%d), V %d (%d), np %d (%d), hist_pad %d (%d), L %ld (%ld), tables %u (%u), mode_req %d\n",
                   w.what, p.use_fft, w.use_fft, p.fft_arith, w.fft_arith, p.decfft, w.decfft, p.ctaps4, w.ctaps4, p.ksteps, w.ksteps, p.fft4k_V, w.fft4k_V, p.fft64_np, w.fft64_np,
                   p.hist_pad, w.hist_pad, p.L, w.L, p.tables, w.tables, p.mode_req);
            bad++;
        }
    }
}

// ---- (b) the tables
// asymmetric taps (a symmetric set hides a reversal or a conjugation): a fixed pseudo-random sequence under a slow one-sided decay
static std::vector<float> make_taps(int M, int taps_complex)
{
    std::vector<float> h((size_t)M * (taps_complex ? 2 : 1));
    unsigned s = 12345u + (unsigned)M;
    for (size_t i = 0; i < h.size(); i++) {
        s = s * 1664525u + 1013904223u;
        h[i] = ((float)(s >> 8) / 8388608.0f - 1.0f) * (1.0f / (1.0f + (float)(i / (taps_complex ? 2 : 1)) / 256.0f));
    }
    return h;
}
// the definition: H[k] = (1 / N) sum over m0 <= m < m1 of h[m] W_N^(k (m - m0)) - only these taps, the partition's delay not folded in
static std::vector<cld> ref_spectrum(const std::vector<float> &h, int taps_complex, int m0, int m1, int N)
{
    std::vector<cld> W((size_t)N), H((size_t)N);
    for (int j = 0; j < N; j++) W[j] = std::polar(1.0L, -PI2L * (long double)j / (long double)N);
    for (int k = 0; k < N; k++) {
        cld s = 0;
        for (int m = m0; m < m1; m++) s += (taps_complex ? cld(h[2 * m], h[2 * m + 1]) : cld(h[m], 0)) * W[(size_t)(((long)k * (m - m0)) % N)];
        H[k] = s / (long double)N;
    }
    return H;
}
// The tolerance of an H slot.  The builder's sum in double is exact to about M * 2^-52 of sum |h| / N, far below a Float32 ulp, so builder and reference are two
// correct Float32 roundings of all but the same number, and |H| <= sum |h| / N: they differ by at most the spacing of Float32 at that magnitude
static float h_tol(const std::vector<float> &h, int taps_complex, int m0, int m1, int N)
{
    double s = 0;
    for (int m = m0; m < m1; m++) s += taps_complex ? std::hypot((double)h[2 * m], (double)h[2 * m + 1]) : std::fabs((double)h[m]);
    const float b = (float)(s / N);
    return std::nextafter(b, INFINITY) - b;
}
static const float TW_TOL = 1.1920929e-07f;      // a phasor: |cos|, |sin| <= 1, the spacing of Float32 below 2 (the angle in double is off by 1e-16)

// slots [o, o + n) of table t against ref[bin(s)]; want_each >= 0: the bins hit are exactly those with (bin % 4 == want_each or want_each == 4: all), once each
template <typename BinOf>
static void check_h(const char *what, const std::vector<float> &t, size_t o, int n, const std::vector<cld> &ref, float tol, BinOf bin, int want_each)
{
    std::vector<int> hits(ref.size(), 0);
    if (2 * (o + n) > t.size()) return fail(what, "section past the end of the table", (long)(o + n), (long)t.size());
    for (int s = 0; s < n; s++) {
        const int k = bin(s);
        if (k < 0 || k >= (int)ref.size()) { fail(what, "bin out of range", s, k); continue; }
        hits[k]++;
        const float wr = (float)ref[k].real(), wi = (float)ref[k].imag(), gr = t[2 * (o + s)], gi = t[2 * (o + s) + 1];
        if (!(std::fabs(gr - wr) <= tol) || !(std::fabs(gi - wi) <= tol)) fail(what, "slot differs from the reference bin", s, k);
    }
    if (want_each >= 0)
        for (int k = 0; k < (int)ref.size(); k++)
            if (hits[k] != ((want_each == 4 || k % 4 == want_each) ? 1 : 0)) { fail(what, "slots are no bijection onto the bins", k, hits[k]); break; }
}
// t[o + r cols + c] = W_N^(r c)
static void check_tw(const char *what, const std::vector<float> &t, size_t o, int rows, int cols, int N)
{
    for (int r = 0; r < rows; r++)
        for (int c = 0; c < cols; c++) {
            const cld w = std::polar(1.0L, -PI2L * (long double)((r * c) % N) / (long double)N);
            const size_t s = o + (size_t)r * cols + c;
            if (!(std::fabs(t[2 * s] - (float)w.real()) <= TW_TOL) || !(std::fabs(t[2 * s + 1] - (float)w.imag()) <= TW_TOL)) fail(what, "twiddle", r, c);
        }
}
// the index maps, from the kernels' descriptions.  1024-point kernels (kernels_firfft.h): register 4 j + k3 of lane (k1, q) = (lane >> 2, lane & 3) holds bin
// k1 + 16 (4 j + q) + 256 k3; with the register <-> row transposes (LRHIP_FFT_E2_SWAP) the lane is (q, k1) = (lane >> 4, lane & 15)
static int bin_round2(int s, bool swapped)
{
    const int reg = s >> 6, lane = s & 63, j = reg >> 2, k3 = reg & 3, q = swapped ? lane >> 4 : lane & 3, k1 = swapped ? lane & 15 : lane >> 2;
    return k1 + 16 * (4 * j + q) + 256 * k3;
}
// 64 x 64 form (kernels_firfft64.h): row r of the table is the transform's row k1 = f64_index(r), column l is bin 64 k1 + l
static int bin_64x64(int s) { return 64 * f64_index(s >> 6) + (s & 63); }

static void check_fft1024(int M, int taps_complex)
{
    char what[96];
    const std::vector<float> h = make_taps(M, taps_complex), t = fir_fft1024_tables(h.data(), (unsigned)M, taps_complex);
    const int nparts = (M + 511) / 512;
    if (t.size() != (size_t)nparts * FFT_TABLE_ELEMS * 2) return fail("1024-point set", "size", M, (long)t.size());
    for (int part = 0; part < nparts; part++) {
        const int m0 = 512 * part, m1 = std::min(M, m0 + 512);
        const std::vector<cld> ref = ref_spectrum(h, taps_complex, m0, m1, 1024);
        const float tol = h_tol(h, taps_complex, m0, m1, 1024);
        const size_t o = (size_t)part * FFT_TABLE_ELEMS;
        snprintf(what, sizeof what, "1024-point set, %d taps%s, partition %d", M, taps_complex ? " (complex)" : "", part);
        check_tw(what, t, o, 16, 64, 1024);
        check_h(what, t, o + 1024, 1024, ref, tol, [](int s) { return bin_round2(s, false); }, 4);
        check_tw(what, t, o + 2048, 16, 4, 64);
#if LRHIP_FFT_E2_SWAP
        check_h(what, t, o + FFT_TABLE_HSW, 1024, ref, tol, [](int s) { return bin_round2(s, true); }, 4);
#endif
    }
}
static void check_fft4k(int M, int taps_complex)
{
    char what[96];
    const std::vector<float> h = make_taps(M, taps_complex);
    std::vector<double> Hr, Hi;
    taps_spectrum(h.data(), taps_complex, 0, (unsigned)M, 4096, Hr, Hi);      // (the builders' input, as fir_build() hands it to them - not the reference)
    const std::vector<float> t4 = fir_fft4k_tables(Hr, Hi), t6 = fir_fft64_tables(Hr, Hi);
    const std::vector<cld> ref = ref_spectrum(h, taps_complex, 0, M, 4096);
    const float tol = h_tol(h, taps_complex, 0, M, 4096);
    snprintf(what, sizeof what, "4096-point workgroup set, %d taps%s", M, taps_complex ? " (complex)" : "");
    if (t4.size() != (size_t)F4K_TABLE_ELEMS * 2) return fail(what, "size");
    check_tw(what, t4, 0, 16, 64, 1024);
    check_tw(what, t4, 1024, 16, 4, 64);
    check_tw(what, t4, 1024 + 64, 4, 16, 64);      // c[w][i] = W_64^(i w)
    check_tw(what, t4, F4K_TAB_B, 4, 64, 4096);    // b[w][t] = W_4096^(t w)
    for (int w = 0; w < 4; w++)                    // wave w holds the bins w + 4 k' in the 1024-point order of k'
        check_h(what, t4, (size_t)F4K_TAB_H + 1024 * w, 1024, ref, tol, [w](int s) { return w + 4 * bin_round2(s, false); }, w);
    snprintf(what, sizeof what, "64 x 64 set, %d taps%s", M, taps_complex ? " (complex)" : "");
    if (t6.size() != (size_t)F64_TABLE_ELEMS * 2) return fail(what, "size");
    check_tw(what, t6, 0, 16, 64, 1024);           // C[c][t] = W_1024^(t c)
    check_tw(what, t6, F64_TAB_D, 4, 64, 4096);    // D[d][t] = W_4096^(t d)
    check_h(what, t6, F64_TAB_H, 4096, ref, tol, bin_64x64, 4);
    for (int k1 = 0; k1 < 64; k1++)                // Hsym[k1][l <= 32] = H(64 k1 + l)
        check_h(what, t6, (size_t)F64_TAB_HSYM + (size_t)k1 * F64_HSYM_ROW, 33, ref, tol, [k1](int s) { return 64 * k1 + s; }, -1);
}
static void check_fft64_long(int M, int taps_complex)
{
    char what[96];
    const std::vector<float> h = make_taps(M, taps_complex);
    const int np = (M + 2046) / 2048, nsets = np > 2 ? 2 : 1;
    const std::vector<float> t = fir_fft64_long_tables(h.data(), (unsigned)M, taps_complex, np);
    if (t.size() != (size_t)nsets * F64_TABLE_ELEMS2 * 2) return fail("long 64 x 64 set", "size", M, (long)t.size());
    for (int set = 0; set < nsets; set++) {
        snprintf(what, sizeof what, "long 64 x 64 set %d, %d taps", set, M);
        check_tw(what, t, (size_t)set * F64_TABLE_ELEMS2, 16, 64, 1024);
        check_tw(what, t, (size_t)set * F64_TABLE_ELEMS2 + F64_TAB_D, 4, 64, 4096);
    }
    for (int part = 0; part < np; part++) {
        // one partition: all taps (up to 2 049); more: 2 048 taps each, the last one what is left (up to 2 049)
        const int m0 = np == 1 ? 0 : 2048 * part, m1 = part + 1 == np ? M : 2048 * (part + 1);
        const std::vector<cld> ref = ref_spectrum(h, taps_complex, m0, m1, 4096);
        const float tol = h_tol(h, taps_complex, m0, m1, 4096);
        snprintf(what, sizeof what, "long 64 x 64 form, %d taps%s, partition %d", M, taps_complex ? " (complex)" : "", part);
        const size_t so = (size_t)(part / 2) * F64_TABLE_ELEMS2;      // partitions (0, 1) in the first set, (2, 3) in the second: H | H1
        check_h(what, t, so + (part % 2 ? F64_TAB_H1 : F64_TAB_H), 4096, ref, tol, bin_64x64, 4);
        if (part == 0)
            for (int k1 = 0; k1 < 64; k1++) check_h(what, t, (size_t)F64_TAB_HSYM + (size_t)k1 * F64_HSYM_ROW, 33, ref, tol, [k1](int s) { return 64 * k1 + s; }, -1);
    }
}
// polyphase-FFT decimator (kernels_firdecfft.h): tw[k1][u] = W_256^(k1 u) | G_rho[k], rho < D, the 256-point response (1 / 256 folded in) of the branch
// g[D q + r], r = D - 1 - rho, of g[i] = h[i] e^{-j w i}, bin k = k1 + 16 k2 at (rho / 4) 1024 + 64 k2 + 16 (rho % 4) + k1 for the D / 4 full quads and at
// 256 (rho - 4 (D / 4)) + 16 k2 + k1 behind them | the output phasors e^{+j w D k}, k < 256
static void check_decfft(int M, int taps_complex, int D, double omega)
{
    char what[96];
    snprintf(what, sizeof what, "decimator set, %d taps%s /%d, omega %g", M, taps_complex ? " (complex)" : "", D, omega);
    const std::vector<float> h = make_taps(M, taps_complex), t = fir_decfft_tables(h.data(), M, taps_complex, D, omega);
    if (t.size() != (size_t)df_table_elems(D) * 2 || df_table_elems(D) != 256 + 256 * D + 256) return fail(what, "size");
    check_tw(what, t, 0, 16, 16, 256);
    long double turns = (long double)omega / PI2L;
    turns -= floorl(turns);
    const auto frac = [](long double f) { return f - floorl(f); };
    const float tol = h_tol(h, taps_complex, 0, M, 256);      // (|g| = |h|; a branch sums a subset of them)
    std::vector<int> used((size_t)256 * D, 0);
    for (int rho = 0; rho < D; rho++) {
        const int r = D - 1 - rho;
        std::vector<cld> ref(256);
        for (int k = 0; k < 256; k++) {
            cld s = 0;
            for (int q = 0; D * q + r < M; q++) {
                const int i = D * q + r;
                s += (taps_complex ? cld(h[2 * i], h[2 * i + 1]) : cld(h[i], 0)) * std::polar(1.0L, -PI2L * frac(turns * i)) * std::polar(1.0L, -PI2L * (long double)((q * k) % 256) / 256.0L);
            }
            ref[k] = s / 256.0L;
        }
        const int A = D / 4;
        const size_t base = rho < 4 * A ? (size_t)256 + (size_t)(rho / 4) * 1024 + 16 * (rho % 4) : (size_t)256 + (size_t)A * 1024 + (size_t)(rho - 4 * A) * 256;
        const int k2_stride = rho < 4 * A ? 64 : 16;
        for (int k = 0; k < 256; k++) {
            const size_t s = base + (size_t)(k >> 4) * k2_stride + (k & 15);
            if (s < 256 || s >= (size_t)256 + 256 * D || used[s - 256]++) { fail(what, "branch slots overlap or leave the section", rho, k); continue; }
            check_h(what, t, s, 1, ref, tol, [k](int) { return k; }, -1);
        }
    }
    for (int u : used) if (u != 1) { fail(what, "branch slots do not cover the section"); break; }
    for (int k = 0; k < 256; k++) {
        const cld w = std::polar(1.0L, PI2L * frac(turns * (long double)D * (long double)k));
        const size_t s = (size_t)256 + 256 * D + k;
        if (!(std::fabs(t[2 * s] - (float)w.real()) <= TW_TOL) || !(std::fabs(t[2 * s + 1] - (float)w.imag()) <= TW_TOL)) fail(what, "output phasor", k);
    }
}
// the tables of the direct forms: exact copies
static void check_direct_tables()
{
    for (int tc = 0; tc < 2; tc++) {
        const int M = 17, ts = tc + 1;
        const std::vector<float> h = make_taps(M, tc), rev = fir_reversed_taps(h.data(), M, tc);
        if (rev.size() != (size_t)M * ts) return fail("reversed taps", "size");
        for (int i = 0; i < M; i++)
            for (int c = 0; c < ts; c++) if (rev[(size_t)i * ts + c] != h[(size_t)(M - 1 - i) * ts + c]) fail("reversed taps", "element", i, c);
    }
    {   // real taps at decimation D: [3 + 15 D zeros | reversed taps | zeros] in fir_taps_len(D, steps) floats
        const int M = 33, D = 5, ks = 28, zl = 3 + 15 * D;
        const std::vector<float> h = make_taps(M, 0), rev = fir_reversed_taps(h.data(), M, 0), t = fir_toeplitz_taps(rev, M, D, ks);
        if (t.size() != (size_t)fir_taps_len(D, ks) || t.size() < (size_t)zl + M) return fail("Toeplitz taps", "size");
        for (size_t i = 0; i < t.size(); i++) if (t[i] != (i >= (size_t)zl && i < (size_t)zl + M ? h[M - 1 - (i - zl)] : 0.f)) fail("Toeplitz taps", "element", (long)i);
    }
    {   // complex taps: two such arrays of 2 M taps at decimation 2 D, re = (hr, -hi), im = (hi, hr) per reversed tap, and the short-window table (re, im, -im, re)
        const int M = 16, D = 2, ks = 24, zl = 3 + 15 * 2 * D, len = fir_taps_len(2 * D, ks);
        const std::vector<float> h = make_taps(M, 1), rev = fir_reversed_taps(h.data(), M, 1), t = fir_toeplitz_cc_taps(rev, M, D, ks), t4 = fir_ctaps4_table(rev, M);
        if (t.size() != (size_t)2 * len || len < zl + 2 * M || t4.size() != (size_t)4 * M) return fail("complex Toeplitz taps", "size");
        for (int i = 0; i < len; i++) {
            const int j = (i - zl) / 2, odd = (i - zl) & 1;
            const bool in = i >= zl && i < zl + 2 * M;
            const float hr = in ? h[2 * (M - 1 - j)] : 0.f, hi = in ? h[2 * (M - 1 - j) + 1] : 0.f;
            if (t[i] != (in ? (odd ? -hi : hr) : 0.f) || t[(size_t)len + i] != (in ? (odd ? hr : hi) : 0.f)) fail("complex Toeplitz taps", "element", i);
        }
        for (int j = 0; j < M; j++) {
            const float hr = h[2 * (M - 1 - j)], hi = h[2 * (M - 1 - j) + 1];
            if (t4[4 * j] != hr || t4[4 * j + 1] != hi || t4[4 * j + 2] != -hi || t4[4 * j + 3] != hr) fail("short-window table", "element", j);
        }
    }
}

int main(int argc, char **argv)
{
    if (argc > 1 && !strcmp(argv[1], "--requests")) {
        for (const Row &w : rows)
            if (!w.refusal) printf("%u %d %d %u %d %d\n", w.r.ntaps, w.r.taps_complex, w.r.input_complex, w.r.decim, w.r.use_fft, (int)w.r.rot);
        return 0;
    }
    check_resolve();
    check_direct_tables();
    // the smallest tap counts that reach each builder: 1 and 2 partitions of the 1024-point set, both ends of the 4096-point sets, 1 / 2 / 3 partitions of the long form
    for (int tc = 0; tc < 2; tc++) {
        check_fft1024(33, tc);
        check_fft1024(600, tc);
        check_fft4k(513, tc);
        check_fft4k(1281, tc);
        check_fft64_long(1282, tc);
        check_fft64_long(2050, tc);
    }
    check_fft64_long(4098, 0);
    check_fft64_long(4098, 1);
    const int ds[4] = {2, 4, 5, 8};
    for (int D : ds)
        for (int tc = 0; tc < 2; tc++) {
            check_decfft(128, tc, D, 0.0);
            check_decfft(128, tc, D, -1.4247585730565955);
        }
    printf("%zu resolve rows, tables of 33 / 600 / 513 / 1281 / 1282 / 2050 / 4098 taps and the decimator at /2 /4 /5 /8\n", rows.size());
    printf(bad ? "FAILED (%d)\n" : "OK\n", bad);
    return bad ? 1 : 0;
}
