// host_fir_form_check.hip - the FIR stage's choice of kernel form (luaradio_amd/csrc/fir_form.h) against a LITERAL table, on the CPU.  The expected
// values were derived by hand from the cascades that FirStage::core(), launch_fft(), the dispatch_* switches, align(), direct_io_ok() and raw_path_ok()
// spelled out before fir_form.h existed - not by running fir_form(): a row that fails is a change of behaviour, to be explained, not re-recorded.
//   hipcc --offload-arch=gfx950 -O1 -std=c++17 -I luaradio_amd/csrc -I include -o /tmp/host_fir_form_check tools/host_fir_form_check.hip && /tmp/host_fir_form_check
#include <cmath>
#include <cstdio>
#include <vector>
#include "common.h"
#include "kernels_elem.h"
#include "kernels_fft.h"
#include "kernels_fir.h"
#include "kernels_firfft.h"
#include "kernels_firdecfft.h"
#include "kernels_firdecim.h"
#include "kernels_firfft4k.h"
using namespace lrhip;
#include "fir_form.h"

typedef FirForm F;
typedef FirFftForm X;
// shapes as fir_resolve() (fir_plan.h) makes them of a request: the resolve table of tools/host_fir_tables_check.hip pins the request behind each of the
// shapes named below to these numbers.  ks: fir_mfma_ksteps(M, D, S) = (4 / S - 1 + 15 D + M + 3) / 4 where a Toeplitz table exists, else 0
static FirShape shp(int M, int S, unsigned D, int ks) { FirShape s; s.M = M; s.S = S; s.D = D; s.ksteps = ks; return s; }
static FirShape ctaps(FirShape s, bool table4 = false) { s.taps_complex = 1; s.ctaps4 = table4; return s; }
static FirShape rot(FirShape s) { s.rot = true; return s; }
static FirShape post(FirShape s) { s.post_disc = true; return s; }
static FirShape pre(FirShape s) { s.pre_disc = true; return s; }
static FirShape rel(FirShape s, bool nw1 = false) { s.rel_rot = true; s.rel_nw1 = nw1; return s; }
static FirShape iir(FirShape s) { s.iir_fused = true; return s; }
static FirShape decf(FirShape s) { s.decfft = true; return s; }
static FirShape framed(FirShape s) { s.use_fft = true; return s; }
// overlap-save arithmetic: V = overlap of the 4096-point kernels (513 .. 1 281 taps: max(768, 256 ceil((M - 1) / 256))), np = partitions of the
// 64 x 64 form at an overlap of 2 048 (1 282 .. 8 192 taps: (M + 2 046) / 2 048)
static FirShape fft(int M, int S, int V = 0, int np = 0) { FirShape s = shp(M, S, 1, 0); s.fft_arith = true; s.fft4k_V = V; s.fft64_np = np; return s; }
template <typename Fn> static FirKnobs K(Fn f) { FirKnobs k; f(k); return k; }
static const FirKnobs DEF;

struct Row {
    const char *what;
    FirShape s; FirKnobs k; bool aligned;
    F form;
    unsigned long align; bool direct_io, raw;      // FirStage::align(), direct_io_ok() (a stage without fix_src), raw_path_ok() (records in front, an aligned chunk with output)
};
struct FftRow {
    const char *what;
    FirShape s; FirKnobs k; long n_out; int num_cus;
    X form;
};
struct Pred { const char *what; bool got, want; };

int main()
{
    const FirShape tuner = shp(128, 2, 5, 51), lp128 = shp(128, 2, 1, 36), lp128r = shp(128, 1, 1, 37), tail = shp(136, 1, 5, 54), nbfm = shp(128, 2, 50, 0);
    const std::vector<Row> rows = {
        // ---- every form (register-window kernels for Float32 / the Tuner are opt-in: no default-knob row can reach them)
        {"decfft /4", decf(shp(128, 2, 4, 48)), DEF, true, F::DecFft, 1, true, false},
        {"decfft /4, unaligned chunk: down the cascade, direct kernel", decf(shp(128, 2, 4, 48)), DEF, false, F::Direct, 1, true, false},
        {"decfft /4 tuner + disc, unaligned: Toeplitz form named, launch errors", post(rot(decf(shp(128, 2, 4, 48)))), DEF, false, F::MfmaPersistent, 1, true, false},
        {"overlap-save 128 taps cf32", fft(128, 2), DEF, true, F::OverlapSave, 896, true, false},
        {"overlap-save 128 taps f32", fft(128, 1), DEF, true, F::OverlapSave, 1792, true, false},
        {"overlap-save 400 taps f32 behind a discriminator", pre(fft(400, 1)), DEF, true, F::OverlapSave, 1152, false, false},
        {"overlap-save, reference framing", framed(fft(128, 2)), DEF, true, F::OverlapSave, 896, false, false},
        {"win-real (LRHIP_FIR_WIN_REAL)", lp128r, K([](FirKnobs &k) { k.win_real = true; }), true, F::WinReal, 1, false, false},
        {"... default knobs: persistent Toeplitz, 37 steps", lp128r, DEF, true, F::MfmaPersistent, 1, true, false},
        {"... LRHIP_NO_FIR_WIN wins over LRHIP_FIR_WIN_REAL", lp128r, K([](FirKnobs &k) { k.win_real = k.no_win = true; }), true, F::MfmaPersistent, 1, true, false},
        {"win-real 32 taps beats short-real", shp(32, 1, 1, 13), K([](FirKnobs &k) { k.win_real = true; }), true, F::WinReal, 1, false, false},
        {"win-cplx (LRHIP_FIR_WIN_CPLX)", tuner, K([](FirKnobs &k) { k.win_cplx = true; }), true, F::WinCplx, 1, false, false},
        {"... tuner + disc: no tile grid to follow", rel(post(rot(tuner))), K([](FirKnobs &k) { k.win_cplx = true; }), true, F::WinCplx, 1, false, false},
        {"... LRHIP_NO_FIR_WIN", tuner, K([](FirKnobs &k) { k.win_cplx = k.no_win = true; }), true, F::MfmaPersistent, 1, true, true},
        {"win-short 16", shp(16, 2, 1, 8), DEF, true, F::WinShort, 1, true, false},
        {"win-short 32", shp(32, 2, 1, 12), DEF, true, F::WinShort, 1, true, false},
        {"win-short 64", shp(64, 2, 1, 20), DEF, true, F::WinShort, 1, true, false},
        {"... LRHIP_NO_FIR_WIN_SHORT", shp(16, 2, 1, 8), K([](FirKnobs &k) { k.no_win_short = true; }), true, F::MfmaGeneric, 1, true, false},
        {"... LRHIP_NO_FIR_WIN", shp(16, 2, 1, 8), K([](FirKnobs &k) { k.no_win = true; }), true, F::MfmaGeneric, 1, true, false},
        {"... with a rotator in front: Toeplitz", rot(shp(16, 2, 1, 8)), DEF, true, F::MfmaGeneric, 1, true, false},
        {"win-short-c 16 complex taps", ctaps(shp(16, 2, 1, 16), true), DEF, true, F::WinShortC, 1, true, false},
        {"... table not built: two-filter Toeplitz", ctaps(shp(16, 2, 1, 16)), DEF, true, F::MfmaCc, 1, true, false},
        {"... LRHIP_NO_FIR_WIN_SHORT", ctaps(shp(16, 2, 1, 16), true), K([](FirKnobs &k) { k.no_win_short = true; }), true, F::MfmaCc, 1, true, false},
        {"short-real 16", shp(16, 1, 1, 9), DEF, true, F::ShortReal, 1, false, false},
        {"short-real 32", shp(32, 1, 1, 13), DEF, true, F::ShortReal, 1, false, false},
        {"... 64 taps f32: Toeplitz", shp(64, 1, 1, 21), DEF, true, F::MfmaGeneric, 1, true, false},
        {"... LRHIP_NO_FIR_WIN leaves it (no window kernel)", shp(16, 1, 1, 9), K([](FirKnobs &k) { k.no_win = true; }), true, F::ShortReal, 1, false, false},
        {"... LRHIP_NO_FIR_WIN_SHORT", shp(16, 1, 1, 9), K([](FirKnobs &k) { k.no_win_short = true; }), true, F::MfmaGeneric, 1, true, false},
        {"win-pair: the WBFM audio filter", tail, DEF, true, F::WinPair, 1, true, false},
        {"... with the de-emphasis recurrence", iir(tail), DEF, true, F::WinPair, 12800, true, false},
        {"... LRHIP_NO_FIR_WIN: 54 steps, generic", tail, K([](FirKnobs &k) { k.no_win = true; }), true, F::MfmaGeneric, 1, true, false},
        {"decim-lds v2: Tuner /50", nbfm, DEF, true, F::DecimLds2, 1, true, true},
        {"... LRHIP_DECIM_V1", nbfm, K([](FirKnobs &k) { k.decim_v1 = true; }), true, F::DecimLds1, 1, true, true},
        {"decim-lds v1: f32 stream /50", shp(128, 1, 50, 0), DEF, true, F::DecimLds1, 1, true, false},
        {"decim-lds v1: complex taps /6", ctaps(shp(64, 2, 6, 0)), DEF, true, F::DecimLds1, 1, true, false},
        {"complex taps + rotator: no LDS-staged form", rot(ctaps(shp(64, 2, 6, 0))), DEF, true, F::Direct, 1, false, false},
        {"mfma-cc /2", ctaps(shp(64, 2, 2, 48)), DEF, true, F::MfmaCc, 1, true, false},
        {"mfma-cc /5", ctaps(shp(64, 2, 5, 70)), DEF, true, F::MfmaCc, 1, true, false},
        {"... unaligned chunk", ctaps(shp(64, 2, 2, 48)), DEF, false, F::Direct, 1, true, false},
        {"... /6 with a table (dispatch_mfma_cc's default arm)", ctaps(shp(64, 2, 6, 80)), DEF, true, F::DecimLds1, 1, true, false},
        // ---- persistent / generic Toeplitz: the three persistent step counts and their neighbours
        {"headline: 128 taps cf32, 36 steps", lp128, DEF, true, F::MfmaPersistent, 1, true, false},
        {"... unaligned chunk: direct kernel", lp128, DEF, false, F::Direct, 1, true, false},
        {"... unaligned with a rotator: Toeplitz named, launch errors", rot(lp128), DEF, false, F::MfmaPersistent, 1, true, false},
        {"... unaligned with a discriminator: the same", post(lp128), DEF, false, F::MfmaPersistent, 1, true, false},
        {"D = 1, 35 steps", shp(124, 2, 1, 35), DEF, true, F::MfmaGeneric, 1, true, false},
        {"D = 1, 38 steps", shp(132, 1, 1, 38), DEF, true, F::MfmaGeneric, 1, true, false},
        {"Tuner D = 5, 51 steps", tuner, DEF, true, F::MfmaPersistent, 1, true, true},
        {"D = 5, 50 steps", shp(124, 2, 5, 50), DEF, true, F::MfmaGeneric, 1, true, false},
        {"D = 5, 52 steps", shp(132, 2, 5, 52), DEF, true, F::MfmaGeneric, 1, true, false},
        {"D = 5, f32 stream, 51 steps", shp(126, 1, 5, 51), DEF, true, F::MfmaPersistent, 1, true, false},
        // tuner + discriminator, window-relative phasors: the chunk follows the tile grid
        {"tuner + disc D = 5", rel(post(rot(tuner))), DEF, true, F::MfmaPersistent, 5120, true, false},
        {"... one-wave workgroups", rel(post(rot(tuner)), true), DEF, true, F::MfmaPersistent, 1280, true, false},
        {"... LRHIP_FIR_D5_NACC=1", rel(post(rot(tuner))), K([](FirKnobs &k) { k.d5_nacc = 1; }), true, F::MfmaPersistent, 2560, true, false},
        {"... exact phasors", post(rot(tuner)), DEF, true, F::MfmaPersistent, 1, true, false},
        {"rotator + filter + disc D = 1", rel(post(rot(lp128))), DEF, true, F::MfmaPersistent, 4096, true, false},
        // disc_ksteps(D) shapes: tuner + discriminator at decimation 4 / 8 / 10, 128 taps
        {"tuner + disc /4, 48 steps", rel(post(rot(shp(128, 2, 4, 48)))), DEF, true, F::MfmaPersistent, 1, true, false},
        {"tuner /4 alone", rot(shp(128, 2, 4, 48)), DEF, true, F::MfmaGeneric, 1, true, false},
        {"decimator /4 + disc, no rotator (launch errors)", post(shp(128, 2, 4, 48)), DEF, true, F::MfmaGeneric, 1, true, false},
        {"tuner + disc /4, 47 steps", post(rot(shp(124, 2, 4, 47))), DEF, true, F::MfmaGeneric, 1, true, false},
        {"tuner + disc /8, 63 steps", post(rot(shp(128, 2, 8, 63))), DEF, true, F::MfmaPersistent, 1, true, false},
        {"tuner + disc /10, 70 steps", post(rot(shp(128, 2, 10, 70))), DEF, true, F::MfmaPersistent, 1, true, false},
        {"tuner + disc /10, 71 steps", post(rot(shp(130, 2, 10, 71))), DEF, true, F::MfmaGeneric, 1, true, false},
        {"tuner + disc /3: no such kernel", post(rot(shp(128, 2, 3, 44))), DEF, true, F::MfmaGeneric, 1, true, false},
        // D = 8 / 9 / 10 / 11: 9 and 11 have no Toeplitz instantiation (fir_build gives them no table; with one, dispatch_mfma's default arm)
        {"/8", shp(128, 2, 8, 63), DEF, true, F::MfmaGeneric, 1, true, false},
        {"/9", shp(128, 2, 9, 0), DEF, true, F::DecimLds2, 1, true, true},
        {"/9 with a table", shp(128, 2, 9, 67), DEF, true, F::DecimLds2, 1, true, false},
        {"/9 f32 stream", shp(128, 1, 9, 0), DEF, true, F::DecimLds1, 1, true, false},
        {"/10", shp(128, 2, 10, 70), DEF, true, F::MfmaGeneric, 1, true, false},
        {"/11", shp(128, 2, 11, 0), DEF, true, F::DecimLds2, 1, true, true},
        {"/11 with a table", shp(128, 2, 11, 74), DEF, true, F::DecimLds2, 1, true, false},
        // M + 255 against DECIM2_SPAN_MAX = 6 128 and DECIM_SPAN_MAX = 6 144
        {"/50, 5 873 taps", shp(5873, 2, 50, 0), DEF, true, F::DecimLds2, 1, true, true},
        {"/50, 5 874 taps", shp(5874, 2, 50, 0), DEF, true, F::DecimLds1, 1, true, true},
        {"/50, 5 889 taps", shp(5889, 2, 50, 0), DEF, true, F::DecimLds1, 1, true, true},
        {"direct: /50, 5 890 taps", shp(5890, 2, 50, 0), DEF, true, F::Direct, 1, false, false},
        {"D = 1 without a table: LDS-staged, but not for in-place input", shp(5000, 2, 1, 0), DEF, true, F::DecimLds1, 1, false, true},
        // ---- the shapes of tests/test_gpu_bounds.py (test_fir_form, test_hilberttransform, test_chain): each case reaches the form it claims to
        {"bounds: decfft", decf(shp(128, 2, 4, 48)), DEF, true, F::DecFft, 1, true, false},
        {"bounds: decfft at an offset of 1 or 3 floats", decf(shp(128, 2, 4, 48)), DEF, false, F::Direct, 1, true, false},
        {"bounds: winshort", shp(16, 2, 1, 8), DEF, true, F::WinShort, 1, true, false},
        {"bounds: winshortc", ctaps(shp(16, 2, 1, 16), true), DEF, true, F::WinShortC, 1, true, false},
        {"bounds: shortreal", shp(16, 1, 1, 9), DEF, true, F::ShortReal, 1, false, false},
        {"bounds: winpair", shp(136, 1, 5, 54), DEF, true, F::WinPair, 1, true, false},
        {"bounds: decimlds1", shp(128, 1, 50, 0), DEF, true, F::DecimLds1, 1, true, false},
        {"bounds: decimlds2", shp(128, 2, 50, 0), DEF, true, F::DecimLds2, 1, true, true},
        {"bounds: direct", shp(128, 2, 1, 36), DEF, false, F::Direct, 1, true, false},
        {"bounds: mfmacc, 64 complex taps = 128 + 2 x 15 + 2 + 3 over 4 steps", ctaps(shp(64, 2, 1, 40)), DEF, true, F::MfmaCc, 1, true, false},
        {"bounds: mfmacc at an offset of 1 or 3 floats", ctaps(shp(64, 2, 1, 40)), DEF, false, F::Direct, 1, true, false},
        {"bounds: persistent-cf32", shp(128, 2, 1, 36), DEF, true, F::MfmaPersistent, 1, true, false},
        {"bounds: persistent-f32", shp(128, 1, 1, 37), DEF, true, F::MfmaPersistent, 1, true, false},
        {"bounds: persistent-cf32-d5", shp(128, 2, 5, 51), DEF, true, F::MfmaPersistent, 1, true, true},
        {"bounds: persistent-cf32-d5 at an offset of 1 or 3 floats", shp(128, 2, 5, 51), DEF, false, F::Direct, 1, true, true},
        {"bounds: generic-cf32", shp(124, 2, 1, 35), DEF, true, F::MfmaGeneric, 1, true, false},
        {"bounds: generic-cf32 at an offset of 1 or 3 floats", shp(124, 2, 1, 35), DEF, false, F::Direct, 1, true, false},
        {"bounds: generic-f32", shp(132, 1, 1, 38), DEF, true, F::MfmaGeneric, 1, true, false},
        {"bounds: chain tuner", rot(shp(128, 2, 5, 51)), DEF, true, F::MfmaPersistent, 1, true, true},
        {"bounds: chain tuner-discriminator", rel(post(rot(shp(128, 2, 5, 51)))), DEF, true, F::MfmaPersistent, 5120, true, false},
        {"bounds: chain tuner-discriminator, exact", post(rot(shp(128, 2, 5, 51))), DEF, true, F::MfmaPersistent, 1, true, false},
        {"bounds: chain filter-discriminator", rel(post(shp(128, 2, 1, 36))), DEF, true, F::MfmaPersistent, 1, true, false},
        {"bounds: chain tuner50-magnitude", rot(shp(128, 2, 50, 0)), DEF, true, F::DecimLds2, 1, true, true},
        {"bounds: chain tuner50-discriminator", rel(post(rot(shp(128, 2, 50, 0)))), DEF, true, F::DecimLds2, 1, true, false},
        {"bounds: chain audio-tail", iir(shp(136, 1, 5, 54)), DEF, true, F::WinPair, 12800, true, false},
        // ---- the one-stage shapes of tests/test_gpu_asym_taps.py (tests/helpers/asym_taps.py fir_cases) that no row above pins.  Steps: (4 + 15 D + M) / 4 on a
        // ComplexFloat32 stream, (6 + 15 D + M) / 4 on a Float32 stream; persistent only at 51 steps (D = 5); no Toeplitz table at D = 9, 12, 18, 25, 50, 75
        {"asym: MfmaPersistent-f32-m124-d5, 205 / 4 = 51 steps: persistent, not generic", shp(124, 1, 5, 51), DEF, true, F::MfmaPersistent, 1, true, false},
        {"asym: MfmaGeneric-f32-m122-d5, 203 / 4 = 50 steps", shp(122, 1, 5, 50), DEF, true, F::MfmaGeneric, 1, true, false},
        {"asym: MfmaGeneric-cf32-m128-d2", shp(128, 2, 2, 40), DEF, true, F::MfmaGeneric, 1, true, false},
        {"asym: MfmaGeneric-cf32-m128-d3", shp(128, 2, 3, 44), DEF, true, F::MfmaGeneric, 1, true, false},
        {"asym: MfmaGeneric-cf32-m128-d4", shp(128, 2, 4, 48), DEF, true, F::MfmaGeneric, 1, true, false},
        {"asym: MfmaGeneric-cf32-m128-d6", shp(128, 2, 6, 55), DEF, true, F::MfmaGeneric, 1, true, false},
        {"asym: MfmaGeneric-cf32-m128-d7", shp(128, 2, 7, 59), DEF, true, F::MfmaGeneric, 1, true, false},
        {"asym: MfmaGeneric-f32-m128-d2", shp(128, 1, 2, 41), DEF, true, F::MfmaGeneric, 1, true, false},
        {"asym: MfmaGeneric-f32-m128-d3", shp(128, 1, 3, 44), DEF, true, F::MfmaGeneric, 1, true, false},
        {"asym: MfmaGeneric-f32-m128-d4", shp(128, 1, 4, 48), DEF, true, F::MfmaGeneric, 1, true, false},
        {"asym: MfmaGeneric-f32-m128-d6", shp(128, 1, 6, 56), DEF, true, F::MfmaGeneric, 1, true, false},
        {"asym: MfmaGeneric-f32-m128-d7", shp(128, 1, 7, 59), DEF, true, F::MfmaGeneric, 1, true, false},
        {"asym: MfmaGeneric-f32-m128-d8", shp(128, 1, 8, 63), DEF, true, F::MfmaGeneric, 1, true, false},
        {"asym: MfmaGeneric-f32-m128-d10", shp(128, 1, 10, 71), DEF, true, F::MfmaGeneric, 1, true, false},
        {"asym: MfmaGeneric-cf32-m33-d2", shp(33, 2, 2, 16), DEF, true, F::MfmaGeneric, 1, true, false},
        {"asym: MfmaGeneric-cf32-m33-d5", shp(33, 2, 5, 28), DEF, true, F::MfmaGeneric, 1, true, false},
        {"asym: MfmaGeneric-f32-m33-d2", shp(33, 1, 2, 17), DEF, true, F::MfmaGeneric, 1, true, false},
        {"asym: MfmaGeneric-f32-m33-d5", shp(33, 1, 5, 28), DEF, true, F::MfmaGeneric, 1, true, false},
        {"asym: DecimLds2-cf32-m33-d9", shp(33, 2, 9, 0), DEF, true, F::DecimLds2, 1, true, true},
        {"asym: DecimLds2-cf32-m40-d12", shp(40, 2, 12, 0), DEF, true, F::DecimLds2, 1, true, true},
        {"asym: DecimLds2-cf32-m77-d18", shp(77, 2, 18, 0), DEF, true, F::DecimLds2, 1, true, true},
        {"asym: DecimLds2-cf32-m128-d75", shp(128, 2, 75, 0), DEF, true, F::DecimLds2, 1, true, true},
        {"asym: DecimLds2-cf32-m13-d50", shp(13, 2, 50, 0), DEF, true, F::DecimLds2, 1, true, true},
        {"asym: DecimLds1-f32-m33-d9", shp(33, 1, 9, 0), DEF, true, F::DecimLds1, 1, true, false},
        {"asym: DecimLds1-f32-m77-d25", shp(77, 1, 25, 0), DEF, true, F::DecimLds1, 1, true, false},
        {"asym: DecFft-cf32-m33-d2", decf(shp(33, 2, 2, 16)), DEF, true, F::DecFft, 1, true, false},
        {"asym: DecFft-cf32-m64-d2", decf(shp(64, 2, 2, 24)), DEF, true, F::DecFft, 1, true, false},
        {"asym: DecFft-cf32-m128-d5", decf(shp(128, 2, 5, 51)), DEF, true, F::DecFft, 1, true, false},
        {"asym: DecFft-cf32-m160-d5", decf(shp(160, 2, 5, 59)), DEF, true, F::DecFft, 1, true, false},
        {"asym: DecFft-cf32-m128-d8", decf(shp(128, 2, 8, 63)), DEF, true, F::DecFft, 1, true, false},
        {"asym: DecFft-cf32-m256-d8", decf(shp(256, 2, 8, 95)), DEF, true, F::DecFft, 1, true, false},
    };
    const FirShape c1276 = fft(1276, 2, 1280), r1276 = fft(1276, 1, 1280), r768 = fft(768, 1, 768), c2048 = fft(2048, 2, 0, 1);
    const std::vector<FftRow> fft_rows = {
        // ---- every form under default knobs
        {"1024-point passes: 128 taps", fft(128, 2), DEF, 1L << 24, 256, X::Pass1024},
        {"1024-point passes: behind a discriminator", pre(fft(400, 1)), DEF, 1L << 24, 256, X::Pass1024},
        {"cf32 1 276 taps, 2^24: 5 958 blocks >= 20 x 256", c1276, DEF, 1L << 24, 256, X::Wave64},
        {"cf32 1 276 taps, 2^23: 2 979 blocks", c1276, DEF, 1L << 23, 256, X::Wg4k},
        {"f32 768 taps, 2^24: 2 521 transforms against 2 048 per round", r768, DEF, 1L << 24, 256, X::Pols},
        {"cf32 2 048 taps: 64 x 64 at an overlap of 2 048", c2048, DEF, 1L << 20, 256, X::Long64},
        // ---- tap counts 512 / 513, 1 281 / 1 282, 2 049 / 2 050, 4 097 / 4 098 (cf32, 2^20 samples)
        {"512 taps", fft(512, 2), DEF, 1L << 20, 256, X::Pass1024},
        {"513 taps", fft(513, 2, 768), DEF, 1L << 20, 256, X::Wg4k},
        {"1 281 taps", fft(1281, 2, 1280), DEF, 1L << 20, 256, X::Wg4k},
        {"1 282 taps", fft(1282, 2, 0, 1), DEF, 1L << 20, 256, X::Long64},
        {"2 049 taps", fft(2049, 2, 0, 1), DEF, 1L << 20, 256, X::Long64},
        {"2 050 taps", fft(2050, 2, 0, 2), DEF, 1L << 20, 256, X::Long64},
        {"4 097 taps", fft(4097, 2, 0, 2), DEF, 1L << 20, 256, X::Long64},
        {"4 098 taps", fft(4098, 2, 0, 3), DEF, 1L << 20, 256, X::Long64},
        {"f32 2 048 taps", fft(2048, 1, 0, 1), DEF, 1L << 20, 256, X::Long64},
        // ---- wave-per-block bound: 20 blocks per CU with real taps, 32 with complex taps (blocks of 4 096 - 1 280 = 2 816 outputs)
        {"5 119 blocks, 256 CUs", c1276, DEF, 5119L * 2816, 256, X::Wg4k},
        {"5 120 blocks, 256 CUs", c1276, DEF, 5119L * 2816 + 1, 256, X::Wave64},
        {"2 560 blocks, 256 CUs", c1276, DEF, 2560L * 2816, 256, X::Wg4k},
        {"2 560 blocks, 128 CUs", c1276, DEF, 2560L * 2816, 128, X::Wave64},
        {"2 559 blocks, 128 CUs", c1276, DEF, 2559L * 2816, 128, X::Wg4k},
        {"complex taps, 2^24", ctaps(c1276), DEF, 1L << 24, 256, X::Wg4k},
        {"complex taps, 8 191 blocks", ctaps(c1276), DEF, 8191L * 2816, 256, X::Wg4k},
        {"complex taps, 8 192 blocks", ctaps(c1276), DEF, 8192L * 2816, 256, X::Wave64},
        // ---- f32_window: 768 taps (blocks of 3 328), one round = 8 x 256 = 2 048 transforms < transforms <= 27 / 20 rounds = 2 764
        {"f32 768 taps, 2 048 transforms", r768, DEF, 4096L * 3328, 256, X::Wave64},
        {"f32 768 taps, 2 049 transforms", r768, DEF, 4096L * 3328 + 1, 256, X::Pols},
        {"f32 768 taps, 2 764 transforms", r768, DEF, 5528L * 3328, 256, X::Pols},
        {"f32 768 taps, 2 765 transforms", r768, DEF, 5528L * 3328 + 1, 256, X::Wave64},
        {"f32 768 taps, 2^24 on 128 CUs: 2.46 rounds", r768, DEF, 1L << 24, 128, X::Wave64},
        {"f32 1 276 taps, 2^24: the window is for an overlap of 768 only", r1276, DEF, 1L << 24, 256, X::Wave64},
        // ---- knobs
        {"LRHIP_FFT_POLS=1, cf32 1 276", c1276, K([](FirKnobs &k) { k.fft_pols = 1; }), 1L << 24, 256, X::Pols},
        {"LRHIP_FFT_POLS=1, cf32 2 048", c2048, K([](FirKnobs &k) { k.fft_pols = 1; }), 1L << 24, 256, X::Pols},
        {"LRHIP_FFT_POLS=1, 128 taps: one partition", fft(128, 2), K([](FirKnobs &k) { k.fft_pols = 1; }), 1L << 24, 256, X::Pass1024},
        {"LRHIP_FFT_POLS=0, cf32 1 276", c1276, K([](FirKnobs &k) { k.fft_pols = 0; }), 1L << 24, 256, X::Wave64},
        {"LRHIP_FFT_POLS=0, f32 768 in the window", r768, K([](FirKnobs &k) { k.fft_pols = 0; }), 1L << 24, 256, X::Pass1024},
        {"LRHIP_F64_F32=0, f32 1 276", r1276, K([](FirKnobs &k) { k.f64_f32 = 0; }), 1L << 24, 256, X::Pols},
        {"LRHIP_F64_F32=0, f32 2 048", fft(2048, 1, 0, 1), K([](FirKnobs &k) { k.f64_f32 = 0; }), 1L << 24, 256, X::Pols},
        // KNOWN INCONSISTENCY, pinned as it is: LRHIP_F64_F32=0 is documented to keep Float32 streams off the 64 x 64 kernel, and with LRHIP_FFT_POLS=0 they take it
        {"LRHIP_F64_F32=0 LRHIP_FFT_POLS=0, f32 1 276", r1276, K([](FirKnobs &k) { k.f64_f32 = 0; k.fft_pols = 0; }), 1L << 24, 256, X::Wave64},
        {"LRHIP_F64_F32=0 LRHIP_FFT_POLS=0, f32 768, 2^22", r768, K([](FirKnobs &k) { k.f64_f32 = 0; k.fft_pols = 0; }), 1L << 22, 256, X::Wave64},
        {"LRHIP_F64_LONG=0, cf32 2 048", c2048, K([](FirKnobs &k) { k.f64_long = 0; }), 1L << 24, 256, X::Pols},
        {"LRHIP_F64_LONG_MIN=8, cf32 2 048, 2^20: 512 blocks", c2048, K([](FirKnobs &k) { k.f64_long_min = 8; }), 1L << 20, 256, X::Pols},
        {"LRHIP_F64_LONG_MIN=8, cf32 2 048, 2^22: 2 048 blocks", c2048, K([](FirKnobs &k) { k.f64_long_min = 8; }), 1L << 22, 256, X::Long64},
        {"LRHIP_F4K_WAVE=0, cf32 1 276, 2^24", c1276, K([](FirKnobs &k) { k.f4k_wave = 0; }), 1L << 24, 256, X::Wg4k},
        {"LRHIP_F4K_WAVE=1, cf32 1 276, 2^23", c1276, K([](FirKnobs &k) { k.f4k_wave = 1; }), 1L << 23, 256, X::Wave64},
        {"LRHIP_F4K_WAVE=0, f32 1 276", r1276, K([](FirKnobs &k) { k.f4k_wave = 0; }), 1L << 24, 256, X::Pols},
        {"LRHIP_F4K_WAVE=1, f32 768 in the window", r768, K([](FirKnobs &k) { k.f4k_wave = 1; }), 1L << 24, 256, X::Wave64},
        {"LRHIP_FFT_NO_4K, cf32 1 276", c1276, K([](FirKnobs &k) { k.fft_no_4k = true; }), 1L << 24, 256, X::Pols},
        {"LRHIP_FFT_NO_4K LRHIP_FFT_POLS=0, cf32 1 276", c1276, K([](FirKnobs &k) { k.fft_no_4k = true; k.fft_pols = 0; }), 1L << 24, 256, X::Pass1024},
        {"LRHIP_FFT_NO_4K, cf32 2 048", c2048, K([](FirKnobs &k) { k.fft_no_4k = true; }), 1L << 24, 256, X::Long64},
        // ---- the shapes of tests/test_gpu_bounds.py (test_fir_fft_form: n_out = 3 T, the largest call of each case; every smaller call takes the same form)
        {"bounds: cf32 128", fft(128, 2), DEF, 3L * 896, 256, X::Pass1024}, {"bounds: cf32 512", fft(512, 2), DEF, 3L * 512, 256, X::Pass1024},
        {"bounds: cf32 513", fft(513, 2, 768), DEF, 3L * 3328, 256, X::Wg4k}, {"bounds: cf32 1 281", fft(1281, 2, 1280), DEF, 3L * 2816, 256, X::Wg4k},
        {"bounds: cf32 1 282", fft(1282, 2, 0, 1), DEF, 3L * 2048, 256, X::Long64}, {"bounds: cf32 2 049", fft(2049, 2, 0, 1), DEF, 3L * 2048, 256, X::Long64},
        {"bounds: cf32 2 050", fft(2050, 2, 0, 2), DEF, 3L * 2048, 256, X::Long64}, {"bounds: cf32 4 097", fft(4097, 2, 0, 2), DEF, 3L * 2048, 256, X::Long64},
        {"bounds: cf32 4 098", fft(4098, 2, 0, 3), DEF, 3L * 2048, 256, X::Long64},
        {"bounds: complex taps 128", ctaps(fft(128, 2)), DEF, 3L * 896, 256, X::Pass1024}, {"bounds: complex taps 512", ctaps(fft(512, 2)), DEF, 3L * 512, 256, X::Pass1024},
        {"bounds: complex taps 513", ctaps(fft(513, 2, 768)), DEF, 3L * 3328, 256, X::Wg4k}, {"bounds: complex taps 1 281", ctaps(fft(1281, 2, 1280)), DEF, 3L * 2816, 256, X::Wg4k},
        {"bounds: complex taps 1 282", ctaps(fft(1282, 2, 0, 1)), DEF, 3L * 2048, 256, X::Long64}, {"bounds: complex taps 2 049", ctaps(fft(2049, 2, 0, 1)), DEF, 3L * 2048, 256, X::Long64},
        {"bounds: complex taps 2 050", ctaps(fft(2050, 2, 0, 2)), DEF, 3L * 2048, 256, X::Long64}, {"bounds: complex taps 4 097", ctaps(fft(4097, 2, 0, 2)), DEF, 3L * 2048, 256, X::Long64},
        {"bounds: complex taps 4 098", ctaps(fft(4098, 2, 0, 3)), DEF, 3L * 2048, 256, X::Long64},
        {"bounds: f32 128", fft(128, 1), DEF, 3L * 1792, 256, X::Pass1024}, {"bounds: f32 512", fft(512, 1), DEF, 3L * 1024, 256, X::Pass1024},
        {"bounds: f32 513", fft(513, 1, 768), DEF, 3L * 6656, 256, X::Wave64}, {"bounds: f32 1 281", fft(1281, 1, 1280), DEF, 3L * 5632, 256, X::Wave64},
        {"bounds: f32 1 282", fft(1282, 1, 0, 1), DEF, 3L * 4096, 256, X::Long64}, {"bounds: f32 2 049", fft(2049, 1, 0, 1), DEF, 3L * 4096, 256, X::Long64},
        {"bounds: f32 2 050", fft(2050, 1, 0, 2), DEF, 3L * 4096, 256, X::Long64}, {"bounds: f32 4 097", fft(4097, 1, 0, 2), DEF, 3L * 4096, 256, X::Long64},
        {"bounds: f32 4 098", fft(4098, 1, 0, 3), DEF, 3L * 4096, 256, X::Long64},
        {"bounds: one-sample calls", fft(513, 2, 768), DEF, 1, 256, X::Wg4k}, {"bounds: one-sample calls, f32", fft(513, 1, 768), DEF, 1, 256, X::Wave64},
        // test_fir_fft_large: the smallest launches that reach the wave-per-block form on a ComplexFloat32 stream and the partitioned form on a Float32 stream
        {"bounds: large wave64, 5 120 blocks", fft(1281, 2, 1280), DEF, 5119L * 2816 + 1, 256, X::Wave64}, {"bounds: one sample less", fft(1281, 2, 1280), DEF, 5119L * 2816, 256, X::Wg4k},
        {"bounds: large wave64, the call of 3 samples behind it", fft(1281, 2, 1280), DEF, 3, 256, X::Wg4k},
        {"bounds: large pols, 2 049 transforms", fft(768, 1, 768), DEF, 4096L * 3328 + 1, 256, X::Pols}, {"bounds: one sample less, f32", fft(768, 1, 768), DEF, 4096L * 3328, 256, X::Wave64},
        // test_chain: the merged cascade of three 256-tap filters, the discriminator in front of an overlap-save filter
        {"bounds: chain fir-cascade, 766 taps", fft(766, 2, 768), DEF, 3L * 3328, 256, X::Wg4k},
        {"bounds: chain discriminator-fir", pre(fft(128, 1)), DEF, 3L * 1792, 256, X::Pass1024},
    };
    // align() / direct_io_ok() of the overlap-save shapes: lcm of the partitions' block advances (x 2 on a Float32 stream); in place only in one launch
    const std::vector<Row> fft_shape_rows = {
        {"512 taps", fft(512, 2), DEF, true, F::OverlapSave, 512, true, false},
        {"513 taps", fft(513, 2, 768), DEF, true, F::OverlapSave, 1024, true, false},
        {"f32 768 taps", r768, DEF, true, F::OverlapSave, 3072, false, false},
        {"cf32 1 276 taps", c1276, DEF, true, F::OverlapSave, 1536, true, false},
        {"f32 1 276 taps", r1276, DEF, true, F::OverlapSave, 3072, false, false},
        {"1 282 taps", fft(1282, 2, 0, 1), DEF, true, F::OverlapSave, 5632, true, false},
        {"2 050 taps", fft(2050, 2, 0, 2), DEF, true, F::OverlapSave, 7680, true, false},
        {"4 097 taps: two partitions, one launch", fft(4097, 2, 0, 2), DEF, true, F::OverlapSave, 1024, true, false},
        {"4 098 taps: the second launch re-reads y", fft(4098, 2, 0, 3), DEF, true, F::OverlapSave, 7680, false, false},
        {"cf32 1 276 taps from an unaligned chunk", c1276, DEF, false, F::OverlapSave, 1536, true, false},
        {"bounds: chain fir-cascade, 766 taps = partitions of 512 and 254", fft(766, 2, 768), DEF, true, F::OverlapSave, 1536, true, false},
        {"bounds: chain discriminator-fir", pre(fft(128, 1)), DEF, true, F::OverlapSave, 1792, false, false},
    };
    const FirKnobs v1 = K([](FirKnobs &k) { k.decim_v1 = true; }), no_lds = K([](FirKnobs &k) { k.no_disc_epi_lds = true; }),
                   no_other = K([](FirKnobs &k) { k.no_disc_epi_other_d = true; }), wc = K([](FirKnobs &k) { k.win_cplx = true; });
    const std::vector<Pred> preds = {
        // ceil(M / D) against DF_V = 32, D in {2, 4, 5, 8}, at least 8 taps, ComplexFloat32 stream
        {"decfft 64 /2", fir_decfft_supported(2, 64, 2), true}, {"decfft 65 /2", fir_decfft_supported(2, 65, 2), false},
        {"decfft 128 /4", fir_decfft_supported(4, 128, 2), true}, {"decfft 129 /4", fir_decfft_supported(4, 129, 2), false},
        {"decfft 160 /5", fir_decfft_supported(5, 160, 2), true}, {"decfft 161 /5", fir_decfft_supported(5, 161, 2), false},
        {"decfft 256 /8", fir_decfft_supported(8, 256, 2), true}, {"decfft 257 /8", fir_decfft_supported(8, 257, 2), false},
        {"decfft 7 /2", fir_decfft_supported(2, 7, 2), false}, {"decfft 8 /2", fir_decfft_supported(2, 8, 2), true},
        {"decfft /3", fir_decfft_supported(3, 64, 2), false}, {"decfft /10", fir_decfft_supported(10, 64, 2), false}, {"decfft f32", fir_decfft_supported(4, 128, 1), false},
        {"mfma /0", fir_mfma_supported_decim(0), false}, {"mfma /1", fir_mfma_supported_decim(1), true}, {"mfma /8", fir_mfma_supported_decim(8), true},
        {"mfma /9", fir_mfma_supported_decim(9), false}, {"mfma /10", fir_mfma_supported_decim(10), true}, {"mfma /11", fir_mfma_supported_decim(11), false},
        {"disc_ksteps", fir_disc_ksteps(4) == 48 && fir_disc_ksteps(8) == 63 && fir_disc_ksteps(10) == 70, true},
        // can_post_disc
        {"disc: decfft", fir_can_post_disc(decf(shp(128, 2, 4, 48)), DEF), true}, {"disc: headline", fir_can_post_disc(lp128, DEF), true},
        {"disc: 37 steps", fir_can_post_disc(shp(132, 2, 1, 37), DEF), false}, {"disc: f32 stream", fir_can_post_disc(lp128r, DEF), false},
        {"disc: tuner", fir_can_post_disc(tuner, DEF), true}, {"disc: overlap-save", fir_can_post_disc(fft(128, 2), DEF), false},
        {"disc: complex taps", fir_can_post_disc(ctaps(shp(64, 2, 5, 70)), DEF), false},
        {"disc: /50", fir_can_post_disc(nbfm, DEF), true}, {"disc: /50 LRHIP_NO_DISC_EPI_LDS", fir_can_post_disc(nbfm, no_lds), false},
        {"disc: /50 LRHIP_DECIM_V1", fir_can_post_disc(nbfm, v1), false}, {"disc: /50, 5 874 taps", fir_can_post_disc(shp(5874, 2, 50, 0), DEF), false},
        {"disc: tuner /4", fir_can_post_disc(rot(shp(128, 2, 4, 48)), DEF), true}, {"disc: decimator /4", fir_can_post_disc(shp(128, 2, 4, 48), DEF), false},
        {"disc: tuner /4 LRHIP_NO_DISC_EPI_OTHER_D", fir_can_post_disc(rot(shp(128, 2, 4, 48)), no_other), false},
        {"disc: tuner /8", fir_can_post_disc(rot(shp(128, 2, 8, 63)), DEF), true}, {"disc: tuner /10", fir_can_post_disc(rot(shp(128, 2, 10, 70)), DEF), true},
        {"disc: tuner /10, 69 steps", fir_can_post_disc(rot(shp(124, 2, 10, 69)), DEF), false}, {"disc: tuner /2", fir_can_post_disc(rot(shp(128, 2, 2, 40)), DEF), false},
        {"disc: win-cplx", fir_can_post_disc(shp(128, 2, 5, 0), wc), true}, {"disc: /5 without a table: LDS-staged", fir_can_post_disc(shp(128, 2, 5, 0), DEF), true},
        // can_post_unary, hilbert_ok
        {"unary: /50", fir_can_post_unary(nbfm), true}, {"unary: tuner", fir_can_post_unary(tuner), false}, {"unary: D = 1", fir_can_post_unary(shp(5000, 2, 1, 0)), false},
        {"unary: + disc", fir_can_post_unary(post(nbfm)), false}, {"unary: f32", fir_can_post_unary(shp(128, 1, 50, 0)), false},
        {"unary: decfft", fir_can_post_unary(decf(shp(128, 2, 11, 0))), false}, {"unary: 5 890 taps", fir_can_post_unary(shp(5890, 2, 50, 0)), false},
        {"hilbert: 129 taps", fir_hilbert_ok(shp(129, 1, 1, 37)), true}, {"hilbert: no table", fir_hilbert_ok(shp(129, 1, 1, 0)), false},
        {"hilbert: overlap-save", fir_hilbert_ok(fft(129, 1)), false}, {"hilbert: cf32", fir_hilbert_ok(shp(129, 2, 1, 37)), false},
        {"bounds: hilbert 33 taps", fir_hilbert_ok(shp(33, 1, 1, 13)), true}, {"bounds: hilbert 65 taps", fir_hilbert_ok(shp(65, 1, 1, 21)), true},
    };

    int bad = 0;
    auto check_rows = [&](const std::vector<Row> &rs) {
        for (const Row &r : rs) {
            const F f = fir_form(r.s, r.k, r.aligned);
            const unsigned long al = fir_align(r.s, r.k);
            const bool dio = fir_direct_io_ok(r.s, r.k), raw = fir_raw_records_ok(r.s, r.k);
            if (f != r.form || al != r.align || dio != r.direct_io || raw != r.raw) {
                printf("MISMATCH %s: form %d (want %d), align %lu (%lu), direct_io %d (%d), raw %d (%d)\n", r.what, (int)f, (int)r.form, al, r.align, dio, r.direct_io, raw, r.raw);
                bad++;
            }
        }
    };
    check_rows(rows);
    check_rows(fft_shape_rows);
    for (const FftRow &r : fft_rows) {
        const X f = fir_fft_form(r.s, r.k, r.n_out, r.num_cus);
        if (f != r.form) { printf("MISMATCH fft %s: form %d (want %d)\n", r.what, (int)f, (int)r.form); bad++; }
    }
    for (const Pred &p : preds)
        if (p.got != p.want) { printf("MISMATCH %s: %d (want %d)\n", p.what, p.got, p.want); bad++; }
    // every form is in the table
    bool seen[14] = {}, seen_fft[5] = {};
    for (const Row &r : rows) seen[(int)r.form] = true;
    for (const FftRow &r : fft_rows) seen_fft[(int)r.form] = true;
    for (int i = 0; i < 14; i++) if (!seen[i]) { printf("form %d has no row\n", i); bad++; }
    for (int i = 0; i < 5; i++) if (!seen_fft[i]) { printf("fft form %d has no row\n", i); bad++; }
    printf("%zu + %zu form rows, %zu overlap-save rows, %zu predicates\n", rows.size(), fft_shape_rows.size(), fft_rows.size(), preds.size());
    printf(bad ? "FAILED (%d)\n" : "OK\n", bad);
    return bad ? 1 : 0;
}
