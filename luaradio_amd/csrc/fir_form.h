// fir_form.h - which kernel form a FIRFilterBlock stage launches: the ONE statement of that choice.  Host-only, plain C++17, no HIP calls; include it after
// the kernel headers (constants DECIM_SPAN_MAX, DECIM2_SPAN_MAX, DF_V, FFTN, F4K_N, FirMfmaGeom).  stage_fir.h launches what fir_form() / fir_fft_form()
// name; tools/host_fir_form_check.hip pins both against a literal table on the CPU.
#pragma once
#include <cstdlib>
#include <numeric>
#ifndef LRHIP_FIR_D1_NACC
#define LRHIP_FIR_D1_NACC 8      /* accumulators per wave of the D = 1 Toeplitz kernel (A/B: 4 with more waves per SIMD) */
#endif
constexpr int FIR_FFT_PART = 512;      // taps per overlap-save partition (V = 512, L = 512 of the 1024-point block)
// Every LRHIP_* environment knob of the FIR stage, read ONCE per process (fir_knobs()).  FirKnobs() holds the defaults, FirKnobs(true) reads the environment.
// (Per stage, read at construction, and therefore not here: LRHIP_TUNER_EXACT, LRHIP_TUNER_NW1 - FirStage::rel_rot / rel_nw1.)
struct FirKnobs {
    explicit FirKnobs(bool from_env = false) : env(from_env) {}
    bool env;
    bool set(const char *k) const { return env && getenv(k) != nullptr; }
    int num(const char *k, int dflt) const { return env && getenv(k) ? atoi(getenv(k)) : dflt; }
    long lnum(const char *k, long dflt) const { return env && getenv(k) ? atol(getenv(k)) : dflt; }
    // ---- which form
    bool no_win = set("LRHIP_NO_FIR_WIN");                  // A/B knob: no register-window kernel (kernels_firwin.h, kernels_firwin2.h)
    // opt-in: 128 taps on 2^26 Float32 samples run at 0.25 ms on the window kernel against 0.19 ms on the Toeplitz-MFMA kernel (same box) - at D = 1 the
    // Toeplitz product wastes only 11 % of its MACs and keeps more waves resident
    bool win_real = set("LRHIP_FIR_WIN_REAL");
    // opt-in: same-box A/B on the WBFM tuner + discriminator, 2^26 samples: 0.204 ms against 0.150 ms + 0.005 ms (fix-up) for the Toeplitz-MFMA kernel - both are
    // bound by the shared MFMA / VALU datapath (rocprofv3: 1 250 VALU instructions per wave and 6 360-sample tile, 640 of them the filter), and the Toeplitz
    // kernel keeps 3 workgroups per CU resident against 2
    bool win_cplx = set("LRHIP_FIR_WIN_CPLX");
    bool no_win_short = set("LRHIP_NO_FIR_WIN_SHORT");      // A/B knob: 16 .. 64 taps at D = 1 stay on the Toeplitz kernel
    bool decim_v1 = set("LRHIP_DECIM_V1");                  // keeps the first LDS-staged decimator form where the second (round 5) applies
    bool no_disc_epi_lds = set("LRHIP_NO_DISC_EPI_LDS");    // A/B knob: no discriminator epilogue on the second LDS-staged decimator form
    bool no_disc_epi_other_d = set("LRHIP_NO_DISC_EPI_OTHER_D");      // A/B knob, the round-4 behaviour: no Tuner + discriminator kernel at decimation 4, 8, 10
    bool fft_no_4k = set("LRHIP_FFT_NO_4K");                // A/B knob: partitions of the 1024-point kernel (round 2)
    // more than 512 taps: the partitioned form (one launch per 1 536 taps) wherever the 4096-point kernels do not apply - Float32 streams, more than
    // 1 281 taps - instead of one accumulating pass of the 1024-point kernel per 512 taps.  1 / 0 forces it on (also for 513 .. 1 281 taps on a
    // ComplexFloat32 stream) / off (A/B)
    int fft_pols = num("LRHIP_FFT_POLS", -1);
    // round 5: 1 282 .. 4 097 taps on a ComplexFloat32 stream as ONE launch of the 64 x 64 kernel at an overlap of 2 048 (two partitions above 2 049 taps) once
    // a wave's run is long enough to pay for its warm-up block; 0 keeps the partitioned 1024-point kernel (A/B)
    int f64_long = num("LRHIP_F64_LONG", 1);
    // (size sweep 2^20 .. 2^26 samples, same box: faster than the partitioned kernel at every size - 4 096 taps 0.072 / 0.106 / 0.196 / 0.575 ms against
    // 0.188 / 0.208 / 0.243 / 1.104 at 2^20 / 2^22 / 2^24 / 2^26, 2 048 taps 0.048 against 0.093 at 2^22 - so there is no lower bound; the knob = blocks per CU)
    long f64_long_min = lnum("LRHIP_F64_LONG_MIN", 0);
    int f64_f32 = num("LRHIP_F64_F32", 1);                  // round 6: Float32 streams (real taps) ride the 64 x 64 kernels, two stream blocks per transform: 0 keeps the partitioned kernel for them (A/B)
    int f4k_wave = num("LRHIP_F4K_WAVE", -1);               // 1 / 0 forces the wave-per-block / the workgroup-per-block 4096-point kernel (A/B); -1: by launch size (fir_fft_form)
    bool tuner_no_raw = set("LRHIP_TUNER_NO_RAW");          // A/B knob: a conversion launch in front of the Tuner instead of its record instantiation
    bool hilbert_mfma = set("LRHIP_HILBERT_MFMA");          // A/B knob: the matrix-core pair epilogue of round 3 instead of the Hilbert window kernel
    // ---- launch parameters
    int d5_nacc = num("LRHIP_FIR_D5_NACC", 2);              // A/B knob: accumulators per wave of the Toeplitz kernel at D = 5
    int fir_rounds = num("LRHIP_FIR_ROUNDS", 0);            // A/B: persistent grid stride (0), or runs of `rounds` consecutive tiles per workgroup in address order
    int hilbert_run = num("LRHIP_HILBERT_RUN", 0);          // A/B knob: tiles per workgroup
    // XCD-major block order (kernels_firfft4k.h), measured on 2^26 samples, same box: 1 276 taps 0.479 -> 0.448 ms (the 31 % overlap becomes L2 hits),
    // 768 taps equal; 0 is the plain order
    int f4k_xcd_map = num("LRHIP_F4K_XCD_MAP", 1);
    // round 6, measured and left OFF: complex taps at eight waves per CU with H read from the global table (1) are 8-10 % SLOWER than four waves with H in
    // the LDS (1 276 taps, 2^26 samples, three alternations on one box: 0.447 / 0.444 / 0.437 against 0.404 / 0.406 / 0.405 ms, profiles/r06_ab_hg.txt) -
    // 64 more global loads per block in a kernel whose block is already a third memory-instruction issue
    int f64_hg = num("LRHIP_F64_HG", 0);
    // A/B knob: blocks per workgroup.  2 (512 threads, shared tables, 16 waves per CU instead of 12) measured SLOWER: 0.505 against 0.479 ms - the barriers
    // then couple eight waves; the kernel is bound by its five workgroup barriers per block, not by occupancy (counters: VALU 27 %, LDS 42 % busy)
    int f4k_ng = num("LRHIP_F4K_NG", 1);
    long pols_run = lnum("LRHIP_POLS_RUN", 0);              // A/B knob: blocks per wave run of the partitioned kernel
    int pols_p = num("LRHIP_POLS_P", 4);                    // 3 is the round-4 split of the partitioned kernel (A/B, launch_pols)
    long fft_lds_pad = lnum("LRHIP_FFT_LDS_PAD", 0);        // A/B knob: unused LDS per workgroup -> fewer resident workgroups per CU
    int fft_rounds = num("LRHIP_FFT_ROUNDS", -1);           // A/B knob: 8 is the one-shot order of the 1024-point kernel (launch_fft)
    bool fft_taper = num("LRHIP_FFT_TAPER", 0) > 0;         // A/B knob, opt-in: tapered tail of that one-shot order
    long decim_span = lnum("LRHIP_DECIM_SPAN", 0);          // A/B: fewer staged samples per LDS-staged decimator tile = smaller tiles, more workgroups per CU
    int decim_rounds = num("LRHIP_DECIM_ROUNDS", 0);        // A/B: runs of consecutive tiles, address order
    int decfft_rounds = num("LRHIP_DECFFT_ROUNDS", 0);      // A/B knob: quads per wave of the polyphase-FFT decimator (0: by launch size)
    long tail_run = lnum("LRHIP_TAIL_RUN", 0);              // A/B knob: tiles per workgroup of the pair-mode window filter
    bool win_oneshot = set("LRHIP_FIR_WIN_ONESHOT");        // A/B knob: a workgroup per window-kernel tile
};
inline const FirKnobs &fir_knobs() { static const FirKnobs k(true); return k; }

// the plain facts the choice depends on (FirStage derives from it: one copy of each)
struct FirShape {
    int M = 0, S = 2, taps_complex = 0;      // taps; floats per stream sample (2: ComplexFloat32); ComplexFloat32 taps
    unsigned D = 1;                       // fused DownsamplerBlock behind
    bool use_fft = false, fft_arith = false;      // the reference's overlap-save emission framing (firfilter.lua:451-485); overlap-save ARITHMETIC (fused FFT kernels), independent of the framing
    bool decfft = false;                  // decimating polyphase-FFT form (kernels_firdecfft.h): ComplexFloat32 stream, D >= 2, ceil(M / D) <= 32
    int ksteps = 0;                       // MFMA steps of the Toeplitz kernel; 0 => unavailable for this (M, D)
    int fft4k_V = 0;                      // 513 .. 1 281 taps: overlap of the 4096-point kernels (768 / 1024 / 1280; 0 = not built)
    int fft64_np = 0;                     // round 5: 1 282 .. 2 049 taps (1) / 2 050 .. 4 097 taps (2 partitions) on the 64 x 64 form at an overlap of 2 048; round 6: 3, 4
    bool rot = false;                     // fused rotator in front
    // fused FrequencyDiscriminatorBlock in front (chains: input is ComplexFloat32, the filter runs on arg(c[i] conj c[i-1])/gain) / behind (ComplexFloat32 in, Float32 out: kernel epilogue)
    bool pre_disc = false, post_disc = false;
    bool iir_fused = false;               // pair mode: y[k] = iir_b0 v[k] + iir_na1 y[k-1] behind the filter
    bool ctaps4 = false;                  // the (re, im, -im, re) tap table of the short complex-taps window kernel was built
    int in_fmt = 0;                       // RX_FMT_*: raw records in front
    bool rel_rot = false, rel_nw1 = false;      // window-relative phasors, one-wave workgroups on the tuner + discriminator kernel (FirStage's constructor)
};
// one value per launcher that FirStage::core() reaches, and per form of the overlap-save arithmetic (FirStage::launch_fft())
enum class FirForm { DecFft, OverlapSave, WinReal, WinCplx, WinShort, WinShortC, ShortReal, WinPair, DecimLds1, DecimLds2, Direct, MfmaCc, MfmaPersistent, MfmaGeneric };
enum class FirFftForm { Long64, Pols, Wave64, Wg4k, Pass1024 };
// decimating polyphase-FFT form (kernels_firdecfft.h): ComplexFloat32 stream, D in {2, 4, 5, 8}, ceil(M / D) <= 32
inline bool fir_decfft_supported(unsigned d, int m, int s) { return s == 2 && (d == 2 || d == 4 || d == 5 || d == 8) && (m + (int)d - 1) / (int)d <= DF_V && m >= 8; }
inline bool fir_mfma_supported_decim(unsigned d) { return (d >= 1 && d <= 8) || d == 10; }
// MFMA steps of the 128-tap ComplexFloat32 Toeplitz filter at decimation d (fir_mfma_ksteps(128, d, 2)): the shapes with a discriminator epilogue
constexpr int fir_disc_ksteps(int d) { return (1 + 15 * d + 128 + 3) / 4; }

inline bool fir_plain(const FirShape &s) { return !s.taps_complex && !s.rot && !s.pre_disc && !s.post_disc && !s.fft_arith; }
// Float32 stream at D = 1 on the register-window kernel (kernels_firwin.h): every issued packed FMA is useful work, against 89 % for the Toeplitz product
inline bool fir_win_real_ok(const FirShape &s, const FirKnobs &k) { return k.win_real && !k.no_win && s.S == 1 && s.D == 1 && fir_plain(s) && (s.M == 32 || s.M == 64 || s.M == 128); }
// ComplexFloat32 stream with decimation (Decimator / Tuner [+ discriminator]) and the decimating Float32 filter with a fused first-order recurrence
// (pair mode), on the register-window kernel (kernels_firwin2.h)
inline bool fir_win_cplx_ok(const FirShape &s, const FirKnobs &k) { return k.win_cplx && !k.no_win && s.S == 2 && !s.taps_complex && s.D == 5 && s.M == 128 && !s.fft_arith && !s.use_fft && !s.decfft && !s.pre_disc; }
inline bool fir_win_pair_ok(const FirShape &s, const FirKnobs &k) { return !k.no_win && s.S == 1 && s.D == 5 && s.M == 136 && fir_plain(s) && !s.use_fft; }
// short filters on the ComplexFloat32 stream at D = 1 (the reference suite's 16-tap entries): at 16 taps the filter is 16 packed FMAs per
// output - nothing against its 16 B of traffic - and the Toeplitz product pays its fixed 16-output blocks (K = 15 + 16, half of it zeros).
// One-shot window kernel, same box, 2^26 samples: 16 taps 0.175 against 0.222 ms (6.1 TB/s = the copy yardstick), 32 taps 0.233 / 0.260,
// 64 taps 0.301 / 0.326 (there the overlap-save kernel, 0.221, is what `automatic` picks)
inline bool fir_win_short_ok(const FirShape &s, const FirKnobs &k) { return !k.no_win_short && !k.no_win && s.S == 2 && s.D == 1 && (s.M == 16 || s.M == 32 || s.M == 64) && fir_plain(s) && !s.use_fft; }
// short ComplexFloat32-taps filters at D = 1 (the reference suite's 16-complex-taps entry): 2 M packed FMAs per output on the window kernel,
// a streaming problem like the real-taps case (the two-Toeplitz-filter form pays 2 x 2 M taps in fixed 16-output blocks)
inline bool fir_win_short_c_ok(const FirShape &s, const FirKnobs &k) { return !k.no_win_short && !k.no_win && s.S == 2 && s.taps_complex && s.D == 1 && (s.M == 16 || s.M == 32) && s.ctaps4 && !s.rot && !s.fft_arith && !s.use_fft && !s.pre_disc && !s.post_disc; }
// (the Float32-stream window kernel was measured the same way and lost: 0.153 / 0.150 ms against 0.136 / 0.136 for the Toeplitz kernel at 16 / 32 taps;
// what wins there is the plain streaming form, fir_short_real_kernel: four outputs per thread, loads shared through L1)
inline bool fir_short_real_ok(const FirShape &s, const FirKnobs &k) { return !k.no_win_short && s.S == 1 && s.D == 1 && (s.M == 16 || s.M == 32) && fir_plain(s) && !s.use_fft; }
// decimations without a Toeplitz instantiation (and taps too long for its LDS table): LDS-staged one-output-per-thread kernel
inline bool fir_decim_lds_ok(const FirShape &s) { return !s.fft_arith && !s.use_fft && s.M + 255 <= DECIM_SPAN_MAX && !(s.taps_complex && s.rot); }
// round 5: its second form (kernels_firdecim.h) for a ComplexFloat32 stream and real taps
inline bool fir_decim_lds2_ok(const FirShape &s, const FirKnobs &k) { return !k.decim_v1 && s.S == 2 && !s.taps_complex && s.D >= 2 && s.M + 255 <= DECIM2_SPAN_MAX; }
// HilbertTransformBlock in one launch: the generic Float32 Toeplitz kernel with the pair epilogue (kernels_fir.h, HILB)
inline bool fir_hilbert_ok(const FirShape &s) { return s.S == 1 && s.D == 1 && s.ksteps > 0 && fir_plain(s) && !s.use_fft; }
// a complex -> real element-wise block folded into the LDS-staged decimator's store
inline bool fir_can_post_unary(const FirShape &s) { return s.S == 2 && s.D > 1 && !s.ksteps && fir_decim_lds_ok(s) && !s.decfft && !s.pre_disc && !s.post_disc; }
// the persistent instantiation of the Toeplitz kernel: M = 128 at D = 1 (36 MFMA steps on ComplexFloat32, the headline; 37 on Float32, slack up to 3 samples)
// and at D = 5 (51 steps, the WBFM Tuner / Decimator(5)).  Round 5: the Tuner of an FM receiver at OTHER input rates - decimation 4, 8, 10 at 128 taps - with
// the discriminator epilogue (only that combination: the plain Tuner / Decimator at these decimations keep the generic kernel)
inline bool fir_mfma_persistent(const FirShape &s)
{
    if (s.D == 1) return s.ksteps == 36 || s.ksteps == 37;
    if (s.D == 5) return s.ksteps == 51;
    return s.S == 2 && (s.D == 4 || s.D == 8 || s.D == 10) && s.post_disc && s.rot && s.ksteps == fir_disc_ksteps((int)s.D);
}
// the discriminator epilogue exists for the persistent instantiations of the complex-stream, real-taps kernel
// (round 5: and for the Tuner - rotator fused - at decimation 4, 8, 10 with 128 taps: FM receivers at other input rates)
inline bool fir_can_post_disc(const FirShape &s, const FirKnobs &k)
{
    if (s.decfft || fir_win_cplx_ok(s, k)) return true;
    if (!(s.S == 2 && !s.taps_complex && !s.fft_arith && !s.use_fft)) return false;
    if ((s.D == 1 && s.ksteps == 36) || (s.D == 5 && s.ksteps == 51)) return true;
    // round 5: the second LDS-staged decimator form (kernels_firdecim.h) has the epilogue at every decimation it takes - Tuner(.., 50) / (.., 80) +
    // FrequencyDiscriminator of rtlsdr_nbfm.lua, rtlsdr_pocsag.lua, rtlsdr_ax25.lua: one launch less, the ComplexFloat32 tuner output never reaches HBM
    if (!k.no_disc_epi_lds && s.ksteps == 0 && s.D > 1 && fir_decim_lds_ok(s) && fir_decim_lds2_ok(s, k)) return true;
    return !k.no_disc_epi_other_d && s.rot && (s.D == 4 || s.D == 8 || s.D == 10) && s.ksteps == fir_disc_ksteps((int)s.D);
}

// THE choice.  `aligned`: the input pointer is a multiple of the sample (raw records: the record) size.  An unaligned pointer sends the polyphase-FFT form down the cascade and
// the Toeplitz forms to the direct kernel - except with a fused rotator / discriminator, which that kernel does not have: the Toeplitz form is still named, and its launch is an error.
inline FirForm fir_form(const FirShape &s, const FirKnobs &k, bool aligned)
{
    if (s.decfft && aligned) return FirForm::DecFft;
    if (s.fft_arith) return FirForm::OverlapSave;
    if (fir_win_real_ok(s, k)) return FirForm::WinReal;
    if (fir_win_cplx_ok(s, k)) return FirForm::WinCplx;
    if (fir_win_short_ok(s, k)) return FirForm::WinShort;
    if (fir_win_short_c_ok(s, k)) return FirForm::WinShortC;
    if (fir_short_real_ok(s, k)) return FirForm::ShortReal;
    if (fir_win_pair_ok(s, k)) return FirForm::WinPair;
    if (!s.ksteps || (s.taps_complex ? s.D > 5 : !fir_mfma_supported_decim(s.D)))      // no Toeplitz table, or no Toeplitz instantiation at this decimation
        return !fir_decim_lds_ok(s) ? FirForm::Direct : fir_decim_lds2_ok(s, k) ? FirForm::DecimLds2 : FirForm::DecimLds1;
    if (s.taps_complex) return aligned ? FirForm::MfmaCc : FirForm::Direct;      // two real Toeplitz filters over the interleaved float stream (launch_mfma_cc)
    if (!aligned && !s.rot && !s.post_disc) return FirForm::Direct;
    return fir_mfma_persistent(s) ? FirForm::MfmaPersistent : FirForm::MfmaGeneric;
}

// ... and among the overlap-save forms, for a launch of n_out outputs on num_cus compute units
inline FirFftForm fir_fft_form(const FirShape &s, const FirKnobs &k, long n_out, int num_cus)
{
    const bool plain = !s.pre_disc && !s.post_disc;
    if (s.fft64_np && k.f64_long && k.fft_pols != 1 && plain && (s.S == 2 || k.f64_f32) && (n_out + 2047) / 2048 >= k.f64_long_min * num_cus) return FirFftForm::Long64;
    // 513 .. 1 281 taps: one wave per 4096-point block (fir_fft64_kernel, one 512- / 256-thread workgroup per CU) once the launch has enough blocks per CU (below);
    // smaller launches keep the workgroup-per-block form, which spreads over more CUs
    const long nblocks4k = s.fft4k_V ? (n_out + (F4K_N - s.fft4k_V) - 1) / (F4K_N - s.fft4k_V) : 0;
    // Float32 streams (round 6, size sweep 2^18 .. 2^26 on one box, profiles/r06_f32_long_filter_sizes.txt): the wave-per-block kernel beats the partitioned
    // one at EVERY size (1 276 taps: 0.034-0.051 against 0.064-0.071 ms up to 2^23 samples - the partitioned kernel has a 40-65 us floor) except where the
    // launch is a little more than one round of the chip's 8 x CUs waves and the filter short (768 taps at 2^24: 2 521 transforms = 1.23 rounds, 0.070 against
    // 0.052 ms): only that window keeps the partitioned kernel
    const long transforms = (nblocks4k + 1) / 2, one_round = 8L * num_cus;
    const bool f32_window = s.fft4k_V == 768 && transforms > one_round && 20 * transforms <= 27 * one_round;
    // ComplexFloat32 streams: the workgroup-per-block kernel up to 20 blocks per CU (real taps; 32 with complex taps, whose wave-per-block form runs four waves per
    // CU) - re-measured in round 6 on the same sweep: at 2^23 samples (2 521-2 979 blocks, the old bound of 8 per CU already on the wave kernel) it is 15-40 %
    // faster (1 276 taps 0.057 against 0.067 ms, 768 taps 0.048 / 0.068, complex taps 0.057 / 0.081), at 2^24 the two cross (0.108 / 0.097, 0.091 / 0.095, 0.108 / 0.119)
    const bool wave4k = k.f4k_wave >= 0 ? k.f4k_wave != 0 : s.S == 1 ? !f32_window : nblocks4k >= (s.taps_complex ? 32L : 20L) * num_cus;
    // (a Float32 stream has no workgroup-per-block kernel: where the wave-per-block kernel is not taken it stays partitioned)
    const bool f32_part = s.S == 1 && (!k.f64_f32 || !wave4k);
    if (s.M > FIR_FFT_PART && plain && k.fft_pols != 0 && (k.fft_pols == 1 || !s.fft4k_V || k.fft_no_4k || f32_part)) return FirFftForm::Pols;
    // (known inconsistency, pinned in the table of tools/host_fir_form_check.hip and left for a follow-up: with LRHIP_F64_F32=0 and LRHIP_FFT_POLS=0 a Float32
    // stream of 513 .. 1 281 taps gets here and takes the very kernel the first knob is documented to switch off)
    if (s.fft4k_V && !k.fft_no_4k && plain && wave4k) return FirFftForm::Wave64;
    if (s.fft4k_V && !k.fft_no_4k && plain && s.S == 2) return FirFftForm::Wg4k;
    return FirFftForm::Pass1024;      // one accumulating pass of the 1024-point kernel per 512 taps
}

// chunk alignment that keeps the rounding independent of how a stream is cut (lrhip_stage::align)
inline unsigned long fir_align(const FirShape &s, const FirKnobs &k)
{
    if (s.iir_fused) return 2UL * 256 * 5 * s.D;                      // pair-mode tile: 2 x 256 lanes x 5 outputs
    if (s.fft_arith) {
        // overlap-save arithmetic: the 1024-point blocks advance by Lf samples from the start of a chunk (two blocks ride together on
        // a Float32 stream); the same grid gives the same rounding
        unsigned long l = 1;
        for (int m = s.M; m > 0; m -= FIR_FFT_PART) {      // partitions of FIR_FFT_PART taps, the last one shorter
            const int Mp = m < FIR_FFT_PART ? m : FIR_FFT_PART;
            l = std::lcm(l, (unsigned long)(FFTN - ((Mp - 1 + 63) / 64) * 64) * (s.S == 1 ? 2UL : 1UL));
        }
        return l;
    }
    if (s.rot && s.post_disc && !s.decfft && !fir_win_cplx_ok(s, k) && s.rel_rot) {
        // tuner + discriminator on the persistent Toeplitz kernel: a tile's window is rotated relative to its first sample
        // (kernels_fir.h, REL), so the rounding follows the tile grid, which starts with the chunk
        if (s.D == 1) return (unsigned long)FirMfmaGeom<2, 1>::tile_out(LRHIP_FIR_D1_NACC);
        if (s.D == 5) return 5UL * FirMfmaGeom<2, 5>::tile_out(k.d5_nacc == 1 ? 1 : 2, s.ksteps == 51 && s.rel_nw1 ? 1 : 4);
    }
    return 1UL;
}

// round 5 (host_execute's direct mode, the ring's in-place input): the forms that stage their input through LDS ONCE in one launch and never read
// their output back - overlap-save in one launch, the Toeplitz kernels, the LDS-staged decimators, the polyphase-FFT decimator.  Not the last-resort
// direct kernel (M global reads per output), the multi-launch partitioned filters (they accumulate into y), the opt-in window kernels
inline bool fir_direct_io_ok(const FirShape &s, const FirKnobs &k)
{
    if (s.pre_disc || s.use_fft) return false;      // (use_fft: the reference's block-emission framing - run() copies x into `pending` / `work` first, a second pass, device-to-device)
    switch (fir_form(s, k, true)) {
        case FirForm::DecFft: return true;
        case FirForm::OverlapSave: return s.M <= FIR_FFT_PART || (s.S == 2 && (s.fft4k_V || (s.fft64_np && s.fft64_np <= 2)));      // (4 098 taps and more: the second launch re-reads y)
        case FirForm::WinReal: case FirForm::WinCplx: case FirForm::ShortReal: return false;
        default: return s.ksteps != 0 || (s.D > 1 && fir_decim_lds_ok(s));      // (deliberately narrower than "not Direct": an LDS-staged launch at D = 1 is left out)
    }
}
// the two kernels with record instantiations (IQFileSource's u8 / s8 / s16le records converted on the way into LDS): the persistent Toeplitz kernel at 128
// taps, decimation 5, and the LDS-staged decimator of a shape without a Toeplitz table
inline bool fir_raw_records_ok(const FirShape &s, const FirKnobs &k)
{
    if (s.post_disc || s.pre_disc || s.use_fft || s.taps_complex || s.S != 2) return false;
    const FirForm f = fir_form(s, k, true);
    return (f == FirForm::MfmaPersistent && s.D == 5) || ((f == FirForm::DecimLds1 || f == FirForm::DecimLds2) && !s.ksteps);
}
