// fir_plan.h - from a FIRFilterBlock request (taps, stream type, decimation, use_fft 0..3, fused rotator) to the shape that fir_form() chooses a kernel from:
// the ONE statement of the tap-count ranges, the LDS bounds of the Toeplitz tap arrays and the fall-backs.  Host-only, plain C++17, no HIP calls; include it
// after the kernel headers, as fir_form.h.  fir_build() (stage_fir.h) refuses or builds what fir_resolve() returns; tools/host_fir_tables_check.hip pins it
// against a literal table on the CPU.
#pragma once
#include <algorithm>
#include <cmath>
#include "fir_form.h"

// (use_fft: 0 direct form, 1 overlap-save as the reference: block emission, 2 overlap-save arithmetic, 3 automatic; rot: a rotator fused in front)
struct FirRequest { unsigned ntaps; int taps_complex, input_complex; unsigned decim; int use_fft; bool rot; };
// the device tables a shape calls for, besides the reversed taps that every stage has (builders: fir_tables.h)
enum : unsigned { FIR_TAB_TOEPLITZ = 1, FIR_TAB_TOEPLITZ_CC = 2, FIR_TAB_CTAPS4 = 4, FIR_TAB_DECFFT = 8, FIR_TAB_FFT1024 = 16, FIR_TAB_FFT4K = 32, FIR_TAB_FFT64 = 64, FIR_TAB_FFT64_LONG = 128 };
struct FirPlan {
    const char *refusal = nullptr;        // why there is no such stage (then nothing below means anything)
    bool use_fft = false, fft_arith = false, decfft = false, ctaps4 = false;      // FirShape's fields of these names
    int ksteps = 0, fft4k_V = 0, fft64_np = 0, hist_pad = 0, mode_req = 0;      // ... and FirStage's hist_pad, mode_req
    long L = 0;                           // block length of the reference's emission framing (use_fft)
    unsigned tables = 0;                  // FIR_TAB_*
};

inline FirPlan fir_resolve(const FirRequest &r)
{
    FirPlan p;
    const auto refuse = [&p](const char *why) { p.refusal = why; return p; };
    const unsigned ntaps = r.ntaps, decim = r.decim; const int S = r.input_complex ? 2 : 1;
    if (ntaps < 1) return refuse("fir: need at least one tap");
    if (r.taps_complex && !r.input_complex) return refuse("fir: complex taps require ComplexFloat32 input (firfilter.lua:69-74)");
    if (decim < 1) return refuse("fir: decimation must be >= 1");
    int mode = p.mode_req = r.use_fft;
    // decimating filters: overlap-save arithmetic exists in the polyphase form (kernels_firdecfft.h) for the complex stream
    if (decim > 1 && (mode == 2 || mode == 3)) {
        // automatic (3) keeps the direct form for decimating filters: on MI355X the Toeplitz MFMA kernel is the faster one there
        // (Tuner + discriminator, 2^26 samples: 0.155 ms against 0.165 ms, same box) and it is bit-exact
        p.decfft = mode == 2 && fir_decfft_supported(decim, (int)ntaps, S);
        // "fast" is an arithmetic preference, not a framing: where no polyphase-FFT kernel exists for (taps, decimation) the direct form runs -
        // stand-alone exactly as lrhip_chain_create does when it fuses filter and downsampler (one behaviour for both front doors)
        mode = 0;
    }
    const bool os_range = decim == 1 && !r.rot && ntaps <= 16 * FIR_FFT_PART;      // where the overlap-save tables exist: automatic takes them from 48 taps, "fast" and the framing from 32
    if (mode == 3) mode = os_range && ntaps >= 48 ? 2 : 0;
    if (mode && decim != 1) return refuse("fir: the reference's block-emission framing (use_fft = 1) cannot be combined with decimation");
    if (mode < 0 || mode > 2) return refuse("fir: use_fft must be 0 (direct form), 1 (overlap-save as the reference: block emission), 2 (overlap-save arithmetic, sample-exact emission) or 3 (automatic)");
    if (ntaps > (1u << 20)) return refuse("fir: too many taps");
    p.use_fft = mode == 1;      // 1: reference emission framing; 2: FFT arithmetic, sample-exact emission
    if (!r.taps_complex && fir_mfma_supported_decim(decim)) {
        const int ks = fir_mfma_ksteps((int)ntaps, (int)decim, S);
        if ((size_t)fir_taps_len((int)decim, ks) * sizeof(float) <= 24 * 1024) { p.ksteps = ks; p.tables |= FIR_TAB_TOEPLITZ; }      // tap array must leave LDS room for the tile
    }
    // short complex filters as a streaming kernel (FirForm::WinShortC)
    if (r.taps_complex && decim == 1 && (ntaps == 16 || ntaps == 32)) { p.ctaps4 = true; p.tables |= FIR_TAB_CTAPS4; }
    if (r.taps_complex && decim <= 5) {
        // two real Toeplitz filters over the interleaved float stream (launch_mfma_cc): 2 M taps at decimation 2 D
        const int ks = fir_mfma_ksteps(2 * (int)ntaps, 2 * (int)decim, 1, 2);          // 8-B aligned complex input => float slack e in {0, 2}
        if ((size_t)2 * fir_taps_len(2 * (int)decim, ks) * sizeof(float) <= 32 * 1024) { p.ksteps = ks; p.hist_pad = 1; p.tables |= FIR_TAB_TOEPLITZ_CC; }
    }
    if (p.decfft) p.tables |= FIR_TAB_DECFFT;
    if (r.rot && !p.decfft && !p.ksteps && !(r.input_complex && !r.taps_complex && (int)ntaps + 255 <= DECIM_SPAN_MAX))
        return refuse("fir: rotator fusion unavailable for this tap count / decimation");
    if (mode && os_range && ntaps >= 32) {
        // fused overlap-save kernels: the 1024-point tables, one set per partition of <= FIR_FFT_PART taps, for every such filter
        p.fft_arith = true; p.tables |= FIR_TAB_FFT1024;
        // (round 6: Float32 streams with real taps take the 64 x 64 kernel too - two stream blocks per transform; the workgroup-per-block kernel of small
        // launches stays ComplexFloat32-only, small Float32 launches keep the partitioned kernel)
        if ((int)ntaps > FIR_FFT_PART && ntaps <= 1281) {
            p.fft4k_V = std::max(768, (int)((ntaps - 1 + 255) / 256) * 256);
            p.tables |= FIR_TAB_FFT64 | (r.input_complex ? FIR_TAB_FFT4K : 0u);
        }
        // round 5: the 64 x 64 form at an overlap of 2 048 - one partition to 2 049 taps, two (taps [0, 2 048) and [2 048, ntaps)) above;
        // round 6: three / four partitions of 2 048 taps - a second table set for the second launch.  (<= 8 193 as the partition count allows; os_range ends at 8 192)
        if (ntaps > 1281 && ntaps <= 8193) {
            p.fft64_np = (int)((ntaps + 2046) / 2048);      // ceil((ntaps - 1) / 2 048): 1 to 2 049 taps, 2 to 4 097, 3 to 6 145, 4 to 8 193
            p.tables |= FIR_TAB_FFT64_LONG;
        }
    }
    if (p.use_fft) p.L = (1L << (long)std::floor(std::log(8.0 * ntaps) / std::log(2.0))) - (long)ntaps + 1;      // firfilter.lua:329
    return p;
}
