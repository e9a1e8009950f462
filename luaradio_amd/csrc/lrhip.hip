// lrhip.hip - liblrhip.so: the C ABI of include/lrhip.h over the CDNA4 kernels in kernels_*.h.
// Build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -shared -fPIC -o luaradio_amd/liblrhip.so lrhip.hip
#include "../../include/lrhip.h"

#include <cmath>
#include <memory>
#include <string>

#include "common.h"
#include "kernels_elem.h"
#include "kernels_fft.h"
#include "kernels_fir.h"
#include "kernels_firfft.h"
#include "kernels_firdecfft.h"
#include "kernels_firdecim.h"
#include "kernels_channelizer.h"
#include "kernels_pfb.h"
#include "kernels_pfbsynth.h"
#include "kernels_iir.h"
#include "kernels_agc.h"
#include "kernels_firwin.h"
#include "kernels_firwin2.h"
#include "kernels_firfft4k.h"
#include "kernels_firpols.h"
#include "kernels_firfft64.h"
#include "kernels_interp.h"
#include "kernels_rx.h"
#include "kernels_digital.h"
#include "kernels_bitscan.h"
#include "kernels_preamble.h"
#include "kernels_varicode.h"
#include "kernels_rdsframer.h"
#include "kernels_ertframer.h"
#include "kernels_ax25framer.h"
#include "kernels_pocsagframer.h"
#include "kernels_phasecorr.h"
#include "kernels_modulator.h"
#include "kernels_demodulator.h"
#include "kernels_pll.h"
#include "kernels_interleave.h"
#include "kernels_source.h"
#include "kernels_arbresample.h"
#include "kernels_viterbi.h"
#include "kernels_reedsolomon.h"
#include "kernels_fecglue.h"

using namespace lrhip;

static int g_launches = 0;   // kernels enqueued since the counter was last cleared (chain diagnostics)
#define LR_LAUNCH_CHECK()                                                                              \
    do {                                                                                               \
        g_launches++;                                                                                  \
        hipError_t e__ = hipGetLastError();                                                            \
        if (e__ != hipSuccess) return set_error("kernel launch failed: %s (%s:%d)", hipGetErrorString(e__), __FILE__, __LINE__); \
    } while (0)

#include "stage.h"
#include "stage_carry.h"
#include "op_string.h"
#include "stage_counted.h"
#include "stage_fir.h"
#include "stage_elem.h"
#include "stage_iir.h"
#include "stage_firwin.h"
#include "stage_spectrum.h"
#include "stage_elem2.h"
#include "stage_resample.h"
#include "stage_pfb.h"
#include "stage_elem3.h"
#include "stage_rx.h"
#include "chain.h"
#include "stage_phasecorr.h"
#include "stage_digital.h"
#include "stage_pll.h"
#include "stage_preamble.h"
#include "stage_framers.h"
#include "stage_modulator.h"
#include "stage_demodulator.h"
#include "stage_pfbsynth.h"
#include "stage_interleave.h"
#include "stage_source.h"
#include "stage_arbresample.h"
#include "stage_viterbi.h"
#include "stage_reedsolomon.h"
#include "stage_fecglue.h"
#include "chain_plan.h"

// =====================================================================================================
// C ABI
// =====================================================================================================
extern "C" {

const char *lrhip_version(void) { return "lrhip 0.1 (gfx950)"; }
const char *lrhip_strerror(void) { return err_buf(); }

int lrhip_init(int device)
{
    err_buf()[0] = 0;
    return ensure_init(device);
}

int lrhip_device(void)
{
    const Context &c = ctx();
    return (c.ready && c.pid == (long)getpid()) ? c.device : -1;
}

int lrhip_device_count(void)
{
    if (ctx().ready && ctx().pid != (long)getpid()) return ensure_init();      // forked after the parent initialised the device: the message, not a hang
    int count = 0;
    LR_HIP(hipGetDeviceCount(&count));
    return count;
}

int lrhip_set_stream(void *hip_stream)
{
    if (ensure_init()) return -1;
    // (void *)1 = hipStreamLegacy: the default ("null") stream, whose handle inside the library is plain 0 - every HIP entry point takes that
    hipStream_t next = hip_stream == (void *)1 ? (hipStream_t) nullptr : hip_stream ? (hipStream_t)hip_stream : ctx().own_stream, prev = ctx().stream;
    if (next != prev) {
        // work already queued on the previous stream (reset() memsets, earlier chunks that carried state forward) is ordered
        // before everything that follows on the new one
        hipEvent_t ev = nullptr;
        LR_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        hipError_t e1 = hipEventRecord(ev, prev), e2 = e1 == hipSuccess ? hipStreamWaitEvent(next, ev, 0) : e1;
        (void)hipEventDestroy(ev);
        if (e2 != hipSuccess) return set_error("set_stream: ordering the streams failed: %s", hipGetErrorString(e2));
    }
    ctx().stream = next;
    return 0;
}

int lrhip_synchronize(void)
{
    if (ensure_init()) return -1;
    LR_HIP(hipStreamSynchronize(ctx().stream));
    return 0;
}

lrhip_stage_t *lrhip_fir_create(const float *taps, unsigned ntaps, int taps_complex, int input_complex, unsigned decim, int use_fft)
{
    return fir_build(taps, ntaps, taps_complex, input_complex, decim, use_fft, false, 0.0);
}

lrhip_stage_t *lrhip_rotator_create(double omega)
{
    if (!std::isfinite(omega)) { set_error("rotator: omega must be finite"); return nullptr; }
    auto q = new_stage<RotatorStage>();
    if (!q) return nullptr;
    q->omega = omega;
    q->step = turns_fixed(omega);
    q->in_size = q->out_size = 8;
    return q.release();
}

lrhip_stage_t *lrhip_downsampler_create(unsigned factor, int elem_size)
{
    if (factor < 1) { set_error("downsampler: factor must be >= 1"); return nullptr; }
    if (elem_size != 4 && elem_size != 8) { set_error("downsampler: element size must be 4 or 8"); return nullptr; }
    auto q = new_stage<DownsamplerStage>();
    if (!q) return nullptr;
    q->factor = factor;
    q->in_size = q->out_size = elem_size;
    return q.release();
}

lrhip_stage_t *lrhip_fmdiscrim_create(double gain)
{
    if (!(gain != 0.0) || !std::isfinite(gain)) { set_error("fmdiscrim: gain must be finite and non-zero"); return nullptr; }
    auto q = new_stage<FmDiscrimStage>();
    if (!q) return nullptr;
    q->gain = gain;
    q->in_size = 8; q->out_size = 4;
    if (q->reset()) return nullptr;
    return q.release();
}

lrhip_stage_t *lrhip_iir_create(const float *b, unsigned nb, const float *a, unsigned na, int input_complex)
{
    if (!b || !a || nb < 1 || na < 1) { set_error("iir: need b_taps and at least one a_tap (iirfilter.lua:56)"); return nullptr; }
    if (nb > IIR_SEQ_MAX || na > IIR_SEQ_MAX) { set_error("iir: at most %d taps supported", IIR_SEQ_MAX); return nullptr; }
    if (a[0] == 0.0f) { set_error("iir: a[0] must be non-zero"); return nullptr; }
    return iir_build(b, nb, a, na, input_complex);
}

lrhip_stage_t *lrhip_psd_create(unsigned n, const float *window, double scale, int logarithmic, int input_complex, int fftshift)
{
    if (!(scale > 0.0)) { set_error("psd: scale must be positive"); return nullptr; }
    FftStage *q = fft_build(n);
    if (!q) return nullptr;
    q->in_real = !input_complex;
    q->in_size = input_complex ? 8 : 4;
    q->out_size = 4;
    q->out_kind = logarithmic ? FFT_OUT_PSD_LOG : FFT_OUT_PSD;
    q->out_scale = (float)(1.0 / scale);
    q->shift = fftshift != 0;
    if (window) {
        if (upload(q->window, window, n * sizeof(float))) { delete q; return nullptr; }
        q->has_window = true;
    }
    return q;
}

lrhip_stage_t *lrhip_welch_create(unsigned n, const float *window, double scale, int logarithmic, int input_complex, unsigned overlap)
{
    if (overlap >= n) { set_error("welch: overlap %u must be smaller than the frame length %u", overlap, n); return nullptr; }
    std::unique_ptr<FftStage> psd((FftStage *)lrhip_psd_create(n, window, scale, logarithmic, input_complex, 1));
    if (!psd) return nullptr;
    std::unique_ptr<WelchStage> q(new (std::nothrow) WelchStage());
    if (!q) { set_error("out of memory"); return nullptr; }
    q->N = (int)n; q->hop = (int)(n - overlap);
    q->in_size = input_complex ? 8 : 4; q->out_size = 4;
    q->psd = std::move(psd);
    if (q->reset()) return nullptr;
    return q.release();
}

long lrhip_welch_read(lrhip_stage_t *q, float *avg_host, int reset)
{
    WelchStage *w = q ? dynamic_cast<WelchStage *>(q) : nullptr;
    if (!w) return set_error("welch_read: not a welch stage");
    long frames = w->count;
    if (frames > 0) {
        if (!avg_host) return set_error("null output buffer");
        size_t bytes = (size_t)w->N * sizeof(float);
        if (w->h_avg.reserve(bytes)) return -1;
        LR_HIP(hipMemcpyAsync(w->h_avg.p, w->sum.p, bytes, hipMemcpyDeviceToHost, ctx().stream));
        LR_HIP(hipStreamSynchronize(ctx().stream));
        const float *src = (const float *)w->h_avg.p;
        for (int i = 0; i < w->N; i++) avg_host[i] = src[i] / (float)frames;      // gnuplotspectrum.lua:179-181
    }
    if (reset && w->clear()) return -1;
    return frames;
}

lrhip_stage_t *lrhip_dft_create(unsigned n, int inverse, int real_side)
{
    FftStage *q = fft_build(n);
    if (!q) return nullptr;
    q->inverse = inverse != 0;
    if (!inverse) {
        q->in_real = real_side != 0;
        q->in_size = real_side ? 4 : 8;
        q->out_size = 8;
        q->out_kind = FFT_OUT_COMPLEX;
        q->out_scale = 1.0f;
    } else {
        q->in_real = 0;
        q->in_size = 8;
        q->out_size = real_side ? 4 : 8;
        q->out_kind = real_side ? FFT_OUT_REAL : FFT_OUT_COMPLEX;
        q->out_scale = (float)(1.0 / (double)n);      // spectrum_utils.lua:335-338
    }
    return q;
}

lrhip_stage_t *lrhip_format_convert_create(const char *format, int complex_out)
{
    if (!format) { set_error("format: missing format name"); return nullptr; }
    int idx = -1;
    for (size_t i = 0; i < sizeof(kFormats) / sizeof(kFormats[0]); i++)
        if (!strcmp(kFormats[i].name, format)) idx = (int)i;
    if (idx < 0) { set_error("Unsupported format (\"%s\")", format); return nullptr; }     // iqfile.lua:48
    auto q = new_stage<FormatStage>();
    if (!q) return nullptr;
    q->fmt = idx;
    q->scalars = complex_out ? 2 : 1;
    q->in_size = kFormats[idx].bytes * q->scalars;
    q->out_size = 4 * q->scalars;
    return q.release();
}

lrhip_stage_t *lrhip_format_pack_create(const char *format, int complex_in)
{
    FormatStage *q = (FormatStage *)lrhip_format_convert_create(format, complex_in);
    if (!q) return nullptr;
    q->pack = true;
    std::swap(q->in_size, q->out_size);
    return q;
}

lrhip_stage_t *lrhip_multiply_constant_create(float re, float im, int constant_complex, int input_complex)
{
    if (constant_complex && !input_complex) { set_error("multiplyconstant: a complex constant takes ComplexFloat32 input only (multiplyconstant.lua:42-44)"); return nullptr; }
    auto q = new_stage<MulConstStage>();
    if (!q) return nullptr;
    q->cr = re; q->ci = constant_complex ? im : 0.f;
    q->mode = !input_complex ? 0 : (constant_complex ? 2 : 1);
    q->in_size = q->out_size = input_complex ? 8 : 4;
    return q.release();
}

lrhip_stage_t *lrhip_upsampler_create(unsigned factor, int elem_size)
{
    if (factor < 1) { set_error("upsampler: factor must be >= 1"); return nullptr; }
    if (elem_size != 4 && elem_size != 8) { set_error("upsampler: element size must be 4 or 8"); return nullptr; }
    auto q = new_stage<UpsamplerStage>();
    if (!q) return nullptr;
    q->factor = factor;
    q->in_size = q->out_size = elem_size;
    return q.release();
}

lrhip_stage_t *lrhip_agc_create(double power_alpha, double gain_alpha, double target, double threshold, int input_complex)
{
    if (!(power_alpha > 0.0 && power_alpha <= 1.0) || !(gain_alpha > 0.0 && gain_alpha <= 1.0)) { set_error("agc: alphas must be in (0, 1]"); return nullptr; }
    if (!(target > 0.0) || !(threshold >= 0.0)) { set_error("agc: target and threshold are linear powers (> 0)"); return nullptr; }
    auto q = new_stage<AgcStage>();
    if (!q) return nullptr;
    q->p = AgcParams{power_alpha, gain_alpha, target, threshold};
    q->S = input_complex ? 2 : 1;
    q->in_size = q->out_size = 4 * q->S;
    if (q->reset()) return nullptr;
    return q.release();
}

lrhip_stage_t *lrhip_powersquelch_create(double alpha, double threshold, int input_complex)
{
    if (!(alpha > 0.0 && alpha <= 1.0)) { set_error("powersquelch: alpha must be in (0, 1]"); return nullptr; }
    AgcStage *q = (AgcStage *)lrhip_agc_create(alpha, 1.0, 1.0, threshold, input_complex);
    if (q) q->squelch = true;
    return q;
}

lrhip_stage_t *lrhip_fmmod_create(double modulation_index)
{
    if (!std::isfinite(modulation_index)) { set_error("fmmod: modulation index must be finite"); return nullptr; }
    auto q = new_stage<FmModStage>();
    if (!q) return nullptr;
    q->k = modulation_index;
    q->in_size = 4; q->out_size = 8;
    if (q->reset()) return nullptr;
    return q.release();
}

lrhip_stage_t *lrhip_unary_create(const char *op, float re, float im, int constant_complex, int input_complex)
{
    if (!op) { set_error("unary: missing operation name"); return nullptr; }
    // the stages that read an op string "name:key=value:..." (op_string.h), and the parameterless ones (plain_create, stage_counted.h)
    static const struct { const char *head; lrhip_stage_t *(*create)(const char *op); } kCreators[] = {
        {"zerocrossingclockrecovery", zc_create}, {"clocksampler", zc_create}, {"slicer", slicer_create}, {"differentialdecoder", diffdec_create},
        {"binaryphasecorrector", phasecorr_create}, {"pll", pll_create}, {"preamblesampler", preamblesampler_create},
        {"manchesterdecoder", manchesterdecoder_create}, {"pam", modulator_create}, {"qam", modulator_create},
        {"pamdemod", demodulator_create}, {"qamdemod", demodulator_create},
        {"pfbsynthesizer", pfb_synthesizer_create}, {"interleave", port_stage_create}, {"deinterleave", port_stage_create},
        {"wavpack", port_stage_create}, {"wavunpack", port_stage_create}, {"signalsource", source_create}, {"uniformrandomsource", source_create},
        {"arbresampler", arbresampler_create}, {"convenc", convenc_create}, {"viterbi", viterbi_create},
        {"rsenc", reedsolomon_create}, {"rsdec", reedsolomon_create}, {"packbits", bitpack_create}, {"unpackbits", bitpack_create},
        {"puncture", puncture_create}, {"depuncture", puncture_create}, {"convinterleave", convinterleave_create},
        {"convdeinterleave", convinterleave_create}, {"scrambler", scrambler_create},
        {"rdsframer", plain_create<RfStage, 8>}, {"scmframer", plain_create<EfStage<EF_SCM>, EfProto<EF_SCM>::REC>},
        {"scmplusframer", plain_create<EfStage<EF_SCMPLUS>, EfProto<EF_SCMPLUS>::REC>}, {"idmframer", plain_create<EfStage<EF_IDM>, EfProto<EF_IDM>::REC>},
        {"ax25framer", plain_create<AxStage, AX_REC>}, {"pocsagframer", plain_create<PgStage, PG_REC>}, {"varicodedecoder", plain_create<VcStage, 1>}};
    const size_t head_len = strcspn(op, ":");
    for (auto &c : kCreators)
        if (strlen(c.head) == head_len && !strncmp(c.head, op, head_len)) return c.create(op);
    struct { const char *name; int code, in, out; } T[] = {
        {"complexmagnitude", UN_CMAG, 8, 4}, {"complexphase", UN_CPHASE, 8, 4}, {"complextoreal", UN_CREAL, 8, 4},
        {"complextoimag", UN_CIMAG, 8, 4},   {"complexconjugate", UN_CCONJ, 8, 8}, {"realtocomplex", UN_R2C, 4, 8},
        {"absolutevalue", UN_ABS, 4, 4}};
    int code = -1, in = 0, out = 0;
    for (auto &t : T)
        if (!strcmp(t.name, op)) { code = t.code; in = t.in; out = t.out; }
    if (!strcmp(op, "addconstant")) {
        if (constant_complex && !input_complex) { set_error("addconstant: a complex constant takes ComplexFloat32 input only (addconstant.lua:42-44)"); return nullptr; }
        code = !input_complex ? UN_ADDC_REAL : (constant_complex ? UN_ADDC_CPLX : UN_ADDC_CPLX_BY_REAL);
        in = out = input_complex ? 8 : 4;
    }
    if (code < 0) { set_error("unary: unknown operation \"%s\"", op); return nullptr; }
    auto q = new_stage<UnaryStage>();
    if (!q) return nullptr;
    q->op = code; q->cr = re; q->ci = im;
    q->in_size = in; q->out_size = out;
    return q.release();
}

lrhip_stage_t *lrhip_delay_create(unsigned num_samples, int elem_size)
{
    if (num_samples < 1) { set_error("Number of samples must be greater than 0"); return nullptr; }      // delay.lua:28
    if (elem_size != 4 && elem_size != 8) { set_error("delay: element size must be 4 or 8"); return nullptr; }
    auto q = new_stage<DelayStage>();
    if (!q) return nullptr;
    q->D = num_samples;
    q->in_size = q->out_size = elem_size;
    if (q->reset()) return nullptr;
    return q.release();
}

lrhip_stage_t *lrhip_hilbert_create(const float *taps, unsigned ntaps)
{
    if (!taps || (ntaps % 2) != 1) { set_error("Number of taps must be odd"); return nullptr; }          // hilberttransform.lua:29
    std::unique_ptr<HilbertStage> q(new (std::nothrow) HilbertStage());
    if (!q) { set_error("out of memory"); return nullptr; }
    q->fir.reset(fir_build(taps, ntaps, 0, 0, 1, 0, false, 0.0));
    if (!q->fir) return nullptr;
    q->in_size = 4; q->out_size = 8;
    return q.release();
}

lrhip_stage_t *lrhip_channelizer_create(const float *taps, unsigned ntaps, unsigned nchannels)
{
    if (!taps || ntaps < 32 || (ntaps % 32) != 0 || ntaps > 8192) { set_error("channelizer: ntaps must be a multiple of 32 in [32, 8192]"); return nullptr; }
    if (nchannels != 32 && nchannels != 64) { set_error("channelizer: nchannels must be 32 or 64"); return nullptr; }
    return channelizer_build(taps, ntaps, nchannels);
}

lrhip_stage_t *lrhip_pfb_channelizer_create(const float *taps, unsigned ntaps, unsigned nchannels)
{
    return lrhip_pfb_oversampled_create(taps, ntaps, nchannels, 1);
}

lrhip_stage_t *lrhip_pfb_oversampled_create(const float *taps, unsigned ntaps, unsigned nchannels, unsigned oversample)
{
    if (const char *why = PfbChannelizerStage::refusal(taps ? ntaps : 0, nchannels, oversample)) { set_error("%s", why); return nullptr; }
    auto q = new_stage<PfbChannelizerStage>();
    if (!q) return nullptr;
    const int M = (int)ntaps, K = (int)nchannels;
    q->M = M; q->K = K; q->P = (M + K - 1) / K;
    q->R = (int)oversample; q->D = K / q->R;
    while ((1 << q->log2k) < K) q->log2k++;
    q->in_size = q->out_size = 8;
    std::vector<float> tw((size_t)K);      // W_K^m = exp(-2 pi i m / K), m < K / 2 (kernels_fft.h), computed in double
    for (int m = 0; m < K / 2; m++) {
        double ang = -2.0 * 3.14159265358979323846 * m / K;
        tw[2 * m] = (float)std::cos(ang);
        tw[2 * m + 1] = (float)std::sin(ang);
    }
    if (upload(q->taps, taps, (size_t)M * sizeof(float)) || upload(q->tw, tw.data(), tw.size() * sizeof(float))) return nullptr;
    if (q->reset()) return nullptr;
    return q.release();
}

lrhip_stage_t *lrhip_binary_create(const char *op, int input_complex)
{
    if (!op) { set_error("binary: missing operation name"); return nullptr; }
    if (!strcmp(op, "sampler")) {
        // SamplerBlock: data (ComplexFloat32 / Float32, input_complex) and a Float32 clock; the output count depends on the clock
        auto q = new_stage<SamplerStage>();
        if (!q) return nullptr;
        q->in_size = q->out_size = input_complex ? 8 : 4;
        q->in2_size = 4;
        if (q->reset()) return nullptr;
        return q.release();
    }
    int code = !strcmp(op, "multiply") ? BIN_MULTIPLY : !strcmp(op, "multiplyconjugate") ? BIN_MULTIPLY_CONJ
             : !strcmp(op, "add") ? BIN_ADD : !strcmp(op, "subtract") ? BIN_SUBTRACT : !strcmp(op, "floattocomplex") ? BIN_F2C : -1;
    if (code < 0) { set_error("binary: unknown operation \"%s\"", op); return nullptr; }
    if (code == BIN_MULTIPLY_CONJ && !input_complex) { set_error("binary: multiplyconjugate takes ComplexFloat32 inputs (multiplyconjugate.lua:26)"); return nullptr; }
    auto q = new_stage<BinaryStage>();
    if (!q) return nullptr;
    q->op = code;
    q->in_size = q->out_size = input_complex ? 8 : 4;
    if (code == BIN_F2C) { q->in_size = 4; q->out_size = 8; }
    return q.release();
}

void lrhip_stage_destroy(lrhip_stage_t *q)
{
    if (!q) return;
    if (ctx().ready) (void)hipStreamSynchronize(ctx().stream);
    delete q;
}

int lrhip_stage_reset(lrhip_stage_t *q) { return q ? q->reset() : set_error("null stage"); }
int lrhip_stage_input_size(const lrhip_stage_t *q) { return q ? q->in_size : set_error("null stage"); }
int lrhip_stage_output_size(const lrhip_stage_t *q) { return q ? q->out_size : set_error("null stage"); }
unsigned long lrhip_stage_max_output(const lrhip_stage_t *q, unsigned long n_in) { return q ? q->max_output(n_in) : 0; }

long lrhip_stage_execute_device(lrhip_stage_t *q, const void *in_dev, unsigned long n_in, void *out_dev, unsigned long out_capacity)
{
    if (!q) return set_error("null stage");
    if (n_in && ((!in_dev && !q->is_source()) || (!out_dev && q->max_output(n_in)))) return set_error("null buffer");
    return q->run(in_dev, n_in, out_dev, out_capacity);
}

long lrhip_stage_execute(lrhip_stage_t *q, const void *in_host, unsigned long n_in, void *out_host, unsigned long out_capacity)
{
    if (!q) return set_error("null stage");
    if (dynamic_cast<PortStage *>(q)) return set_error("%s stage takes a port table of device pointers: use lrhip_stage_execute_device", q->kind());
    return host_execute(q->h_in, q->h_out, q->d_in, q->d_out, q->in_size, q->out_size, q->max_output(n_in), in_host, n_in,
                        out_host, out_capacity,
                        [&](const void *di, unsigned long n, void *dout, unsigned long cap) { return q->run(di, n, dout, cap); }, q->align(), q->direct_io_ok());
}

long lrhip_stage_execute2_device(lrhip_stage_t *q, const void *in1_dev, const void *in2_dev, unsigned long n_in, void *out_dev,
                                 unsigned long out_capacity)
{
    if (!q) return set_error("null stage");
    if (n_in && (!in1_dev || !in2_dev || !out_dev)) return set_error("null buffer");
    return q->run2(in1_dev, in2_dev, n_in, out_dev, out_capacity);
}

long lrhip_stage_execute2(lrhip_stage_t *q, const void *in1_host, const void *in2_host, unsigned long n_in, void *out_host,
                          unsigned long out_capacity)
{
    if (!q) return set_error("null stage");
    BinaryStage *b = dynamic_cast<BinaryStage *>(q);
    if (!b) return set_error("%s is not a two-input stage", q->kind());
    if (n_in && !in2_host) return set_error("null input buffer");
    const int in2_size = q->input2_size();
    size_t bytes = (size_t)n_in * in2_size;
    if (b->h_in2.reserve(bytes ? bytes : 16) || b->d_in2.reserve(bytes ? bytes : 16)) return -1;
    if (bytes) {
        memcpy(b->h_in2.p, in2_host, bytes);
        LR_HIP(hipMemcpyAsync(b->d_in2.p, b->h_in2.p, bytes, hipMemcpyHostToDevice, ctx().stream));
    }
    // (a piece of a long call starts at the same sample of both inputs)
    return host_execute(q->h_in, q->h_out, q->d_in, q->d_out, q->in_size, q->out_size, q->max_output(n_in), in1_host, n_in, out_host, out_capacity,
                        [&](const void *di, unsigned long n, void *dout, unsigned long cap) {
                            const size_t first = (size_t)((const char *)di - (const char *)q->d_in.p) / (size_t)q->in_size;
                            return q->run2(di, (const char *)b->d_in2.p + first * (size_t)in2_size, n, dout, cap);
                        });
}

// ---- chains ---------------------------------------------------------------------------------------------
lrhip_chain_t *lrhip_chain_create(lrhip_stage_t **stages, unsigned nstages) { return lrhip_chain_create_ex(stages, nstages, 0u); }

lrhip_chain_t *lrhip_chain_create_ex(lrhip_stage_t **stages, unsigned nstages, unsigned flags)
{
    if (!stages || nstages < 1) { set_error("chain: need at least one stage"); return nullptr; }
    if (flags & ~(unsigned)(LRHIP_CHAIN_EXACT_ROTATOR | LRHIP_CHAIN_NO_POLYPHASE_TAIL | LRHIP_CHAIN_NO_FUSION | LRHIP_CHAIN_NO_SINGLE_LAUNCH)) {
        set_error("chain: unknown flag bits 0x%x", flags);
        return nullptr;
    }
    for (unsigned i = 0; i < nstages; i++)
        if (!stages[i]) { set_error("chain: stage %u is null", i); return nullptr; }
    for (unsigned i = 0; i < nstages; i++)
        if (dynamic_cast<PortStage *>(stages[i])) { set_error("chain: stage %u (%s) takes a port table and cannot be part of a chain", i, stages[i]->kind()); return nullptr; }
    // a source has no input: it can only be the head of a chain, where n_in counts the samples to generate
    for (unsigned i = 1; i < nstages; i++)
        if (stages[i]->is_source()) { set_error("chain: stage %u (%s) is a source and can only be the first stage of a chain", i, stages[i]->kind()); return nullptr; }
    for (unsigned i = 0; i + 1 < nstages; i++)
        if (stages[i]->out_size != stages[i + 1]->in_size) {
            set_error("chain: stage %u (%s) emits %d-byte samples but stage %u (%s) takes %d-byte samples", i, stages[i]->kind(),
                      stages[i]->out_size, i + 1, stages[i + 1]->kind(), stages[i + 1]->in_size);
            return nullptr;
        }
    std::unique_ptr<lrhip_chain> c(new (std::nothrow) lrhip_chain());
    if (!c) { set_error("out of memory"); return nullptr; }
    c->flags = flags;
    const PlanFlags pf{!(flags & LRHIP_CHAIN_NO_FUSION), (flags & LRHIP_CHAIN_EXACT_ROTATOR) != 0, (flags & LRHIP_CHAIN_NO_POLYPHASE_TAIL) != 0,
                       !(flags & LRHIP_CHAIN_NO_SINGLE_LAUNCH)};
    // Downsampler(1) is the identity (downsampler.lua:45-56 with factor 1 copies every sample; its index stays 0): it gets no launch of its own
    // (a Tuner / Decimator built with decimation 1) - unless it is the whole chain
    std::vector<lrhip_stage_t *> kept;
    if (pf.fusion && nstages > 1) {
        for (unsigned k = 0; k < nstages; k++) {
            DownsamplerStage *d1 = dynamic_cast<DownsamplerStage *>(stages[k]);
            if (!(d1 && d1->factor == 1)) kept.push_back(stages[k]);
        }
        if (!kept.empty() && kept.size() < nstages) { stages = kept.data(); nstages = (unsigned)kept.size(); }
    }
    // fusion (chain_plan.h): at each stage the first rule that applies builds the fused stage; a stage no rule takes runs its own kernels
    Plan plan{stages, nstages, pf, c->ops};
    for (unsigned i = 0; i < nstages;) {
        int used = 0;
        for (size_t r = 0; pf.fusion && !used && r < sizeof kPlanRules / sizeof kPlanRules[0]; r++) used = kPlanRules[r](plan, i);
        if (used < 0) return nullptr;
        if (!used) { c->ops.emplace_back(stages[i]); used = 1; }
        i += (unsigned)used;
    }
    if (pf.fusion) {
        fold_fixups(c->ops);
        if (merge_receivers(c->ops, pf)) return nullptr;
        fold_tuner_records(c->ops);
        if (digital_fuse_tail(c->ops)) return nullptr;
    }
    for (size_t k = 0; k + 1 < c->ops.size(); k++) c->edges.emplace_back(new DeviceBuf());
    return c.release();
}

void lrhip_chain_destroy(lrhip_chain_t *c)
{
    if (!c) return;
    if (ctx().ready) (void)hipStreamSynchronize(ctx().stream);
    delete c;
}

int lrhip_chain_reset(lrhip_chain_t *c)
{
    if (!c) return set_error("null chain");
    if (c->inflight) return set_error("chain reset: %u chunks still in flight", c->inflight);
    c->fill = 0;
    c->discard_in = 0;
    if (ctx().ready) LR_HIP(hipStreamSynchronize(ctx().stream));
    for (auto &o : c->ops)
        if (o.stage->reset()) return -1;
    return 0;
}

unsigned long lrhip_chain_max_output(const lrhip_chain_t *c, unsigned long n_in)
{
    if (!c) return 0;
    unsigned long n = n_in;
    for (auto &o : c->ops) n = o.stage->max_output(n);
    return n;
}

static unsigned long chain_output_bound(const lrhip_chain *c, unsigned long n);

long lrhip_chain_execute_device(lrhip_chain_t *c, const void *in_dev, unsigned long n_in, void *out_dev, unsigned long out_capacity)
{
    if (!c) return set_error("null chain");
    g_launches = 0;
    if (c->discard_in && n_in) {
        // lrhip_chain_start_at(): the first samples after the seek are the partition's replayed halo - state only, their output is dropped
        const unsigned long k = c->discard_in < n_in ? (unsigned long)c->discard_in : n_in;
        const unsigned long bound = chain_output_bound(c, k);
        if (c->d_discard.reserve((size_t)bound * c->ops.back().stage->out_size + 16)) return -1;
        c->discard_in -= k;
        const unsigned long long left = c->discard_in;
        c->discard_in = 0;
        long rc = lrhip_chain_execute_device(c, in_dev, k, c->d_discard.p, bound);
        c->discard_in = left;
        if (rc < 0) return rc;
        in_dev = (const char *)in_dev + (size_t)k * c->ops.front().stage->in_size;
        n_in -= k;
        if (!n_in) return 0;
    }
    const void *cur = in_dev;
    unsigned long n = n_in;
    for (size_t k = 0; k < c->ops.size(); k++) {
        lrhip_stage *s = c->ops[k].stage;
        bool last = k + 1 == c->ops.size();
        unsigned long need = s->max_output(n);
        void *dst;
        unsigned long cap;
        if (last) {
            dst = out_dev;
            cap = out_capacity;
        } else {
            if (c->edges[k]->reserve((size_t)need * s->out_size + 16)) return -1;
            dst = c->edges[k]->p;
            cap = need;
        }
        long got = s->run(cur, n, dst, cap);
        if (got < 0) return got;
        cur = dst;
        n = (unsigned long)got;
    }
    c->last_launches = g_launches;
    return (long)n;
}

long lrhip_chain_execute(lrhip_chain_t *c, const void *in_host, unsigned long n_in, void *out_host, unsigned long out_capacity)
{
    if (!c) return set_error("null chain");
    return host_execute(c->h_in, c->h_out, c->d_in, c->d_out, c->ops.front().stage->in_size, c->ops.back().stage->out_size,
                        lrhip_chain_max_output(c, n_in), in_host, n_in, out_host, out_capacity,
                        [&](const void *di, unsigned long n, void *dout, unsigned long cap) { return lrhip_chain_execute_device(c, di, n, dout, cap); },
                        lrhip_chain_shard_align(c), c->ops.front().stage->direct_io_ok() && c->ops.back().stage->direct_io_ok());
}

int lrhip_chain_last_launches(const lrhip_chain_t *c) { return c ? c->last_launches : set_error("null chain"); }

int lrhip_chain_in_flight(const lrhip_chain_t *c) { return c ? (int)c->inflight : set_error("null chain"); }

// Upper bound on what a stage emits for n inputs in ANY carried state (max_output() is evaluated in the current state).
static unsigned long stage_output_bound(const lrhip_stage *s, unsigned long n)
{
    unsigned long m = s->max_output(n);
    if (const FirStage *f = dynamic_cast<const FirStage *>(s))
        if (f->use_fft) m = n + (unsigned long)f->L;            // block-emission framing: up to L - 1 retained samples come out as well
    return (m > n ? m : n) + 64;
}
static unsigned long chain_output_bound(const lrhip_chain *c, unsigned long n)
{
    for (auto &o : c->ops) n = stage_output_bound(o.stage, n);
    return n;
}

int lrhip_chain_set_ring(lrhip_chain_t *c, unsigned depth, unsigned long max_chunk)
{
    if (!c) return set_error("null chain");
    if (depth < 1 || depth > 16) return set_error("ring depth must be 1..16");
    if (max_chunk < 1) return set_error("ring: max_chunk must be >= 1");
    if (c->inflight) return set_error("ring: %u chunks still in flight", c->inflight);
    if (ensure_init()) return -1;
    if (!c->s_in) LR_HIP(hipStreamCreateWithFlags(&c->s_in, hipStreamNonBlocking));
    if (!c->s_out) LR_HIP(hipStreamCreateWithFlags(&c->s_out, hipStreamNonBlocking));
    LR_HIP(hipStreamSynchronize(ctx().stream));
    c->ring.clear();
    int in_size = c->ops.front().stage->in_size, out_size = c->ops.back().stage->out_size;
    // bound on the output of one chunk WHATEVER the carried state: rate-changing stages may emit one extra sample, a FIR with the
    // reference's block-emission framing up to a whole retained block (L - 1 samples) more than its stateless max_output() says
    unsigned long max_out = chain_output_bound(c, max_chunk);
    for (unsigned i = 0; i < depth; i++) {
        std::unique_ptr<lrhip_chain::Slot> sl(new (std::nothrow) lrhip_chain::Slot());
        if (!sl) return set_error("out of memory");
        if (sl->h_in.reserve((size_t)max_chunk * in_size) || sl->d_in.reserve((size_t)max_chunk * in_size)) return -1;
        if (sl->h_out.reserve((size_t)max_out * out_size) || sl->d_out.reserve((size_t)max_out * out_size)) return -1;
        LR_HIP(hipEventCreateWithFlags(&sl->ev_in, hipEventDisableTiming));
        LR_HIP(hipEventCreateWithFlags(&sl->ev_done, hipEventDisableTiming));
        LR_HIP(hipEventCreateWithFlags(&sl->ev_out, hipEventDisableTiming));
        c->ring.push_back(std::move(sl));
    }
    // size the device-resident edges once, so no reallocation happens while chunks are in flight
    unsigned long nmax = max_chunk;
    for (size_t k = 0; k + 1 < c->ops.size(); k++) {
        nmax = stage_output_bound(c->ops[k].stage, nmax);
        if (c->edges[k]->reserve((size_t)nmax * c->ops[k].stage->out_size + 16)) return -1;
    }
    c->ring_chunk = max_chunk;
    c->ring_out_cap = max_out;
    c->fill = 0;
    c->head = 0;
    c->inflight = 0;
    return 0;
}

// the entry points that move input BYTES have nothing to do for a chain whose first stage is a source: it is run by count (execute / submit with a null input)
static int chain_refuse_source(const lrhip_chain *c, const char *what)
{
    const lrhip_stage *s = c->ops.front().stage;
    return s->is_source() ? set_error("%s: the chain starts with a source (%s) and takes no input: call lrhip_chain_execute or lrhip_chain_submit with a "
                                      "null input and the number of samples to generate", what, s->kind()) : 0;
}
static long chain_submit(lrhip_chain_t *c, const void *in_host, unsigned long n_in, bool allow_inplace);
long lrhip_chain_submit(lrhip_chain_t *c, const void *in_host, unsigned long n_in) { return chain_submit(c, in_host, n_in, true); }
static long chain_submit(lrhip_chain_t *c, const void *in_host, unsigned long n_in, bool allow_inplace)
{
    if (!c) return set_error("null chain");
    if (c->ring.empty()) return set_error("chain has no ring: call lrhip_chain_set_ring first");
    if (n_in > c->ring_chunk) return set_error("chunk of %lu samples exceeds the ring's max_chunk %lu", n_in, c->ring_chunk);
    if (c->inflight == c->ring.size()) return set_error("ring full: collect a chunk first (%u in flight)", c->inflight);
    if (c->fill) return set_error("chain has %lu pushed samples pending: flush before mixing submit() with push()", c->fill);
    lrhip_chain::Slot &sl = *c->ring[c->head];
    int in_size = c->ops.front().stage->in_size, out_size = c->ops.back().stage->out_size;
    if (n_in && !in_host && in_size) return set_error("null input buffer");
    size_t bytes = (size_t)n_in * in_size;             // a source at the head: nothing to copy, n_in samples are generated
    const void *zin = nullptr;           // input read in place across the link
    // the slot was collected (ev_out waited) before it can be reused, so its buffers are free on host and device
    if (bytes) {
        // lrhip_chain_ring_input(): the caller filled the slot itself.  A vector inside a range registered with lrhip_host_register() is DMA'd from where it
        // lies (a recording mmap()ed and registered once: the page cache is the staging buffer); the caller keeps it valid until the batch is collected.
        const bool direct = in_host != sl.h_in.p && host_ranges().has(in_host, bytes);
        if (in_host != sl.h_in.p && !direct) host_copy(sl.h_in.p, in_host, bytes);
        // round 5: a chain whose first stage reads its input once takes the slot's pinned input (or the caller's registered vector) AS its input - the
        // kernel loads the records across the link itself; no copy engine, no event hop in front of the launch.  Same box, u8 records -> receiver: pushes of
        // 131 072 records 7.4 -> 9.2 GS/s, read(2) into the slot 9.6 -> 10.6; NOT for lrhip_chain_submit_fd, whose copy threads are the bound either way
        // (15.2 -> 14.3 GS/s: the copy engine costs the GPU nothing while they read).  LRHIP_RING_DIRECT=0: always the copy (A/B)
        static const bool ring_direct = !getenv("LRHIP_RING_DIRECT") || atoi(getenv("LRHIP_RING_DIRECT")) != 0;
        if (ring_direct && allow_inplace && c->ops.front().stage->direct_io_ok()) zin = direct ? host_ranges().device_ptr(in_host, bytes) : sl.h_in.p;
        if (!zin) LR_HIP(hipMemcpyAsync(sl.d_in.p, direct ? in_host : sl.h_in.p, bytes, hipMemcpyHostToDevice, c->s_in));
    }
    if (!zin && in_size) {
        LR_HIP(hipEventRecord(sl.ev_in, c->s_in));
        LR_HIP(hipStreamWaitEvent(ctx().stream, sl.ev_in, 0));
    }
    unsigned long cap = (unsigned long)(sl.d_out.cap / out_size);
    long n_out = lrhip_chain_execute_device(c, zin ? zin : sl.d_in.p, n_in, sl.d_out.p, cap);
    if (n_out < 0) return n_out;
    LR_HIP(hipEventRecord(sl.ev_done, ctx().stream));
    LR_HIP(hipStreamWaitEvent(c->s_out, sl.ev_done, 0));
    if (n_out) LR_HIP(hipMemcpyAsync(sl.h_out.p, sl.d_out.p, (size_t)n_out * out_size, hipMemcpyDeviceToHost, c->s_out));
    LR_HIP(hipEventRecord(sl.ev_out, c->s_out));
    sl.n_out = n_out;
    sl.used = true;
    c->head = (c->head + 1) % c->ring.size();
    c->inflight++;
    return n_out;
}

// File-fed chains (radio/blocks/sources/iqfile.lua:82-96 without the interpreter in the data path): the raw records of a regular file go from the page cache
// straight into the pinned input of the next ring slot - positional reads split over the library's copy threads - and the slot is submitted.
long lrhip_chain_submit_fd(lrhip_chain_t *c, int fd, unsigned long long offset, unsigned long max_in)
{
    if (!c) return set_error("null chain");
    if (chain_refuse_source(c, "lrhip_chain_submit_fd")) return -1;
    if (c->ring.empty()) return set_error("chain has no ring: call lrhip_chain_set_ring first");
    if (c->inflight == c->ring.size()) { set_error("ring full: collect a chunk first (%u in flight)", c->inflight); return -3; }
    if (c->fill) return set_error("chain has %lu pushed samples pending: flush before mixing submit() with push()", c->fill);
    struct stat st;
    if (fstat(fd, &st) != 0) return set_error("fstat(%d): %s", fd, strerror(errno));
    if (!S_ISREG(st.st_mode)) { set_error("lrhip_chain_submit_fd: descriptor %d is not a regular file (read() into lrhip_chain_ring_input() instead)", fd); return -4; }
    const int in_size = c->ops.front().stage->in_size;
    unsigned long long avail = (unsigned long long)st.st_size > offset ? ((unsigned long long)st.st_size - offset) / (unsigned)in_size : 0;
    unsigned long n = max_in < c->ring_chunk ? max_in : c->ring_chunk;
    if (avail < n) n = (unsigned long)avail;
    if (!n) return 0;                                        // end of the file (or less than one whole record left)
    lrhip_chain::Slot &sl = *c->ring[c->head];
    const int err = host_pread(sl.h_in.p, fd, (long long)offset, (size_t)n * in_size);
    if (err) return set_error("pread(%d): %s", fd, strerror(err));
    const long rc = chain_submit(c, sl.h_in.p, n, false);
    return rc < 0 ? rc : (long)n;
}

void *lrhip_chain_ring_input(lrhip_chain_t *c)
{
    if (!c) { set_error("null chain"); return nullptr; }
    if (chain_refuse_source(c, "lrhip_chain_ring_input")) return nullptr;
    if (c->ring.empty()) { set_error("chain has no ring: call lrhip_chain_set_ring first"); return nullptr; }
    if (c->inflight == c->ring.size()) { set_error("ring full: collect a chunk first (%u in flight)", c->inflight); return nullptr; }
    return c->ring[c->head]->h_in.p;
}

long lrhip_chain_collect(lrhip_chain_t *c, void *out_host, unsigned long out_capacity)
{
    if (!c) return set_error("null chain");
    if (!c->inflight) { set_error("nothing in flight"); return -2; }
    unsigned tail = (c->head + (unsigned)c->ring.size() - c->inflight) % c->ring.size();
    lrhip_chain::Slot &sl = *c->ring[tail];
    if ((unsigned long)sl.n_out > out_capacity) return set_error("output capacity %lu < %ld", out_capacity, sl.n_out);
    if (sl.n_out && !out_host) return set_error("null output buffer");
    LR_HIP(hipEventSynchronize(sl.ev_out));
    if (sl.n_out) host_copy(out_host, sl.h_out.p, (size_t)sl.n_out * c->ops.back().stage->out_size);
    c->inflight--;
    return sl.n_out;
}

// ---- chunk coalescing on the ring ---------------------------------------------------------------------------------
// launch the head slot with its `fill` accumulated samples (they already sit in the slot's pinned input)
static long push_launch(lrhip_chain_t *c)
{
    unsigned long n = c->fill;
    c->fill = 0;                        // lrhip_chain_submit() refuses to run while pushed samples are pending
    long rc = lrhip_chain_submit(c, c->ring[c->head]->h_in.p, n);
    if (rc < 0) c->fill = n;            // nothing was launched: the samples are still in the slot, the caller may collect and retry
    else c->fill_t0 = 0.0;
    return rc;
}
static double monotonic_seconds()
{
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec;
}

int lrhip_chain_set_latency(lrhip_chain_t *c, double max_seconds)
{
    if (!c) return set_error("null chain");
    if (!(max_seconds >= 0.0)) return set_error("latency bound must be >= 0 (0 = batches run when full)");
    c->max_latency = max_seconds;
    return 0;
}
// copy the oldest slot's output out (waiting for it when `wait`); returns samples copied, -2 when it is not finished yet
static long push_collect(lrhip_chain_t *c, char *out, unsigned long cap, bool wait)
{
    unsigned tail = (c->head + (unsigned)c->ring.size() - c->inflight) % c->ring.size();
    lrhip_chain::Slot &sl = *c->ring[tail];
    if (!wait) {
        hipError_t q = hipEventQuery(sl.ev_out);
        if (q == hipErrorNotReady) return -2;
        if (q != hipSuccess) return set_error("hipEventQuery failed: %s", hipGetErrorString(q));
    }
    return lrhip_chain_collect(c, out, cap);
}

// the tail of push() and all of poll(): run the partial batch if its oldest sample has waited out the latency bound (and then wait for it: a live
// flow graph is far from the GPU's throughput, so the wait costs a launch, not the stream rate), then hand out whatever has finished, in stream order
static long push_drain(lrhip_chain_t *c, char *dst, unsigned long out_capacity, long total)
{
    const int out_size = c->ops.back().stage->out_size;
    if (c->fill && c->max_latency > 0.0 && monotonic_seconds() - c->fill_t0 >= c->max_latency) {
        if (c->inflight == c->ring.size()) {
            long got = push_collect(c, dst + (size_t)total * out_size, out_capacity - (unsigned long)total, true);
            if (got < 0) return got;
            total += got;
        }
        long rc = push_launch(c);
        if (rc < 0) return rc;
        while (c->inflight) {
            long got = push_collect(c, dst + (size_t)total * out_size, out_capacity - (unsigned long)total, true);
            if (got < 0) return got;
            total += got;
        }
    }
    while (c->inflight) {                                    // whatever has finished meanwhile, without waiting
        long got = push_collect(c, dst + (size_t)total * out_size, out_capacity - (unsigned long)total, false);
        if (got == -2) break;
        if (got < 0) return got;
        total += got;
    }
    return total;
}

unsigned long lrhip_chain_push_bound(const lrhip_chain_t *c, unsigned long n_in)
{
    if (!c || c->ring.empty()) return 0;
    // every slot in flight, the head slot, and the slots this call itself can fill
    return (unsigned long)(c->ring.size() + 1 + n_in / c->ring_chunk + 1) * c->ring_out_cap;
}

long lrhip_chain_push(lrhip_chain_t *c, const void *in_host, unsigned long n_in, void *out_host, unsigned long out_capacity)
{
    if (!c) return set_error("null chain");
    if (chain_refuse_source(c, "lrhip_chain_push")) return -1;
    if (c->ring.empty()) return set_error("chain has no ring: call lrhip_chain_set_ring first");
    if (n_in && !in_host) return set_error("null input buffer");
    if (out_capacity < lrhip_chain_push_bound(c, n_in)) return set_error("output capacity %lu < lrhip_chain_push_bound() = %lu", out_capacity, lrhip_chain_push_bound(c, n_in));
    const int in_size = c->ops.front().stage->in_size, out_size = c->ops.back().stage->out_size;
    const char *src = (const char *)in_host;
    char *dst = (char *)out_host;
    long total = 0;
    while (n_in) {
        if (c->inflight == c->ring.size()) {                 // the head slot is still in flight: its turn to be collected
            long got = push_collect(c, dst + (size_t)total * out_size, out_capacity - (unsigned long)total, true);
            if (got < 0) return got;
            total += got;
        }
        unsigned long take = c->ring_chunk - c->fill;
        if (take > n_in) take = n_in;
        host_copy((char *)c->ring[c->head]->h_in.p + (size_t)c->fill * in_size, src, (size_t)take * in_size);
        if (!c->fill && c->max_latency > 0.0) c->fill_t0 = monotonic_seconds();
        c->fill += take; src += (size_t)take * in_size; n_in -= take;
        if (c->fill == c->ring_chunk) {
            long rc = push_launch(c);
            if (rc < 0) return rc;
        }
    }
    return push_drain(c, dst, out_capacity, total);
}

// The wall-clock side of the latency bound.  push() can only look at the clock when it is called; a live source that STALLS (an SDR that
// drops out, a squelched upstream block, a paused network source) would leave the partial batch on the device side of the host forever,
// where the reference streams every chunk through as it arrives (radio/core/block.lua:575-602).  The host calls poll() whenever its wait for
// input timed out (lua/radio/composites/devicechain.lua: DeviceChainBlock:run polls its input descriptors for lrhip_chain_poll_due()
// seconds instead of forever): a partial batch whose oldest sample has waited max_seconds is launched and its output returned from this
// call, like the same check at the end of push(); finished batches are handed out either way.  Nothing due: returns 0 at once.
long lrhip_chain_poll(lrhip_chain_t *c, void *out_host, unsigned long out_capacity)
{
    if (!c) return set_error("null chain");
    if (c->ring.empty()) return 0;
    if (out_capacity < lrhip_chain_push_bound(c, 0)) return set_error("output capacity %lu < lrhip_chain_push_bound() = %lu", out_capacity, lrhip_chain_push_bound(c, 0));
    return push_drain(c, (char *)out_host, out_capacity, 0);
}

double lrhip_chain_poll_due(const lrhip_chain_t *c)
{
    if (!c) { set_error("null chain"); return -1.0; }
    if (!(c->max_latency > 0.0)) return -1.0;                             // batches only run when full: wait for input forever
    if (!c->fill) {
        // nothing accumulating, but a batch launched by the last push() may still be in flight (batch == chunk, then the source stalls): its output
        // is handed out by the next poll(), so the wait for input stays bounded by the latency bound until the ring has drained
        return c->inflight ? c->max_latency : -1.0;
    }
    const double left = c->fill_t0 + c->max_latency - monotonic_seconds();
    return left > 0.0 ? left : 0.0;
}

long lrhip_chain_flush(lrhip_chain_t *c, void *out_host, unsigned long out_capacity)
{
    if (!c) return set_error("null chain");
    if (c->ring.empty()) return 0;                           // nothing is ever pending without a ring
    if (out_capacity < lrhip_chain_push_bound(c, 0)) return set_error("output capacity %lu < lrhip_chain_push_bound() = %lu", out_capacity, lrhip_chain_push_bound(c, 0));
    const int out_size = c->ops.back().stage->out_size;
    char *dst = (char *)out_host;
    long total = 0;
    if (c->fill) {
        if (c->inflight == c->ring.size()) {
            long got = push_collect(c, dst, out_capacity, true);
            if (got < 0) return got;
            total += got;
        }
        long rc = push_launch(c);
        if (rc < 0) return rc;
    }
    while (c->inflight) {
        long got = push_collect(c, dst + (size_t)total * out_size, out_capacity - (unsigned long)total, true);
        if (got < 0) return got;
        total += got;
    }
    return total;
}

// ---- memory helpers ----------------------------------------------------------------------------------------
void *lrhip_malloc(unsigned long bytes)
{
    if (ensure_init()) return nullptr;
    void *p = nullptr;
    LR_HIP_NULL(hipMalloc(&p, bytes ? bytes : 4));
    return p;
}
void lrhip_free(void *p)
{
    if (p) (void)hipFree(p);
}
int lrhip_memcpy_h2d(void *dst, const void *src, unsigned long bytes)
{
    if (ensure_init()) return -1;
    LR_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ctx().stream));
    LR_HIP(hipStreamSynchronize(ctx().stream));
    return 0;
}
int lrhip_memcpy_d2h(void *dst, const void *src, unsigned long bytes)
{
    if (ensure_init()) return -1;
    LR_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx().stream));
    LR_HIP(hipStreamSynchronize(ctx().stream));
    return 0;
}
int lrhip_memcpy_d2d(void *dst, const void *src, unsigned long bytes)
{
    if (ensure_init()) return -1;
    if (bytes) LR_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, ctx().stream));
    return 0;
}
void *lrhip_host_alloc(unsigned long bytes)
{
    if (ensure_init()) return nullptr;
    void *p = nullptr;
    LR_HIP_NULL(hipHostMalloc(&p, bytes ? bytes : 4, hipHostMallocDefault));
    return p;
}
void lrhip_host_free(void *p)
{
    if (p) (void)hipHostFree(p);
}
int lrhip_host_register(void *ptr, unsigned long bytes)
{
    if (!ptr || !bytes) return set_error("host_register: null range");
    if (ensure_init()) return -1;
    HostRanges &h = host_ranges();
    {
        std::lock_guard<std::mutex> lk(h.m);
        if (h.pid != (long)getpid()) { h.r.clear(); h.dev.clear(); h.pid = (long)getpid(); }
        for (auto &e : h.r)
            if (e.first == (const char *)ptr) {
                if (e.second == bytes) return 0;
                return set_error("host_register: %p is already registered with another size", ptr);
            }
    }
    LR_HIP(hipHostRegister(ptr, bytes, hipHostRegisterDefault));
    void *d = nullptr;
    if (hipHostGetDevicePointer(&d, ptr, 0) != hipSuccess) { (void)hipGetLastError(); d = nullptr; }      // not mapped: the staged path only
    std::lock_guard<std::mutex> lk(h.m);
    h.r.emplace_back((const char *)ptr, (size_t)bytes);
    h.dev.push_back((char *)d);
    return 0;
}
int lrhip_host_unregister(void *ptr)
{
    if (!ptr) return 0;
    HostRanges &h = host_ranges();
    {
        std::lock_guard<std::mutex> lk(h.m);
        auto it = h.r.begin();
        for (; it != h.r.end(); ++it)
            if (it->first == (const char *)ptr) break;
        if (it == h.r.end()) return set_error("host_unregister: %p is not registered", ptr);
        if (h.dev.size() == h.r.size()) h.dev.erase(h.dev.begin() + (it - h.r.begin()));
        h.r.erase(it);
    }
    // nothing of this range may still be in flight: every host-pointer entry point has synchronised before it returned
    LR_HIP(hipHostUnregister(ptr));
    return 0;
}

// ---- timers ----------------------------------------------------------------------------------------------------
struct lrhip_timer {
    hipEvent_t a, b;
};
lrhip_timer_t *lrhip_timer_create(void)
{
    if (ensure_init()) return nullptr;
    lrhip_timer *t = new (std::nothrow) lrhip_timer();
    if (!t) { set_error("out of memory"); return nullptr; }
    if (hipEventCreate(&t->a) != hipSuccess || hipEventCreate(&t->b) != hipSuccess) {
        set_error("hipEventCreate failed");
        delete t;
        return nullptr;
    }
    return t;
}
void lrhip_timer_destroy(lrhip_timer_t *t)
{
    if (!t) return;
    (void)hipEventDestroy(t->a);
    (void)hipEventDestroy(t->b);
    delete t;
}
int lrhip_timer_start(lrhip_timer_t *t)
{
    if (!t) return set_error("null timer");
    LR_HIP(hipEventRecord(t->a, ctx().stream));
    return 0;
}
int lrhip_timer_stop(lrhip_timer_t *t)
{
    if (!t) return set_error("null timer");
    LR_HIP(hipEventRecord(t->b, ctx().stream));
    return 0;
}
double lrhip_timer_elapsed_ms(lrhip_timer_t *t)
{
    if (!t) return (double)set_error("null timer");
    if (hipEventSynchronize(t->b) != hipSuccess) return (double)set_error("hipEventSynchronize failed");
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, t->a, t->b) != hipSuccess) return (double)set_error("hipEventElapsedTime failed");
    return (double)ms;
}

// ---- time-axis sharding ---------------------------------------------------------------------------------------------
int lrhip_stage_seek(lrhip_stage_t *q, unsigned long long n0)
{
    if (!q) return set_error("null stage");
    unsigned long long out = 0;
    return q->seek(n0, &out);
}

int lrhip_chain_seek(lrhip_chain_t *c, unsigned long long n0)
{
    if (!c) return set_error("null chain");
    if (c->inflight || c->fill) return set_error("chain seek: chunks still in flight or pushed and not flushed");
    if (ctx().ready) LR_HIP(hipStreamSynchronize(ctx().stream));
    c->discard_in = 0;
    unsigned long long n = n0;
    for (auto &o : c->ops) {
        unsigned long long nn = 0;
        if (o.stage->seek(n, &nn)) return -1;
        n = nn;
    }
    return 0;
}

long lrhip_chain_halo(const lrhip_chain_t *c)
{
    if (!c) return set_error("null chain");
    // H = sum_k memory_k * (input samples of the chain per input sample of stage k), rounded up
    long double scale = 1.0L, h = 0.0L;
    for (auto &o : c->ops) {
        const long m = o.stage->memory();
        if (m < 0) return set_error("chain halo: stage '%s' has unbounded memory - this chain cannot be sharded in time", o.stage->kind());
        h += (long double)m * scale;
        unsigned long num = 1, den = 1;
        o.stage->rate(&num, &den);
        scale = scale * (long double)num / (long double)den;
    }
    return (long)ceill(h);
}

unsigned long lrhip_chain_shard_align(const lrhip_chain_t *c)
{
    if (!c) return 0;
    // a chain-input count `a` reaches stage k as a * den / num samples (num / den = product of the rates before it); the smallest a that is
    // a multiple of align_k there is align_k * num / gcd(align_k * num, den); the chain's alignment is the lcm over its stages
    auto gcd = [](unsigned long long x, unsigned long long y) { while (y) { unsigned long long t = x % y; x = y; y = t; } return x; };
    unsigned long long num = 1, den = 1, l = 1;
    for (auto &o : c->ops) {
        unsigned long long a = (unsigned long long)o.stage->align() * num;
        a /= gcd(a, den);
        l = l / gcd(l, a) * a;
        unsigned long rn = 1, rd = 1;
        o.stage->rate(&rn, &rd);
        num *= rn; den *= rd;
        unsigned long long g = gcd(num, den);
        num /= g; den /= g;
    }
    return (unsigned long)l;
}

int lrhip_chain_start_at(lrhip_chain_t *c, unsigned long long first_sample, unsigned long long *seek_sample)
{
    if (!c) return set_error("null chain");
    const long halo = lrhip_chain_halo(c);
    if (halo < 0) return -1;
    const unsigned long long align = lrhip_chain_shard_align(c);
    unsigned long long s = first_sample > (unsigned long long)halo ? first_sample - (unsigned long long)halo : 0ULL;
    s -= s % (align ? align : 1ULL);
    if (lrhip_chain_seek(c, s)) return -1;
    c->discard_in = first_sample - s;
    if (seek_sample) *seek_sample = s;
    return 0;
}

// ---- interprocess memory / events / peer copies --------------------------------------------------------------------
struct lrhip_ipc_event {
    hipEvent_t ev = nullptr;
};
static hipStream_t copy_stream()
{
    static hipStream_t s = nullptr;
    static long pid = 0;
    if (!s || pid != (long)getpid()) {
        if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) s = nullptr;
        pid = (long)getpid();
    }
    return s;
}

int lrhip_ipc_export(const void *dev_ptr, void *handle_out)
{
    static_assert(sizeof(hipIpcMemHandle_t) <= LRHIP_IPC_HANDLE_BYTES && sizeof(hipIpcEventHandle_t) <= LRHIP_IPC_HANDLE_BYTES, "handle size");
    if (!dev_ptr || !handle_out) return set_error("ipc_export: null argument");
    if (ensure_init()) return -1;
    hipIpcMemHandle_t h;
    LR_HIP(hipIpcGetMemHandle(&h, const_cast<void *>(dev_ptr)));
    memset(handle_out, 0, LRHIP_IPC_HANDLE_BYTES);
    memcpy(handle_out, &h, sizeof(h));
    return 0;
}

void *lrhip_ipc_open(const void *handle)
{
    if (!handle) { set_error("ipc_open: null handle"); return nullptr; }
    if (ensure_init()) return nullptr;
    hipIpcMemHandle_t h;
    memcpy(&h, handle, sizeof(h));
    void *p = nullptr;
    LR_HIP_NULL(hipIpcOpenMemHandle(&p, h, hipIpcMemLazyEnablePeerAccess));
    return p;
}

int lrhip_ipc_close(void *dev_ptr)
{
    if (!dev_ptr) return 0;
    LR_HIP(hipIpcCloseMemHandle(dev_ptr));
    return 0;
}

lrhip_ipc_event_t *lrhip_ipc_event_create(void *handle_out)
{
    if (!handle_out) { set_error("ipc_event_create: null handle buffer"); return nullptr; }
    if (ensure_init()) return nullptr;
    std::unique_ptr<lrhip_ipc_event> e(new (std::nothrow) lrhip_ipc_event());
    if (!e) { set_error("out of memory"); return nullptr; }
    LR_HIP_NULL(hipEventCreateWithFlags(&e->ev, hipEventDisableTiming | hipEventInterprocess));
    hipIpcEventHandle_t h;
    if (hipIpcGetEventHandle(&h, e->ev) != hipSuccess) {
        (void)hipEventDestroy(e->ev);
        set_error("hipIpcGetEventHandle failed");
        return nullptr;
    }
    memset(handle_out, 0, LRHIP_IPC_HANDLE_BYTES);
    memcpy(handle_out, &h, sizeof(h));
    return e.release();
}

lrhip_ipc_event_t *lrhip_ipc_event_open(const void *handle)
{
    if (!handle) { set_error("ipc_event_open: null handle"); return nullptr; }
    if (ensure_init()) return nullptr;
    std::unique_ptr<lrhip_ipc_event> e(new (std::nothrow) lrhip_ipc_event());
    if (!e) { set_error("out of memory"); return nullptr; }
    hipIpcEventHandle_t h;
    memcpy(&h, handle, sizeof(h));
    LR_HIP_NULL(hipIpcOpenEventHandle(&e->ev, h));
    return e.release();
}

void lrhip_ipc_event_destroy(lrhip_ipc_event_t *e)
{
    if (!e) return;
    if (e->ev) (void)hipEventDestroy(e->ev);
    delete e;
}

int lrhip_ipc_event_record(lrhip_ipc_event_t *e, int on_copy_stream)
{
    if (!e) return set_error("null event");
    hipStream_t s = on_copy_stream ? copy_stream() : ctx().stream;
    if (!s) return set_error("no stream");
    LR_HIP(hipEventRecord(e->ev, s));
    return 0;
}

int lrhip_ipc_event_wait(lrhip_ipc_event_t *e, int on_copy_stream)
{
    if (!e) return set_error("null event");
    hipStream_t s = on_copy_stream ? copy_stream() : ctx().stream;
    if (!s) return set_error("no stream");
    LR_HIP(hipStreamWaitEvent(s, e->ev, 0));
    return 0;
}

int lrhip_ipc_event_query(lrhip_ipc_event_t *e)
{
    if (!e) return set_error("null event");
    hipError_t r = hipEventQuery(e->ev);
    if (r == hipSuccess) return 1;
    if (r == hipErrorNotReady) { (void)hipGetLastError(); return 0; }
    return set_error("hipEventQuery failed: %s", hipGetErrorString(r));
}

int lrhip_ipc_event_synchronize(lrhip_ipc_event_t *e)
{
    if (!e) return set_error("null event");
    LR_HIP(hipEventSynchronize(e->ev));
    return 0;
}

int lrhip_peer_copy(void *dst, int dst_device, const void *src, int src_device, unsigned long bytes)
{
    if (ensure_init()) return -1;
    if (!bytes) return 0;
    if (!dst || !src) return set_error("peer_copy: null pointer");
    hipStream_t s = copy_stream();
    if (!s) return set_error("peer_copy: no copy stream");
    if (dst_device != src_device) {
        int can = 0;
        LR_HIP(hipDeviceCanAccessPeer(&can, src_device, dst_device));
        if (!can) return set_error("peer_copy: device %d cannot reach device %d", src_device, dst_device);
        LR_HIP(hipMemcpyPeerAsync(dst, dst_device, src, src_device, bytes, s));
    } else {
        LR_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, s));
    }
    return 0;
}

int lrhip_copy_stream_synchronize(void)
{
    hipStream_t s = copy_stream();
    if (!s) return set_error("no copy stream");
    LR_HIP(hipStreamSynchronize(s));
    return 0;
}

}  // extern "C"
