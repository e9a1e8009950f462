// fir_tables.h - every device table of the FIR stage, built on the host in double: one function per table, each returning the floats that fir_build()
// (stage_fir.h) uploads.  Host-only, plain C++17, no HIP calls; include it after the kernel headers (the layouts: FFT_TABLE_*, F4K_TAB_*, F64_TAB_*,
// df_table_elems, fir_taps_len).  All spectra come from taps_spectrum(), all twiddle sections from fill_twiddles(); tools/host_fir_tables_check.hip holds
// every section to its definition (an independent DFT, the kernels' documented index maps) on the CPU.
#pragma once
#include <cmath>
#include <vector>
#include "fir_form.h"

constexpr double FIR_PI2 = 6.283185307179586476925286766559;
inline void put_cis(float *t, size_t o, double a) { t[2 * o] = (float)std::cos(a); t[2 * o + 1] = (float)std::sin(a); }
// t[o + r cols + c] = W_N^(r c)
inline void fill_twiddles(float *t, size_t o, int rows, int cols, int N)
{
    for (int r = 0; r < rows; r++)
        for (int c = 0; c < cols; c++) put_cis(t, o + (size_t)r * cols + c, -FIR_PI2 * (double)((r * c) % N) / N);
}
// H[k] = (1 / N) sum over m0 <= m < m1 of h[m] W_N^(k (m - m0)), k < N: the response of one partition of the taps, its delay m0 NOT folded in (the kernels
// apply it), the 1 / N of the inverse transform (spectrum_utils.lua:335-338) folded in.  The sum ascends in m, in double
inline void taps_spectrum(const float *taps, int taps_complex, unsigned m0, unsigned m1, int N, std::vector<double> &Hr, std::vector<double> &Hi)
{
    std::vector<double> cs((size_t)N), sn((size_t)N);
    for (int j = 0; j < N; j++) { const double a = -FIR_PI2 * (double)j / N; cs[j] = std::cos(a); sn[j] = std::sin(a); }
    Hr.assign((size_t)N, 0.0); Hi.assign((size_t)N, 0.0);
    for (int k = 0; k < N; k++) {
        double sr = 0, si = 0;
        for (unsigned m = m0; m < m1; m++) {
            const int a = (int)(((long)k * (m - m0)) % N);
            const double hr = taps_complex ? taps[2 * m] : taps[m], hi = taps_complex ? taps[2 * m + 1] : 0.0;
            sr += hr * cs[a] - hi * sn[a];
            si += hr * sn[a] + hi * cs[a];
        }
        Hr[k] = sr / N; Hi[k] = si / N;
    }
}
// H in the (register, lane) order behind the second round of the 1024-point transform: slot (4 j + k3) 64 + lane holds bin w + stride k',
// k' = k1 + 16 (4 j + q) + 256 k3 with (q, k1) = (lane & 3, lane >> 2); swapped - fir_fft_kernel's numbering with the register <-> row transposes
// (LRHIP_FFT_E2_SWAP): q = the lane's row of 16, k1 = its position in the row
inline void put_h_round2(float *t, size_t o, const std::vector<double> &Hr, const std::vector<double> &Hi, int w, int stride, bool swapped)
{
    for (int j = 0; j < 4; j++)
        for (int k3 = 0; k3 < 4; k3++)
            for (int lane = 0; lane < 64; lane++) {
                const int q = swapped ? lane >> 4 : lane & 3, k1 = swapped ? lane & 15 : lane >> 2, k = w + stride * (k1 + 16 * (4 * j + q) + 256 * k3);
                const size_t s = o + (size_t)(4 * j + k3) * 64 + lane;
                t[2 * s] = (float)Hr[k]; t[2 * s + 1] = (float)Hi[k];
            }
}
// H in the order of the 64 x 64 form: H[r][l] = H(64 k1(r) + l), k1(r) = f64_index(r); with o_sym >= 0 also the half rows Hsym[k1][l <= 32] = H(64 k1 + l)
inline void put_h_64x64(float *t, size_t o, long o_sym, const std::vector<double> &Hr, const std::vector<double> &Hi)
{
    for (int r = 0; r < 64; r++)
        for (int l = 0; l < 64; l++) {
            const int k = 64 * f64_index(r) + l;
            const auto put = [&](size_t s) { t[2 * s] = (float)Hr[k]; t[2 * s + 1] = (float)Hi[k]; };
            put(o + (size_t)r * 64 + l);
            if (o_sym >= 0 && l <= 32) put((size_t)o_sym + (size_t)f64_index(r) * F64_HSYM_ROW + l);
        }
}
// the taps reversed (firfilter.lua:234-238): what every kernel of the direct forms reads
inline std::vector<float> fir_reversed_taps(const float *taps, unsigned ntaps, int taps_complex)
{
    const int ts = taps_complex ? 2 : 1;
    std::vector<float> rev((size_t)ntaps * ts);
    for (unsigned i = 0; i < ntaps; i++)
        for (int c = 0; c < ts; c++) rev[(size_t)i * ts + c] = taps[(size_t)(ntaps - 1 - i) * ts + c];
    return rev;
}
// the zero-padded Toeplitz tap array of real taps at decimation D (kernels_fir.h)
inline std::vector<float> fir_toeplitz_taps(const std::vector<float> &rev, int M, int D, int ksteps) { std::vector<float> tab; fir_mfma_build_taps(rev.data(), M, D, ksteps, tab); return tab; }
// complex taps as two real filters of 2 M taps at decimation 2 D over the float stream (re | im): taps'_re = interleave(hr_rev, -hi_rev), taps'_im = interleave(hi_rev, hr_rev)
inline std::vector<float> fir_toeplitz_cc_taps(const std::vector<float> &rev, int M, int D, int ksteps)
{
    std::vector<float> tre((size_t)2 * M), tim((size_t)2 * M);
    for (int j = 0; j < M; j++) {
        const float hr = rev[2 * j], hi = rev[2 * j + 1];
        tre[2 * j] = hr; tre[2 * j + 1] = -hi;
        tim[2 * j] = hi; tim[2 * j + 1] = hr;
    }
    std::vector<float> tab = fir_toeplitz_taps(tre, 2 * M, 2 * D, ksteps), aim = fir_toeplitz_taps(tim, 2 * M, 2 * D, ksteps);
    tab.insert(tab.end(), aim.begin(), aim.end());
    return tab;
}
// the short complex-taps window kernel's table (FirForm::WinShortC): (re, im, -im, re) per reversed tap
inline std::vector<float> fir_ctaps4_table(const std::vector<float> &rev, int M)
{
    std::vector<float> t4((size_t)4 * M);
    for (int j = 0; j < M; j++) {
        const float hr = rev[2 * j], hi = rev[2 * j + 1];
        t4[4 * j] = hr; t4[4 * j + 1] = hi; t4[4 * j + 2] = -hi; t4[4 * j + 3] = hr;
    }
    return t4;
}
// the 1024-point kernels (kernels_firfft.h, kernels_firpols.h), one set per partition of <= FIR_FFT_PART taps: tw1[k1][t] | Hperm[4j+k3][lane] | tw2[k2][t2] | H swapped
inline std::vector<float> fir_fft1024_tables(const float *taps, unsigned ntaps, int taps_complex)
{
    const int nparts = ((int)ntaps + FIR_FFT_PART - 1) / FIR_FFT_PART;
    std::vector<float> tab((size_t)nparts * FFT_TABLE_ELEMS * 2);
    std::vector<double> Hr, Hi;
    for (int part = 0; part < nparts; part++) {
        float *tp = tab.data() + (size_t)part * FFT_TABLE_ELEMS * 2;
        const unsigned m0 = (unsigned)part * FIR_FFT_PART;
        taps_spectrum(taps, taps_complex, m0, std::min<unsigned>(ntaps, m0 + FIR_FFT_PART), FFTN, Hr, Hi);
        fill_twiddles(tp, 0, 16, 64, FFTN);
        put_h_round2(tp, 16 * 64, Hr, Hi, 0, 1, false);
        fill_twiddles(tp, 2 * 16 * 64, 16, 4, 64);
#if LRHIP_FFT_E2_SWAP
        put_h_round2(tp, FFT_TABLE_HSW, Hr, Hi, 0, 1, true);
#endif
    }
    return tab;
}
// the 4096-point workgroup-per-block kernel (kernels_firfft4k.h), from the 4096-point spectrum of all taps:
// tw1 | tw2 | c[w][i] = W_64^(i w) | b[w][t] = W_4096^(t w) | H[w][16 x 64] of the bins w + 4 k'
inline std::vector<float> fir_fft4k_tables(const std::vector<double> &Hr, const std::vector<double> &Hi)
{
    std::vector<float> t4((size_t)F4K_TABLE_ELEMS * 2);
    fill_twiddles(t4.data(), 0, 16, 64, FFTN);
    fill_twiddles(t4.data(), 16 * 64, 16, 4, 64);
    fill_twiddles(t4.data(), 16 * 64 + 64, 4, 16, 64);
    fill_twiddles(t4.data(), F4K_TAB_B, 4, 64, F4K_N);
    for (int w = 0; w < 4; w++) put_h_round2(t4.data(), (size_t)F4K_TAB_H + (size_t)w * 1024, Hr, Hi, w, 4, false);
    return t4;
}
// the 64 x 64 form (kernels_firfft64.h), from the same spectrum: C[c][t] = W_1024^(t c) | D[d][t] = W_4096^(t d) | H[r][l] | Hsym[k1][l <= 32]
inline void fill_f64_twiddles(float *t, size_t o) { fill_twiddles(t, o, 16, 64, FFTN); fill_twiddles(t, o + F64_TAB_D, 4, 64, F4K_N); }
inline std::vector<float> fir_fft64_tables(const std::vector<double> &Hr, const std::vector<double> &Hi)
{
    std::vector<float> t6((size_t)F64_TABLE_ELEMS * 2, 0.f);
    fill_f64_twiddles(t6.data(), 0);
    put_h_64x64(t6.data(), F64_TAB_H, F64_TAB_HSYM, Hr, Hi);
    return t6;
}
// the long 64 x 64 form at an overlap of 2 048: np = 1 is all taps; above, partitions of 2 048 taps (the last one up to 2 049), two per table set
// (H | H1, Hsym for the first partition only) and a second set for the second launch of partitions 2 and 3
inline std::vector<float> fir_fft64_long_tables(const float *taps, unsigned ntaps, int taps_complex, int np)
{
    const int nsets = np > 2 ? 2 : 1;
    std::vector<float> t6((size_t)F64_TABLE_ELEMS2 * 2 * nsets, 0.f);
    for (int set = 0; set < nsets; set++) fill_f64_twiddles(t6.data(), (size_t)set * F64_TABLE_ELEMS2);
    std::vector<double> Hr, Hi;
    for (int part = 0; part < np; part++) {
        const unsigned m0 = np == 1 ? 0 : part * 2048u, m1 = np == 1 || part + 1 == np ? ntaps : (part + 1) * 2048u;
        taps_spectrum(taps, taps_complex, m0, m1, F4K_N, Hr, Hi);
        put_h_64x64(t6.data(), (size_t)(part / 2) * F64_TABLE_ELEMS2 + (part & 1 ? F64_TAB_H1 : F64_TAB_H), part == 0 ? F64_TAB_HSYM : -1, Hr, Hi);
    }
    return t6;
}
// Tables of fir_decfft_kernel (layout: df_table_elems): 256-point twiddles, the D polyphase branch responses G_rho (1/256 of the
// inverse transform folded in) in the lane order of the forward batches, and the output phasors e^{j w D k}.  All in double.
// Window position j = D mm + rho of a block is input x[first + D m - r] with r = D - 1 - rho, so branch rho uses g_r[q] = g[D q + r],
// g[i] = h[i] e^{-j w i}.
inline std::vector<float> fir_decfft_tables(const float *taps, int M, int taps_complex, int D, double omega)
{
    const int A = D / 4, C = D % 4;
    std::vector<float> out((size_t)df_table_elems(D) * 2, 0.f);
    float *tw = out.data(), *Gf = tw + 2 * 256, *Gl = Gf + 2 * (size_t)A * 1024, *rt = Gl + 2 * (size_t)C * 256;
    fill_twiddles(tw, 0, 16, 16, DF_N);
    long double turns = (long double)omega / (2.0L * 3.14159265358979323846264338327950288L);
    turns -= floorl(turns);
    std::vector<double> gr((size_t)M), gi((size_t)M);
    for (int i = 0; i < M; i++) {
        long double f = turns * (long double)i;
        f -= floorl(f);
        double a = -FIR_PI2 * (double)f, c = std::cos(a), sn = std::sin(a);
        double hr = taps_complex ? taps[2 * i] : taps[i], hi = taps_complex ? taps[2 * i + 1] : 0.0;
        gr[i] = hr * c - hi * sn;
        gi[i] = hr * sn + hi * c;
    }
    std::vector<double> Gr(DF_N), Gi(DF_N);
    for (int rho = 0; rho < D; rho++) {
        const int r = D - 1 - rho;
        for (int k = 0; k < DF_N; k++) {
            double sr = 0, si = 0;
            for (int qq = 0; D * qq + r < M; qq++) {
                double a = -FIR_PI2 * (double)((qq * k) % DF_N) / DF_N, c = std::cos(a), sn = std::sin(a);
                sr += gr[D * qq + r] * c - gi[D * qq + r] * sn;
                si += gr[D * qq + r] * sn + gi[D * qq + r] * c;
            }
            Gr[k] = sr / DF_N;
            Gi[k] = si / DF_N;
        }
        for (int k2 = 0; k2 < 16; k2++)
            for (int k1 = 0; k1 < 16; k1++) {
                const int k = k1 + 16 * k2;
                float *dst = rho < 4 * A ? Gf + 2 * ((size_t)(rho / 4) * 1024 + k2 * 64 + 16 * (rho % 4) + k1)
                                         : Gl + 2 * ((size_t)(rho - 4 * A) * 256 + k2 * 16 + k1);
                dst[0] = (float)Gr[k];
                dst[1] = (float)Gi[k];
            }
    }
    for (int w = 0; w < DF_N; w++) {
        long double f = turns * (long double)D * (long double)w;
        f -= floorl(f);
        double a = FIR_PI2 * (double)f;
        rt[2 * w] = (float)std::cos(a);
        rt[2 * w + 1] = (float)std::sin(a);
    }
    return out;
}
