// kernels_pfbsynth.h - K-channel synthesis filterbank in its polyphase + FFT form: the inverse of kernels_pfb.h.  K a power of two in [8, 4096],
// frames of K channel values in, D = K / R samples out per frame (R = 1, 2 or 4: the oversampling of the analysis bank that made the frames).
//
// The block is K parallel chains Upsampler(D) -> FIR(g) -> FrequencyTranslator(+c / K), summed:
//     xhat[n] = sum_c exp(+j 2 pi c n / K) sum_m g[n - m D] Y[m, c]
// evaluated as
//     V[m, :] = unnormalised inverse DFT of Y[m, :]                                                  (fft_lds, kernels_fft.h)
//     xhat[n] = sum_{q < Q, n mod D + q D < M} g[n mod D + q D] V[floor(n / D) - q, n mod K]           Q = ceil(M / D)
// in two launches per call:
//
// pfb_synth_ifft_kernel: a workgroup takes a tile of T frames (from the carried partial frame followed by the call's input), transforms them in
//   LDS G at a time - the T / G tiling of the analysis kernel per K - and stores them as rows Q - 1 + f of the V scratch, whose first Q - 1 rows are
//   the V frames the calls before left behind (zero at the start of the stream).  A frame's V depends on its K values alone and goes through the
//   same butterflies wherever it falls in a group, a tile or a call.
//
// pfb_synth_sums_kernel: every term of one output reads column k = n mod K, and the outputs of one column are K samples = R frames apart.  A work
//   item is (column k along the lanes, F consecutive outputs of that column): frames fl + R i, i < F, where the column fixes the frames' class
//   j = k / D (frame number modulo R, counted from the start of the stream) and the tap phase d = k mod D.  With q = q' R + s the term of frame
//   fl + R i reads V row fl - s + R (i - q') with tap g[d + s D + q' K]: for each s < R that is the analysis kernel's window turned around - rows R
//   frames apart, row u serves output i at q' and output i + 1 at q' + 1 - so the item keeps R windows in registers, walks q' from Q' - 1 down to 0
//   (Q' = ceil(Q / R)) and per step and per s loads ONE new V value and ONE tap for F complex-by-real FMAs.  Steps run in chunks whose loads are all
//   issued in front of the chunk's FMAs (16 V loads and 16 taps in flight whatever R is).
//   The chain of an output is q = Q - 1 ... 0 (oldest frame first; q' descending, s descending inside a step) in one fmaf chain wherever the
//   output falls in its block, its tile or the call, and both load paths (checked against the scratch's ends / unchecked inside it) return the
//   same values: chunking is bit-invariant.  Only the step q' = Q' - 1 can hold taps past M; those terms are SKIPPED, not multiplied by zero, so
//   a NaN in frame m reaches outputs m D .. m D + M - 1 and no other.
//   Lanes hold consecutive columns: reads of V are contiguous across a wave (in runs of D columns where a wave spans classes, K < 64 R), and so
//   are the stores of xhat (frame (fl + R i), sample d: the classes of a tile's columns are consecutive frames).
//   Tiles are handed out by the XCD remap of pfb_channelizer_kernel, so the (Q - 1)-row halo a tile shares with its predecessor is an L2 hit.
//
// Tiles (PfbSynthesizerStage): the ifft kernel uses the R = 1 table of kernels_pfb.h (T, G, threads by K); the sums kernel takes
//   TS = R F max(1, 512 / K) frames per workgroup of 256 threads (max(K, 512) items), F = 8 at R = 1, F = 4 at R = 2 and 4.
// The instantiations live in a code section of their own, as the oversampled analysis kernels do: every older kernel keeps its address.
#pragma once
#include "common.h"
#include "kernels_fft.h"

namespace lrhip {

constexpr int PFBS_LOADS = 16;           // V loads (and taps) in flight per chunk of the sums walk: R windows x 16 / R steps

// value e of the call's frame stream: the carried partial frame (npend values) followed by the call's input
__device__ __forceinline__ float2 pfb_synth_value(const float2 *__restrict__ pend, const float2 *__restrict__ x, long e, long npend)
{
    return e < npend ? pend[e] : x[e - npend];
}

// T frames per workgroup, transformed G at a time: LDS = [a: T frames | b: G frames of fft_lds scratch | K / 2 twiddles]
template <int NT>
__global__ __launch_bounds__(NT) __attribute__((section("lrhip_pfb_synth"))) void pfb_synth_ifft_kernel(const float2 *__restrict__ pend, const float2 *__restrict__ x,
                                                             const float2 *__restrict__ tw, float2 *__restrict__ v, int log2k, int T, int G,
                                                             long npend, long nframes)
{
    extern __shared__ __attribute__((aligned(16))) float2 pfbs_lds[];
    const int K = 1 << log2k;
    float2 *a = pfbs_lds, *b = pfbs_lds + ((size_t)T << log2k), *twl = b + ((size_t)G << log2k);
    for (int i = threadIdx.x; i < K / 2; i += NT) twl[i] = tw[i];
    const long f0 = (long)blockIdx.x * T;
    const int valid = (nframes - f0) < T ? (int)(nframes - f0) : T;
    const int count = valid << log2k;
    const long e0 = f0 << log2k;
    if (e0 >= npend) {                                        // every tile but the first: the input alone
        const float2 *src = x + (e0 - npend);
        for (int i = threadIdx.x; i < count; i += NT) a[i] = src[i];
    } else {
        for (int i = threadIdx.x; i < count; i += NT) a[i] = pfb_synth_value(pend, x, e0 + i, npend);
    }
    __syncthreads();
    for (int g0 = 0; g0 < valid; g0 += G) {
        const int ng = valid - g0 < G ? valid - g0 : G;
        const float2 *res = fft_lds(a + ((size_t)g0 << log2k), b, K, log2k, ng, twl, true);
        // rows of the scratch are K * 8 >= 64 bytes and the scratch is an allocation of its own: 16-byte stores always
        const float4 *src = reinterpret_cast<const float4 *>(res);
        float4 *dst = reinterpret_cast<float4 *>(v + ((f0 + g0) << log2k));
        const int total = ng << log2k;
        for (int i = threadIdx.x; i < total / 2; i += NT) dst[i] = src[i];
        if (g0 + G < valid) __syncthreads();                 // the next group's first pass overwrites the scratch this one may have left its result in
    }
}

// row `row` of the V scratch (row 0 = the oldest carried frame, row Q - 1 = the call's first frame), column k.  Rows outside the scratch are read
// only by terms that are skipped (before row 0: q >= Q) or by outputs that are not stored (past the last frame); they read as zero.
template <bool FAST>
__device__ __forceinline__ float2 pfb_synth_v(const float2 *__restrict__ v, long row, int k, int log2k, long nrows)
{
    if (!FAST && (row < 0 || row >= nrows)) return make_float2(0.f, 0.f);
    return v[(row << log2k) + k];
}

template <int R, int F, bool FAST>
__device__ __forceinline__ void pfb_synth_sums(const float2 *__restrict__ v, const float *__restrict__ taps, float2 *__restrict__ y, int M, int log2k,
                                               int Q, int TS, long f0, long nframes, int class0)
{
    constexpr int LOG2R = R == 1 ? 0 : R == 2 ? 1 : 2;
    constexpr int U = PFBS_LOADS / R;
    static_assert(R == 1 || R == 2 || R == 4, "oversampling by 1, 2 or 4");
    const int K = 1 << log2k, log2d = log2k - LOG2R, D = 1 << log2d;
    const int QP = (Q + R - 1) >> LOG2R;                      // steps: q' = QP - 1 ... 0
    const long nrows = nframes + Q - 1;
    const int items = (TS / (R * F)) << log2k;
    for (int id = threadIdx.x; id < items; id += blockDim.x) {
        const int k = id & (K - 1), fb = id >> log2k;
        const int j = k >> log2d, d = k & (D - 1);
        const int fl = ((j - class0) & (R - 1)) + R * fb * F;                      // the item's first frame in the tile; its frames are fl + R i
        // window s, row u: scratch row base - s + u R; output i at step t (q' = QP - 1 - t) reads u = i + t
        const long base = (long)(Q - 1) + f0 + fl - (long)(QP - 1) * R;
        bool row0[R];                                        // step 0 is the only one whose taps can lie past M (or whose q past Q - 1)
#pragma unroll
        for (int s = 0; s < R; s++) row0[s] = d + (s << log2d) + ((QP - 1) << log2k) < M;
        float2 acc[F], win[R][U + F - 1];
#pragma unroll
        for (int i = 0; i < F; i++) acc[i] = make_float2(0.f, 0.f);
#pragma unroll
        for (int s = 0; s < R; s++)
#pragma unroll
            for (int u = 0; u + 1 < F; u++) {
                const long row = base - s + (long)u * R;
                win[s][u] = pfb_synth_v<FAST>(v, row, k, log2k, nrows);
            }
        for (int t0 = 0; t0 < QP; t0 += U) {                 // win[s][0 .. F-2] = rows t0 .. t0 + F - 2 of window s
            float h[R][U];
#pragma unroll
            for (int c = 0; c < U; c++) {                    // steps past the last one reload its row and tap (in range) and are not accumulated
                const int t = t0 + c < QP ? t0 + c : QP - 1;
#pragma unroll
                for (int s = 0; s < R; s++) {
                    const long row = base - s + (long)(F - 1 + t) * R;
                    win[s][F - 1 + c] = pfb_synth_v<FAST>(v, row, k, log2k, nrows);
                    const int i = d + (s << log2d) + ((QP - 1 - t) << log2k);
                    h[s][c] = taps[i < M ? i : d];           // i >= M only at t = 0, where row0 keeps it out of the sum
                }
            }
#pragma unroll
            for (int c = 0; c < U; c++) {
                if (t0 + c < QP) {
#pragma unroll
                    for (int s = R - 1; s >= 0; s--) {       // q = q' R + s descending: oldest frame first
                        if (t0 + c > 0 || row0[s]) {
#pragma unroll
                            for (int i = 0; i < F; i++) {
                                acc[i].x = fmaf(h[s][c], win[s][i + c].x, acc[i].x);
                                acc[i].y = fmaf(h[s][c], win[s][i + c].y, acc[i].y);
                            }
                        }
                    }
                }
            }
#pragma unroll
            for (int s = 0; s < R; s++)
#pragma unroll
                for (int u = 0; u + 1 < F; u++) win[s][u] = win[s][U + u];
        }
#pragma unroll
        for (int i = 0; i < F; i++) {
            const long f = f0 + fl + R * i;
            if (f < nframes) y[(f << log2d) + d] = acc[i];
        }
    }
}

// TS frames (TS D outputs) per workgroup; phase = class of the call's first frame (frames emitted before this call, modulo R)
template <int R, int F>
__global__ __launch_bounds__(256) __attribute__((section("lrhip_pfb_synth"))) void pfb_synth_sums_kernel(const float2 *__restrict__ v, const float *__restrict__ taps,
                                                             float2 *__restrict__ y, int M, int log2k, int Q, int TS, long nframes, int phase)
{
    // the tile remap of pfb_channelizer_kernel: the workgroups of one XCD take consecutive tiles, which share Q - 1 rows of V
    const unsigned nwg = gridDim.x, xcd = blockIdx.x & 7, qq = nwg >> 3, rem = nwg & 7;
    const unsigned tile = (xcd < rem ? xcd * (qq + 1) : rem * (qq + 1) + (xcd - rem) * qq) + (blockIdx.x >> 3);
    const long f0 = (long)tile * TS;
    const int class0 = (int)((phase + f0) & (R - 1));
    const int QP = (Q + R - 1) / R;
    // the tile reads scratch rows lo .. hi; rows 0 .. nframes + Q - 2 exist
    const long lo = (long)(Q - 1) + f0 - (long)(QP - 1) * R - (R - 1), hi = (long)(Q - 1) + f0 + TS - 1;
    if (lo >= 0 && hi < nframes + Q - 1) pfb_synth_sums<R, F, true>(v, taps, y, M, log2k, Q, TS, f0, nframes, class0);
    else pfb_synth_sums<R, F, false>(v, taps, y, M, log2k, Q, TS, f0, nframes, class0);
}

// dst[i] = src[i], 16 bytes each: the last Q - 1 rows of the V scratch on their way to its front
__global__ __launch_bounds__(256) __attribute__((section("lrhip_pfb_synth"))) void pfb_synth_copy_kernel(const float4 *__restrict__ src, float4 *__restrict__ dst, long n4)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n4) dst[i] = src[i];
}

// the partial frame a call leaves behind: pend[i] = x[first + i], start <= i < count (a call that completes no frame appends: start = what was pending)
__global__ __launch_bounds__(256) __attribute__((section("lrhip_pfb_synth"))) void pfb_synth_pending_kernel(const float2 *__restrict__ x, float2 *__restrict__ pend,
                                                             long first, int start, int count)
{
    const int i = start + (int)(blockIdx.x * 256 + threadIdx.x);
    if (i < count) pend[i] = x[first + i];
}

}  // namespace lrhip
