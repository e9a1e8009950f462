// kernels_pfb.h - critically sampled K-channel analysis filterbank in its polyphase + FFT form, K a power of two in [8, 4096].
//
// The same block as kernels_channelizer.h (output frame m, channel c:  y_c[m] = sum_{i<M} h[i] x[mK - i] exp(+j 2 pi c i / K)),
// evaluated as
//     u_r[m] = sum_{p<P} h[r + pK] x[mK - r - pK],   r < K,  P = ceil(M / K)          (K real-by-complex dot products of P terms)
//     y[m, :] = unnormalised inverse DFT over r of u[m, :]                             (fft_lds, kernels_fft.h)
// i.e. 2 P + 5 log2 K flop per sample where the GEMM form spends 8 M.
//
// A workgroup takes a tile of T consecutive frames (chosen on the host by K, table below):
//   1. polyphase sums into the LDS frame buffer.  A work item is (block of F consecutive frames, branch r) with r along the lanes,
//      so every read of x is contiguous across a wave (in reverse).  Branch r of frame f reads x[(f - p) K - r]: one sample row serves
//      frame f at tap row p and frame f + 1 at tap row p + 1, so the item keeps a window of rows in registers, walks p from P - 1
//      down to 0 and loads ONE new sample and ONE tap per step for F complex-by-real FMAs (P + F - 1 sample loads per F P FMAs).
//      The accumulation order of a frame is p = P - 1 ... 0 wherever the frame falls in its block, its tile or the call, and both
//      load paths (checked against the carried history / unchecked inside the call) return the same values: chunking is bit-invariant.
//   2. fft_lds(inverse) over the tile's frames, G frames at a time (G = T where the LDS allows it).
//   3. whole frames stored with 16-byte stores (8-byte when y is not 16-byte aligned).
// Tap rows past M (the padding from M to P K) are SKIPPED, not multiplied by zero: a NaN in x must not reach a frame whose M-sample
// window does not hold it.
//
// LDS: T frames of polyphase sums + G frames of fft_lds scratch + K / 2 twiddles (8 B each), F = frames per register block:
//   K <= 256      T = 2048 / K, G = T, F = 8     256 threads    32 KiB + <= 1 KiB      4 workgroups per CU
//   K = 512       T = 8,  G = 8, F = 8          1024 threads    64 KiB + 2 KiB         2 workgroups per CU
//   K = 1024      T = 4,  G = 4, F = 4           512 threads    64 KiB + 4 KiB         2
//   K = 2048      T = 4,  G = 2, F = 4          1024 threads    96 KiB + 8 KiB         1 workgroup per CU
//   K = 4096      T = 2,  G = 1, F = 2          1024 threads    96 KiB + 16 KiB        1
// At K >= 2048 one frame of fft_lds ping-pong is 32-64 KiB, so the tile keeps its sums in place and transforms them through a smaller
// scratch.  K = 1024 measured both ways on one box, alternating: T = 8, G = 4, F = 8 in one workgroup of 1024 threads per CU 0.149-0.152 ms per
// 2^24 samples (M = 16 384), two workgroups of 512 threads with half the tile 0.123-0.136; the same exchange at K = 4096 (T = 1, F = 1,
// 80 KiB) is inside the spread (0.252-0.289 against 0.267-0.277), so the larger register block stays there.
// x is NOT staged in LDS in any class: the window rows come from global memory, where the (P - 1)-row halo a tile shares with
// its predecessor and the rows an item shares with the next frame block are L1 / L2 hits, not HBM traffic (measured; see the tile
// remap in the kernel).
#pragma once
#include "common.h"
#include "kernels_fft.h"
#include "kernels_fir.h"

namespace lrhip {

constexpr int PFB_TILE_SMALL = 2048;     // samples (frames x K) per workgroup, K <= 256
constexpr int PFB_TILE_LARGE = 8192;     // K >= 2048 (K = 512: 8 frames, K = 1024: 4)
constexpr int PFB_SCRATCH = 4096;        // samples of fft_lds scratch at K >= 2048

// stream position p (0 .. M-2 = carried history, M-1 .. = this call's x) as one complex sample; zero before the stream and after the call
template <bool FAST>
__device__ __forceinline__ float2 pfb_sample(const float2 *__restrict__ hist, const float2 *__restrict__ x, long p, int M, long n)
{
    if (FAST) return x[p - (M - 1)];
    if (p < 0) return make_float2(0.f, 0.f);
    if (p < M - 1) return hist[p];
    const long xi = p - (M - 1);
    return xi < n ? x[xi] : make_float2(0.f, 0.f);
}

// polyphase sums of one tile into u[T][K].  q0 = stream position of the newest sample of the tile's first frame.
// Rows of an item are numbered from its oldest one: row j = samples base + j K; at step t (tap row p = P - 1 - t) frame f reads row f + t,
// and row F - 1 + t is the one new row of the step.  Steps run in chunks of PFB_U whose PFB_U samples and PFB_U taps are loaded together
// in front of the chunk's FMAs: one memory latency per chunk, not per step - at P <= 16 every load of an item is in flight at once.
// Step 0 is the only tap row that can be part padding.
constexpr int PFB_U = 16;

template <int F, bool FAST>
__device__ __forceinline__ void pfb_sums(const float2 *__restrict__ hist, const float2 *__restrict__ x, const float *__restrict__ taps,
                                         float2 *u, int M, int K, int log2k, int P, int T, int valid, long q0, long n)
{
    constexpr int U = PFB_U;
    const int items = (T / F) << log2k;
    for (int id = threadIdx.x; id < items; id += blockDim.x) {
        const int r = id & (K - 1), fb = id >> log2k;
        const long base = q0 + (long)fb * F * K - r - (long)(P - 1) * K;          // row j of the item: base + j K
        const bool row0 = r + ((P - 1) << log2k) < M;         // the padded part of the last tap row is skipped, not multiplied
        float2 acc[F], win[U + F - 1];
#pragma unroll
        for (int f = 0; f < F; f++) acc[f] = make_float2(0.f, 0.f);
#pragma unroll
        for (int f = 0; f + 1 < F; f++) win[f] = pfb_sample<FAST>(hist, x, base + (long)f * K, M, n);
        for (int t0 = 0; t0 < P; t0 += U) {                   // win[0 .. F-2] = rows t0 .. t0 + F - 2
            float h[U];
#pragma unroll
            for (int s = 0; s < U; s++) {                     // steps past the last one reload its row and tap (in range) and are not accumulated
                const int t = t0 + s < P ? t0 + s : P - 1;
                win[F - 1 + s] = pfb_sample<FAST>(hist, x, base + (long)(F - 1 + t) * K, M, n);
                const int i = r + ((P - 1 - t) << log2k);
                h[s] = taps[i < M ? i : r];                   // i >= M only at t = 0, where row0 keeps it out of the sum
            }
#pragma unroll
            for (int s = 0; s < U; s++) {
                if (t0 + s < P && (t0 + s > 0 || row0)) {
#pragma unroll
                    for (int f = 0; f < F; f++) {
                        acc[f].x = fmaf(h[s], win[f + s].x, acc[f].x);
                        acc[f].y = fmaf(h[s], win[f + s].y, acc[f].y);
                    }
                }
            }
#pragma unroll
            for (int j = 0; j + 1 < F; j++) win[j] = win[U + j];
        }
#pragma unroll
        for (int f = 0; f < F; f++)
            if (fb * F + f < valid) u[((fb * F + f) << log2k) + r] = acc[f];
    }
}

// T frames per workgroup, transformed G at a time: LDS = [u: T frames | scratch: G frames | K / 2 twiddles]
template <int F, int NT>
__global__ __launch_bounds__(NT) void pfb_channelizer_kernel(const float *__restrict__ hist, const float *__restrict__ x,
                                                             const float *__restrict__ taps, const float2 *__restrict__ tw,
                                                             float *__restrict__ y, int M, int log2k, int P, int T, int G, long n,
                                                             long nframes, long first)
{
    extern __shared__ __attribute__((aligned(16))) float2 pfb_lds[];
    const int K = 1 << log2k;
    float2 *a = pfb_lds, *b = pfb_lds + ((size_t)T << log2k), *twl = b + ((size_t)G << log2k);
    for (int i = threadIdx.x; i < K / 2; i += NT) twl[i] = tw[i];
    // Tiles are handed out so that the workgroups sharing an L2 take CONSECUTIVE tiles (blockIdx % 8 labels the workgroups of one XCD; the
    // bijective form of the remap, any grid size).  In launch order neighbouring tiles sit on different XCDs and every tile fetched its
    // whole (T + P - 1)-row span from HBM: FETCH_SIZE was (T + P - 1) / T of the input to the percent in every class (1.48x at K = 64,
    // 8.4x at K = 4096, P = 16); with the remap it is 1.00x up to K = 512, 1.01 / 1.08 / 1.25x at K = 1024 / 2048 / 4096
    // (profiles/pfb_channelizer_rocprofv3_summary.txt), and 2^24 samples went 0.084 -> 0.069 ms at K = 256, 0.275 -> 0.215 ms at K = 4096.
    const unsigned nwg = gridDim.x, xcd = blockIdx.x & 7, q = nwg >> 3, rem = nwg & 7;
    const unsigned tile = (xcd < rem ? xcd * (q + 1) : rem * (q + 1) + (xcd - rem) * q) + (blockIdx.x >> 3);
    const long f0 = (long)tile * T;
    const int valid = (nframes - f0) < T ? (int)(nframes - f0) : T;
    // newest sample of frame f is x[first + f K] = stream position first + f K + (M - 1); the tile reads positions lo .. hi
    const long q0 = first + f0 * K + (M - 1);
    const long lo = q0 - (long)(P - 1) * K - (K - 1), hi = q0 + (long)(T - 1) * K;
    const float2 *h2 = reinterpret_cast<const float2 *>(hist), *x2 = reinterpret_cast<const float2 *>(x);
    if (lo >= M - 1 && hi - (M - 1) < n) pfb_sums<F, true>(h2, x2, taps, a, M, K, log2k, P, T, valid, q0, n);
    else pfb_sums<F, false>(h2, x2, taps, a, M, K, log2k, P, T, valid, q0, n);
    __syncthreads();
    const bool vec4 = (reinterpret_cast<uintptr_t>(y) & 15) == 0;
    for (int g0 = 0; g0 < valid; g0 += G) {
        const int ng = valid - g0 < G ? valid - g0 : G;
        const float2 *res = fft_lds(a + ((size_t)g0 << log2k), b, K, log2k, ng, twl, true);
        float *yt = y + 2 * ((f0 + g0) << log2k);
        const int total = ng << log2k;                       // complex outputs of this group; K >= 8, so a multiple of 2
        if (vec4) {
            const float4 *src = reinterpret_cast<const float4 *>(res);
            float4 *dst = reinterpret_cast<float4 *>(yt);
            for (int i = threadIdx.x; i < total / 2; i += NT) dst[i] = src[i];
        } else {
            float2 *dst = reinterpret_cast<float2 *>(yt);
            for (int i = threadIdx.x; i < total; i += NT) dst[i] = res[i];
        }
        if (g0 + G < valid) __syncthreads();                 // the next group's first pass overwrites the scratch this one may have left its result in
    }
}

}  // namespace lrhip
