// kernels_pfb.h - K-channel analysis filterbank in its polyphase + FFT form, K a power of two in [8, 4096]: critically sampled (below) and
// oversampled by 2 or 4 (pfb_oversampled_kernel, at the end).
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

// ---- oversampled by R = 2 or 4: frame hop D = K / R, one frame per D input samples, each channel at R rate / K
//
//     u_r[m] = sum_{p<P} h[r + pK] x[mD - r - pK]          v[(r - mD) mod K] = u_r[m]          y[m, :] = unnormalised inverse DFT of v
//
// mD mod K = (m mod R) D: a frame's class m mod R (m counted from the start of the stream, so the kernel is told the class of the call's first frame)
// fixes its rotation.  Frames m and m + R read the same rows one tap row apart, as frames m and m + 1 do at R = 1, so an item is (branch r, residue
// j of the frame's place in the tile mod R, block of F frames of that residue) and the window walk of pfb_sums carries over with its base shifted by
// j D: row i of the item is base + i K, its frames are j + R (fb F + f), f < F.  The accumulation order is p = P - 1 ... 0 in one fmaf chain per output
// wherever the frame falls, so chunking is bit-invariant and frame m R has the bytes of the R = 1 kernel's frame m (same window, rotation 0).
// The rotation is in the column of the store into the frame buffer, (r - class D) & (K - 1).  At K >= 64 the lanes of a wave hold consecutive r of one
// frame, and any 32 cyclically consecutive float2 columns are distinct modulo 32: the rotated store touches the banks the unrotated one does.  Below
// K = 64 a wave holds 64 / K frames, each rotated inside its own K columns, so the wave writes the same set of addresses as without the rotation; the
// frames of a wave are R (and at K = 8, 16 also R F) frames apart, a multiple of 32 columns, as in the R = 1 kernel where they are F frames apart.
// No LDS bank-conflict counter was taken for either kernel.
// fft_lds, the output stores and the tile remap are those of the kernel above; a tile now brings T D new samples against the same (P - 1) K halo.
//
// Tiles (PfbChannelizerStage::launch_oversampled_by_k), F per residue, T a multiple of R F wherever F > 1; R = 2 | R = 4:
//   K <= 64       T = 2048 / K, G = T, F = 8    256 threads            | the same                                     as R = 1
//   K = 128       T = 16, G = 16, F = 8         256                    | F = 4                                        as R = 1
//   K = 256       T = 8,  G = 8,  F = 4         256                    | F = 2                                        as R = 1
//   K = 512       T = 8,  G = 8,  F = 4        1024   66 KiB           | T = 16, G = 4, F = 4   1024   82 KiB, 1 workgroup per CU
//   K = 1024      T = 4,  G = 4,  F = 2         512   68 KiB           | T = 8,  G = 1, F = 2    512   76 KiB, 2 per CU
//   K = 2048      T = 8,  G = 1,  F = 4        1024  152 KiB           | T = 8,  G = 1, F = 2   1024  152 KiB
//   K = 4096      T = 2,  G = 1,  F = 1        1024  112 KiB           | the same (a tile is half a round of classes)
// F = 1 is the walk without reuse: P sample loads per P FMAs, the rows shared with the other residues and with the neighbouring tiles come from L1 / L2.
// Measured on one box in one session, one process per line, 5 windows of 100 calls of 2^24 samples, P = 16, ms per call (median; the windows of a
// process agree to 0.001, the two runs of the R = 1 tile that bracket each group to 0.001-0.007; profiles/pfb_oversampled_tiles.txt):
//   K = 1024 R = 4   T = 4, G = 4, F = 1 (the R = 1 tile) 0.737 / 0.738   T = 8, G = 1, F = 2, 512 threads 0.546 (kept)
//                    T = 8, G = 2, F = 2 (84 KiB, 1 workgroup per CU) 0.758 with 512 threads, 0.771 with 1024;  T = 16, G = 1, F = 4, 1024 threads 0.774
//   K = 1024 R = 2   T = 4, G = 4, F = 2 0.263 / 0.263 (kept)   T = 8, G = 1, F = 4 0.265   T = 8, G = 2, F = 4, 1024 threads 0.334
//   K = 2048 R = 4   T = 4, G = 2, F = 1 (the R = 1 tile) 1.047 / 1.048   T = 8, G = 1, F = 2 0.816 (kept)
//   K = 2048 R = 2   T = 4, G = 2, F = 2 0.412 / 0.412                    T = 8, G = 1, F = 4 0.361 (kept)
//   K = 512  R = 4   T = 8, G = 8, F = 2 0.732 / 0.732   T = 16, G = 2, F = 4 (74 KiB, 2 per CU) 0.742   T = 16, G = 4, F = 4 0.585 (kept)
//   K = 4096         T = 2, F = 1: 0.577-0.584 (R = 2), 1.096-1.097 (R = 4).  There is no other tile to set against it: 4 frames of sums + 1 of scratch +
//                    the twiddles are 176 KiB of the 160 KiB, so a class never has two frames in a tile and F stays 1.
// So where the LDS holds 2 R frames the register block pays (1.26-1.35x at R = 4), transforming one frame at a time (G = 1) costs less than the
// occupancy a second scratch frame takes, and K = 1024 at R = 2 already has its block in the R = 1 tile.  K = 512 at R = 2 and K <= 256 were not varied.
template <int R, int F, bool FAST>
__device__ __forceinline__ void pfb_sums_oversampled(const float2 *__restrict__ hist, const float2 *__restrict__ x, const float *__restrict__ taps,
                                                     float2 *u, int M, int K, int log2k, int P, int T, int valid, long q0, long n, int class0)
{
    constexpr int U = PFB_U;
    constexpr int LOG2R = R == 2 ? 1 : 2;
    static_assert(R == 2 || R == 4, "oversampling by 2 or 4");
    const int D = K >> LOG2R;
    const int items = (T / F) << log2k;
    for (int id = threadIdx.x; id < items; id += blockDim.x) {
        const int r = id & (K - 1), rest = id >> log2k, j = rest & (R - 1), fb = rest >> LOG2R;
        const int fl = j + R * fb * F;                        // the item's first frame in the tile; its frames are fl + R f
        const long base = q0 + (long)fl * D - r - (long)(P - 1) * K;              // row i of the item: base + i K
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
            for (int i = 0; i + 1 < F; i++) win[i] = win[U + i];
        }
        const int col = (r - ((class0 + j) & (R - 1)) * D) & (K - 1);            // every frame of the item has the class of its residue
#pragma unroll
        for (int f = 0; f < F; f++)
            if (fl + R * f < valid) u[((fl + R * f) << log2k) + col] = acc[f];
    }
}

// as pfb_channelizer_kernel with hop K / R; phase = class of the call's first frame (frames emitted before this call, modulo R)
// The instantiations live in a code section of their own, behind the library's .text: every kernel that was there before them keeps its address.
template <int R, int F, int NT>
__global__ __launch_bounds__(NT) __attribute__((section("lrhip_pfb_oversampled"))) void pfb_oversampled_kernel(const float *__restrict__ hist, const float *__restrict__ x,
                                                             const float *__restrict__ taps, const float2 *__restrict__ tw,
                                                             float *__restrict__ y, int M, int log2k, int P, int T, int G, long n,
                                                             long nframes, long first, int phase)
{
    extern __shared__ __attribute__((aligned(16))) float2 pfb_lds[];
    const int K = 1 << log2k, D = K / R;
    float2 *a = pfb_lds, *b = pfb_lds + ((size_t)T << log2k), *twl = b + ((size_t)G << log2k);
    for (int i = threadIdx.x; i < K / 2; i += NT) twl[i] = tw[i];
    // the tile remap of pfb_channelizer_kernel: the workgroups of one XCD take consecutive tiles, which share (P - 1) K - T D samples of halo
    const unsigned nwg = gridDim.x, xcd = blockIdx.x & 7, q = nwg >> 3, rem = nwg & 7;
    const unsigned tile = (xcd < rem ? xcd * (q + 1) : rem * (q + 1) + (xcd - rem) * q) + (blockIdx.x >> 3);
    const long f0 = (long)tile * T;
    const int valid = (nframes - f0) < T ? (int)(nframes - f0) : T;
    // newest sample of frame f is x[first + f D] = stream position first + f D + (M - 1); the tile reads positions lo .. hi
    const long q0 = first + f0 * D + (M - 1);
    const long lo = q0 - (long)(P - 1) * K - (K - 1), hi = q0 + (long)(T - 1) * D;
    const int class0 = (int)((phase + f0) & (R - 1));
    const float2 *h2 = reinterpret_cast<const float2 *>(hist), *x2 = reinterpret_cast<const float2 *>(x);
    if (lo >= M - 1 && hi - (M - 1) < n) pfb_sums_oversampled<R, F, true>(h2, x2, taps, a, M, K, log2k, P, T, valid, q0, n, class0);
    else pfb_sums_oversampled<R, F, false>(h2, x2, taps, a, M, K, log2k, P, T, valid, q0, n, class0);
    __syncthreads();
    const bool vec4 = (reinterpret_cast<uintptr_t>(y) & 15) == 0;
    for (int g0 = 0; g0 < valid; g0 += G) {
        const int ng = valid - g0 < G ? valid - g0 : G;
        const float2 *res = fft_lds(a + ((size_t)g0 << log2k), b, K, log2k, ng, twl, true);
        float *yt = y + 2 * ((f0 + g0) << log2k);
        const int total = ng << log2k;
        if (vec4) {
            const float4 *src = reinterpret_cast<const float4 *>(res);
            float4 *dst = reinterpret_cast<float4 *>(yt);
            for (int i = threadIdx.x; i < total / 2; i += NT) dst[i] = src[i];
        } else {
            float2 *dst = reinterpret_cast<float2 *>(yt);
            for (int i = threadIdx.x; i < total; i += NT) dst[i] = res[i];
        }
        if (g0 + G < valid) __syncthreads();
    }
}

}  // namespace lrhip
