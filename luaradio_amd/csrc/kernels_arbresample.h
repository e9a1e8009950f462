// kernels_arbresample.h - the arbitrary-ratio resampler (ArbitraryResamplerBlock): a polyphase bank of P phases, linearly interpolated between
// neighbouring phases, as GNU Radio's pfb_arb_resampler and liquid-dsp's resamp.  Not a block of the reference.
//
// Absolute output m sits at u = m * step in 16.48 fixed point of an input sample (arbresample_plan.h: i, p, mu of m).  With the Float32 tables
// G[p][k] = h[k P + p] and D[p][k] = fl32(G[p + 1][k] - G[p][k]) (row P = row 0 one tap later, stage_arbresample.h)
//     c_k  = fmaf(mu, D[p][k], G[p][k])
//     y[m] = sum_{k = 0}^{T - 1} c_k x[i - k],   x[j] = 0 for j < 0
// summed as ONE fmaf chain per output component, acc = fmaf(c_k, x[i - k], acc) from acc = 0 in ASCENDING k (the newest sample first).  Nothing else
// is a floating-point sum or product that could be contracted: mu24 -> Float32 and the scale by 2^-24 are exact.  y[m] is a function of m and the
// stream alone, so any cut of the stream, a seek and a time partition give the same bits.
//
// Shape.  A workgroup of 256 lanes owns tiles of ARB_TILE = 512 consecutive outputs; a lane computes outputs t and t + 256 of the tile, so a wave's
// stores are consecutive and the two chains of a lane interleave.  Per tile the workgroup stages the input span of the tile - samples
// i(first) - (T - 1) .. i(last), at most floor(511 step / 2^48) + 1 + T of them - from [history | x] (fir_resample_kernel's layout) into LDS.  The
// tables are staged once per workgroup: the grid is persistent (launch_prep.h), a workgroup strides through the tiles.  The workgroup with the
// highest index writes the next call's T - 1 history samples into the other ping-pong slot; a call without outputs is a launch of that alone.
//
// LDS.  Neighbouring outputs read DIFFERENT rows p, so the register-window FIR forms do not apply and every tap costs LDS reads.  G and D are stored
// interleaved, one {G[p][k], D[p][k]} pair per tap, so a tap is ONE 8-byte table read, one sample read and three fmaf (S = 2).  A row holds T pairs
// and T is even: at a stride of T pairs the rows of a wave would start on only 32 / gcd(T, 32) of the 32 pair-wide bank slots an 8-byte read sees
// (two of them at T = 16).  The row stride is T + 1 pairs, odd, so 32 consecutive rows start on 32 different slots; which rows a wave reads
// depends on the ratio, and two lanes on the same row read the same address (a broadcast).  The stage uploads the table already padded.
// The samples are not padded: at ratio >= 1 neighbouring lanes read the same or neighbouring samples; when decimating by s the lanes of a wave read
// s samples apart, an about s-way conflict that only a transposed layout would remove.  Not built, not measured.
//
// Tile size.  The worst case is ratio 1 / 16 with T = 256 (P = 32): 8176 + 258 ComplexFloat32 samples of span = 67 472 bytes next to 32 * 257 pairs
// = 65 792 bytes of tables (67 584 at P = 256, T = 32), 133 KB of the CU's 160 KB; a tile of 1024 would need 199 KB.  With the defaults at ratio >= 1
// (P = 64, T = 16) a workgroup takes 8.7 KB of tables and 4.2 KB of span, and the 32 waves of a CU, not the LDS, bound the residency
// (the compiler reports 48 VGPRs for S = 2 and 40 for S = 1, no scratch: 8 waves per SIMD).
//
// An output pointer that is not 8-byte aligned (ComplexFloat32) is written with two 4-byte stores per sample; the input and the history are read
// with 4-byte loads while staging, whatever their alignment.
// (part of liblrhip.so; included by lrhip.hip in this order, one translation unit)
#pragma once
#include "common.h"
#include "arbresample_plan.h"

namespace lrhip {

constexpr int ARB_NT = 256, ARB_PER = 2, ARB_TILE = ARB_NT * ARB_PER;

// samples of LDS span a tile can need: i(last) - i(first) <= floor(511 step / 2^48) + 1, plus the T - 1 samples behind the first, plus one of slack
inline int arb_span_cap(uint64_t step, int T) { return (int)(((uint64_t)(ARB_TILE - 1) * step) >> arbplan::FRAC_BITS) + 1 + T + 1; }
inline size_t arb_lds_bytes(int P, int T, uint64_t step, int S) { return ((size_t)2 * P * (T + 1) + (size_t)arb_span_cap(step, T) * S) * sizeof(float); }

template <int S>
__global__ __launch_bounds__(ARB_NT) void arb_resample_kernel(const float *__restrict__ hist, const float *__restrict__ x, const float2 *__restrict__ tab,
                                                              float *__restrict__ y, int T, int log2p, uint64_t step, long n_in, long n_out, uint64_t m0,
                                                              uint64_t Q0, int span_cap, int y_vec, float *__restrict__ hist_out)
{
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int TS = T + 1, H = T - 1, npairs = TS << log2p;
    float2 *ldsT = reinterpret_cast<float2 *>(lds);      // {G, D} pairs, row stride T + 1
    float *ldsX = lds + 2 * npairs;                      // the tile's input span, S floats per sample
    const int tid = threadIdx.x;
    // history carry: the last T - 1 raw input samples of [hist | x]
    if (blockIdx.x == gridDim.x - 1)
        for (int i = tid; i < H * S; i += ARB_NT) {
            const long g = n_in - H + i / S;             // index into x (negative: history)
            hist_out[i] = g >= 0 ? x[g * S + i % S] : hist[(g + H) * S + i % S];
        }
    const long ntiles = (n_out + ARB_TILE - 1) / ARB_TILE;
    if ((long)blockIdx.x >= ntiles) return;
    for (int i = tid; i < npairs; i += ARB_NT) ldsT[i] = tab[i];
    for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const long mb = tile * ARB_TILE;
        const long ml = mb + ARB_TILE - 1 < n_out - 1 ? mb + ARB_TILE - 1 : n_out - 1;
        // i of the tile's first and last output modulo 2^64: differences to Q0 and to each other are small (inside the chunk and its history)
        const uint64_t ib = arbplan::position(m0 + (uint64_t)mb, step, log2p).i_lo;
        const uint64_t il = arbplan::position(m0 + (uint64_t)ml, step, log2p).i_lo;
        const long base = (long)(ib - Q0) - H;           // chunk-relative input index of ldsX[0]
        int span = (int)(il - ib) + T;
        if (span > span_cap) span = span_cap;
        __syncthreads();                                 // the previous tile's reads are done
        for (int j = tid; j < span; j += ARB_NT) {
            const long g = base + j;
#pragma unroll
            for (int cc = 0; cc < S; cc++) {
                float v = 0.f;
                if (g >= 0) { if (g < n_in) v = x[g * S + cc]; }
                else if (g + H >= 0) v = hist[(g + H) * S + cc];
                ldsX[j * S + cc] = v;
            }
        }
        __syncthreads();
        const float2 *tp[ARB_PER];
        const float *xp[ARB_PER];
        float mu[ARB_PER], re[ARB_PER], im[ARB_PER];
        long m[ARB_PER];
#pragma unroll
        for (int r = 0; r < ARB_PER; r++) {
            m[r] = mb + r * ARB_NT + tid;
            const arbplan::Pos q = arbplan::position(m0 + (uint64_t)(m[r] <= ml ? m[r] : ml), step, log2p);      // a lane behind the end computes the last output again
            tp[r] = ldsT + q.p * TS;
            xp[r] = ldsX + ((int)(q.i_lo - ib) + H) * S;                                                       // x[i]; the taps walk back from it
            mu[r] = (float)q.mu24 * 0x1p-24f;
            re[r] = im[r] = 0.f;
        }
        for (int k = 0; k < T; k++) {
#pragma unroll
            for (int r = 0; r < ARB_PER; r++) {
                const float2 gd = tp[r][k];
                const float c = fmaf(mu[r], gd.y, gd.x);
                if (S == 2) {
                    const float2 v = *reinterpret_cast<const float2 *>(xp[r] - 2 * k);
                    re[r] = fmaf(c, v.x, re[r]);
                    im[r] = fmaf(c, v.y, im[r]);
                } else {
                    re[r] = fmaf(c, xp[r][-k], re[r]);
                }
            }
        }
#pragma unroll
        for (int r = 0; r < ARB_PER; r++) {
            if (m[r] > ml) continue;
            if (S == 2 && y_vec) reinterpret_cast<float2 *>(y)[m[r]] = make_float2(re[r], im[r]);
            else if (S == 2) { y[2 * m[r]] = re[r]; y[2 * m[r] + 1] = im[r]; }
            else y[m[r]] = re[r];
        }
    }
}

}  // namespace lrhip
