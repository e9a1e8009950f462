// kernels_digital.h - the four blocks between a filtered baseband and a bit stream, as tile scans:
//   ZeroCrossingClockRecoveryBlock (radio/blocks/signal/zerocrossingclockrecovery.lua:35-73), SamplerBlock (sampler.lua:33-53),
//   SlicerBlock (slicer.lua), DifferentialDecoderBlock (differentialdecoder.lua), and "clocksampler" = sampler(data = x, clock = ZC(x))
//   with an optional slicer and differential decoder folded into its final pass.
//
// Clock recovery.  A hysteresis flip at sample i sets the offset to P/2; then every sample subtracts 1 and a sample whose offset
// drops below 1 is a +1 pulse and adds P.  So after a crossing the output is a function of the samples since that crossing only (before
// the first crossing: of the samples since the stream start, from offset P): out[i] = F_kind(i - last_reset(i)), and last_reset is a
// max-scan of the crossing positions.  F is evaluated per thread (ZcEval):
//   closed form (ZcParams.closed, decided and proven on the host, stage_digital.h): P >= 2 and P + 1 <= 2^(e+1) where 2^e <= P.  From the
//     first pulse after a reset on, the offset after every add lies in [P, P + 1) on the ulp(P) grid, every "- 1" and "+ P" is exact, and
//     with U = 1/ulp(P), Pi = P/ulp(P) the pulses are the k with W(k) = (c0 + k U) mod Pi < U (k >= ks) - 64-bit integers, one 128-bit
//     mulmod per thread, O(1) per sample however long a crossing-free run is.
//   otherwise the literal offset in double (exact: subtracting integers from an offset >= 1 does not round), carried across calls and
//     from tile start to tile start by the carry kernel, then advanced to each thread's first sample in whole-symbol jumps: O(call length / P)
//     serial steps in the carry kernel and O(DG_TILE / P) per thread, however long the crossing-free stretch around the call is.
// The carried state between calls is (samples since the reset, kind of reset, hysteresis, and the literal offset for the fallback).
//
// Passes (tile = 256 threads x DG_LC samples), 4 launches and 2 reads of the input for the clocksampler:
//   zc_summary_kernel   hysteresis summary per tile (first / last decisive sample, last crossing inside)      reads x
//   zc_carry_kernel     one workgroup: hysteresis and last reset at every tile start, the next call's state
//   zc_emit_kernel      the +-1 clock (ZC), or each tile's emitted samples / sliced bits into its staging slot  reads x
//   dg_compact_kernel   clocksampler: packs the slots, applies the differential decoder, writes the count
// The stand-alone sampler runs sampler_summary / sampler_carry / sampler_final on its clock input.
#pragma once
#include "common.h"

namespace lrhip {

constexpr int DG_LC = 16, DG_TILE = 256 * DG_LC;

struct ZcParams {
    double P, T;                     // symbol period (rate / baudrate) and threshold, Lua numbers
    int closed;                      // the closed form holds for this P
    unsigned long long U, Pi;        // 1 / ulp(P), P / ulp(P)
    unsigned long long c0[2];        // W at k = 0 of a reset of each kind (0: stream start, offset P; 1: crossing, offset P/2)
    long long ks[2];                 // first pulse after a reset of each kind
};

// carried between calls (ping-pong on the device)
struct DgState {
    long long k;                     // samples since the last reset
    int kind;                        // 0: stream start, 1: crossing
    int h;                           // hysteresis / sampler clock state: +1 HIGH, -1 LOW
    int prev;                        // clocksampler: the clock (pulse) of the last sample, 1 / 0
    int bit;                         // clocksampler + decoder: the last emitted (sliced) bit
    unsigned long long count;        // outputs of the last call
    double o;                        // without the closed form: the literal offset before the next sample
};

// output of the fused final pass
enum { DG_OUT_FLOAT = 0, DG_OUT_SLICE = 1, DG_OUT_DECODE = 2 };
struct DgTail { int out; double slice_t; int invert; };

// ---- hysteresis summary of a range: first and last decisive sample (+1 above T, -1 below), last crossing strictly inside
struct HSum { int f, l; long long pf, lc; };
__device__ __forceinline__ HSum hsum_empty() { return HSum{0, 0, -1, -1}; }
__device__ __forceinline__ HSum hsum_compose(const HSum &a, const HSum &b)
{
    if (!a.f) return b;
    if (!b.f) return a;
    HSum r;
    r.f = a.f; r.pf = a.pf; r.l = b.l;
    r.lc = b.lc >= 0 ? b.lc : (b.f != a.l ? b.pf : a.lc);
    return r;
}
// state (h, rpos, kind) after the range
__device__ __forceinline__ void hsum_apply(const HSum &s, int &h, long long &rpos, int &kind)
{
    if (!s.f) return;
    const long long c = s.lc >= 0 ? s.lc : (s.f != h ? s.pf : -1);
    if (c >= 0) { rpos = c; kind = 1; }
    h = s.l;
}
__device__ __forceinline__ int decisive(float x, double t) { return (double)x > t ? 1 : ((double)x < t ? -1 : 0); }

// exclusive scan of HSum over the 256 threads (Hillis-Steele in LDS); returns the composition of threads 0 .. tid-1, *tot = all 256
__device__ HSum hsum_scan_excl(HSum v, HSum *tot, HSum (*sh)[256])
{
    const int tid = threadIdx.x;
    int buf = 0;
    sh[0][tid] = v;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
        HSum a = sh[buf][tid];
        if (tid >= off) a = hsum_compose(sh[buf][tid - off], a);
        sh[buf ^ 1][tid] = a;
        buf ^= 1;
        __syncthreads();
    }
    *tot = sh[buf][255];
    HSum r = tid ? sh[buf][tid - 1] : hsum_empty();
    __syncthreads();
    return r;
}

// exclusive sum and "last defined value" (bit >= 0) over the 256 threads
__device__ void count_scan_excl(unsigned cnt, int bit, unsigned *excl, int *bit_before, unsigned *tot, int *bit_last, unsigned (*sc)[256], int (*sb)[256])
{
    const int tid = threadIdx.x;
    int buf = 0;
    sc[0][tid] = cnt; sb[0][tid] = bit;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
        unsigned c = sc[buf][tid];
        int b = sb[buf][tid];
        if (tid >= off) {
            c += sc[buf][tid - off];
            if (b < 0) b = sb[buf][tid - off];
        }
        sc[buf ^ 1][tid] = c; sb[buf ^ 1][tid] = b;
        buf ^= 1;
        __syncthreads();
    }
    *tot = sc[buf][255]; *bit_last = sb[buf][255];
    *excl = tid ? sc[buf][tid - 1] : 0u;
    *bit_before = tid ? sb[buf][tid - 1] : -1;
    __syncthreads();
}

// ---- F_kind(k): the clock recovery's pulse at k samples after a reset
struct ZcEval {
    int kind;
    unsigned long long k, W;
    double o;
    // o: the offset before sample k is processed
    __device__ void init(const ZcParams &p, int kind_, unsigned long long k_)
    {
        kind = kind_; k = k_;
        W = (unsigned long long)(((unsigned __int128)k * p.U + p.c0[kind]) % p.Pi);     // closed form only; the fallback sets o
        o = 0.0;
    }
    __device__ __forceinline__ void reset(const ZcParams &p)
    {
        kind = 1; k = 0;
        if (p.closed) W = p.c0[1];
        else o = p.P * 0.5;
    }
    __device__ __forceinline__ bool step(const ZcParams &p)
    {
        bool pulse;
        if (p.closed) {
            pulse = (long long)k >= p.ks[kind] && W < p.U;
            W += p.U;
            if (W >= p.Pi) W -= p.Pi;
        } else {
            o = o - 1.0;                                     // zerocrossingclockrecovery.lua:57-66 operation order
            pulse = o < 1.0;
            if (pulse) o = o + p.P;
        }
        k++;
        return pulse;
    }
};

__global__ __launch_bounds__(256) void zc_summary_kernel(const float *__restrict__ x, unsigned long n, double t, HSum *__restrict__ tiles)
{
    __shared__ HSum sh[2][256];
    const unsigned long c0 = (unsigned long)blockIdx.x * DG_TILE + (unsigned long)threadIdx.x * DG_LC;
    HSum s = hsum_empty();
#pragma unroll
    for (int j = 0; j < DG_LC; j++) {
        const unsigned long i = c0 + j;
        const int d = i < n ? decisive(x[i], t) : 0;
        if (d) {
            if (!s.f) { s.f = d; s.pf = (long long)i; }
            else if (d != s.l) s.lc = (long long)i;
            s.l = d;
        }
    }
    HSum tot;
    (void)hsum_scan_excl(s, &tot, sh);
    if (threadIdx.x == 0) tiles[blockIdx.x] = tot;
}

// the literal offset after n more samples (whole-symbol jumps: an offset >= 2 loses floor(o) - 1 integers without a pulse and without rounding)
__device__ double zc_advance(const ZcParams &p, double o, unsigned long long n)
{
    while (n) {
        if (o >= 2.0) {
            const double s = floor(o) - 1.0;
            const unsigned long long m = (double)n < s ? n : (unsigned long long)s;
            o -= (double)m;
            n -= m;
        } else {
            o = o - 1.0;
            if (o < 1.0) o = o + p.P;
            n--;
        }
    }
    return o;
}

// tile starts: hysteresis, last reset position (relative to this call's sample 0; negative: carried), kind.  One workgroup, threads own
// contiguous segments of tiles.  Writes the next call's (k, kind, h) into *so.  Without the closed form thread 0 then carries the literal offset
// from tile start to tile start (t_o) with the clock of the sample before each tile (t_prev): O(call length / P) serial steps, whatever the
// length of the crossing-free stretch the call sits in - the offset at the call's start comes with the carried state (DgState.o).
__global__ __launch_bounds__(256) void zc_carry_kernel(const HSum *__restrict__ tiles, unsigned long ntiles, unsigned long n, ZcParams p,
                                                       const DgState *__restrict__ si, DgState *__restrict__ so,
                                                       int *__restrict__ t_h, long long *__restrict__ t_rpos, int *__restrict__ t_kind,
                                                       double *__restrict__ t_o, int *__restrict__ t_prev)
{
    __shared__ HSum sh[2][256];
    const int tid = threadIdx.x;
    const unsigned long seg = (ntiles + 255) / 256, t0 = tid * seg, t1 = t0 + seg < ntiles ? t0 + seg : ntiles;
    HSum s = hsum_empty();
    for (unsigned long t = t0; t < t1; t++) s = hsum_compose(s, tiles[t]);
    HSum tot;
    const HSum pre = hsum_scan_excl(s, &tot, sh);
    int h = si->h, kind = si->kind;
    long long rpos = -si->k;
    hsum_apply(pre, h, rpos, kind);
    for (unsigned long t = t0; t < t1; t++) {
        t_h[t] = h; t_rpos[t] = rpos; t_kind[t] = kind;
        hsum_apply(tiles[t], h, rpos, kind);
    }
    if (tid == 0) {
        int hh = si->h, kk = si->kind;
        long long rp = -si->k;
        hsum_apply(tot, hh, rp, kk);
        so->h = hh; so->kind = kk; so->k = (long long)n - rp;
    }
    if (p.closed) return;
    __threadfence_block();
    __syncthreads();
    if (tid) return;
    double o = si->o;
    t_o[0] = o; t_prev[0] = si->prev;
    for (unsigned long t = 1; t < ntiles; t++) {
        const long long ts = (long long)t * DG_TILE;
        // the offset before sample ts - 1 of its segment, then that sample
        if (t_rpos[t] == t_rpos[t - 1] && t_kind[t] == t_kind[t - 1]) o = zc_advance(p, o, DG_TILE - 1);
        else o = ts - 1 == t_rpos[t] ? p.P * 0.5 : zc_advance(p, p.P * 0.5, (unsigned long long)(ts - 1 - t_rpos[t]));
        o = o - 1.0;
        const bool pulse = o < 1.0;
        if (pulse) o = o + p.P;
        t_o[t] = o; t_prev[t] = pulse ? 1 : 0;
    }
}

// ZC = 0: the clock stream itself (+1 / -1 per sample), written in place.  ZC = 1: clocksampler - the emitted samples (Float32, or the sliced
// bit) go to the tile's own slot of the staging buffer (DG_TILE / 2 entries: a rising edge needs a sample without pulse before it), with the
// tile's count and last sliced bit; dg_compact_kernel packs them.  The thread's samples are loaded once and walked from registers.
template <int ZC>
__global__ __launch_bounds__(256) void zc_emit_kernel(const float *__restrict__ x, unsigned long n, ZcParams p, DgTail tail, void *__restrict__ y,
                                                      const DgState *__restrict__ si, DgState *__restrict__ so,
                                                      const int *__restrict__ t_h, const long long *__restrict__ t_rpos, const int *__restrict__ t_kind,
                                                      const double *__restrict__ t_o, const int *__restrict__ t_prev,
                                                      unsigned *__restrict__ t_cnt, int *__restrict__ t_bit)
{
    __shared__ HSum sh[2][256];
    __shared__ unsigned sc[2][256];
    __shared__ int sb[2][256];
    const unsigned b = blockIdx.x;
    const unsigned long ts = (unsigned long)b * DG_TILE, c0 = ts + (unsigned long)threadIdx.x * DG_LC;
    float xv[DG_LC];
    HSum s = hsum_empty();
#pragma unroll
    for (int j = 0; j < DG_LC; j++) {
        const unsigned long i = c0 + j;
        xv[j] = i < n ? x[i] : 0.f;
        const int d = i < n ? decisive(xv[j], p.T) : 0;
        if (d) {
            if (!s.f) { s.f = d; s.pf = (long long)i; }
            else if (d != s.l) s.lc = (long long)i;
            s.l = d;
        }
    }
    HSum tot;
    const HSum pre = hsum_scan_excl(s, &tot, sh);
    int h = t_h[b], kind = t_kind[b];
    long long rpos = t_rpos[b];
    hsum_apply(pre, h, rpos, kind);
    const bool in_tile_reset = !(rpos == t_rpos[b] && kind == t_kind[b]);
    ZcEval ev;
    int prev = 0;
    if (c0 < n) {
        if (p.closed) {
            if (c0 == 0) { ev.init(p, kind, (unsigned long long)(-rpos)); prev = si->prev; }
            else { ev.init(p, kind, (unsigned long long)((long long)c0 - 1 - rpos)); prev = ev.step(p) ? 1 : 0; }
        } else {
            ev.kind = kind; ev.k = 0; ev.W = 0;
            if (c0 == ts) { ev.o = t_o[b]; prev = t_prev[b]; }
            else {
                ev.o = in_tile_reset ? ((long long)c0 - 1 == rpos ? p.P * 0.5 : zc_advance(p, p.P * 0.5, (unsigned long long)((long long)c0 - 1 - rpos)))
                                     : zc_advance(p, t_o[b], c0 - 1 - ts);
                prev = ev.step(p) ? 1 : 0;
            }
        }
    }
    if (ZC == 0) {
        if (c0 >= n) return;
#pragma unroll
        for (int j = 0; j < DG_LC; j++) {
            const unsigned long i = c0 + j;
            if (i >= n) break;
            const int d = decisive(xv[j], p.T);
            if (d && d != h) { h = d; ev.reset(p); }
            const bool pulse = ev.step(p);
            ((float *)y)[i] = pulse ? 1.f : -1.f;
            if (i == n - 1) { so->prev = pulse ? 1 : 0; so->o = ev.o; }
        }
        return;
    }
    // count, scan, then the same walk again from the saved state to store
    const ZcEval ev0 = ev;
    const int h0 = h, prev0 = prev;
    unsigned cnt = 0;
    int bit = -1;
#pragma unroll
    for (int j = 0; j < DG_LC; j++) {
        const unsigned long i = c0 + j;
        if (i >= n) break;
        const int d = decisive(xv[j], p.T);
        if (d && d != h) { h = d; ev.reset(p); }
        const int pulse = ev.step(p) ? 1 : 0;
        if (pulse && !prev) { cnt++; bit = (double)xv[j] > tail.slice_t ? 1 : 0; }
        prev = pulse;
        if (i == n - 1) { so->prev = pulse; so->o = ev.o; }
    }
    unsigned ex, tcnt;
    int bb, bl;
    count_scan_excl(cnt, bit, &ex, &bb, &tcnt, &bl, sc, sb);
    if (threadIdx.x == 0) { t_cnt[b] = tcnt; t_bit[b] = bl; }
    if (!cnt) return;
    ev = ev0; h = h0; prev = prev0;
    const unsigned long base = (unsigned long)b * (DG_TILE / 2);
    unsigned o = ex;
#pragma unroll
    for (int j = 0; j < DG_LC; j++) {
        const unsigned long i = c0 + j;
        if (i >= n) break;
        const int d = decisive(xv[j], p.T);
        if (d && d != h) { h = d; ev.reset(p); }
        const int pulse = ev.step(p) ? 1 : 0;
        if (pulse && !prev && o < DG_TILE / 2) {
            if (tail.out == DG_OUT_FLOAT) ((float *)y)[base + o] = xv[j];
            else ((uint8_t *)y)[base + o] = (double)xv[j] > tail.slice_t ? 1 : 0;                 // slicer.lua
            o++;
        }
        prev = pulse;
    }
}

// pack the tiles' staged outputs: each workgroup owns a run of tiles, sums the counts of the tiles before it (and finds the last sliced bit
// before it), then copies - applying the differential decoder (differentialdecoder.lua) across its tiles.  The last group writes the call's count.
template <int OUT>
__global__ __launch_bounds__(256) void dg_compact_kernel(const void *__restrict__ stage, const unsigned *__restrict__ t_cnt, const int *__restrict__ t_bit,
                                                         unsigned long ntiles, unsigned long per, DgTail tail, void *__restrict__ y, unsigned long cap,
                                                         const DgState *__restrict__ si, DgState *__restrict__ so)
{
    __shared__ unsigned long long ssum[256];
    __shared__ long long slast[256];
    const int tid = threadIdx.x;
    const unsigned long g0 = (unsigned long)blockIdx.x * per, g1 = g0 + per < ntiles ? g0 + per : ntiles;
    unsigned long long c = 0;
    long long last = -1;
    for (unsigned long t = tid; t < g0; t += 256) {
        c += t_cnt[t];
        if (t_bit[t] >= 0) last = (long long)t;
    }
    ssum[tid] = c; slast[tid] = last;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (tid < off) {
            ssum[tid] += ssum[tid + off];
            if (slast[tid + off] > slast[tid]) slast[tid] = slast[tid + off];
        }
        __syncthreads();
    }
    unsigned long long o = ssum[0];
    int prev = slast[0] >= 0 ? t_bit[slast[0]] : si->bit;
    for (unsigned long t = g0; t < g1; t++) {
        const unsigned ct = t_cnt[t];
        const unsigned long base = t * (DG_TILE / 2);
        for (unsigned j = tid; j < ct; j += 256) {
            if (o + j >= cap) break;
            if (OUT == DG_OUT_FLOAT) ((float *)y)[o + j] = ((const float *)stage)[base + j];
            else {
                const uint8_t *sb = (const uint8_t *)stage + base;
                const int bv = sb[j];
                if (OUT == DG_OUT_SLICE) ((uint8_t *)y)[o + j] = (uint8_t)bv;
                else {
                    const int pb = j ? sb[j - 1] : prev;
                    ((uint8_t *)y)[o + j] = (uint8_t)(tail.invert ? (((pb ^ bv) + 1) & 1) : (pb ^ bv));
                }
            }
        }
        if (ct && OUT != DG_OUT_FLOAT) prev = ((const uint8_t *)stage)[base + ct - 1];
        o += ct;
    }
    if (g1 == ntiles && tid == 0) { so->count = o; so->bit = prev; }
}

// ---- SamplerBlock on its own: summary of the clock = first / last decisive sign and the rising edges inside
struct SSum { int f, l; unsigned long long r; };
__device__ __forceinline__ SSum ssum_compose(const SSum &a, const SSum &b)
{
    if (!a.f) return SSum{b.f, b.l, a.r + b.r};
    if (!b.f) return SSum{a.f, a.l, a.r + b.r};
    return SSum{a.f, b.l, a.r + b.r + ((a.l < 0 && b.f > 0) ? 1ull : 0ull)};
}
// emissions of the range entered in state h, and the state after it
__device__ __forceinline__ unsigned long long ssum_count(const SSum &s, int h) { return s.r + ((s.f > 0 && h < 0) ? 1ull : 0ull); }
__device__ __forceinline__ int ssum_state(const SSum &s, int h) { return s.f ? s.l : h; }

__device__ SSum ssum_scan_excl(SSum v, SSum *tot, SSum (*sh)[256])
{
    const int tid = threadIdx.x;
    int buf = 0;
    sh[0][tid] = v;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
        SSum a = sh[buf][tid];
        if (tid >= off) a = ssum_compose(sh[buf][tid - off], a);
        sh[buf ^ 1][tid] = a;
        buf ^= 1;
        __syncthreads();
    }
    *tot = sh[buf][255];
    SSum r = tid ? sh[buf][tid - 1] : SSum{0, 0, 0ull};
    __syncthreads();
    return r;
}
__device__ __forceinline__ SSum sampler_thread_sum(const float *__restrict__ clk, unsigned long n, unsigned long c0)
{
    SSum s{0, 0, 0ull};
#pragma unroll
    for (int j = 0; j < DG_LC; j++) {
        const unsigned long i = c0 + j;
        const int d = i < n ? decisive(clk[i], 0.0) : 0;
        if (d) {
            if (!s.f) s.f = d;
            else if (s.l < 0 && d > 0) s.r++;
            s.l = d;
        }
    }
    return s;
}

__global__ __launch_bounds__(256) void sampler_summary_kernel(const float *__restrict__ clk, unsigned long n, SSum *__restrict__ tiles)
{
    __shared__ SSum sh[2][256];
    SSum tot;
    (void)ssum_scan_excl(sampler_thread_sum(clk, n, (unsigned long)blockIdx.x * DG_TILE + (unsigned long)threadIdx.x * DG_LC), &tot, sh);
    if (threadIdx.x == 0) tiles[blockIdx.x] = tot;
}

__global__ __launch_bounds__(256) void sampler_carry_kernel(const SSum *__restrict__ tiles, unsigned long ntiles, const DgState *__restrict__ si,
                                                            DgState *__restrict__ so, int *__restrict__ t_h, unsigned long long *__restrict__ t_off)
{
    __shared__ SSum sh[2][256];
    const int tid = threadIdx.x;
    const unsigned long seg = (ntiles + 255) / 256, t0 = tid * seg, t1 = t0 + seg < ntiles ? t0 + seg : ntiles;
    SSum s{0, 0, 0ull};
    for (unsigned long t = t0; t < t1; t++) s = ssum_compose(s, tiles[t]);
    SSum tot;
    const SSum pre = ssum_scan_excl(s, &tot, sh);
    int h = ssum_state(pre, si->h);
    unsigned long long off = ssum_count(pre, si->h);
    for (unsigned long t = t0; t < t1; t++) {
        t_h[t] = h; t_off[t] = off;
        off += ssum_count(tiles[t], h);
        h = ssum_state(tiles[t], h);
    }
    if (tid == 0) { so->count = ssum_count(tot, si->h); so->h = ssum_state(tot, si->h); }
}

// S = 1: Float32 data, 2: ComplexFloat32 data
template <int S>
__global__ __launch_bounds__(256) void sampler_final_kernel(const float *__restrict__ data, const float *__restrict__ clk, unsigned long n, float *__restrict__ y,
                                                            unsigned long cap, const int *__restrict__ t_h, const unsigned long long *__restrict__ t_off)
{
    __shared__ SSum sh[2][256];
    const unsigned long c0 = (unsigned long)blockIdx.x * DG_TILE + (unsigned long)threadIdx.x * DG_LC;
    SSum tot;
    const SSum pre = ssum_scan_excl(sampler_thread_sum(clk, n, c0), &tot, sh);
    const int h0 = t_h[blockIdx.x];
    int h = ssum_state(pre, h0);
    unsigned long long o = t_off[blockIdx.x] + ssum_count(pre, h0);
#pragma unroll
    for (int j = 0; j < DG_LC; j++) {
        const unsigned long i = c0 + j;
        if (i >= n) break;
        const int d = decisive(clk[i], 0.0);
        if (d > 0 && h < 0) {                            // sampler.lua:42-45
            if (o < cap)
#pragma unroll
                for (int c = 0; c < S; c++) y[o * S + c] = data[i * S + c];
            o++;
        }
        if (d) h = d;
    }
}

// ---- SlicerBlock, DifferentialDecoderBlock: element-wise
__global__ __launch_bounds__(256) void slicer_kernel(const float *__restrict__ x, uint8_t *__restrict__ y, unsigned long n, double t)
{
    const unsigned long i = (unsigned long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) y[i] = (double)x[i] > t ? 1 : 0;
}
// prev = the previous input byte (state[cur] for sample 0); the last input byte goes to *prev_out
__global__ __launch_bounds__(256) void diffdec_kernel(const uint8_t *__restrict__ x, uint8_t *__restrict__ y, unsigned long n, int invert,
                                                      const uint8_t *__restrict__ prev_in, uint8_t *__restrict__ prev_out)
{
    const unsigned long i = (unsigned long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int prev = i ? x[i - 1] : *prev_in, v = prev ^ x[i];
    y[i] = (uint8_t)(invert ? (v + 1) % 2 : v);
    if (i == n - 1) *prev_out = x[i];
}

}  // namespace lrhip
