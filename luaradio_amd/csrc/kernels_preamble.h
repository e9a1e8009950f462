// kernels_preamble.h - PreambleSamplerBlock (radio/blocks/signal/preamblesampler.lua:49-138) and ManchesterDecoderBlock
// (manchesterdecoder.lua:31-61): the two remaining PLL-free blocks between a matched filter and a framer.
//
// PreambleSampler.  T = symbol period, L = preamble length, N = samples per frame, B = 2^ceil_log2(T L + 1) the reference's circular buffer.
// x[i] is the stream by absolute index (0 before the start: the buffer starts as zeros).  After sample i is shifted in, tap k of the
// reference's compute_energy() (:64-80) reads v_k(i) = x[i + 2 - B + k T]  (:68 with the increment at :88).  Two predicates of a window:
//   M(i)  every (v_k(i) > 0) equals preamble[k]                      (NaN, -0.0 and 0.0 give bit 0, as `value > 0` does)
//   E(i)  sum over k = 0, 1, ... of |v_k(i)| in double, in that order
//   D(j)  !M(j) || E(j) < E(j-1)   - in OPTIMIZING the saved energy is always the previous sample's, so "degraded" is local
// and the automaton only hops: from a search position s,  i* = first i >= s with M(i),  j* = first j > i* with D(j), the frame emits
// x[j* + 1 - B + m T] (m = 0 .. N-1), output 0 AT sample j* and output m >= 1 at sample j* + m T - 1, and the search resumes at
// s' = j* + (N - 1) T.  A call emits the outputs whose emission sample lies inside it.
//
// Passes (3 launches, one count read-back):
//   ps_match_kernel  one thread per sample: M and D as bit masks (one 64-bit word per wave) and per-tile (PS_TILE samples) summaries
//                    "first M" / "first D".  A lane stops reading at its first mismatch and the tap loop stops wave-wide once no lane still
//                    matches; E(i) and E(i-1) are summed only by the lanes whose M holds.  For each k adjacent lanes read adjacent
//                    addresses.  Traffic: 4 B per sample and tap actually read (the taps of one sample are T samples apart, so nothing is
//                    shared between them; other waves re-read the same lines from L2) - on random signs two taps per lane, 8 B per sample,
//                    while a wave of 64 stays in the loop for about seven taps.
//   ps_walk_kernel   ONE workgroup hops from frame to frame.  "first set bit at or after p" (ps_find_first, kernels_bitscan.h) scans the mask words of p's tile (16 lanes, one
//                    word each) and from the next tile on the tile summaries, 256 tiles per step by the whole workgroup.  Serial cost: one hop (two searches of two barriers and one round of loads each, about 2 us) per frame
//                    plus O(tiles / 256) search steps in total - a stretch without a match or a long non-degrading run costs
//                    tiles / 256 steps, not samples.  Writes the frame list (j*, output base, first m, last m inside this call), the
//                    count and the next call's state.
//   ps_emit_kernel   frames x N gathers of x[j* + 1 - B + m T] into the packed output, and the next call's history (the last B samples).
// Carried between calls, ping-pong on the device: the last B input samples - the reference's buffer; they hold every window and every
// emitted sample a call can reach back to - and PsState.
//
// ManchesterDecoder.  Three states (nothing pending, a 0 pending, a 1 pending); every input bit is a map of the state that may emit one bit.
// The maps compose (MSum: exit state and emissions for each of the three entry states), so: md_summary_kernel (per tile),
// md_carry_kernel (one workgroup: entry state and output offset of every tile), md_final_kernel (each thread replays its DG_LC bits from
// its entry state and stores at its offset - the output comes out packed).  3 launches, one count read-back.
#pragma once
#include "common.h"
#include "kernels_digital.h"
#include "kernels_bitscan.h"

namespace lrhip {

enum { PS_SEARCHING = 0, PS_OPTIMIZING = 1, PS_SAMPLING = 2 };

struct PsParams {
    int T, L, N;
    long long B;
};

// carried between calls (ping-pong on the device).  A frame that ends inside a call leaves SEARCHING from the next call's sample 0 at the
// latest (s' <= n: the last output is emitted at s' - 1).
struct PsState {
    int mode;
    int m_next;                      // SAMPLING: the next output of the frame in progress
    long long j;                     // SAMPLING: j* relative to the next call's sample 0 (negative)
    unsigned long long count;        // outputs of the last call
    unsigned long long frames;       // frame list entries of the last call
    int overflow;                    // the frame list or the output capacity was too small (never, by the bounds of PsStage)
    int pad;
};

struct PsFrame {
    long long j;                     // j* relative to this call's sample 0
    unsigned long long base;         // index of output m0 in the call's output
    int m0, m1;                      // outputs m0 .. m1 are emitted inside this call
};

// x by call-relative index i >= -B: the call's input, or the carried history (hist[q] = x[q - B])
__device__ __forceinline__ float ps_load(const float *__restrict__ x, const float *__restrict__ hist, long long B, long long i)
{
    return i >= 0 ? x[i] : hist[i + B];
}

__global__ __launch_bounds__(256) void ps_match_kernel(const float *__restrict__ x, const float *__restrict__ hist, unsigned long n, PsParams p,
                                                       const uint32_t *__restrict__ pre, unsigned long long *__restrict__ mask_m,
                                                       unsigned long long *__restrict__ mask_d, int *__restrict__ tile_m, int *__restrict__ tile_d)
{
    __shared__ int first_m, first_d;
    if (threadIdx.x == 0) { first_m = PS_TILE; first_d = PS_TILE; }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll 1
    for (int r = 0; r < PS_TILE / 256; r++) {
        const int in_tile = r * 256 + (int)threadIdx.x;
        const unsigned long i = (unsigned long)blockIdx.x * PS_TILE + (unsigned long)in_tile;
        const long long base = (long long)i + 2 - p.B;
        bool alive = i < n;
        for (int k = 0; k < p.L; k++) {
            if (!__any(alive)) break;
            if (alive) {
                const float v = ps_load(x, hist, p.B, base + (long long)k * p.T);
                const int bit = v > 0.f ? 1 : 0;
                alive = bit == (int)((pre[k >> 5] >> (k & 31)) & 1u);
            }
        }
        bool d = i < n;                                  // !M(i): degraded
        if (alive) {
            double e = 0.0, ep = 0.0;
            for (int k = 0; k < p.L; k++) {
                const long long a = base + (long long)k * p.T;
                e = e + fabs((double)ps_load(x, hist, p.B, a));
                ep = ep + fabs((double)ps_load(x, hist, p.B, a - 1));
            }
            d = e < ep;                                  // false when either is NaN, as `energy < self.preamble_energy` is
        }
        const unsigned long long bm = __ballot(alive), bd = __ballot(d);
        if (lane == 0) {
            const unsigned long w = (unsigned long)blockIdx.x * PS_WORDS + (unsigned long)(r * 4 + wave);
            mask_m[w] = bm;
            mask_d[w] = bd;
            if (bm) atomicMin(&first_m, r * 256 + wave * 64 + __ffsll((long long)bm) - 1);
            if (bd) atomicMin(&first_d, r * 256 + wave * 64 + __ffsll((long long)bd) - 1);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        tile_m[blockIdx.x] = first_m < PS_TILE ? first_m : -1;
        tile_d[blockIdx.x] = first_d < PS_TILE ? first_d : -1;
    }
}

__global__ __launch_bounds__(256) void ps_walk_kernel(const unsigned long long *__restrict__ mask_m, const unsigned long long *__restrict__ mask_d,
                                                      const int *__restrict__ tile_m, const int *__restrict__ tile_d, unsigned long ntiles,
                                                      unsigned long n, PsParams p, const PsState *__restrict__ si, PsState *__restrict__ so,
                                                      PsFrame *__restrict__ frames, unsigned long max_frames, unsigned long cap)
{
    __shared__ unsigned long long s_res;
    const long long nn = (long long)n;
    int mode = si->mode, m_next = si->m_next;
    long long j = si->j, s = 0;
    unsigned long long count = 0, nframes = 0;
    int overflow = 0;
    // every thread runs the same automaton on the same values; thread 0 writes
    for (;;) {
        if (mode == PS_SEARCHING) {
            if (s >= nn) break;
            const long long i = ps_find_first(mask_m, tile_m, ntiles, s, &s_res);
            if (i == PS_NONE) break;
            mode = PS_OPTIMIZING;
            s = i + 1;
        }
        if (mode == PS_OPTIMIZING) {
            if (s >= nn) break;
            const long long jj = ps_find_first(mask_d, tile_d, ntiles, s, &s_res);
            if (jj == PS_NONE) break;
            mode = PS_SAMPLING;
            j = jj;
            m_next = 0;
        }
        // SAMPLING: output 0 at sample j, output m >= 1 at sample j + m T - 1 - inside this call while m T <= n - j
        long long m1 = (nn - j) / p.T;
        if (m1 > p.N - 1) m1 = p.N - 1;
        if (m1 >= m_next) {
            const unsigned long long cnt = (unsigned long long)(m1 - m_next + 1);
            if (nframes >= max_frames || count + cnt > cap) { overflow = 1; break; }
            if (threadIdx.x == 0) frames[nframes] = PsFrame{j, count, m_next, (int)m1};
            nframes++;
            count += cnt;
            m_next = (int)m1 + 1;
        }
        if (m_next < p.N) break;                         // the frame goes on in the next call
        mode = PS_SEARCHING;
        s = j + (long long)(p.N - 1) * p.T;              // <= n
    }
    if (threadIdx.x == 0) {
        so->mode = mode;
        so->m_next = mode == PS_SAMPLING ? m_next : 0;
        so->j = mode == PS_SAMPLING ? j - nn : 0;
        so->count = count;
        so->frames = nframes;
        so->overflow = overflow;
        so->pad = 0;
    }
}

// one wave per frame (grid-stride), then the next call's history
__global__ __launch_bounds__(64) void ps_emit_kernel(const float *__restrict__ x, const float *__restrict__ hist, float *__restrict__ hist_out,
                                                     unsigned long n, PsParams p, const PsState *__restrict__ so,
                                                     const PsFrame *__restrict__ frames, float *__restrict__ y, unsigned long cap)
{
    const unsigned long long nframes = so->overflow ? 0ull : so->frames;
    for (unsigned long long f = blockIdx.x; f < nframes; f += gridDim.x) {
        const PsFrame fr = frames[f];
        for (int m = fr.m0 + (int)threadIdx.x; m <= fr.m1; m += 64) {
            const unsigned long long o = fr.base + (unsigned long long)(m - fr.m0);
            if (o < cap) y[o] = ps_load(x, hist, p.B, fr.j + 1 - p.B + (long long)m * p.T);
        }
    }
    const long long nn = (long long)n;
    for (long long q = (long long)blockIdx.x * 64 + threadIdx.x; q < p.B; q += (long long)gridDim.x * 64)
        hist_out[q] = ps_load(x, hist, p.B, nn - p.B + q);
}

// ---- ManchesterDecoderBlock.  States: 0 nothing pending, 1 a 0 pending, 2 a 1 pending.
struct MSum {
    unsigned to;                     // exit state for entry state s in bits 2s, 2s + 1
    unsigned long long c[3];         // emissions for entry state s
};
__device__ __forceinline__ MSum msum_identity() { return MSum{0u | (1u << 2) | (2u << 4), {0ull, 0ull, 0ull}}; }
__device__ __forceinline__ int msum_to(const MSum &a, int s) { return (int)((a.to >> (2 * s)) & 3u); }
__device__ __forceinline__ MSum msum_compose(const MSum &a, const MSum &b)
{
    MSum r;
    r.to = 0;
#pragma unroll
    for (int s = 0; s < 3; s++) {
        const int mid = msum_to(a, s);
        r.to |= (unsigned)msum_to(b, mid) << (2 * s);
        r.c[s] = a.c[s] + b.c[mid];
    }
    return r;
}
// one input bit from state s: manchesterdecoder.lua:39-54.  Returns the new state; *emit = the pending bit when a transition completes, else -1
__device__ __forceinline__ int md_step(int s, int b, int *emit)
{
    *emit = -1;
    if (s == 0 || s - 1 == b) return 1 + b;              // nothing pending, or an equal pair (clock slip): the newer bit stays pending
    *emit = s - 1;                                       // 0,1 emits 0 and 1,0 emits 1
    return 0;
}
__device__ __forceinline__ MSum md_thread_sum(const uint8_t *__restrict__ x, unsigned long n, unsigned long c0)
{
    int st[3] = {0, 1, 2};
    unsigned c[3] = {0, 0, 0};
#pragma unroll
    for (int q = 0; q < DG_LC; q++) {
        const unsigned long i = c0 + q;
        if (i >= n) break;
        const int b = x[i] & 1;
#pragma unroll
        for (int s = 0; s < 3; s++) {
            int e;
            st[s] = md_step(st[s], b, &e);
            c[s] += e >= 0 ? 1u : 0u;
        }
    }
    return MSum{(unsigned)st[0] | ((unsigned)st[1] << 2) | ((unsigned)st[2] << 4), {c[0], c[1], c[2]}};
}
__device__ MSum msum_scan_excl(MSum v, MSum *tot, MSum (*sh)[256])
{
    const int tid = threadIdx.x;
    int buf = 0;
    sh[0][tid] = v;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
        MSum a = sh[buf][tid];
        if (tid >= off) a = msum_compose(sh[buf][tid - off], a);
        sh[buf ^ 1][tid] = a;
        buf ^= 1;
        __syncthreads();
    }
    *tot = sh[buf][255];
    MSum r = tid ? sh[buf][tid - 1] : msum_identity();
    __syncthreads();
    return r;
}

// carried between calls (ping-pong on the device)
struct MdState {
    int pending;                     // 0 nothing, 1 a 0, 2 a 1
    int pad;
    unsigned long long count;        // outputs of the last call
};

__global__ __launch_bounds__(256) void md_summary_kernel(const uint8_t *__restrict__ x, unsigned long n, MSum *__restrict__ tiles)
{
    __shared__ MSum sh[2][256];
    MSum tot;
    (void)msum_scan_excl(md_thread_sum(x, n, (unsigned long)blockIdx.x * DG_TILE + (unsigned long)threadIdx.x * DG_LC), &tot, sh);
    if (threadIdx.x == 0) tiles[blockIdx.x] = tot;
}

__global__ __launch_bounds__(256) void md_carry_kernel(const MSum *__restrict__ tiles, unsigned long ntiles, const MdState *__restrict__ si,
                                                       MdState *__restrict__ so, int *__restrict__ t_state, unsigned long long *__restrict__ t_off)
{
    __shared__ MSum sh[2][256];
    const int tid = threadIdx.x;
    const unsigned long seg = (ntiles + 255) / 256, t0 = tid * seg, t1 = t0 + seg < ntiles ? t0 + seg : ntiles;
    MSum s = msum_identity();
    for (unsigned long t = t0; t < t1; t++) s = msum_compose(s, tiles[t]);
    MSum tot;
    const MSum pre = msum_scan_excl(s, &tot, sh);
    const int s0 = si->pending;
    int st = msum_to(pre, s0);
    unsigned long long off = pre.c[s0];
    for (unsigned long t = t0; t < t1; t++) {
        t_state[t] = st; t_off[t] = off;
        off += tiles[t].c[st];
        st = msum_to(tiles[t], st);
    }
    if (tid == 0) { so->pending = msum_to(tot, s0); so->pad = 0; so->count = tot.c[s0]; }
}

__global__ __launch_bounds__(256) void md_final_kernel(const uint8_t *__restrict__ x, unsigned long n, int invert, uint8_t *__restrict__ y, unsigned long cap,
                                                       const int *__restrict__ t_state, const unsigned long long *__restrict__ t_off)
{
    __shared__ MSum sh[2][256];
    const unsigned long c0 = (unsigned long)blockIdx.x * DG_TILE + (unsigned long)threadIdx.x * DG_LC;
    MSum tot;
    const MSum pre = msum_scan_excl(md_thread_sum(x, n, c0), &tot, sh);
    const int s0 = t_state[blockIdx.x];
    int st = msum_to(pre, s0);
    unsigned long long o = t_off[blockIdx.x] + pre.c[s0];
#pragma unroll
    for (int q = 0; q < DG_LC; q++) {
        const unsigned long i = c0 + q;
        if (i >= n) break;
        int e;
        st = md_step(st, x[i] & 1, &e);
        if (e >= 0) {
            if (o < cap) y[o] = (uint8_t)(e ^ invert);
            o++;
        }
    }
}

}  // namespace lrhip
