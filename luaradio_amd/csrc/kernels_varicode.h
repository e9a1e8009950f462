// kernels_varicode.h - VaricodeDecoderBlock (radio/blocks/protocol/varicodedecoder.lua:61-87): Bit -> Byte, the characters of a PSK31 bit stream.
//
// The reference's loop is a segmentation automaton of 21 states (the state's length and whether its last byte is 0, varicode_plan.h) and, at
// each 00 delimiter, a table lookup of the bytes in front of it.  The bytes are not state - they are read from the stream, "the carried bytes,
// then the call's" (BsStream) - so every input byte is a map of the 21 states, and the maps compose, as the Manchester decoder's do
// (kernels_preamble.h).  They have to be composed: the entry states need not converge (on a run of ones 11 of them stay distinct for ever), so
// starting a few bytes early is not an option.
//
// A map with one emission count per entry state would be about 100 bytes per thread, and the count for a hypothetical entry state needs the
// lookups of that state.  So the states are scanned alone (a map is 21 x 5 bits, two 64-bit words) and the characters are counted afterwards,
// from the true entry states only, with an ordinary prefix sum.  Passes (tile = 256 threads x DG_LC bytes), 5 launches, one count read-back:
//   vc_summary_kernel  the composed map of every tile
//   vc_carry_kernel    ONE workgroup: the entry state of every tile from the carried state (256 tiles per step), the next call's state length
//                      and its bytes (the last `len` bytes of the stream)
//   vc_count_kernel    every thread's true entry state (the tile's maps scanned again, entered at the tile's state), its characters counted by
//                      replaying its bytes, their prefix sum inside the tile; per thread "entry state, offset in the tile", per tile the count
//   vc_offsets_kernel  ONE workgroup: the prefix sum of the tile counts, and the call's count
//   vc_final_kernel    each thread replays its bytes from its entry state and stores its characters at its offset - the output comes out packed
// Serial work: O(tiles / 256) per thread in the two one-workgroup kernels, whatever the data holds.  A delimiter whose code reaches back before
// the thread's chunk, the tile or the call reads the stream there: at most 9 bytes back, at most `len` of them carried.
#pragma once
#include "common.h"
#include "kernels_digital.h"
#include "kernels_bitscan.h"
#include "varicode_plan.h"

namespace lrhip {

__constant__ VcTable VC_TABLE = vc_make_table();

// carried between calls (ping-pong on the device), with the state's bytes (VC_MAX_LEN of them) beside it
struct VcState {
    int len;                         // entries of the reference's `state`, 0 .. 10
    int pad;
    unsigned long long count;        // outputs of the last call
};

__device__ __forceinline__ int vc_entry_state(const VcState *__restrict__ si, const uint8_t *__restrict__ carried)
{
    const int len = si->len;
    return vc_state(len, len > 0 && carried[len - 1] == 0);
}

// the thread's DG_LC bytes from c0 on: which of them equal 0, and how many there are
__device__ __forceinline__ unsigned vc_chunk_zeros(const uint8_t *__restrict__ x, unsigned long n, unsigned long c0, int *count)
{
    unsigned zeros = 0;
    int k = 0;
    for (; k < DG_LC && c0 + k < n; k++) zeros |= (x[c0 + k] == 0 ? 1u : 0u) << k;
    *count = k;
    return zeros;
}

// exclusive scan over the 256 threads of a workgroup: of maps under composition, and of counts under addition
__device__ VcMap vc_scan_excl(VcMap v, VcMap *tot, VcMap (*sh)[256])
{
    const int tid = threadIdx.x;
    int buf = 0;
    sh[0][tid] = v;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
        VcMap a = sh[buf][tid];
        if (tid >= off) a = vc_map_compose(sh[buf][tid - off], a);
        sh[buf ^ 1][tid] = a;
        buf ^= 1;
        __syncthreads();
    }
    *tot = sh[buf][255];
    const VcMap r = tid ? sh[buf][tid - 1] : vc_map_identity();
    __syncthreads();
    return r;
}
__device__ unsigned long long vc_sum_excl(unsigned long long v, unsigned long long *tot, unsigned long long (*sh)[256])
{
    const int tid = threadIdx.x;
    int buf = 0;
    sh[0][tid] = v;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
        unsigned long long a = sh[buf][tid];
        if (tid >= off) a += sh[buf][tid - off];
        sh[buf ^ 1][tid] = a;
        buf ^= 1;
        __syncthreads();
    }
    *tot = sh[buf][255];
    const unsigned long long r = tid ? sh[buf][tid - 1] : 0ull;
    __syncthreads();
    return r;
}

__global__ __launch_bounds__(256) void vc_summary_kernel(const uint8_t *__restrict__ x, unsigned long n, VcMap *__restrict__ tiles)
{
    __shared__ VcMap sh[2][256];
    int count;
    const unsigned zeros = vc_chunk_zeros(x, n, (unsigned long)blockIdx.x * DG_TILE + (unsigned long)threadIdx.x * DG_LC, &count);
    VcMap tot;
    (void)vc_scan_excl(vc_map_of(zeros, count), &tot, sh);
    if (threadIdx.x == 0) tiles[blockIdx.x] = tot;
}

__global__ __launch_bounds__(256) void vc_carry_kernel(const VcMap *__restrict__ tiles, unsigned long ntiles, const uint8_t *__restrict__ x, unsigned long n,
                                                       const VcState *__restrict__ si, const uint8_t *__restrict__ ci, VcState *__restrict__ so,
                                                       uint8_t *__restrict__ co, int *__restrict__ t_state)
{
    __shared__ VcMap sh[2][256];
    const int tid = threadIdx.x;
    const unsigned long seg = (ntiles + 255) / 256, t0 = tid * seg, t1 = t0 + seg < ntiles ? t0 + seg : ntiles;
    VcMap s = vc_map_identity();
    for (unsigned long t = t0; t < t1; t++) s = vc_map_compose(s, tiles[t]);
    VcMap tot;
    const VcMap pre = vc_scan_excl(s, &tot, sh);
    const int s0 = vc_entry_state(si, ci);
    int st = vc_map_to(pre, s0);
    for (unsigned long t = t0; t < t1; t++) {
        t_state[t] = st;
        st = vc_map_to(tiles[t], st);
    }
    // the state's entries are the last `len` bytes of the stream (len <= carried + n: they were appended one by one)
    const int carry = si->len, len = vc_len(vc_map_to(tot, s0));
    const BsStream in{x, ci, carry};
    if (tid < len) co[tid] = (uint8_t)in((long long)carry + (long long)n - len + tid);
    if (tid == 0) { so->len = len; so->pad = 0; }
}

// The thread's bytes replayed from state st; byte q of the chunk is byte u0 + q of the stream.  STORE: the characters go to y from o on;
// returns the number of characters.
template <bool STORE>
__device__ __forceinline__ unsigned vc_replay(const BsStream &in, long long u0, unsigned zeros, int count, int st, uint8_t *__restrict__ y, unsigned long long o,
                                              unsigned long cap)
{
    unsigned emitted = 0;
    for (int q = 0; q < count; q++) {
        int L;
        st = vc_step(st, (zeros >> q) & 1u, &L);
        if (L) {
            const int ch = vc_lookup(in, u0 + q, L, VC_TABLE.ch);
            if (ch != VC_NONE) {
                if (STORE && o + emitted < cap) y[o + emitted] = (uint8_t)ch;
                emitted++;
            }
        }
    }
    return emitted;
}

__global__ __launch_bounds__(256) void vc_count_kernel(const uint8_t *__restrict__ x, unsigned long n, const VcState *__restrict__ si,
                                                       const uint8_t *__restrict__ ci, const int *__restrict__ t_state, unsigned *__restrict__ t_cnt,
                                                       unsigned *__restrict__ t_thread)
{
    __shared__ VcMap sh[2][256];
    __shared__ unsigned long long sc[2][256];
    const unsigned long c0 = (unsigned long)blockIdx.x * DG_TILE + (unsigned long)threadIdx.x * DG_LC;
    int count;
    const unsigned zeros = vc_chunk_zeros(x, n, c0, &count);
    VcMap tot;
    const VcMap pre = vc_scan_excl(vc_map_of(zeros, count), &tot, sh);
    const int st = vc_map_to(pre, t_state[blockIdx.x]);
    const int carry = si->len;
    const BsStream in{x, ci, carry};
    const unsigned mine = vc_replay<false>(in, (long long)carry + (long long)c0, zeros, count, st, nullptr, 0ull, 0ul);
    unsigned long long all;
    const unsigned long long before = vc_sum_excl(mine, &all, sc);
    // (a tile holds at most DG_TILE / 3 + 4 characters: the offset fits in 24 bits)
    t_thread[(unsigned long)blockIdx.x * 256 + threadIdx.x] = (unsigned)st | ((unsigned)before << 8);
    if (threadIdx.x == 0) t_cnt[blockIdx.x] = (unsigned)all;
}

__global__ __launch_bounds__(256) void vc_offsets_kernel(const unsigned *__restrict__ t_cnt, unsigned long ntiles, unsigned long long *__restrict__ t_off,
                                                         VcState *__restrict__ so)
{
    __shared__ unsigned long long sc[2][256];
    const int tid = threadIdx.x;
    const unsigned long seg = (ntiles + 255) / 256, t0 = tid * seg, t1 = t0 + seg < ntiles ? t0 + seg : ntiles;
    unsigned long long s = 0;
    for (unsigned long t = t0; t < t1; t++) s += t_cnt[t];
    unsigned long long tot;
    unsigned long long off = vc_sum_excl(s, &tot, sc);
    for (unsigned long t = t0; t < t1; t++) {
        t_off[t] = off;
        off += t_cnt[t];
    }
    if (tid == 0) so->count = tot;
}

__global__ __launch_bounds__(256) void vc_final_kernel(const uint8_t *__restrict__ x, unsigned long n, const VcState *__restrict__ si,
                                                       const uint8_t *__restrict__ ci, const unsigned *__restrict__ t_thread,
                                                       const unsigned long long *__restrict__ t_off, uint8_t *__restrict__ y, unsigned long cap)
{
    const unsigned long c0 = (unsigned long)blockIdx.x * DG_TILE + (unsigned long)threadIdx.x * DG_LC;
    int count;
    const unsigned zeros = vc_chunk_zeros(x, n, c0, &count);
    const unsigned mine = t_thread[(unsigned long)blockIdx.x * 256 + threadIdx.x];
    const int carry = si->len;
    const BsStream in{x, ci, carry};
    (void)vc_replay<true>(in, (long long)carry + (long long)c0, zeros, count, (int)(mine & 0xffu), y, t_off[blockIdx.x] + (mine >> 8), cap);
}

}  // namespace lrhip
