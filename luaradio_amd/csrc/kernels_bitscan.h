// kernels_bitscan.h - the device pieces shared by the stages that scan a stream for events and emit a data-dependent count: the preamble
// sampler (kernels_preamble.h) and the RDS, ERT, AX.25 and POCSAG framers (kernels_rdsframer.h, kernels_ertframer.h, kernels_ax25framer.h,
// kernels_pocsagframer.h).  Their common shape:
//   match   one workgroup of 256 threads per tile of PS_TILE positions writes a bit mask of the positions where something happens (PS_WORDS
//           64-bit words) and the tile's first set bit (bs_pack, bs_window, bs_store_tile)
//   walk    ONE workgroup hops from event to event: the bit at hand (bs_test), else ps_find_first over the masks and the tile summaries
//   emit    the records, from the list the walk left
// with the state and the unconsumed bytes carried between calls in two device slots that alternate (BsStream reads "the carried bytes, then
// the call's bytes" as one stream).  What differs per protocol - the predicates, the automata, the records - is in the protocol's own header.
#pragma once
#include "common.h"

namespace lrhip {

constexpr int PS_TILE = 1024, PS_WORDS = PS_TILE / 64;      // samples and mask words per tile (one workgroup of 256 threads, 4 samples each)
constexpr long long PS_NONE = 0x7fffffffffffffffll;

// a pattern of `bits` bits (MSB first) in stream order: bit k = the k-th byte received
constexpr unsigned bs_stream_order(unsigned pattern, int bits)
{
    unsigned r = 0;
    for (int k = 0; k < bits; k++) r |= ((pattern >> (bits - 1 - k)) & 1u) << k;
    return r;
}

// byte u of "carried bytes, then the call's bytes" (0 <= u < carry + n)
struct BsStream {
    const uint8_t *__restrict__ x, *__restrict__ carried;
    int carry;
    __device__ __forceinline__ unsigned operator()(long long u) const { return u < carry ? carried[u] : x[u - carry]; }
    // as a bit (Bit.tonumber: a byte counts as 1 only when it equals 1)
    __device__ __forceinline__ bool one(long long u) const { return (*this)(u) == 1u; }
};

// Packs the `== 1` bytes of positions base .. base + 64 nwords - 1 of the stream into s_one[0 .. nwords), bit j of word w = position
// base + 64 w + j; positions at or beyond `total` pack as 0.  With BIG the `> 1` bytes of the same load go to s_big.  Called by all 256 threads;
// the words are complete after the caller's next barrier.
template <bool BIG = false>
__device__ __forceinline__ void bs_pack(const BsStream &in, long long base, long long total, int nwords, unsigned long long *s_one,
                                        unsigned long long *s_big = nullptr)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int w = wave; w < nwords; w += 4) {
        const long long u = base + w * 64 + lane;
        const unsigned b = u < total ? in(u) : 0u;
        const unsigned long long one = __ballot(b == 1u), big = BIG ? __ballot(b > 1u) : 0ull;
        if (lane == 0) {
            s_one[w] = one;
            if (BIG) s_big[w] = big;
        }
    }
}

// the 64 bits from bit `lane` (0 .. 63) of word w of a packed array on: bit k = position 64 w + lane + k (words[w + 1] must exist)
__device__ __forceinline__ unsigned long long bs_window(const unsigned long long *words, int w, int lane)
{
    const unsigned long long lo = words[w], hi = words[w + 1];
    return lane ? (lo >> lane) | (hi << (64 - lane)) : lo;
}

// Stores a tile's PS_WORDS mask words (s_mask, LDS, complete: call behind a barrier) and its first set bit, -1 for none.  Called by all 256
// threads of the tile's workgroup.  WORDS = false where the caller has already stored each word as it was made (rf, ax, pg: a tile is so
// little work that sending the words out only behind the barrier cost the POCSAG match pass 9 %, profiles/counted_scaffold_refactor_ab.txt
// section 3 (a); ef has its words in LDS only).
template <bool WORDS = true>
__device__ __forceinline__ void bs_store_tile(const unsigned long long *s_mask, unsigned long long *__restrict__ mask, int *__restrict__ tile_first)
{
    const int tid = threadIdx.x;
    if (WORDS && tid < PS_WORDS) mask[(unsigned long)blockIdx.x * PS_WORDS + tid] = s_mask[tid];
    if (tid == 0) {
        int first = -1;
        for (int w = PS_WORDS - 1; w >= 0; w--)
            if (s_mask[w]) first = w * 64 + __ffsll((long long)s_mask[w]) - 1;
        tile_first[blockIdx.x] = first;
    }
}

// bit q of a mask
__device__ __forceinline__ bool bs_test(const unsigned long long *__restrict__ mask, long long q) { return (mask[q >> 6] >> (q & 63)) & 1ull; }

// first set bit at or after `from` (call-relative sample, from < ntiles * PS_TILE), or PS_NONE.  Called by all 256 threads with equal arguments;
// every thread gets the same answer.
__device__ long long ps_find_first(const unsigned long long *__restrict__ words, const int *__restrict__ tsum, unsigned long ntiles, long long from,
                                   unsigned long long *s_res)
{
    const int tid = threadIdx.x;
    const unsigned long tile = (unsigned long)(from / PS_TILE);
    if (tid == 0) *s_res = (unsigned long long)PS_NONE;  // (every read of *s_res below is followed by a barrier)
    __syncthreads();
    if (tid < PS_WORDS) {
        const long long lo = (long long)tile * PS_TILE + tid * 64;
        unsigned long long w = words[tile * PS_WORDS + tid];
        if (from >= lo + 64) w = 0;
        else if (from > lo) w &= ~0ull << (from - lo);
        if (w) atomicMin(s_res, (unsigned long long)(lo + __ffsll((long long)w) - 1));
    }
    __syncthreads();
    long long r = (long long)*s_res;
    __syncthreads();
    // (the summaries only after the own tile has failed.  Both in one step was slower, 4.3 against 2.0 ms per 2^24 samples with a frame every
    // 20 000: nearly every tile has a "first D", so all 256 lanes then update the one LDS word)
    for (unsigned long t0 = tile + 1; r == PS_NONE && t0 < ntiles; t0 += 256) {
        const unsigned long t = t0 + tid;
        const int f = t < ntiles ? tsum[t] : -1;
        if (f >= 0) atomicMin(s_res, (unsigned long long)((long long)t * PS_TILE + f));
        __syncthreads();
        r = (long long)*s_res;
        __syncthreads();
    }
    return r;
}

}  // namespace lrhip
