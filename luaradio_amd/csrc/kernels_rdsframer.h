// kernels_rdsframer.h - RDSFramerBlock (radio/blocks/protocol/rdsframer.lua:95-201): Bit -> RDSFrameType (uint16_t blocks[4], 8 bytes).
//
// The reference shifts bits into a 104-bit buffer and tests it whenever it is full (:143-198).  Whether a window is a frame is a pure function of its
// 104 bits (:163-175), and the automaton around the test only hops: an accepted window empties the buffer (:188), so the next window starts 104
// bits later; a rejected one shifts by one bit (:153).  The `synchronized` flag feeds a debug print alone.  With u the index in the stream of
// "carried bits, then this call's bits" (u = 0 is the first bit no accepted frame has consumed):
//   block value   v(b) = bits b .. b + 25, MSB first (Bit.tonumber: a byte counts as 1 only when it equals 1)
//   syndrome      S(b) = XOR of row k of H^T (:45-54) over the set bits k of the block.  It is linear and the offset words have their ten check
//                 bits only, so syndrome(v ^ offset) = S ^ offset: one syndrome per position serves all five offsets
//   correctable   S ^ offset is 0 or one of the 26 rows (the keys of the correction matrix, :58-67): a 1024-entry table of four flags - as A, as B,
//                 as C or C', as D - built once on the host (rf_flag_table)
//   V(s)          = A(s) & B(s + 26) & C(s + 52) & D(s + 78)
// and from the first unconsumed bit q the walk takes the first s >= q with V(s), emits it and sets q = s + 104: a valid window that starts inside an
// accepted frame is never emitted.
//
// Passes (3 launches, one count read-back), the shape of kernels_bitscan.h:
//   rf_match_kernel  one workgroup per tile of PS_TILE window starts.  The `== 1` bytes of the tile and of the 192 bits behind it are packed into
//                    64-bit words by wave ballots (LDS); each lane then takes one block start, computes S by 26 conditional XORs of immediates on
//                    the funnel-shifted window and looks its four flags up in the LDS copy of the table; four ballots give the flag masks, and V
//                    is the AND of the masks shifted by 26, 52 and 78 bits.  (Conditional XORs, not chunk tables: a table indexed by data bits is
//                    a gather from LDS - 32 lanes on random banks serialise several ways and each dependent ds_read costs about 50 cycles of
//                    latency - while 26 v_bfe / v_and / v_xor pairs stay in registers, are independent of each other, and this stage is nowhere near a
//                    hot path at 1187.5 bit/s.  The one flag lookup per position stays: it replaces five 27-way membership tests.)
//                    Stores the V mask (one word per 64 starts) and the tile's "first V".
//   rf_walk_kernel   ONE workgroup hops from frame to frame: bit q first (back-to-back frames are the normal case in lock), else
//                    ps_find_first over q's tile and then the tile summaries.  Serial cost: one hop per frame plus tiles / 256 search steps.
//   rf_emit_kernel   one thread per frame recomputes its four corrected blocks (:105-137, C before C') and writes the record with one 8-byte store;
//                    block 0 also writes the next call's carried bits.
// Carried between calls, ping-pong on the device: the bits since q (at most 103: every window that ends inside a call is tested in it) and RfState.
#pragma once
#include "common.h"
#include "kernels_bitscan.h"

namespace lrhip {

constexpr int RF_FRAME = 104, RF_BLOCK = 26;
constexpr int RF_CARRY = 128;                                // bytes of one carried-bits slot (103 used)
constexpr int RF_BIT_WORDS = PS_WORDS + 3;                   // packed bits a tile reads: its own and the 192 behind it (the last block start + 25 needed)
constexpr int RF_FLAG_WORDS = PS_WORDS + 2;                  // block starts a tile needs flags of: its own and the 78 behind it
constexpr unsigned RF_OFFSET_A = 0x0fc, RF_OFFSET_B = 0x198, RF_OFFSET_C = 0x168, RF_OFFSET_CP = 0x350, RF_OFFSET_D = 0x1b4;      // rdsframer.lua:38-40
enum { RF_FLAG_A = 1, RF_FLAG_B = 2, RF_FLAG_C = 4, RF_FLAG_D = 8 };

// row of H^T (rdsframer.lua:45-54) for bit k of a block in stream order: k = 0 is the first bit received, value 1 << 25
__host__ __device__ constexpr unsigned rf_row(int k)
{
    constexpr unsigned R[RF_BLOCK] = {0x077, 0x2e7, 0x3af, 0x30b, 0x359, 0x370, 0x1b8, 0x0dc, 0x06e, 0x037, 0x2c7, 0x3bf, 0x303,
                                      0x35d, 0x372, 0x1b9, 0x200, 0x100, 0x080, 0x040, 0x020, 0x010, 0x008, 0x004, 0x002, 0x001};
    return R[k];
}

// host: syndrome -> RF_FLAG_* of the offsets under which it is zero or a single-bit error (the correction matrix :58-67 has exactly the rows as keys)
inline void rf_flag_table(uint8_t *table)
{
    bool ok[1024] = {false};
    ok[0] = true;
    for (int k = 0; k < RF_BLOCK; k++) ok[rf_row(k)] = true;
    for (unsigned s = 0; s < 1024; s++)
        table[s] = (uint8_t)((ok[s ^ RF_OFFSET_A] ? RF_FLAG_A : 0) | (ok[s ^ RF_OFFSET_B] ? RF_FLAG_B : 0) |
                             (ok[s ^ RF_OFFSET_C] || ok[s ^ RF_OFFSET_CP] ? RF_FLAG_C : 0) | (ok[s ^ RF_OFFSET_D] ? RF_FLAG_D : 0));
}

// carried between calls (ping-pong on the device)
struct RfState {
    int carry;                       // bits since q, the first bit no accepted frame has consumed (0 .. 103)
    int overflow;                    // the frame list was too small (never, by the bound of RfStage)
    unsigned long long count;        // frames of the last call
};

// syndrome of a block given in stream order: bit k of r = bit k of the block as received
__device__ __forceinline__ unsigned rf_syndrome(unsigned r)
{
    unsigned s = 0;
#pragma unroll
    for (int k = 0; k < RF_BLOCK; k++) s ^= ((r >> k) & 1u) ? rf_row(k) : 0u;
    return s;
}

__global__ __launch_bounds__(256) void rf_match_kernel(const uint8_t *__restrict__ x, const uint8_t *__restrict__ carried, unsigned long n,
                                                       const RfState *__restrict__ si, const uint8_t *__restrict__ table,
                                                       unsigned long long *__restrict__ mask_v, int *__restrict__ tile_v)
{
    __shared__ unsigned long long s_bits[RF_BIT_WORDS];
    __shared__ unsigned long long s_flag[4][RF_FLAG_WORDS], s_v[PS_WORDS];
    __shared__ __attribute__((aligned(16))) uint8_t s_table[1024];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const BsStream in{x, carried, si->carry};
    const long long total = (long long)in.carry + (long long)n, base = (long long)blockIdx.x * PS_TILE;
    ((uint32_t *)s_table)[tid] = ((const uint32_t *)table)[tid];
    bs_pack(in, base, total, RF_BIT_WORDS, s_bits);
    __syncthreads();
    for (int w = wave; w < RF_FLAG_WORDS; w += 4) {
        // the 26 bits from block start b = 64 w + lane, bit k = the k-th received (w + 1 < RF_BIT_WORDS)
        const unsigned r = (unsigned)bs_window(s_bits, w, lane) & ((1u << RF_BLOCK) - 1u);
        const unsigned f = s_table[rf_syndrome(r)];
        const unsigned long long fa = __ballot(f & RF_FLAG_A), fb = __ballot(f & RF_FLAG_B), fc = __ballot(f & RF_FLAG_C), fd = __ballot(f & RF_FLAG_D);
        if (lane == 0) { s_flag[0][w] = fa; s_flag[1][w] = fb; s_flag[2][w] = fc; s_flag[3][w] = fd; }
    }
    __syncthreads();
    if (tid < PS_WORDS) {
        // bit j of word tid: V(base + 64 tid + j) = A & B >> 26 & C >> 52 & D >> 78 (78 = 64 + 14; tid + 2 < RF_FLAG_WORDS)
        unsigned long long v = s_flag[0][tid];
        v &= (s_flag[1][tid] >> 26) | (s_flag[1][tid + 1] << 38);
        v &= (s_flag[2][tid] >> 52) | (s_flag[2][tid + 1] << 12);
        v &= (s_flag[3][tid + 1] >> 14) | (s_flag[3][tid + 2] << 50);
        // only windows that end inside the stream: s + 104 <= total
        const long long lo = base + tid * 64, last = total - RF_FRAME;
        if (last < lo) v = 0;
        else if (last < lo + 63) v &= ~0ull >> (63 - (last - lo));
        mask_v[(unsigned long)blockIdx.x * PS_WORDS + tid] = v;
        s_v[tid] = v;
    }
    __syncthreads();
    bs_store_tile<false>(s_v, mask_v, tile_v);
}

__global__ __launch_bounds__(256) void rf_walk_kernel(const unsigned long long *__restrict__ mask_v, const int *__restrict__ tile_v, unsigned long ntiles,
                                                      unsigned long n, const RfState *__restrict__ si, RfState *__restrict__ so,
                                                      long long *__restrict__ starts, unsigned long max_frames)
{
    __shared__ unsigned long long s_res;
    const long long total = (long long)si->carry + (long long)n;
    long long q = 0;
    unsigned long long nframes = 0;
    int overflow = 0;
    // every thread runs the same automaton on the same values; thread 0 writes
    while (q + RF_FRAME <= total) {
        long long s = q;
        if (!bs_test(mask_v, q)) {
            s = ps_find_first(mask_v, tile_v, ntiles, q, &s_res);
            if (s == PS_NONE) { q = total - (RF_FRAME - 1); break; }      // every window up to total - 104 was rejected
        }
        if (nframes >= max_frames) { overflow = 1; break; }
        if (threadIdx.x == 0) starts[nframes] = s;
        nframes++;
        q = s + RF_FRAME;
    }
    if (threadIdx.x == 0) {
        so->carry = (int)(total - q);
        so->overflow = overflow;
        so->count = nframes;
    }
}

// one received block (bit k = the k-th received) under one offset word: rds_correct_block (:105-137).  Returns the corrected 26-bit value, MSB first,
// or -1 when it is uncorrectable.
__device__ __forceinline__ int rf_correct(unsigned r, unsigned offset)
{
    const unsigned v = __brev(r) >> (32 - RF_BLOCK), s = rf_syndrome(r) ^ offset;
    if (s == 0) return (int)v;
#pragma unroll 1
    for (int k = 0; k < RF_BLOCK; k++)
        if (rf_row(k) == s) return (int)(v ^ (1u << (RF_BLOCK - 1 - k)));
    return -1;
}

__global__ __launch_bounds__(256) void rf_emit_kernel(const uint8_t *__restrict__ x, const uint8_t *__restrict__ carried, uint8_t *__restrict__ carried_out,
                                                      unsigned long n, const RfState *__restrict__ si, const RfState *__restrict__ so,
                                                      const long long *__restrict__ starts, unsigned long long *__restrict__ y, unsigned long cap)
{
    const BsStream in{x, carried, si->carry};
    const unsigned long long nframes = so->overflow ? 0ull : so->count;
    const unsigned long long f = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    if (f < nframes && f < cap) {
        const long long s = starts[f];
        unsigned long long rec = 0;
#pragma unroll 1
        for (int b = 0; b < 4; b++) {
            unsigned r = 0;
            for (int k = 0; k < RF_BLOCK; k++) r |= (unsigned)in.one(s + b * RF_BLOCK + k) << k;
            int v = rf_correct(r, b == 0 ? RF_OFFSET_A : b == 1 ? RF_OFFSET_B : b == 2 ? RF_OFFSET_C : RF_OFFSET_D);
            if (b == 2 && v < 0) v = rf_correct(r, RF_OFFSET_CP);
            rec |= (unsigned long long)(((unsigned)v >> 10) & 0xffffu) << (16 * b);       // blocks[b], little-endian
        }
        y[f] = rec;
    }
    if (blockIdx.x == 0 && !so->overflow) {
        const int next = so->carry;                          // <= 103 < RF_CARRY
        const long long total = (long long)in.carry + (long long)n;
        // (carried as 0 / 1, where the other framers carry raw bytes: every read of this slot goes through `== 1`)
        if ((int)threadIdx.x < next) carried_out[threadIdx.x] = (uint8_t)in.one(total - next + threadIdx.x);
    }
}

}  // namespace lrhip
