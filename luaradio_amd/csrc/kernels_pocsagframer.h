// kernels_pocsagframer.h - POCSAGFramerBlock (radio/blocks/protocol/pocsagframer.lua:120-277): Bit -> struct lrhip_pocsag_frame (256 bytes,
// include/lrhip.h).
//
// The reference keeps a buffer of up to 544 bytes.  FRAME_SYNC with 32 or more bytes: the correlation of the first 32 with the sync word,
// sum(s_i * (2 * value_i - 1)) on the byte VALUES (one byte of 255 under a +1 tap outweighs every mismatch), of at least 28 switches to BATCH
// without consuming anything, less shifts by one.  BATCH with 544 bytes: codeword 0 (Bit.tonumber: a byte counts as 1 only when it equals 1)
// must correct (pocsag_correct_codeword: 11-bit syndrome, zero or a single-bit error) to exactly 0x7cd215d8, else the pending frame goes out, 32
// bytes are consumed and the state is FRAME_SYNC again.  Then codewords 1 .. 16 run the frame automaton - an uncorrectable, idle or address
// codeword emits the pending frame, an address codeword opens one, a data codeword appends to an open one, two uncorrectable codewords in a
// row at position j consume (j + 1) * 32 bytes and return to FRAME_SYNC - and otherwise 544 bytes are consumed and the state stays BATCH.
//
// Timing.  The reference takes one step per loop iteration after refilling its buffer, so it stops with up to 543 buffered bytes unexamined
// and how far it gets depends on how the stream was cut into calls.  The device is EAGER: it takes every step the bytes seen so far allow (32
// or more in FRAME_SYNC, 544 in BATCH).  Its output is therefore the same however the stream is cut, whatever the reference emits for any
// cutting is a prefix of it, and it is a prefix of the reference's output once 544 further bits have been fed.
//
// A frame has no upper length (a message runs on across batches), a record holds 62 data words: when the 63rd word arrives the full record is
// written with bit 0 of `flags` set, and its successor carries bit 1 and the same address and func.  Nothing is dropped.
//
// Passes (2 launches, one count read-back), with u the index in "carried bytes, then this call's bytes":
//   pg_match_kernel  one workgroup per tile of PS_TILE positions.  Two ballot-packed masks, "byte == 1" and "byte > 1"; where the 32 bytes at a
//                    position are all 0 / 1 the correlation is 32 - 2 popcount(bits ^ sync) on the funnel-shifted word, else the lane sums the
//                    32 products.  Stores the mask S(p) (p + 32 <= total) and the tile's "first S".
//   pg_walk_kernel   ONE workgroup.  FRAME_SYNC: ps_find_first over S.  BATCH: 17 lanes read and correct one codeword each (32 conditional XORs
//                    of immediates, the error position by 32 compares: no 2048-entry table), then every thread runs the automaton on the 17
//                    results with the pending frame's words in LDS, and wave 0 writes each record as one wave-wide store, one dword per lane.
//                    It hops from batch to batch without a search, and leaves the pending frame and the unconsumed bytes (at most 543) in the
//                    next call's slot.
#pragma once
#include "common.h"
#include "kernels_bitscan.h"

namespace lrhip {

constexpr int PG_BATCH_LEN = 544, PG_CODEWORD = 32;
constexpr int PG_CARRY = 576;                                // bytes of one carried slot (at most 543 used)
constexpr int PG_WORDS = 62, PG_REC = 256;                   // struct lrhip_pocsag_frame
constexpr unsigned PG_SYNC_CODEWORD = 0x7cd215d8u, PG_IDLE_CODEWORD = 0x7a89c197u;
enum { PG_FRAME_SYNC = 0, PG_IN_BATCH = 1 };
enum { PG_CONTINUES = 1, PG_CONTINUED = 2 };

// row of H^T (pocsagframer.lua:54-64) for bit 31 - k of a codeword
__host__ __device__ constexpr unsigned pg_row(int k)
{
    constexpr unsigned R[32] = {0x769, 0x3b5, 0x1db, 0x784, 0x3c2, 0x689, 0x345, 0x1a3, 0x7b8, 0x3dc, 0x1ee, 0x79f, 0x4a6, 0x53b, 0x5f4, 0x2fa,
                                0x615, 0x30b, 0x6ec, 0x376, 0x6d3, 0x400, 0x200, 0x100, 0x080, 0x040, 0x020, 0x010, 0x008, 0x004, 0x002, 0x001};
    return R[k];
}

// carried between calls (ping-pong on the device)
struct PgState {
    int mode;                        // PG_IN_BATCH: u = 0 is where the sync word was found
    int carry;                       // carried bytes: at most 31 in FRAME_SYNC, 543 in BATCH
    int overflow;                    // more records than the bound (never, by the bound of PgStage)
    int has;                         // a frame is pending
    unsigned address, func, flags, count;
    unsigned long long nrec;         // records of the last call
    unsigned data[PG_WORDS];
};

__global__ __launch_bounds__(256) void pg_match_kernel(const uint8_t *__restrict__ x, const uint8_t *__restrict__ carried, unsigned long n,
                                                       const PgState *__restrict__ si, unsigned long long *__restrict__ mask_s, int *__restrict__ tile_s)
{
    __shared__ unsigned long long s_bits[PS_WORDS + 1], s_big[PS_WORDS + 1];      // the tile and the 31 positions behind it
    __shared__ unsigned long long s_s[PS_WORDS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const BsStream raw{x, carried, si->carry};
    const long long total = (long long)raw.carry + (long long)n, base = (long long)blockIdx.x * PS_TILE;
    bs_pack<true>(raw, base, total, PS_WORDS + 1, s_bits, s_big);
    __syncthreads();
    constexpr unsigned SYNC = bs_stream_order(PG_SYNC_CODEWORD, 32);             // bit k = the k-th byte received
    for (int w = wave; w < PS_WORDS; w += 4) {
        const long long p = base + w * 64 + lane;
        const unsigned r = (unsigned)bs_window(s_bits, w, lane), g = (unsigned)bs_window(s_big, w, lane);
        bool hit = false;
        if (p + PG_CODEWORD <= total) {
            if (!g) {
                hit = __popc(r ^ SYNC) <= 2;                                     // corr = 32 - 2 mismatches >= 28
            } else {
                int corr = 0;
                for (int i = 0; i < 32; i++) corr += (((SYNC >> i) & 1u) ? 1 : -1) * (2 * (int)raw(p + i) - 1);
                hit = corr >= 28;
            }
        }
        const unsigned long long m = __ballot(hit);
        if (lane == 0) {
            s_s[w] = m;
            mask_s[(unsigned long)blockIdx.x * PS_WORDS + w] = m;
        }
    }
    __syncthreads();
    bs_store_tile<false>(s_s, mask_s, tile_s);
}

// pocsag_correct_codeword (:120-149).  Returns false when the codeword is uncorrectable.
__device__ __forceinline__ bool pg_correct(unsigned *codeword)
{
    const unsigned cw = *codeword;
    unsigned syn = 0;
#pragma unroll
    for (int k = 0; k < 32; k++) syn ^= ((cw >> (31 - k)) & 1u) ? pg_row(k) : 0u;
    if (syn == 0) return true;
#pragma unroll 1
    for (int k = 0; k < 32; k++)
        if (pg_row(k) == syn) { *codeword = cw ^ (1u << (31 - k)); return true; }
    return false;
}

__global__ __launch_bounds__(256) void pg_walk_kernel(const uint8_t *__restrict__ x, const uint8_t *__restrict__ carried, uint8_t *__restrict__ carried_out,
                                                      unsigned long n, const PgState *__restrict__ si, PgState *__restrict__ so,
                                                      const unsigned long long *__restrict__ mask_s, const int *__restrict__ tile_s, unsigned long ntiles,
                                                      uint32_t *__restrict__ y, unsigned long max_records)
{
    __shared__ unsigned long long s_res;
    __shared__ unsigned s_data[PG_WORDS], s_cw[17];
    __shared__ int s_ok[17];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const BsStream raw{x, carried, si->carry};
    const long long total = (long long)raw.carry + (long long)n;
    int mode = si->mode, has = si->has;
    unsigned address = si->address, func = si->func, flags = si->flags, count = si->count;
    if (tid < PG_WORDS) s_data[tid] = si->data[tid];
    __syncthreads();
    long long q = 0;
    unsigned long long nrec = 0;
    // every thread runs the same automaton on the same values; thread 0 appends data words and wave 0 writes records.
    // One record: address | func, flags, count | 62 words, one dword per lane
    auto emit = [&](unsigned fl) {
        __syncthreads();                                     // thread 0's words are visible
        if (wave == 0 && nrec < max_records) {
            const unsigned v = lane == 0 ? address : lane == 1 ? (func | (fl << 8) | (count << 16)) : (unsigned)(lane - 2) < count ? s_data[lane - 2] : 0u;
            y[nrec * (PG_REC / 4) + lane] = v;
        }
        nrec++;
        __syncthreads();                                     // before the next frame's words replace them
    };
    auto flush = [&]() {
        if (has) {
            emit(flags);
            has = 0;
        }
    };
    for (;;) {
        if (mode == PG_FRAME_SYNC) {
            if (q + PG_CODEWORD > total) break;
            const long long p = ps_find_first(mask_s, tile_s, ntiles, q, &s_res);
            if (p == PS_NONE) { q = max(q, total - (PG_CODEWORD - 1)); break; }      // every position up to total - 32 was tested
            q = p;
            mode = PG_IN_BATCH;
        }
        if (q + PG_BATCH_LEN > total) break;
        if (tid < 17) {
            unsigned cw = 0;
            for (int k = 0; k < 32; k++) cw = (cw << 1) | (raw(q + 32 * tid + k) == 1u ? 1u : 0u);
            s_ok[tid] = pg_correct(&cw) ? 1 : 0;
            s_cw[tid] = cw;
        }
        __syncthreads();
        if (!s_ok[0] || s_cw[0] != PG_SYNC_CODEWORD) {
            flush();
            q += PG_CODEWORD;
            mode = PG_FRAME_SYNC;
        } else {
            int invalid = 0, j;
            for (j = 1; j <= 16; j++) {
                const unsigned cw = s_cw[j];
                if (!s_ok[j]) {
                    invalid++;
                    flush();
                    if (invalid == 2) break;
                    continue;
                }
                invalid = 0;
                if (cw == PG_IDLE_CODEWORD) {
                    flush();
                } else if (!(cw & 0x80000000u)) {
                    flush();
                    has = 1;
                    address = ((cw >> 10) & 0x1ffff8u) | (unsigned)((j - 1) >> 1);
                    func = (cw >> 11) & 3u;
                    flags = 0;
                    count = 0;
                } else if (has) {
                    if (count == PG_WORDS) {
                        emit(flags | PG_CONTINUES);
                        flags = PG_CONTINUED;
                        count = 0;
                    }
                    if (tid == 0) s_data[count] = (cw >> 11) & 0xfffffu;
                    count++;
                }
            }
            if (j <= 16) {
                q += (j + 1) * PG_CODEWORD;
                mode = PG_FRAME_SYNC;
            } else {
                q += PG_BATCH_LEN;
            }
        }
        __syncthreads();                                     // every read of s_cw is done
    }
    __syncthreads();
    const int next = (int)(total - q);                       // <= 543 < PG_CARRY
    for (int i = tid; i < next; i += 256) carried_out[i] = (uint8_t)raw(q + i);
    if (tid < PG_WORDS) so->data[tid] = has && (unsigned)tid < count ? s_data[tid] : 0u;
    if (tid == 0) {
        so->mode = mode;
        so->carry = next;
        so->overflow = nrec > max_records;
        so->has = has;
        so->address = has ? address : 0u;
        so->func = has ? func : 0u;
        so->flags = has ? flags : 0u;
        so->count = has ? count : 0u;
        so->nrec = nrec;
    }
}

}  // namespace lrhip
