// kernels_ax25framer.h - AX25FramerBlock (radio/blocks/protocol/ax25framer.lua:94-284): Bit -> struct lrhip_ax25_frame (416 bytes, include/lrhip.h).
//
// The reference shifts bytes through an 8-byte buffer.  IDLE: a buffer that reads 0x7e (Bit.tonumber, "lsb": a byte counts as 1 only when it
// equals 1) opens a frame and empties the buffer, anything else shifts by one.  FRAME: a flag closes the raw frame - it is unstuffed, validated
// (whole octets, at least 120 bits, FCS) and extracted; a frame goes out and the state returns to IDLE, anything else keeps FRAME with the
// flag as the next opening flag - a raw frame that has grown beyond 3184 bits without a flag drops to IDLE, else the buffer's first byte
// moves to the raw frame.  With u the index in "carried bytes, then this call's bytes":
//   F(p)       the 8 bytes at p read 0x7e
//   flags      the consumed flags are the greedy chain "first F at or after q, then q = p + 8", in IDLE and in FRAME alike
//   segment k  the bytes between two consecutive consumed flags, [a + 8, b).  It is a candidate unless segment k - 1 was emitted (the
//              reference is IDLE behind an emitted frame: a frame that shares its opening flag with an emitted frame's closing flag is lost)
//   valid_k    at most 3185 raw bytes, and the checks above: a pure function of the segment's bytes
//   emitted_k  = valid_k and not emitted_(k-1): the only sequential part
// Bytes other than 0 and 1 are read as the reference reads them: the unstuffer drops byte i only when it equals 0 and exactly five bytes equal
// to 1 precede it (ones_count is not capped, so the byte in front of the five must differ from 1); the CRC feeds back only when
// (crc & 1) ^ value == 1, so a byte of 2 or more never feeds back - the CRC is linear only over 0 / 1 bytes, and a span that holds a larger byte
// takes the literal loop.
//
// Passes (5 launches, one count read-back):
//   ax_match_kernel   one workgroup per tile of PS_TILE positions: the `== 1` bytes packed into 64-bit words by wave ballots, F by one compare
//                     per lane on the funnel-shifted word; stores the F mask and the tile's "first F".
//   ax_walk_kernel    ONE workgroup lists the consumed flags: the 64 positions from q are tested on two mask words (no barrier: the next flag
//                     of a flag run or of noise is nearly always among them), else ps_find_first.
//   ax_eval_kernel    one wave per segment: the drop mask is a window function, the compaction a ballot / popcount prefix sum into LDS; the
//                     CRC-16 over 0 / 1 bytes is the XOR of rows A^k P (P = 0x8408 reflected, A the zero-input step; the initial 0xffff equals
//                     an inversion of the first 16 bits) built on the host and held in LDS; the octets, then the address chain by one ballot.
//   ax_select_kernel  ONE workgroup: the alternation emitted_k as a composition of per-chunk maps of the incoming bit, the list of emitted
//                     segments, the count, and the next call's state and carried bytes.
//   ax_emit_kernel    one wave per emitted frame evaluates it again and writes its record, 104 dwords by vector stores.
// Carried between calls, ping-pong on the device: AxState and, in FRAME, the raw bytes since the opening flag (at most 3185 + 7), in IDLE the
// last 7 or fewer bytes no flag has consumed.  The bytes are carried raw: their values matter beyond `== 1`.
#pragma once
#include "common.h"
#include "kernels_bitscan.h"

namespace lrhip {

constexpr int AX_RAW_MAX = 3185;                             // raw bits of the longest frame that still closes (AX25_RAW_FRAME_MAXLEN + 1)
constexpr int AX_MIN_BITS = 120;                             // AX25_FRAME_MINLEN - 16: unstuffed bits, the FCS included
constexpr int AX_CARRY = 3200;                               // bytes of one carried slot (at most AX_RAW_MAX + 7 used)
constexpr int AX_CRC_ROWS = AX_RAW_MAX / 8 * 8 - 16;         // 3168: the most bits the FCS covers
constexpr int AX_DATA = 400, AX_REC = 416;                   // struct lrhip_ax25_frame
constexpr unsigned AX_FLAG = 0x7eu;                          // the same LSB first and MSB first
enum { AX_IDLE = 0, AX_FRAME = 1 };

// host: rows[k] = A^k P - what a 1 at the CRC's input contributes k bits later (ax25_compute_crc, :94-111, on 0 / 1 bytes)
inline void ax_crc_rows(uint16_t *rows)
{
    unsigned r = 0x8408u;
    for (int k = 0; k < AX_CRC_ROWS; k++) {
        rows[k] = (uint16_t)r;
        r = (r >> 1) ^ ((r & 1u) ? 0x8408u : 0u);
    }
}

// carried between calls (ping-pong on the device)
struct AxState {
    int mode;                        // AX_FRAME: a frame is open and u = 0 is its first raw byte; AX_IDLE: u = 0 is the first byte no flag has consumed
    int carry;                       // carried bytes
    int overflow;                    // a list was too small (never, by the bounds of AxStage)
    int pad;
    unsigned long long count;        // frames of the last call
    unsigned long long nflags;       // consumed flags of the last call
};

__global__ __launch_bounds__(256) void ax_match_kernel(const uint8_t *__restrict__ x, const uint8_t *__restrict__ carried, unsigned long n,
                                                       const AxState *__restrict__ si, unsigned long long *__restrict__ mask_f, int *__restrict__ tile_f)
{
    __shared__ unsigned long long s_bits[PS_WORDS + 1];      // the tile and the 7 bits behind it
    __shared__ unsigned long long s_f[PS_WORDS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const BsStream raw{x, carried, si->carry};
    const long long total = (long long)raw.carry + (long long)n, base = (long long)blockIdx.x * PS_TILE;
    bs_pack(raw, base, total, PS_WORDS + 1, s_bits);
    __syncthreads();
    for (int w = wave; w < PS_WORDS; w += 4) {
        // the 8 bits from position 64 w + lane, bit k = the k-th received; only flags that end inside the stream: p + 8 <= total
        const unsigned r = (unsigned)bs_window(s_bits, w, lane) & 0xffu;
        const unsigned long long f = __ballot(r == AX_FLAG && base + w * 64 + lane + 8 <= total);
        if (lane == 0) {
            s_f[w] = f;
            mask_f[(unsigned long)blockIdx.x * PS_WORDS + w] = f;
        }
    }
    __syncthreads();
    bs_store_tile<false>(s_f, mask_f, tile_f);
}

__global__ __launch_bounds__(256) void ax_walk_kernel(const unsigned long long *__restrict__ mask_f, const int *__restrict__ tile_f, unsigned long ntiles,
                                                      unsigned long n, const AxState *__restrict__ si, AxState *__restrict__ so,
                                                      long long *__restrict__ flags, unsigned long max_flags)
{
    __shared__ unsigned long long s_res;
    const long long total = (long long)si->carry + (long long)n;
    const unsigned long nwords = ntiles * PS_WORDS;
    long long q = 0;
    unsigned long long nf = 0;
    int overflow = 0;
    // every thread runs the same automaton on the same values; thread 0 writes
    while (q + 8 <= total) {
        const unsigned long wi = (unsigned long)(q >> 6);
        const int sh = (int)(q & 63);
        unsigned long long w = mask_f[wi] >> sh;
        if (sh && wi + 1 < nwords) w |= mask_f[wi + 1] << (64 - sh);
        long long p;
        if (w) {
            p = q + __ffsll((long long)w) - 1;
        } else {
            p = ps_find_first(mask_f, tile_f, ntiles, q, &s_res);
            if (p == PS_NONE) break;
        }
        if (nf >= max_flags) { overflow = 1; break; }
        if (threadIdx.x == 0) flags[nf] = p;
        nf++;
        q = p + 8;
    }
    if (threadIdx.x == 0) {
        so->nflags = nf;
        so->overflow = overflow;
    }
}

// One wave (a workgroup of 64) evaluates the segment of R raw bytes at u = s: ax25_unstuff_frame, ax25_validate_frame and ax25_extract_frame
// (:113-216).  Every thread calls with the same arguments and gets the same answer.  With rec != nullptr a valid frame's record is written.
// buf: AX_CARRY bytes, oct: AX_DATA bytes, rows: AX_CRC_ROWS entries, all LDS.
__device__ bool ax_evaluate(const BsStream &raw, long long s, long long R, int lane, uint8_t *buf, uint8_t *oct, const uint16_t *rows, uint32_t *rec)
{
    if (R > AX_RAW_MAX || R < AX_MIN_BITS) return false;     // (unstuffing only shortens)
    __syncthreads();                                          // the previous segment's reads of buf and oct are done
    int J = 0;
    for (int at = 0; at < (int)R; at += 64) {
        const int i = at + lane;
        const bool in = i < (int)R;
        const unsigned b = in ? raw(s + i) : 0u;
        bool keep = in;
        if (in && b == 0u && i >= 5) {
            // dropped when ones_count == 5: exactly five bytes equal to 1 in front of it (ones_count starts at 0 and is not capped)
            bool five = true;
            for (int k = 1; k <= 5; k++) five = five && raw(s + i - k) == 1u;
            if (five && (i < 6 || raw(s + i - 6) != 1u)) keep = false;
        }
        const unsigned long long m = __ballot(keep);
        if (keep) buf[J + __popcll(m & ((1ull << lane) - 1ull))] = (uint8_t)b;
        J += __popcll(m);
    }
    __syncthreads();
    if ((J & 7) || J < AX_MIN_BITS) return false;
    const int N = J - 16, L = N / 8;                         // bits the FCS covers, octets in front of it
    // the CRC: linear over 0 / 1 bytes
    unsigned crc = 0;
    bool big = false;
    for (int i = lane; i < N; i += 64) {
        const unsigned b = buf[i];
        big = big || b > 1u;
        if ((b ^ (i < 16 ? 1u : 0u)) & 1u) crc ^= rows[N - 1 - i];
    }
    if (__any(big)) {
        // the literal loop, by every lane alike: a byte of 2 or more never feeds back
        crc = 0xffffu;
        for (int i = 0; i < N; i++) crc = (crc >> 1) ^ ((((crc & 1u) ^ (unsigned)buf[i]) == 1u) ? 0x8408u : 0u);
    } else {
#pragma unroll
        for (int o = 32; o; o >>= 1) crc ^= (unsigned)__shfl_xor((int)crc, o);
    }
    unsigned fcs = 0;
    for (int k = 0; k < 16; k++) fcs |= (buf[N + k] == 1 ? 1u : 0u) << k;
    if ((~crc & 0xffffu) != fcs) return false;
    for (int m = lane; m < L; m += 64) {
        unsigned v = 0;
        for (int k = 0; k < 8; k++) v |= (buf[8 * m + k] == 1 ? 1u : 0u) << k;
        oct[m] = (uint8_t)v;
    }
    __syncthreads();
    // the address chain ends at the first address k whose last octet has bit 0 set; it must end, and the control octet follow, before the FCS
    const unsigned long long ends = __ballot(7 * lane + 6 < L && (oct[7 * lane + 6] & 1u));
    if (!ends) return false;
    const int naddr = __ffsll((long long)ends);
    int at = 7 * naddr;
    if (at >= L) return false;
    if (rec) {
        const unsigned control = oct[at++];
        const bool has_pid = at < L;
        const unsigned pid = has_pid ? oct[at++] : 0u;
        for (int d = lane; d < AX_REC / 4; d += 64) {
            unsigned v = 0;
            if (d == 0) v = (unsigned)L | (fcs << 16);
            else if (d == 1) v = (unsigned)naddr | (control << 8) | (pid << 16) | ((has_pid ? 1u : 0u) << 24);
            else if (d == 2) v = (unsigned)at | ((unsigned)(has_pid ? L - at : 0) << 16);
            else if (d >= 4)
                for (int j = 0; j < 4; j++) {
                    const int m = (d - 4) * 4 + j;
                    if (m < L) v |= (unsigned)oct[m] << (8 * j);
                }
            rec[d] = v;
        }
    }
    return true;
}

// segment k lies between consumed flags k - 1 and k; segment 0 of a call starts at u = 0 and exists only while a frame is open
__device__ __forceinline__ long long ax_segment_start(const long long *__restrict__ flags, unsigned long long k) { return k ? flags[k - 1] + 8 : 0; }

__global__ __launch_bounds__(64) void ax_eval_kernel(const uint8_t *__restrict__ x, const uint8_t *__restrict__ carried, const AxState *__restrict__ si,
                                                     const AxState *__restrict__ so, const uint16_t *__restrict__ rows,
                                                     const long long *__restrict__ flags, uint8_t *__restrict__ valid)
{
    __shared__ uint8_t s_buf[AX_CARRY], s_oct[AX_DATA];
    __shared__ uint16_t s_rows[AX_CRC_ROWS];
    const int lane = threadIdx.x;
    const unsigned long long nf = so->overflow ? 0ull : so->nflags;
    if (blockIdx.x >= nf) return;
    const BsStream raw{x, carried, si->carry};
    for (int i = lane; i < AX_CRC_ROWS; i += 64) s_rows[i] = rows[i];
    __syncthreads();
    for (unsigned long long k = blockIdx.x; k < nf; k += gridDim.x) {
        const long long s = ax_segment_start(flags, k);
        const bool ok = (k || si->mode == AX_FRAME) && ax_evaluate(raw, s, flags[k] - s, lane, s_buf, s_oct, s_rows, nullptr);
        if (lane == 0) valid[k] = ok ? 1 : 0;
    }
}

__global__ __launch_bounds__(256) void ax_select_kernel(const uint8_t *__restrict__ x, const uint8_t *__restrict__ carried, uint8_t *__restrict__ carried_out,
                                                        unsigned long n, const AxState *__restrict__ si, AxState *__restrict__ so,
                                                        const long long *__restrict__ flags, const uint8_t *__restrict__ valid,
                                                        unsigned long long *__restrict__ segs, unsigned long max_frames)
{
    __shared__ int s_to[2][256], s_in[256], s_last;
    __shared__ unsigned long long s_cnt[2][256], s_base[256], s_total;
    const int tid = threadIdx.x;
    const BsStream raw{x, carried, si->carry};
    const long long total = (long long)raw.carry + (long long)n;
    const int failed = so->overflow;
    const unsigned long long nf = failed ? 0ull : so->nflags;
    // emitted_k = valid_k and not emitted_(k-1): each thread's chunk as a map of the incoming bit, composed by thread 0, then replayed
    const unsigned long long chunk = (nf + 255) / 256, lo = min(nf, tid * chunk), hi = min(nf, lo + chunk);
    for (int e0 = 0; e0 < 2; e0++) {
        int e = e0;
        unsigned long long c = 0;
        for (unsigned long long k = lo; k < hi; k++) {
            e = valid[k] && !e;
            c += e;
        }
        s_to[e0][tid] = e;
        s_cnt[e0][tid] = c;
    }
    __syncthreads();
    if (tid == 0) {
        int e = 0;
        unsigned long long at = 0;
        for (int t = 0; t < 256; t++) {
            s_in[t] = e;
            s_base[t] = at;
            at += s_cnt[e][t];
            e = s_to[e][t];
        }
        s_last = e;
        s_total = at;
    }
    __syncthreads();
    {
        int e = s_in[tid];
        unsigned long long j = s_base[tid];
        for (unsigned long long k = lo; k < hi; k++) {
            e = valid[k] && !e;
            if (e) {
                if (j < max_frames) segs[j] = k;
                j++;
            }
        }
    }
    // the next call: a frame is open behind the last consumed flag unless that flag closed an emitted frame, and not once 3185 raw bytes have been
    // followed by a buffer that is no flag (every position up to total - 8 has been tested)
    const int overflow = failed || s_total > max_frames;
    long long s = nf ? flags[nf - 1] + 8 : 0;
    bool open = nf ? !s_last : si->mode == AX_FRAME;
    if (open && total - 8 - s >= AX_RAW_MAX) open = false;
    if (!open && total - 7 > s) s = total - 7;
    const int next = overflow ? 0 : (int)(total - s);                    // <= AX_RAW_MAX + 7 < AX_CARRY
    for (int i = tid; i < next; i += 256) carried_out[i] = (uint8_t)raw(s + i);
    if (tid == 0) {
        so->mode = open && !overflow ? AX_FRAME : AX_IDLE;
        so->carry = next;
        so->overflow = overflow;
        so->pad = 0;
        so->count = s_total;
    }
}

__global__ __launch_bounds__(64) void ax_emit_kernel(const uint8_t *__restrict__ x, const uint8_t *__restrict__ carried, const AxState *__restrict__ si,
                                                     const AxState *__restrict__ so, const uint16_t *__restrict__ rows,
                                                     const long long *__restrict__ flags, const unsigned long long *__restrict__ segs,
                                                     uint32_t *__restrict__ y, unsigned long cap)
{
    __shared__ uint8_t s_buf[AX_CARRY], s_oct[AX_DATA];
    __shared__ uint16_t s_rows[AX_CRC_ROWS];
    const int lane = threadIdx.x;
    unsigned long long nframes = so->overflow ? 0ull : so->count;
    if (nframes > cap) nframes = cap;
    if (blockIdx.x >= nframes) return;
    const BsStream raw{x, carried, si->carry};
    for (int i = lane; i < AX_CRC_ROWS; i += 64) s_rows[i] = rows[i];
    __syncthreads();
    for (unsigned long long f = blockIdx.x; f < nframes; f += gridDim.x) {
        const unsigned long long k = segs[f];
        const long long s = ax_segment_start(flags, k);
        ax_evaluate(raw, s, flags[k] - s, lane, s_buf, s_oct, s_rows, y + f * (AX_REC / 4));
    }
}

}  // namespace lrhip
