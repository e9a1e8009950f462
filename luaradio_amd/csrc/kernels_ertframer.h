// kernels_ertframer.h - SCMFramerBlock, SCMPlusFramerBlock and IDMFramerBlock (radio/blocks/protocol/scmframer.lua:166-211,
// scmplusframer.lua:181-225, idmframer.lua:187-243): Bit -> one fixed record per frame (include/lrhip.h).  One kernel family over EfProto<K>:
//                       L    preamble / sync       codeword at, bits   initial syndrome   checks after the correction
//   EF_SCM     scm      96   21 bits 0x1f2a60      21, 75              0                  none
//   EF_SCMPLUS scm+    128   16 bits 0x16a3        16, 112             0x7b06             protocol_id == 0x1e
//   EF_IDM     idm     736   32 bits 0x555516a3    32, 704             0x866b             packet type 0x1c, length 0x5cc6, serial CRC
// The reference shifts bytes into a buffer of L and tests it whenever it is full: the preamble (Bit.tonumber: a byte counts as 1 only when it
// equals 1), then *_correct_codeword - the syndrome is the initial value XOR row i of the check matrix over the set bits i of the codeword; zero
// passes, the syndrome of exactly one row i passes after byte i has been replaced by (~b) & 1 (Bit:bnot) - then the protocol's remaining checks
// on the corrected buffer.  An accepted frame empties the buffer (the next window starts L bytes on), anything else shifts it by one.
//
// As for RDS (kernels_rdsframer.h) the automaton only hops, but two of the three tests are NOT a pure function of the window: the SCM+ and the
// IDM correction is made inside the shift buffer before the remaining checks run, so a window that corrects a byte and then fails a check is
// rejected with its flip left behind, seen by every later window that still holds the byte.  (SCM accepts whenever the codeword corrects.)  This
// happens in use: the IDM preamble ends in the SCM+ sync word, so the SCM+ framer of an ERT receiver meets a matching sync in every IDM frame,
// 113 of the 65 536 syndromes are zero or a single-bit error, and the IDM packet type 0x1c sits where SCM+ wants 0x1e.  A window is therefore
// classified three ways - reject, accept, MUTATING reject (non-zero correctable syndrome, then a failed check) - and the walk switches to a
// literal mode behind a mutating reject.
//
// Passes (3 launches, one count read-back), with u the index in "carried bytes, then this call's bytes":
//   ef_match_kernel  one workgroup per tile of PS_TILE window starts.  The `== 1` bytes of the tile and of the 31 behind it are packed into 64-bit
//                    words by wave ballots; each lane compares the preamble at one start on the funnel-shifted words.  The preamble matches at
//                    one start in 2^16 .. 2^32 of noise, so the codeword is evaluated only there, one wave per candidate (ef_classify): each
//                    lane XORs the rows of its share of the set bits (rows in LDS, loaded only by a tile that has a candidate), a butterfly of
//                    six cross-lane XORs gives the syndrome, the error index is the lane whose row equals it (compare + cross-lane max; no
//                    64 K-entry table), and every lane runs the remaining checks on the corrected bytes.  Stores the mask of "event" starts
//                    (accept or mutating reject), the mask of accepts and the tile's first event.  Windows that end beyond the stream are masked.
//   ef_walk_kernel   ONE workgroup.  From q, the first byte no accepted frame has consumed: q itself, else ps_find_first over the event mask.  An
//                    accept records its start and hops L.  A mutating reject enters the literal mode: windows s, s + 1, ... are evaluated one
//                    after another on the EFFECTIVE bytes - the raw bytes under a ring of L override bytes in LDS, indexed by u mod L (a
//                    pending flip lies inside the current window, and one byte leaves the ring per step, so L entries always suffice) - adding
//                    flips as they occur, until a window is accepted (the buffer is emptied: all flips die) or no pending flip lies at or
//                    beyond the current start; then the masks are valid again.  A frame accepted in literal mode is written by the walk itself,
//                    from the effective bytes, and its start is recorded as -1 so that the emit pass skips it.  The walk also writes the next
//                    call's carried bytes: the effective bytes since q (at most L - 1), so a flip still pending at the end of a call survives it.
//                    The bytes are carried raw, not as 0 / 1: idm_compute_crc tells a byte of 2 from a byte of 0 (ef_idm_crc).
//   ef_emit_kernel   one wave per frame accepted from the masks recomputes its correction and writes the record: one 16-byte store for SCM and
//                    SCM+, eleven 8-byte stores (one lane each) for IDM.
// Carried between calls, ping-pong on the device: the effective bytes since q and EfState.
#pragma once
#include "common.h"
#include "kernels_bitscan.h"

namespace lrhip {

enum { EF_SCM = 0, EF_SCMPLUS = 1, EF_IDM = 2 };
enum { EF_REJECT = 0, EF_ACCEPT = 1, EF_MUTATE = 2 };
constexpr int EF_CARRY = 768;                                // bytes of one carried slot (at most 735 used)
constexpr int EF_NO_OVERRIDE = 0xff;                         // ring entry of a byte without a pending flip (an override is 0 or 1)

// The codeword starts where the preamble ends in all three protocols.
template <int K> struct EfProto;
template <> struct EfProto<EF_SCM> { static constexpr int L = 96, PRE = 21, CW = 75, REC = 16; static constexpr unsigned PATTERN = 0x1f2a60u, INIT = 0u; };
template <> struct EfProto<EF_SCMPLUS> { static constexpr int L = 128, PRE = 16, CW = 112, REC = 16; static constexpr unsigned PATTERN = 0x16a3u, INIT = 0x7b06u; };
template <> struct EfProto<EF_IDM> { static constexpr int L = 736, PRE = 32, CW = 704, REC = 88; static constexpr unsigned PATTERN = 0x555516a3u, INIT = 0x866bu; };

// idm_compute_crc (idmframer.lua:140-154) on byte values: (crc & 0x8000) ^ (b << 15) is compared with 0x8000, so a byte of 1 takes the XOR
// branch when the top bit is clear, a byte of 0 when it is set, and a byte of 2 or more never does
template <class Get> __host__ __device__ inline unsigned ef_idm_crc(const Get &get, int offset, int length)
{
    unsigned crc = 0xffffu;
    for (int i = 0; i < length; i++) {
        const unsigned b = get(offset + i);
        crc = (crc << 1) ^ ((((crc & 0x8000u) ^ (b << 15)) == 0x8000u) ? 0x1021u : 0u);
    }
    return (crc ^ 0xffffu) & 0xffffu;
}

// host: the check matrix, row i for codeword bit i.  SCM and SCM+ are the tables SCM_CHECK_SYNDROMES (scmframer.lua:53-73) and
// SCM_PLUS_CHECK_SYNDROMES (scmplusframer.lua:51-80): row i = x^(CW - 1 - i) modulo the generator 0x16f63 (SCM) / 0x11021 (SCM+), which is how
// they end in the identity.  IDM's is built as idm_initialize_crc does (idmframer.lua:156-176): the CRC of each unit message XOR 0x866b, then
// the identity for the 16 check bits.
inline void ef_rows(int kind, uint16_t *rows)
{
    if (kind == EF_IDM) {
        constexpr int CW = EfProto<EF_IDM>::CW, MSG = CW - 16;
        for (int i = 0; i < MSG; i++) rows[i] = (uint16_t)(ef_idm_crc([i](int k) { return k == i ? 1u : 0u; }, 0, MSG) ^ 0x866bu);
        for (int i = 0; i < 16; i++) rows[MSG + i] = (uint16_t)(1u << (15 - i));
        return;
    }
    const int cw = kind == EF_SCM ? EfProto<EF_SCM>::CW : EfProto<EF_SCMPLUS>::CW;
    const unsigned poly = kind == EF_SCM ? 0x6f63u : 0x1021u;
    unsigned r = 1;
    for (int i = cw - 1; i >= 0; i--) {
        rows[i] = (uint16_t)r;
        r <<= 1;
        if (r & 0x10000u) r ^= 0x10000u | poly;
    }
}

// carried between calls (ping-pong on the device)
struct EfState {
    int carry;                       // bytes since q, the first byte no accepted frame has consumed (0 .. L - 1)
    int overflow;                    // the frame list was too small (never, by the bound of EfStage)
    unsigned long long count;        // frames of the last call
};

// byte i of the window that starts at u = s, raw
struct EfWindow {
    BsStream raw;
    long long s;
    __device__ __forceinline__ unsigned operator()(int i) const { return raw(s + i); }
};

// byte i of the window that starts at u = s under the ring of pending flips: ring[u mod L] overrides byte u (at = s mod L, 0 <= i < L)
template <int L> struct EfRing {
    BsStream raw;
    const uint8_t *ring;
    long long s;
    int at;
    __device__ __forceinline__ unsigned operator()(int i) const
    {
        int k = at + i;
        if (k >= L) k -= L;
        const unsigned o = ring[k];
        return o != EF_NO_OVERRIDE ? o : raw(s + i);
    }
};

// a window with byte `flip` corrected as Bit:bnot does (flip < 0: none)
template <class Get> struct EfCorrected {
    const Get &get;
    int flip;
    __device__ __forceinline__ unsigned operator()(int i) const
    {
        const unsigned b = get(i);
        return i == flip ? (~b & 1u) : b;
    }
};

// Bit.tonumber(offset, length <= 32), MSB first
template <class Get> __device__ __forceinline__ unsigned ef_num(const Get &get, int offset, int length)
{
    unsigned v = 0;
    for (int i = 0; i < length; i++) v = (v << 1) | (get(offset + i) == 1u ? 1u : 0u);
    return v;
}

// the checks behind *_correct_codeword (scmplusframer.lua:207-209, idmframer.lua:214-218), on the corrected window
template <int K, class Get> __device__ __forceinline__ bool ef_checks(const Get &get)
{
    if (K == EF_SCMPLUS) return ef_num(get, 16, 8) == 0x1eu;
    if (K == EF_IDM) return ef_num(get, 32, 8) == 0x1cu && ef_num(get, 40, 16) == 0x5cc6u && ef_num(get, 704, 16) == ef_idm_crc(get, 72, 32);
    return true;
}

// One wave classifies the window `get` whose preamble has matched (all 64 lanes call with the same window; every lane gets the same answer).
// *flip is the window index of the byte the correction replaces, -1 when there is none.
template <int K, class Get> __device__ int ef_classify(const Get &get, const uint16_t *rows, int lane, int *flip)
{
    using P = EfProto<K>;
    unsigned syn = 0;
    for (int i = lane; i < P::CW; i += 64)
        if (get(P::PRE + i) == 1u) syn ^= rows[i];
#pragma unroll
    for (int o = 32; o; o >>= 1) syn ^= (unsigned)__shfl_xor((int)syn, o);
    syn ^= P::INIT;
    int e = -1;
    if (syn) {
        // *_CORRECT_SYNDROMES[syndrome]: the row equal to the syndrome (the rows are distinct; were two equal, the table would hold the later)
        for (int i = lane; i < P::CW; i += 64)
            if (rows[i] == syn) e = i;
#pragma unroll
        for (int o = 32; o; o >>= 1) e = max(e, __shfl_xor(e, o));
        if (e < 0) { *flip = -1; return EF_REJECT; }
        e += P::PRE;
    }
    *flip = e;
    const EfCorrected<Get> fixed{get, e};
    if (ef_checks<K>(fixed)) return EF_ACCEPT;
    return e >= 0 ? EF_MUTATE : EF_REJECT;
}

// frame bit offset of the 8 bits (MSB first) of byte j of the IDM record, -1 for the pad: ert_id, last_consumption_count (u32), transmit_time_offset,
// serial_crc, packet_crc (u16), application_version, ert_type, then frame bits 104 .. 231 and 264 .. 687 in frame order
__device__ __forceinline__ int ef_idm_byte_at(int j)
{
    if (j < 4) return 72 + 8 * (3 - j);
    if (j < 8) return 232 + 8 * (7 - j);
    if (j < 10) return 688 + 8 * (9 - j);
    if (j < 12) return 704 + 8 * (11 - j);
    if (j < 14) return 720 + 8 * (13 - j);
    if (j == 14) return 56;
    if (j == 15) return 64;
    if (j < 32) return 104 + 8 * (j - 16);
    if (j < 85) return 264 + 8 * (j - 32);
    return -1;
}

// One wave writes the record of the corrected window `get` to rec (REC bytes, 8-byte aligned)
template <int K, class Get> __device__ void ef_write_record(const Get &get, int lane, unsigned long long *rec)
{
    typedef unsigned long long u64;
    if (K == EF_SCM) {
        if (lane == 0) {
            // ert_id u32, consumption u32 | crc u16, ert_type, physical_tamper, encoder_tamper, reserved, pad[2]  (scmframer.lua:192-201)
            const u64 ert_id = (ef_num(get, 21, 2) << 24) | ef_num(get, 56, 24);
            ulonglong2 r;
            r.x = ert_id | ((u64)ef_num(get, 32, 24) << 32);
            r.y = (u64)ef_num(get, 80, 16) | ((u64)ef_num(get, 26, 4) << 16) | ((u64)ef_num(get, 24, 2) << 24) | ((u64)ef_num(get, 30, 2) << 32) |
                  ((u64)ef_num(get, 23, 1) << 40);
            *(ulonglong2 *)rec = r;
        }
    } else if (K == EF_SCMPLUS) {
        if (lane == 0) {
            // ert_id u32, consumption u32 | tamper u16, crc u16, protocol_id, ert_type, pad[2]  (scmplusframer.lua:207-214)
            ulonglong2 r;
            r.x = (u64)ef_num(get, 32, 32) | ((u64)ef_num(get, 64, 32) << 32);
            r.y = (u64)ef_num(get, 96, 16) | ((u64)ef_num(get, 112, 16) << 16) | ((u64)ef_num(get, 16, 8) << 32) | ((u64)ef_num(get, 24, 8) << 40);
            *(ulonglong2 *)rec = r;
        }
    } else {
        if (lane < EfProto<EF_IDM>::REC / 8) {
            u64 w = 0;
            for (int b = 0; b < 8; b++) {
                const int at = ef_idm_byte_at(lane * 8 + b);
                if (at >= 0) w |= (u64)ef_num(get, at, 8) << (8 * b);
            }
            rec[lane] = w;
        }
    }
}

template <int K>
__global__ __launch_bounds__(256) void ef_match_kernel(const uint8_t *__restrict__ x, const uint8_t *__restrict__ carried, unsigned long n,
                                                       const EfState *__restrict__ si, const uint16_t *__restrict__ rows,
                                                       unsigned long long *__restrict__ mask_e, unsigned long long *__restrict__ mask_a,
                                                       int *__restrict__ tile_e)
{
    using P = EfProto<K>;
    __shared__ unsigned long long s_bits[PS_WORDS + 1];      // the tile and the PRE - 1 <= 31 bits behind it
    __shared__ unsigned long long s_cand[PS_WORDS], s_event[PS_WORDS], s_accept[PS_WORDS];
    __shared__ uint16_t s_rows[P::CW];
    __shared__ int any;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const BsStream raw{x, carried, si->carry};
    const long long total = (long long)raw.carry + (long long)n, base = (long long)blockIdx.x * PS_TILE;
    if (tid == 0) any = 0;
    bs_pack(raw, base, total, PS_WORDS + 1, s_bits);
    __syncthreads();
    for (int w = wave; w < PS_WORDS; w += 4) {
        // the PRE bits from start 64 w + lane, bit k = the k-th received (PATTERN is MSB first); only windows that end inside the stream:
        // s + L <= total
        const unsigned r = (unsigned)bs_window(s_bits, w, lane) & (unsigned)((1ull << P::PRE) - 1ull);
        const unsigned long long c = __ballot(r == bs_stream_order(P::PATTERN, P::PRE) && base + w * 64 + lane + P::L <= total);
        if (lane == 0) {
            s_cand[w] = c;
            if (c) any = 1;
        }
    }
    __syncthreads();
    const bool some = any != 0;                              // the same in every thread
    if (some) {
        for (int i = tid; i < P::CW; i += 256) s_rows[i] = rows[i];
        __syncthreads();
    }
    for (int w = wave; w < PS_WORDS; w += 4) {
        unsigned long long c = some ? s_cand[w] : 0ull, ev = 0, ac = 0;
        while (c) {
            const int j = __ffsll((long long)c) - 1;
            c &= c - 1;
            const EfWindow win{raw, base + w * 64 + j};
            int flip;
            const int cls = ef_classify<K>(win, s_rows, lane, &flip);
            if (cls != EF_REJECT) ev |= 1ull << j;
            if (cls == EF_ACCEPT) ac |= 1ull << j;
        }
        if (lane == 0) { s_event[w] = ev; s_accept[w] = ac; }
    }
    __syncthreads();
    bs_store_tile(s_event, mask_e, tile_e);
    if (tid < PS_WORDS) mask_a[(unsigned long)blockIdx.x * PS_WORDS + tid] = s_accept[tid];
}

template <int K>
__global__ __launch_bounds__(256) void ef_walk_kernel(const uint8_t *__restrict__ x, const uint8_t *__restrict__ carried, uint8_t *__restrict__ carried_out,
                                                      unsigned long n, const EfState *__restrict__ si, EfState *__restrict__ so,
                                                      const uint16_t *__restrict__ rows, const unsigned long long *__restrict__ mask_e,
                                                      const unsigned long long *__restrict__ mask_a, const int *__restrict__ tile_e, unsigned long ntiles,
                                                      long long *__restrict__ starts, unsigned long long *__restrict__ y, unsigned long max_frames)
{
    using P = EfProto<K>;
    __shared__ unsigned long long s_res;
    __shared__ uint16_t s_rows[P::CW];
    __shared__ uint8_t s_ring[P::L];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const BsStream raw{x, carried, si->carry};
    const long long total = (long long)raw.carry + (long long)n;
    for (int i = tid; i < P::CW; i += 256) s_rows[i] = rows[i];
    for (int i = tid; i < P::L; i += 256) s_ring[i] = EF_NO_OVERRIDE;
    __syncthreads();
    long long q = 0;
    unsigned long long nframes = 0;
    int overflow = 0;
    // every thread runs the same automaton on the same values (each wave classifies for itself); thread 0 and wave 0 write
    while (q + P::L <= total) {
        long long s = q;
        if (!bs_test(mask_e, q)) {
            s = ps_find_first(mask_e, tile_e, ntiles, q, &s_res);
            if (s == PS_NONE) { q = total - (P::L - 1); break; }         // every window up to total - L was rejected without a trace
        }
        if (nframes >= max_frames) { overflow = 1; break; }
        if (bs_test(mask_a, s)) {
            if (tid == 0) starts[nframes] = s;
            nframes++;
            q = s + P::L;
            continue;
        }
        // a mutating reject at s: the literal mode, window by window on the effective bytes, while a flip is pending at or beyond the start
        long long t = s, last_flip = -1;
        for (;;) {
            const EfRing<P::L> win{raw, s_ring, t, (int)(t % P::L)};
            int cls = EF_REJECT, flip = -1;
            if (ef_num(win, 0, P::PRE) == P::PATTERN) cls = ef_classify<K>(win, s_rows, lane, &flip);
            unsigned flipped = 0;
            if (cls == EF_ACCEPT) {
                if (nframes >= max_frames) { overflow = 1; break; }
                const EfCorrected<EfRing<P::L>> fixed{win, flip};
                if (wave == 0) ef_write_record<K>(fixed, lane, y + nframes * (P::REC / 8));
                if (tid == 0) starts[nframes] = -1;                       // written here: the emit pass skips it
            } else if (cls == EF_MUTATE) {
                flipped = ~win(flip) & 1u;
            }
            __syncthreads();                                              // every read of the ring for window t is done
            if (cls == EF_ACCEPT) {
                for (int i = tid; i < P::L; i += 256) s_ring[i] = EF_NO_OVERRIDE;          // the buffer is emptied: all flips die
            } else if (tid == 0) {
                if (cls == EF_MUTATE) s_ring[(win.at + flip) % P::L] = (uint8_t)flipped;
                s_ring[win.at] = EF_NO_OVERRIDE;                          // byte t leaves the buffer (flip >= PRE > 0: another entry)
            }
            __syncthreads();
            if (cls == EF_ACCEPT) { nframes++; q = t + P::L; break; }
            if (cls == EF_MUTATE) last_flip = max(last_flip, t + flip);
            t++;
            q = t;
            if (last_flip < t) break;                                     // no flip is pending: the masks hold from here
            if (t + P::L > total) break;                                  // the call ends with flips pending: they go into the carried bytes
        }
        if (overflow) break;
    }
    // the next call's carried bytes: the effective bytes since q
    const int next = overflow ? 0 : (int)(total - q);                    // <= L - 1 < EF_CARRY
    for (int i = tid; i < next; i += 256) {
        const long long u = q + i;
        const unsigned o = s_ring[(int)(u % P::L)];
        carried_out[i] = (uint8_t)(o != EF_NO_OVERRIDE ? o : raw(u));
    }
    if (tid == 0) {
        so->carry = next;
        so->overflow = overflow;
        so->count = nframes;
    }
}

template <int K>
__global__ __launch_bounds__(256) void ef_emit_kernel(const uint8_t *__restrict__ x, const uint8_t *__restrict__ carried, unsigned long n,
                                                      const EfState *__restrict__ si, const EfState *__restrict__ so, const uint16_t *__restrict__ rows,
                                                      const long long *__restrict__ starts, unsigned long long *__restrict__ y, unsigned long cap)
{
    using P = EfProto<K>;
    __shared__ uint16_t s_rows[P::CW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned long long nframes = so->overflow ? 0ull : so->count;
    if ((unsigned long long)blockIdx.x * 4 >= nframes) return;
    for (int i = tid; i < P::CW; i += 256) s_rows[i] = rows[i];
    __syncthreads();
    const unsigned long long f = (unsigned long long)blockIdx.x * 4 + wave;
    if (f >= nframes || f >= cap) return;
    const long long s = starts[f];
    if (s < 0) return;                                                    // accepted in literal mode: the walk has written it
    const EfWindow win{BsStream{x, carried, si->carry}, s};
    int flip;
    ef_classify<K>(win, s_rows, lane, &flip);
    const EfCorrected<EfWindow> fixed{win, flip};
    ef_write_record<K>(fixed, lane, y + f * (P::REC / 8));
}

}  // namespace lrhip
