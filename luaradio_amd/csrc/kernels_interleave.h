// kernels_interleave.h - InterleaveBlock / DeinterleaveBlock (radio/blocks/signal/interleave.lua:47-58, deinterleave.lua:49-63) and the record
// side of WAVFileSink / WAVFileSource (sinks/wavfile.lua:171-176, sources/wavfile.lua:235-239): N planar streams <-> one interleaved stream,
// with the sample format conversion of kernels_elem.h in the same pass for the two WAV directions.
//
// Pure data movement, so the shape is set by the two memory sides.  A workgroup of 256 threads moves a tile of F frames (F * N elements):
//   planar side       every channel is read / written as 16 bytes per lane, contiguous across the wave;
//   interleaved side  the tile's F * N elements are one contiguous run, read / written as 16 bytes per lane, contiguous across the wave;
// and the transpose between the two goes through LDS.  The LDS image is PLANAR (row k = channel k, pitch F + 4 elements): the planar side moves
// whole 16-byte slots (ds_*_b128, consecutive lanes on consecutive slots), the interleaved side gathers / scatters the 16 / IB elements of its
// 16 bytes one by one, walking (frame, channel) incrementally from one division per lane.  Consecutive elements of a lane sit in consecutive rows;
// the pitch F + 4 with F a multiple of 16 puts rows 4 banks apart (N = 8: the two lanes that share a frame land 16 banks apart, N = 4: lanes read
// consecutive words of a row), so the element accesses stay at most two lanes to a bank for N = 2, 3, 4, 8 with 4- and 8-byte elements.  The WAV forms gather
// 8 (s16le) or 16 (u8) floats per lane, whose lanes step 8 / N or 16 / N words through a row: up to 8 (16) lanes to a bank for mono, paid in LDS
// cycles the double arithmetic next to them hides.
//
// F = IL_TILE_WORDS / (N * W) rounded down to a multiple of 16 (W = words per planar element), so the image stays 16 KiB + N rows of padding at every
// N, a tile starts on a 16-byte boundary of every stream whose pointer is 16-byte aligned (F * 4 W bytes planar, F * N * IB bytes interleaved, IB >= 1),
// and rows start on 16-byte LDS slots.
//
// Narrower paths, each a plain element-wise copy with consecutive lanes on consecutive elements: a port whose pointer is not 16-byte aligned (decided
// per port: the others keep their vectors), the last frames of a channel that do not fill 16 bytes, and the last elements of the tile's interleaved
// run that do not (frame sizes that are no multiple of 16 bytes end a tile anywhere).  No access leaves [ptr, ptr + count) of any port: every
// vector index is bounded by the whole vectors inside the port's count, every element index by the count.
// Traffic: every sample crosses HBM once in each direction.
// (part of liblrhip.so; included by lrhip.hip after kernels_elem.h, one translation unit)
#pragma once

namespace lrhip {

constexpr int IL_MAX_CH = 32;            // channels of one stage: the port pointers travel by value in the kernel's argument block
constexpr int IL_TILE_WORDS = 4096;      // 32-bit words of planar payload per workgroup tile
constexpr int IL_THREADS = 256;

struct IlPorts { void *p[IL_MAX_CH]; };

// frames per workgroup tile (host and device)
__host__ __device__ inline unsigned il_tile_frames(unsigned N, unsigned W) { return ((unsigned)IL_TILE_WORDS / (N * W)) & ~15u; }

// the forms: element copies of 4 and 8 bytes, and the three WAV sample formats (format_utils.lua: u8, s16le, s32le)
enum { IL_COPY4 = 0, IL_COPY8 = 1, IL_U8 = 2, IL_S16 = 3, IL_S32 = 4 };
template <int M> struct IlForm;
template <> struct IlForm<IL_COPY4> { static constexpr int W = 1; using I = uint32_t; using VAL = uint32_t; };
template <> struct IlForm<IL_COPY8> { static constexpr int W = 2; using I = uint2; using VAL = uint2; };
template <> struct IlForm<IL_U8> { static constexpr int W = 1; using I = uint8_t; using VAL = uint8_t; };
template <> struct IlForm<IL_S16> { static constexpr int W = 1; using I = uint16_t; using VAL = int16_t; };
template <> struct IlForm<IL_S32> { static constexpr int W = 1; using I = uint32_t; using VAL = int32_t; };

// planar LDS element (k, i) -> interleaved element
template <int M>
__device__ __forceinline__ typename IlForm<M>::I il_to_interleaved(const uint32_t *lds, unsigned at, double offset, double scale)
{
    using Fm = IlForm<M>;
    if constexpr (M == IL_COPY4) return lds[at];
    else if constexpr (M == IL_COPY8) return *reinterpret_cast<const uint2 *>(lds + 2 * at);
    else return format_pack_value<typename Fm::I, typename Fm::VAL, false>(__uint_as_float(lds[at]), offset, scale);
}
// interleaved element -> planar LDS element (k, i); lut: the 256 results of the 8-bit format
template <int M>
__device__ __forceinline__ void il_to_planar(uint32_t *lds, unsigned at, typename IlForm<M>::I e, const float *lut, double offset, double scale)
{
    using Fm = IlForm<M>;
    if constexpr (M == IL_COPY4) lds[at] = e;
    else if constexpr (M == IL_COPY8) *reinterpret_cast<uint2 *>(lds + 2 * at) = e;
    else if constexpr (M == IL_U8) lds[at] = __float_as_uint(lut[e]);
    else lds[at] = __float_as_uint(format_convert_value<typename Fm::I, typename Fm::VAL, false>(e, offset, scale));
}

constexpr int IL_LDS_SLOTS = IL_TILE_WORDS / 4 + IL_MAX_CH * 2;     // uint4 slots: the payload and 4 elements (of up to 2 words) of padding per row

// N planar inputs -> one interleaved output.  n: frames; aligned: bit k = port k may be read as uint4, bit 31 of aligned_out likewise for out
template <int M>
__global__ __launch_bounds__(IL_THREADS) void interleave_kernel(const IlPorts in, void *__restrict__ out, unsigned long n, unsigned N, unsigned aligned_in,
                                                                unsigned aligned_out, double offset, double scale)
{
    using Fm = IlForm<M>;
    using I = typename Fm::I;
    constexpr unsigned W = Fm::W, VE = 4 / W, S = 16 / sizeof(I);
    __shared__ uint4 lds4[IL_LDS_SLOTS];
    uint32_t *lds = reinterpret_cast<uint32_t *>(lds4);
    const unsigned F = il_tile_frames(N, W), Fp = F + 4, tid = threadIdx.x;
    const unsigned long f0 = (unsigned long)blockIdx.x * F;
    const unsigned nf = (unsigned)(n - f0 < F ? n - f0 : F);            // frames of this tile (the grid covers n: nf >= 1)
    const unsigned nv = nf / VE;                                         // whole 16-byte vectors per channel
    const bool all_aligned = aligned_in == (N >= 32 ? 0xffffffffu : (1u << N) - 1u);

    // ---- planar side: global -> LDS rows
    if (nv)
        for (unsigned idx = tid; idx < N * nv; idx += IL_THREADS) {
            const unsigned k = idx / nv, v = idx - k * nv;
            if (!((aligned_in >> k) & 1u)) continue;
            const uint4 *src = reinterpret_cast<const uint4 *>(static_cast<const uint32_t *>(in.p[k]) + f0 * W);
            lds4[(k * Fp * W) / 4 + v] = src[v];
        }
    if (all_aligned) {
        const unsigned tl = nf - nv * VE;                                // the frames behind the last whole vector (< VE)
        for (unsigned idx = tid; idx < N * tl; idx += IL_THREADS) {
            const unsigned k = idx / tl, i = nv * VE + (idx - k * tl);
            for (unsigned w = 0; w < W; w++) lds[(k * Fp + i) * W + w] = (static_cast<const uint32_t *>(in.p[k]) + f0 * W)[i * W + w];
        }
    } else {
        for (unsigned idx = tid; idx < N * nf; idx += IL_THREADS) {
            const unsigned k = idx / nf, i = idx - k * nf;
            if (((aligned_in >> k) & 1u) && i < nv * VE) continue;
            for (unsigned w = 0; w < W; w++) lds[(k * Fp + i) * W + w] = (static_cast<const uint32_t *>(in.p[k]) + f0 * W)[i * W + w];
        }
    }
    __syncthreads();

    // ---- interleaved side: LDS -> global, the tile's nf * N elements in order
    I *dst = static_cast<I *>(out) + f0 * N;
    const unsigned tot = nf * N, nvo = aligned_out ? tot / S : 0;
    for (unsigned q = tid; q < nvo; q += IL_THREADS) {
        unsigned i = (q * S) / N, k = q * S - i * N;
        I r[S];
#pragma unroll
        for (unsigned j = 0; j < S; j++) {
            r[j] = il_to_interleaved<M>(lds, k * Fp + i, offset, scale);
            if (++k == N) { k = 0; i++; }
        }
        uint4 o;
        __builtin_memcpy(&o, r, 16);
        reinterpret_cast<uint4 *>(dst)[q] = o;
    }
    for (unsigned e = nvo * S + tid; e < tot; e += IL_THREADS) {
        const unsigned i = e / N, k = e - i * N;
        dst[e] = il_to_interleaved<M>(lds, k * Fp + i, offset, scale);
    }
}

// one interleaved input -> N planar outputs.  n: interleaved elements (any count: port k receives ceil((n - k) / N))
template <int M>
__global__ __launch_bounds__(IL_THREADS) void deinterleave_kernel(const void *__restrict__ in, const IlPorts out, unsigned long n, unsigned N, unsigned aligned_in,
                                                                  unsigned aligned_out, double offset, double scale)
{
    using Fm = IlForm<M>;
    using I = typename Fm::I;
    constexpr unsigned W = Fm::W, VE = 4 / W, S = 16 / sizeof(I);
    __shared__ uint4 lds4[IL_LDS_SLOTS];
    __shared__ float lut[M == IL_U8 ? 256 : 1];
    uint32_t *lds = reinterpret_cast<uint32_t *>(lds4);
    const unsigned F = il_tile_frames(N, W), Fp = F + 4, tid = threadIdx.x;
    const unsigned long f0 = (unsigned long)blockIdx.x * F, e0 = f0 * N;
    const unsigned tot = (unsigned)(n - e0 < (unsigned long)F * N ? n - e0 : (unsigned long)F * N);      // interleaved elements of this tile (>= 1)
    if constexpr (M == IL_U8) {
        lut[tid] = format_convert_value<uint8_t, uint8_t, false>((uint8_t)tid, offset, scale);
        __syncthreads();
    }

    // ---- interleaved side: global -> LDS rows
    const I *src = static_cast<const I *>(in) + e0;
    const unsigned nvi = aligned_in ? tot / S : 0;
    for (unsigned q = tid; q < nvi; q += IL_THREADS) {
        const uint4 w = reinterpret_cast<const uint4 *>(src)[q];
        I r[S];
        __builtin_memcpy(r, &w, 16);
        unsigned i = (q * S) / N, k = q * S - i * N;
#pragma unroll
        for (unsigned j = 0; j < S; j++) {
            il_to_planar<M>(lds, k * Fp + i, r[j], lut, offset, scale);
            if (++k == N) { k = 0; i++; }
        }
    }
    for (unsigned e = nvi * S + tid; e < tot; e += IL_THREADS) {
        const unsigned i = e / N, k = e - i * N;
        il_to_planar<M>(lds, k * Fp + i, src[e], lut, offset, scale);
    }
    __syncthreads();

    // ---- planar side: LDS rows -> global; channel k holds cnt(k) = ceil((tot - k) / N) elements of this tile
    const unsigned c0 = (tot + N - 1) / N;                               // cnt(0), the largest
    const unsigned full = tot / N, part = tot - full * N;                // cnt(k) = full + (k < part)
    const unsigned nv0 = c0 / VE;
    const bool all_aligned = aligned_out == (N >= 32 ? 0xffffffffu : (1u << N) - 1u);
    if (nv0)
        for (unsigned idx = tid; idx < N * nv0; idx += IL_THREADS) {
            const unsigned k = idx / nv0, v = idx - k * nv0, cnt = full + (k < part ? 1u : 0u);
            if (!((aligned_out >> k) & 1u) || v >= cnt / VE) continue;
            reinterpret_cast<uint4 *>(static_cast<uint32_t *>(out.p[k]) + f0 * W)[v] = lds4[(k * Fp * W) / 4 + v];
        }
    if (all_aligned) {
        for (unsigned idx = tid; idx < N * VE; idx += IL_THREADS) {      // at most VE - 1 elements behind the last whole vector of each channel
            const unsigned k = idx / VE, cnt = full + (k < part ? 1u : 0u), i = cnt / VE * VE + (idx - k * VE);
            if (i >= cnt) continue;
            for (unsigned w = 0; w < W; w++) (static_cast<uint32_t *>(out.p[k]) + f0 * W)[i * W + w] = lds[(k * Fp + i) * W + w];
        }
    } else {
        for (unsigned idx = tid; idx < N * c0; idx += IL_THREADS) {
            const unsigned k = idx / c0, i = idx - k * c0, cnt = full + (k < part ? 1u : 0u);
            if (i >= cnt || (((aligned_out >> k) & 1u) && i < cnt / VE * VE)) continue;
            for (unsigned w = 0; w < W; w++) (static_cast<uint32_t *>(out.p[k]) + f0 * W)[i * W + w] = lds[(k * Fp + i) * W + w];
        }
    }
}

// Interleave of two channels without LDS (the A/B of stage_interleave.h): a lane loads 16 bytes of each channel and stores the 32 bytes they
// interleave to as two 16-byte vectors, 32 bytes from lane to lane - each store instruction covers every other 16 bytes of its lines, the second
// one fills them.  All three pointers 16-byte aligned; nitems = whole vectors per channel, the frames behind them by the spare thread.
template <int W>
__global__ __launch_bounds__(IL_THREADS) void interleave2_reg_kernel(const uint32_t *__restrict__ a, const uint32_t *__restrict__ b, uint32_t *__restrict__ out,
                                                                     unsigned long nitems, unsigned long n)
{
    constexpr unsigned VE = 4 / W;
    const unsigned long i = (unsigned long)blockIdx.x * IL_THREADS + threadIdx.x;
    if (i == nitems)
        for (unsigned long f = nitems * VE; f < n; f++)
            for (unsigned w = 0; w < (unsigned)W; w++) { out[(2 * f) * W + w] = a[f * W + w]; out[(2 * f + 1) * W + w] = b[f * W + w]; }
    if (i >= nitems) return;
    const uint4 x = reinterpret_cast<const uint4 *>(a)[i], y = reinterpret_cast<const uint4 *>(b)[i];
    uint4 lo, hi;
    if (W == 1) { lo = make_uint4(x.x, y.x, x.y, y.y); hi = make_uint4(x.z, y.z, x.w, y.w); }
    else { lo = make_uint4(x.x, x.y, y.x, y.y); hi = make_uint4(x.z, x.w, y.z, y.w); }
    reinterpret_cast<uint4 *>(out)[2 * i] = lo;
    reinterpret_cast<uint4 *>(out)[2 * i + 1] = hi;
}

}  // namespace lrhip
