// kernels_fecglue.h - PunctureBlock, DepunctureBlock, ConvolutionalInterleaverBlock / ConvolutionalDeinterleaverBlock and AdditiveScramblerBlock:
// the glue between the convolutional and the Reed-Solomon stages, none of them a block of the reference.  fecglue_plan.h has the rules; all four
// kernels move bytes and interpret none (depuncture's Bit input apart), on indices that the stage hands in relative to the absolute stream.
//
// Stores.  The three kernels with byte outputs write ALIGNED 16-byte words whatever the output pointer is: with a = (address of y) mod 16, word w holds
// the outputs 16 w - a .. 16 w - a + 15; a lane builds one word in registers and stores it once, and the at most two words that stick out of
// [0, n) go byte by byte.  Divisions by a frame length, a table length or the branch count are made once per word and the index then steps; a call
// below 2^32 elements makes them in 32 bits.
// Puncture / depuncture.  [carry | x] is the virtual stream of stage_reedsolomon.h's FramedStage, counted in elements; the map of a frame (64 bytes,
// fecglue_plan.h) sits in LDS.  The puncturer gathers single bytes: neighbouring lanes read neighbouring frames, every line is requested a few times
// and served by the vector cache.  The depuncturer is one lane per Float32 written.
// Scrambler.  The table lies in device memory with its first 15 bytes repeated behind it, so the 16 table bytes of a word are one unaligned load.
// Interleaver.  Output i is input i - d(i mod I) with delays d up to D = (I - 1) M I, so a tile of T outputs reads the T + D inputs that end with it.
// A workgroup copies them - the carried D bytes of the previous calls standing in front of the call's vector - into LDS with 16-byte loads that are
// aligned in memory and in LDS at once (the LDS image starts at the byte offset the input has within its 16-byte word), gathers each output byte from
// LDS and stores words.  A naive gather would request every input line I times; this one requests it 1 + D / T times.  One form serves both
// directions and every shape: the direction only decides which branch has which delay.
// (part of liblrhip.so; included by lrhip.hip in this order, one translation unit)
#pragma once
#include "common.h"
#include "fecglue_plan.h"

namespace lrhip {

constexpr int FG_NT = 256;

// v / m and v mod m for v below 2^32 (small) or not
__device__ __forceinline__ void fg_divmod(unsigned long v, uint32_t m, bool small, unsigned long *quot, uint32_t *rem)
{
    if (small) {
        *quot = (uint32_t)v / m;
        *rem = (uint32_t)v % m;
    } else {
        *quot = v / m;
        *rem = (uint32_t)(v % m);
    }
}

// PunctureBlock: output o = frame o div FO, kept element o mod FO; bytes
__global__ __launch_bounds__(FG_NT) void puncture_kernel(const uint8_t *__restrict__ carry, const uint8_t *__restrict__ x, uint8_t *__restrict__ y,
                                                         const uint8_t *__restrict__ map, uint32_t c, uint32_t fi, uint32_t fo, unsigned long n_out, int small)
{
    __shared__ uint8_t pos[fgplan::PATTERN_MAX];
    if (threadIdx.x < fgplan::PATTERN_MAX) pos[threadIdx.x] = map[threadIdx.x];
    __syncthreads();
    const unsigned a = (unsigned)((uintptr_t)y & 15);
    const unsigned long words = (n_out + a + 15) / 16;
    for (unsigned long w = (unsigned long)blockIdx.x * FG_NT + threadIdx.x; w < words; w += (unsigned long)gridDim.x * FG_NT) {
        const long o0 = (long)(16 * w) - (long)a;
        const unsigned long lo = o0 < 0 ? 0ul : (unsigned long)o0, hi = (unsigned long)(o0 + 16) < n_out ? (unsigned long)(o0 + 16) : n_out;
        unsigned long f;
        uint32_t k;
        fg_divmod(lo, fo, small != 0, &f, &k);
        uint64_t v = (uint64_t)f * fi;                                   // the first element of the frame in [carry | x]
        if (hi - lo == 16) {
            uint32_t word[4] = {0, 0, 0, 0};
#pragma unroll
            for (int b = 0; b < 16; b++) {
                word[b >> 2] |= (uint32_t)rs_fetch(carry, x, c, v + pos[k]) << (8 * (b & 3));
                if (++k == fo) { k = 0; v += fi; }
            }
            *(uint4 *)(y + lo) = make_uint4(word[0], word[1], word[2], word[3]);
        } else {
            for (unsigned long o = lo; o < hi; o++) {
                y[o] = rs_fetch(carry, x, c, v + pos[k]);
                if (++k == fo) { k = 0; v += fi; }
            }
        }
    }
}

// DepunctureBlock: output o = frame o div FO, position j = o mod FO: the input element map[j] of the frame as its 32 bits (LLR) or +-1.0f from bit 0 of
// a byte (BIT), +0.0f where map[j] says punctured.  carry, x: elements of 4 bytes (LLR) or 1
template <bool BIT>
__global__ __launch_bounds__(FG_NT) void depuncture_kernel(const void *__restrict__ carry, const void *__restrict__ x, uint32_t *__restrict__ y,
                                                           const uint8_t *__restrict__ map, uint32_t c, uint32_t fi, uint32_t fo, unsigned long n_out, int small)
{
    __shared__ uint8_t pos[fgplan::PATTERN_MAX];
    if (threadIdx.x < fgplan::PATTERN_MAX) pos[threadIdx.x] = map[threadIdx.x];
    __syncthreads();
    for (unsigned long o = (unsigned long)blockIdx.x * FG_NT + threadIdx.x; o < n_out; o += (unsigned long)gridDim.x * FG_NT) {
        unsigned long f;
        uint32_t j;
        fg_divmod(o, fo, small != 0, &f, &j);
        const uint32_t m = pos[j];
        uint32_t bits = 0;                                               // +0.0f
        if (m != fgplan::PUNCTURED) {
            const uint64_t v = (uint64_t)f * fi + m;
            if (BIT) {
                const uint8_t b = v < c ? ((const uint8_t *)carry)[v] : ((const uint8_t *)x)[v - c];
                bits = (b & 1u) ? 0xBF800000u : 0x3F800000u;
            } else {
                bits = v < c ? ((const uint32_t *)carry)[v] : ((const uint32_t *)x)[v - c];
            }
        }
        y[o] = bits;
    }
}

// AdditiveScramblerBlock: y[o] = x[o] ^ table[(phase + o) mod P]; ext = the table and its first 15 bytes again (periodically, where P < 15)
__global__ __launch_bounds__(FG_NT) void scrambler_kernel(const uint8_t *__restrict__ x, uint8_t *__restrict__ y, const uint8_t *__restrict__ ext,
                                                          uint32_t phase, uint32_t P, unsigned long n, int small)
{
    const unsigned a = (unsigned)((uintptr_t)y & 15);
    const unsigned long words = (n + a + 15) / 16;
    for (unsigned long w = (unsigned long)blockIdx.x * FG_NT + threadIdx.x; w < words; w += (unsigned long)gridDim.x * FG_NT) {
        const long o0 = (long)(16 * w) - (long)a;
        const unsigned long lo = o0 < 0 ? 0ul : (unsigned long)o0, hi = (unsigned long)(o0 + 16) < n ? (unsigned long)(o0 + 16) : n;
        uint32_t t = small ? (phase + (uint32_t)lo % P) % P : fgplan::table_advance(phase, lo, P);      // phase < P <= 8192
        if (hi - lo == 16) {
            uint4 in, key;
            __builtin_memcpy(&in, x + lo, 16);
            __builtin_memcpy(&key, ext + t, 16);
            *(uint4 *)(y + lo) = make_uint4(in.x ^ key.x, in.y ^ key.y, in.z ^ key.z, in.w ^ key.w);
        } else {
            for (unsigned long o = lo; o < hi; o++, t++) y[o] = (uint8_t)(x[o] ^ ext[t]);      // t < P + 15
        }
    }
}

// ConvolutionalInterleaverBlock / ConvolutionalDeinterleaverBlock.  V = [carry (D bytes) | x (n bytes)]: output o is V[D + o - d(j)], j = (q0 + o) mod I,
// d(j) = j M I (interleaver) or (I - 1 - j) M I (deinterleaver).  A tile is T outputs (T a multiple of 16) counted in the aligned words of y;
// its LDS image is V[lo .. hi + D) from LDS byte s on.  Dynamic LDS: T + D + 32 bytes
__global__ __launch_bounds__(FG_NT) void convinterleave_kernel(const uint8_t *__restrict__ carry, const uint8_t *__restrict__ x, uint8_t *__restrict__ y,
                                                               uint32_t I, uint32_t M, uint32_t D, int deinterleave, uint32_t q0, unsigned long n, uint32_t T,
                                                               int small)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t fg_lds[];
    const unsigned a = (unsigned)((uintptr_t)y & 15);
    const uint32_t MI = M * I;
    const unsigned long tiles = (n + a + T - 1) / T;
    for (unsigned long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const long t0 = (long)(tile * T) - (long)a;                      // the output of the tile's first word byte
        const unsigned long lo = t0 < 0 ? 0ul : (unsigned long)t0, hi = (unsigned long)(t0 + (long)T) < n ? (unsigned long)(t0 + (long)T) : n;
        const uint32_t s = (uint32_t)(((uintptr_t)x + lo - D) & 15);     // LDS byte s + u is V[lo + u], which lies at x + lo + u - D: the same byte of a word
        const uint32_t len = (uint32_t)(hi - lo) + D, nwords = (s + len + 15) / 16;
        for (uint32_t k = threadIdx.x; k < nwords; k += FG_NT) {
            const long v0 = (long)lo + 16 * (long)k - (long)s;           // V index of LDS byte 16 k
            uint4 word;
            if (v0 >= (long)D && (unsigned long)v0 + 16 <= (unsigned long)D + n) {
                word = *(const uint4 *)(x + (v0 - (long)D));             // aligned, by the choice of s
            } else if (v0 >= 0 && v0 + 16 <= (long)D) {
                __builtin_memcpy(&word, carry + v0, 16);
            } else {
                uint32_t part[4] = {0, 0, 0, 0};
#pragma unroll
                for (int b = 0; b < 16; b++) {
                    const long v = v0 + b;
                    uint32_t byte = 0;
                    if (v >= 0 && (unsigned long)v < (unsigned long)D + n) byte = v < (long)D ? carry[v] : x[v - (long)D];
                    part[b >> 2] |= byte << (8 * (b & 3));
                }
                word = make_uint4(part[0], part[1], part[2], part[3]);
            }
            ((uint4 *)fg_lds)[k] = word;
        }
        __syncthreads();
        const uint8_t *image = fg_lds + s + D;                           // image[o - lo - d] is output o
        for (uint32_t wl = threadIdx.x; wl < T / 16; wl += FG_NT) {
            const long o0 = t0 + 16 * (long)wl;
            if (o0 >= (long)hi) break;
            const unsigned long first = o0 < 0 ? 0ul : (unsigned long)o0, last = (unsigned long)(o0 + 16) < hi ? (unsigned long)(o0 + 16) : hi;
            unsigned long quot;
            uint32_t j;
            fg_divmod(first, I, small != 0, &quot, &j);
            j += q0;
            if (j >= I) j -= I;                                          // q0 < I
            uint32_t d = fgplan::branch_delay(j, I, M, deinterleave != 0);
            uint32_t u = (uint32_t)(first - lo);
            if (last - first == 16) {
                uint32_t part[4] = {0, 0, 0, 0};
#pragma unroll
                for (int b = 0; b < 16; b++, u++) {
                    part[b >> 2] |= (uint32_t)image[(int)u - (int)d] << (8 * (b & 3));
                    if (++j == I) { j = 0; d = deinterleave ? D : 0; } else { d = deinterleave ? d - MI : d + MI; }
                }
                *(uint4 *)(y + first) = make_uint4(part[0], part[1], part[2], part[3]);
            } else {
                for (unsigned long o = first; o < last; o++, u++) {
                    y[o] = image[(int)u - (int)d];
                    if (++j == I) { j = 0; d = deinterleave ? D : 0; } else { d = deinterleave ? d - MI : d + MI; }
                }
            }
        }
        __syncthreads();
    }
}

}  // namespace lrhip
