// kernels_source.h - the generator sources: SignalSource (radio/blocks/sources/signal.lua) and UniformRandomSource (uniformrandom.lua).
// No input: sample n is a closed-form function of the parameters and the ABSOLUTE index n, so any chunking, any seek and any time partition
// give the same bits (the contract of the translator above, kernels_elem.h:12-15; the reference's running phase and math.random can do neither).
//
// SignalSource.  turns(n) = p0 + n * step in wrapping 0.64 fixed point (p0 = phase / 2 pi, step = frequency / rate, both as fractions of a turn).
//   exponential           amplitude * (c, s), (c, s) = phasor_from_turns(turns) of kernels_elem.h; the offset is ignored (signal.lua:80-94)
//   cosine / sine         c * amplitude + offset / s * amplitude + offset
//   square                w = turns < 2^63 ? 1 : -1                                            }
//   triangle              w = turns < 2^63 ? 1 - 4 td : 4 td - 3,  td = (turns >> 11) * 2^-53   }  w * amplitude + offset
//   sawtooth              w = 2 td - 1                                                         }
//   constant              amplitude
// The products and sums are double (one multiply, one add, not contracted: a numpy restatement is bit-equal) and round once to Float32.
// The phasor is evaluated PER SAMPLE: one polynomial of ~25 VALU operations per output, so the value is a function of turns(n) alone.  The translator's
// block-of-8 form (P(n & ~7) * W[n & 7]) trades polynomials for complex multiplies and a second rounding; it was not needed: at 2^26 samples the cosine
// writes 0.98 and the exponential 0.96 of the bytes per second of the streaming yardstick in the same run - the stores are the bound.
//
// UniformRandomSource.  Word j of the stream is output (j & 3) of Philox4x32-10 with counter (lo32(j >> 2), hi32(j >> 2), 0, 0) and key
// (lo32(seed), hi32(seed)); u(j) = w(j) * 2^-32.
//   Float32               lo + (hi - lo) * u(n)                     ComplexFloat32     re from w(2 n), im from w(2 n + 1)
//   Byte                  lo + ((w(n) * (hi - lo + 1)) >> 32)       Bit                w(n) >> 31
// One Philox call fills a 16-byte store of Float32 or ComplexFloat32 when the store starts on a multiple of four words (always, unless the stream
// was cut or sought at an index that is not one); otherwise two calls do.
//
// The kernels only write: a lane stores 16-byte vectors, consecutive lanes consecutive vectors, SRC_U stores per thread 256 vectors apart
// (kernels_modulator.h has the shape).  The thread behind the last whole vector writes the samples that do not fill one; an output pointer that
// is not 16-byte aligned takes the one-sample-per-thread kernel.
// (part of liblrhip.so; included by lrhip.hip in this order, one translation unit)
#pragma once
#include "kernels_elem.h"

namespace lrhip {

constexpr int SRC_U = 4;                 // 16-byte stores per thread, 256 stores apart

// a * b + c as one double multiply and one double add: the compiler's default contraction into a single fused operation is switched off here,
// so that the value is the one plain IEEE double arithmetic gives on any host
__device__ __forceinline__ double src_mul_add(double a, double b, double c)
{
#pragma clang fp contract(off)
    const double prod = a * b;
    return prod + c;
}

enum { SRC_EXPONENTIAL = 0, SRC_COSINE, SRC_SINE, SRC_SQUARE, SRC_TRIANGLE, SRC_SAWTOOTH, SRC_CONSTANT };
enum { RND_CF32 = 0, RND_F32, RND_BYTE, RND_BIT };

// ---- SignalSource -----------------------------------------------------------------------------------------------------------------------------
template <int SIG>
struct SigGen {
    typedef float T;
    static constexpr int PER = 4;
    uint64_t p0, step;
    double amp, off;
    __device__ __forceinline__ float at(uint64_t n) const
    {
        if (SIG == SRC_CONSTANT) return (float)amp;
        const uint64_t t = p0 + n * step;
        double w;
        if (SIG == SRC_COSINE || SIG == SRC_SINE) {
            float c, s;
            phasor_from_turns(t, c, s);
            w = (double)(SIG == SRC_COSINE ? c : s);
        } else {
            const double td = (double)(t >> 11) * 0x1p-53;          // exact: 53 bits
            const bool first = t < (1ull << 63);
            if (SIG == SRC_SQUARE) w = first ? 1.0 : -1.0;
            else if (SIG == SRC_TRIANGLE) w = first ? 1.0 - 4.0 * td : 4.0 * td - 3.0;      // (4 td is exact, so fused or not is the same value)
            else w = 2.0 * td - 1.0;
        }
        return (float)src_mul_add(w, amp, off);
    }
    __device__ __forceinline__ float4 item(uint64_t n) const { return make_float4(at(n), at(n + 1), at(n + 2), at(n + 3)); }
};

struct ExpGen {
    typedef float2 T;
    static constexpr int PER = 2;
    uint64_t p0, step;
    double amp;
    __device__ __forceinline__ float2 at(uint64_t n) const
    {
        float c, s;
        phasor_from_turns(p0 + n * step, c, s);
        return make_float2((float)((double)c * amp), (float)((double)s * amp));
    }
    __device__ __forceinline__ float4 item(uint64_t n) const
    {
        const float2 a = at(n), b = at(n + 1);
        return make_float4(a.x, a.y, b.x, b.y);
    }
};

// ---- UniformRandomSource ----------------------------------------------------------------------------------------------------------------------
// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11) on counter (lo32(b), hi32(b), 0, 0)
__device__ __forceinline__ void philox4x32_10(uint64_t b, uint64_t seed, uint32_t (&w)[4])
{
    uint32_t c0 = (uint32_t)b, c1 = (uint32_t)(b >> 32), c2 = 0, c3 = 0;
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
    for (int r = 0; r < 10; r++) {
        const uint64_t m0 = (uint64_t)0xD2511F53u * c0, m1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(m1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(m0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)m1; c3 = (uint32_t)m0; c0 = n0; c2 = n2;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    w[0] = c0; w[1] = c1; w[2] = c2; w[3] = c3;
}
// words j .. j + 3 of the stream: one call when j is a multiple of four (wave-uniform: j = base + 4 i), else two
__device__ __forceinline__ void philox_words4(uint64_t j, uint64_t seed, uint32_t (&w)[4])
{
    uint32_t a[4];
    philox4x32_10(j >> 2, seed, a);
    const unsigned r = (unsigned)j & 3u;
    if (r == 0) { w[0] = a[0]; w[1] = a[1]; w[2] = a[2]; w[3] = a[3]; return; }
    uint32_t c[4];
    philox4x32_10((j >> 2) + 1, seed, c);
    // constant register indices in every arm
    if (r == 1) { w[0] = a[1]; w[1] = a[2]; w[2] = a[3]; w[3] = c[0]; }
    else if (r == 2) { w[0] = a[2]; w[1] = a[3]; w[2] = c[0]; w[3] = c[1]; }
    else { w[0] = a[3]; w[1] = c[0]; w[2] = c[1]; w[3] = c[2]; }
}
__device__ __forceinline__ uint32_t philox_word(uint64_t j, uint64_t seed)
{
    uint32_t a[4];
    philox4x32_10(j >> 2, seed, a);
    const unsigned r = (unsigned)j & 3u;
    return r == 0 ? a[0] : r == 1 ? a[1] : r == 2 ? a[2] : a[3];
}

struct RndParams {
    uint64_t seed;
    double lo, span;                     // the float types: lo, hi - lo
    uint32_t blo, bcount;                // Byte: lo, hi - lo + 1
};
__device__ __forceinline__ float rnd_float(const RndParams &p, uint32_t w) { return (float)src_mul_add(p.span, (double)w * 0x1p-32, p.lo); }
template <int KIND>
__device__ __forceinline__ uint8_t rnd_small(const RndParams &p, uint32_t w)
{
    return KIND == RND_BIT ? (uint8_t)(w >> 31) : (uint8_t)(p.blo + (uint32_t)(((uint64_t)w * p.bcount) >> 32));
}

struct RndF32Gen {
    typedef float T;
    static constexpr int PER = 4;
    RndParams p;
    __device__ __forceinline__ float at(uint64_t n) const { return rnd_float(p, philox_word(n, p.seed)); }
    __device__ __forceinline__ float4 item(uint64_t n) const
    {
        uint32_t w[4];
        philox_words4(n, p.seed, w);
        return make_float4(rnd_float(p, w[0]), rnd_float(p, w[1]), rnd_float(p, w[2]), rnd_float(p, w[3]));
    }
};
struct RndCf32Gen {
    typedef float2 T;
    static constexpr int PER = 2;
    RndParams p;
    __device__ __forceinline__ float2 at(uint64_t n) const
    {
        uint32_t a[4];
        philox4x32_10(n >> 1, p.seed, a);          // words 2 n and 2 n + 1 lie in one call
        return (n & 1) ? make_float2(rnd_float(p, a[2]), rnd_float(p, a[3])) : make_float2(rnd_float(p, a[0]), rnd_float(p, a[1]));
    }
    __device__ __forceinline__ float4 item(uint64_t n) const
    {
        uint32_t w[4];
        philox_words4(2 * n, p.seed, w);
        return make_float4(rnd_float(p, w[0]), rnd_float(p, w[1]), rnd_float(p, w[2]), rnd_float(p, w[3]));
    }
};
template <int KIND>
struct RndSmallGen {
    typedef uint8_t T;
    static constexpr int PER = 16;
    RndParams p;
    __device__ __forceinline__ uint8_t at(uint64_t n) const { return rnd_small<KIND>(p, philox_word(n, p.seed)); }
    __device__ __forceinline__ float4 item(uint64_t n) const
    {
        uint32_t q[4];
#pragma unroll
        for (int g = 0; g < 4; g++) {
            uint32_t w[4];
            philox_words4(n + 4 * (uint64_t)g, p.seed, w);
            q[g] = (uint32_t)rnd_small<KIND>(p, w[0]) | (uint32_t)rnd_small<KIND>(p, w[1]) << 8 | (uint32_t)rnd_small<KIND>(p, w[2]) << 16 |
                   (uint32_t)rnd_small<KIND>(p, w[3]) << 24;
        }
        float4 v;
        __builtin_memcpy(&v, q, sizeof(float4));
        return v;
    }
};

// ---- the two kernel forms ---------------------------------------------------------------------------------------------------------------------
// y 16-byte aligned; `nitems` whole stores of G::PER samples; the thread that would own store number `nitems` writes the samples behind them.
// n0: the absolute index of the call's first sample.  A workgroup covers 256 * SRC_U * G::PER samples.
template <typename G>
__global__ __launch_bounds__(256) void source_vec_kernel(float4 *__restrict__ y, G g, uint64_t n0, unsigned long nitems, unsigned long n_out)
{
    const unsigned long i0 = (unsigned long)blockIdx.x * (256 * SRC_U) + threadIdx.x;
    float4 w[SRC_U];
#pragma unroll
    for (int j = 0; j < SRC_U; j++) {
        const unsigned long i = i0 + 256ul * j;
        w[j] = i < nitems ? g.item(n0 + (uint64_t)i * G::PER) : float4{};
    }
#pragma unroll
    for (int j = 0; j < SRC_U; j++) {
        const unsigned long i = i0 + 256ul * j;
        if (i < nitems) nt_store(y + i, w[j]);
        else if (i == nitems)
            for (unsigned long o = nitems * G::PER; o < n_out; o++) reinterpret_cast<typename G::T *>(y)[o] = g.at(n0 + o);
    }
}

// an output pointer that is not 16-byte aligned (a slice of a caller's vector may start anywhere): one sample per thread
template <typename G>
__global__ __launch_bounds__(256) void source_scalar_kernel(typename G::T *__restrict__ y, G g, uint64_t n0, unsigned long n_out)
{
    const unsigned long o = (unsigned long)blockIdx.x * 256 + threadIdx.x;
    if (o < n_out) y[o] = g.at(n0 + o);
}

}  // namespace lrhip
