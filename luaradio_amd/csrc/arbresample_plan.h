// arbresample_plan.h - the position arithmetic of the arbitrary-ratio resampler (ArbitraryResamplerBlock): where output m sits in the input stream,
// how many outputs a stream of Q inputs has produced, where a seek lands.  Shared by the stage (stage_arbresample.h), the kernel
// (kernels_arbresample.h) and a CPU checker (tools/host_arbresample_check.hip).  Host + device, plain integer C++: no HIP call, no header of the library.
//
// The position of absolute output m is u = m * step in 16.48 fixed point of an input sample, step = rint(2^48 / ratio), 2^44 <= step <= 2^52
// (ratios 16 .. 1/16).  With P = 2^log2p phases:
//     i  = u >> 48                                   the newest input sample the output reads (taps reach back to i - (T - 1))
//     f  = u & (2^48 - 1)
//     p  = f >> (48 - log2p)                         the coefficient row
//     mu = ((f >> (24 - log2p)) & (2^24 - 1)) * 2^-24   the weight of row p + 1 against row p, exact in Float32
// m goes up to 2^64 - 1, so u needs 116 bits and i up to 68: the product is formed in unsigned __int128 and i is handed out in two 64-bit pieces.
// A caller that knows i - Q0 to be small (the kernel: it lies inside the call's chunk and history) works with i_lo - Q0 modulo 2^64.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ARB_HD __host__ __device__
#else
#define ARB_HD
#endif

namespace arbplan {

typedef unsigned __int128 u128;

constexpr int FRAC_BITS = 48;
constexpr uint64_t STEP_MIN = 1ull << 44, STEP_MAX = 1ull << 52, ONE = 1ull << FRAC_BITS;     // ratio 16 .. 1/16
constexpr int LOG2P_MIN = 4, LOG2P_MAX = 8;                                                    // 16 .. 256 phases
constexpr int T_MIN = 4, T_MAX = 512, TABLE_MAX = 8192;                                        // taps per phase; P * T, 64 KB of {G, D} pairs

struct Pos {
    uint64_t i_hi, i_lo;      // i = i_hi * 2^64 + i_lo
    uint32_t p, mu24;         // mu = mu24 * 2^-24
};

ARB_HD inline Pos position(uint64_t m, uint64_t step, int log2p)
{
    const u128 u = (u128)m * step;
    const u128 i = u >> FRAC_BITS;
    const uint64_t f = (uint64_t)u & (ONE - 1);
    Pos r;
    r.i_hi = (uint64_t)(i >> 64);
    r.i_lo = (uint64_t)i;
    r.p = (uint32_t)(f >> (FRAC_BITS - log2p));
    r.mu24 = (uint32_t)(f >> (24 - log2p)) & 0xFFFFFFu;
    return r;
}

// The divisions are host functions only (the device has no 128-bit divide, and needs none: counts come from the lengths, on the host)
// outputs that exist after Q inputs in total: the m with (m * step) >> 48 < Q, that is ceil(Q * 2^48 / step).  Up to 2^68: two pieces
struct Count { uint64_t hi, lo; };
inline Count output_count(uint64_t Q, uint64_t step)
{
    const u128 c = (((u128)Q << FRAC_BITS) + (step - 1)) / step;
    return Count{(uint64_t)(c >> 64), (uint64_t)c};
}
// the first output of a stream that continues at input n0 (seek): the same count
inline Count seek_output(uint64_t n0, uint64_t step) { return output_count(n0, step); }
// an upper bound of the outputs of ANY call of n inputs, whatever came before: floor(n * 2^48 / step) + 2 (saturating at 2^64 - 1)
inline uint64_t max_output(uint64_t n, uint64_t step)
{
    const u128 c = ((u128)n << FRAC_BITS) / step + 2;
    return (c >> 64) ? ~0ull : (uint64_t)c;
}

}  // namespace arbplan
