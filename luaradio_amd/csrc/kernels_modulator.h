// kernels_modulator.h - PulseAmplitudeModulatorBlock / QuadratureAmplitudeModulatorBlock: Bit (1 B) -> Float32 / ComplexFloat32.
// b bits make one symbol value (a bit counts as 1 only when its byte equals 1, bit.lua:141), the symbol's table entry is held for P output samples
// (pulseamplitudemodulator.lua:69-87).  The bit stream of a call is the up to b - 1 bytes carried from the previous call followed by the call's input.
// The kernels are bound by their stores: a lane writes 16-byte vectors (4 Float32 or 2 ComplexFloat32 samples), consecutive lanes consecutive vectors;
// the bits come through L2 (one byte per bit, b bytes per symbol), the table from LDS up to 256 entries and from L2 above.
// (part of liblrhip.so; included by lrhip.hip in this order, one translation unit)
#pragma once

namespace lrhip {

constexpr int MOD_U = 4;                 // 16-byte stores per thread, 256 stores apart
constexpr int MOD_LDS_BITS = 8;          // tables of up to 2^8 entries are staged in LDS (2 KiB of ComplexFloat32)
constexpr int MOD_MAX_BITS = 16;         // 2^16 table entries at most; the carried bits fit 16 bytes

struct ModParams {
    unsigned P;                          // output samples per symbol
    int b, msb;                          // bits per symbol; 1: the first bit of a symbol is its most significant
    int pend;                            // bits carried in from the previous call (< b)
    unsigned long n, nsym;               // input bits of this call; symbols it completes: (pend + n) / b
};

// the value of symbol s of this call: stream positions s b .. s b + b - 1, position t < pend in the carried bytes, else x[t - pend]
__device__ __forceinline__ unsigned mod_symbol(const uint8_t *__restrict__ x, const uint8_t *__restrict__ carry, const ModParams &p, unsigned long s)
{
    const int b = p.b;
    const unsigned long t0 = s * (unsigned long)b;
    unsigned v = 0;
    if (t0 >= (unsigned long)p.pend) {
        const uint8_t *q = x + (t0 - (unsigned long)p.pend);
        for (int j = 0; j < b; j++) v |= (unsigned)(q[j] == 1) << (p.msb ? b - 1 - j : j);
    } else {
        for (int j = 0; j < b; j++) {
            const unsigned long t = t0 + (unsigned long)j;
            const uint8_t w = t < (unsigned long)p.pend ? carry[t] : x[t - (unsigned long)p.pend];
            v |= (unsigned)(w == 1) << (p.msb ? b - 1 - j : j);
        }
    }
    return v;
}

// the bits behind the last whole symbol become the next call's carried bytes (workgroup 0, the first b - 1 threads)
__device__ __forceinline__ void mod_carry(const uint8_t *__restrict__ x, const uint8_t *__restrict__ carry_in, uint8_t *__restrict__ carry_out, const ModParams &p)
{
    const unsigned long first = p.nsym * (unsigned long)p.b, left = (unsigned long)p.pend + p.n - first;
    if (blockIdx.x == 0 && threadIdx.x < left) {
        const unsigned long t = first + threadIdx.x;
        carry_out[threadIdx.x] = t < (unsigned long)p.pend ? carry_in[t] : x[t - (unsigned long)p.pend];
    }
}

// the table where the lookups read it: LDS up to 2^MOD_LDS_BITS entries (the caller synchronises), global memory above
template <typename T>
__device__ __forceinline__ const T *mod_stage_table(const T *__restrict__ gtab, T *sh_tab, int b)
{
    if (b > MOD_LDS_BITS) return gtab;
    for (unsigned e = threadIdx.x; e < (1u << b); e += 256) sh_tab[e] = gtab[e];
    return sh_tab;
}

template <typename T, int PER>
__device__ __forceinline__ float4 mod_pack(const T (&e)[PER])
{
    float4 w;
    __builtin_memcpy(&w, e, sizeof(float4));
    return w;
}

// P = 1, the plain symbol map: no position arithmetic at all.  y 16-byte aligned, `nitems` whole stores; the thread that would own store number
// `nitems` writes the samples behind them.
template <typename T, int PER>
__global__ __launch_bounds__(256) void mod_map_kernel(const uint8_t *__restrict__ x, const uint8_t *__restrict__ carry_in, uint8_t *__restrict__ carry_out,
                                                      const T *__restrict__ gtab, float4 *__restrict__ y, ModParams p, unsigned long nitems, unsigned long n_out)
{
    __shared__ T sh_tab[1 << MOD_LDS_BITS];
    const T *tab = mod_stage_table(gtab, sh_tab, p.b);
    mod_carry(x, carry_in, carry_out, p);
    __syncthreads();
    const unsigned long i0 = (unsigned long)blockIdx.x * (256 * MOD_U) + threadIdx.x;
    float4 w[MOD_U];
#pragma unroll
    for (int j = 0; j < MOD_U; j++) {
        const unsigned long i = i0 + 256ul * j;
        T e[PER] = {};
        if (i < nitems) {
#pragma unroll
            for (int k = 0; k < PER; k++) e[k] = tab[mod_symbol(x, carry_in, p, i * PER + k)];
        }
        w[j] = mod_pack<T, PER>(e);
    }
#pragma unroll
    for (int j = 0; j < MOD_U; j++) {
        const unsigned long i = i0 + 256ul * j;
        if (i < nitems) nt_store(y + i, w[j]);
        else if (i == nitems)
            for (unsigned long o = nitems * PER; o < n_out; o++) reinterpret_cast<T *>(y)[o] = tab[mod_symbol(x, carry_in, p, o)];
    }
}

// P >= 2: every symbol held for P samples.  A store may straddle a symbol boundary (odd P, or P < 4) and a symbol may span many workgroups (P in the
// thousands), so the position is (symbol, sample inside it): ONE 64-bit division per workgroup gives its first sample's pair, a 32-bit division per thread
// the thread's first store, and from store to store and sample to sample the pair is carried.  P < 2^30 (the stage refuses more), so the sums stay in 32 bits.
template <typename T, int PER>
__global__ __launch_bounds__(256) void mod_hold_kernel(const uint8_t *__restrict__ x, const uint8_t *__restrict__ carry_in, uint8_t *__restrict__ carry_out,
                                                       const T *__restrict__ gtab, float4 *__restrict__ y, ModParams p, unsigned long nitems, unsigned long n_out)
{
    __shared__ T sh_tab[1 << MOD_LDS_BITS];
    __shared__ unsigned long sh_s0;
    __shared__ unsigned sh_r0;
    const T *tab = mod_stage_table(gtab, sh_tab, p.b);
    mod_carry(x, carry_in, carry_out, p);
    const unsigned long i_base = (unsigned long)blockIdx.x * (256 * MOD_U);
    if (threadIdx.x == 0) {
        const unsigned long o0 = i_base * PER, s0 = o0 / p.P;
        sh_s0 = s0;
        sh_r0 = (unsigned)(o0 - s0 * p.P);
    }
    __syncthreads();
    const unsigned long s0 = sh_s0;
    const unsigned P = p.P, step = 256u * PER, dq = step / P, dr = step - dq * P;      // 256 stores further on
    const unsigned t = sh_r0 + threadIdx.x * PER;
    unsigned q = t / P, r = t - q * P;
    float4 w[MOD_U];
#pragma unroll
    for (int j = 0; j < MOD_U; j++) {
        const unsigned long i = i_base + threadIdx.x + 256ul * j;
        T e[PER] = {};
        if (i < nitems) {                                     // a whole store lies below n_out = nsym P, so every symbol it touches is below nsym
            unsigned long s = s0 + q;
            unsigned rr = r;
            T v = tab[mod_symbol(x, carry_in, p, s)];
#pragma unroll
            for (int k = 0; k < PER; k++) {
                e[k] = v;
                if (k + 1 < PER && ++rr == P) {
                    rr = 0;
                    v = tab[mod_symbol(x, carry_in, p, ++s)];
                }
            }
        }
        w[j] = mod_pack<T, PER>(e);
        q += dq; r += dr;
        if (r >= P) { r -= P; q++; }
    }
#pragma unroll
    for (int j = 0; j < MOD_U; j++) {
        const unsigned long i = i_base + threadIdx.x + 256ul * j;
        if (i < nitems) nt_store(y + i, w[j]);
        else if (i == nitems)                                 // the samples behind the last whole store
            for (unsigned long o = nitems * PER; o < n_out; o++) reinterpret_cast<T *>(y)[o] = tab[mod_symbol(x, carry_in, p, o / P)];
    }
}

// an output buffer that is not 16-byte aligned (a piece of a long host call may start anywhere): one sample per thread, any P
template <typename T>
__global__ __launch_bounds__(256) void mod_scalar_kernel(const uint8_t *__restrict__ x, const uint8_t *__restrict__ carry_in, uint8_t *__restrict__ carry_out,
                                                         const T *__restrict__ gtab, T *__restrict__ y, ModParams p, unsigned long n_out)
{
    mod_carry(x, carry_in, carry_out, p);
    const unsigned long o = (unsigned long)blockIdx.x * 256 + threadIdx.x;
    if (o < n_out) y[o] = gtab[mod_symbol(x, carry_in, p, o / p.P)];
}

}  // namespace lrhip
