// kernels_phasecorr.h - BinaryPhaseCorrectorBlock (radio/blocks/signal/binaryphasecorrector.lua:36-73): a phase is measured at the absolute
// samples 0, I, 2I, ...; every sample is rotated by -avg, avg = the mean of the last N measurements (a window that starts as N zeros).
//
// Fixed-point window sums.  Each clamped phase is quantised to q = llrint(phi 2^s), s = min(52, 61 - ceil(log2(2N))), so that any window sum
// |W| <= N 2^(s+1) fits in 62 bits.  The sums are taken in unsigned 64-bit arithmetic: prefix sums are exact and independent of the order of
// addition, and a window sum Q[k] - Q[k-N] is exact even where a prefix wraps.  avg = (double)W / (N 2^s): a function of the last N measured
// samples alone, so the output is bit-identical however the stream is cut into calls, and a time partition reproduces the single stream.
// The reference's own running double sum drifts from this window mean; its spec generator computes the mean, as here.
//
// With e_k the measurement the k-th one of the call evicts (the carried ring for k < N, measurement k - N of the call otherwise),
// W_k = S + sum_{j <= k} (q_j - e_j): one prefix scan over d_k = q_k - e_k on top of the carried window sum S.
//
// Passes (a tile = 256 threads x PC_LC measurements), 4 launches, the stream read once in full plus one 8-B read per measurement:
//   pc_measure_kernel   q of each measurement of the call, the tile's sum of d and its first NaN measurement            reads x[off + k I]
//   pc_carry_kernel     one workgroup: tile bases, the call's first NaN, the next call's state
//   pc_window_kernel    W_k -> the rotation (cos(-avg), sin(-avg)) in double, rounded to float: once per measurement
//   pc_rotate_kernel    y = x * rotation of the last measurement at or before the sample (the carried one before the first); the last
//                       min(M, N) q into the ring.  REAL: only the real part, Float32 (a following ComplexToRealBlock folded in)
// A NaN measurement makes the reference's running sum NaN for ever: every output from it on is NaN (a sticky flag; reset() clears it).
// q of a NaN phase is stored as 0, llrint(NaN) is never evaluated.
#pragma once
#include "common.h"

namespace lrhip {

constexpr int PC_LC = 8, PC_TILE = 256 * PC_LC;

struct PcParams {
    unsigned long long N, I;          // window length (measurements) and measurement interval (samples)
    double scale, den;                // 2^s, N 2^s
};

// carried between calls (ping-pong on the device, like DgState); the ring of the last N q is a separate buffer, slot = measurement index mod N
struct PcState {
    unsigned long long S;             // window sum after the last measurement (mod 2^64)
    unsigned long long g;             // measurements so far, mod N: the ring slot of the next measurement
    unsigned long long off;           // samples from the call's start to its first measurement, < I
    int nan;                          // a NaN phase has been measured
    int pad;
    float rot[2];                     // rotation of the last measurement
};

__device__ __forceinline__ unsigned long long pc_quant(float2 v, const PcParams &p, bool &isnan_)
{
    double phi = atan2((double)v.y, (double)v.x);
    // binaryphasecorrector.lua:51-52, in this order
    const double hp = 3.141592653589793 / 2.0;
    phi = phi < -hp ? phi + 3.141592653589793 : phi;
    phi = phi > hp ? phi - 3.141592653589793 : phi;
    isnan_ = phi != phi;
    return isnan_ ? 0ull : (unsigned long long)__double2ll_rn(phi * p.scale);
}

// the measurement the k-th measurement of the call evicts from the window
__device__ __forceinline__ unsigned long long pc_evicted(const unsigned long long *Q, const unsigned long long *ring, unsigned long long k, unsigned long long g0,
                                                         const PcParams &p)
{
    if (k >= p.N) return Q[k - p.N];
    unsigned long long slot = g0 + k;
    if (slot >= p.N) slot -= p.N;
    return ring[slot];
}

__device__ unsigned long long pc_block_sum(unsigned long long v, unsigned long long *sh)
{
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
        __syncthreads();
    }
    const unsigned long long r = sh[0];
    __syncthreads();
    return r;
}
__device__ unsigned long long pc_block_min(unsigned long long v, unsigned long long *sh)
{
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o && sh[threadIdx.x + o] < sh[threadIdx.x]) sh[threadIdx.x] = sh[threadIdx.x + o];
        __syncthreads();
    }
    const unsigned long long r = sh[0];
    __syncthreads();
    return r;
}
// exclusive sum over the 256 threads (Hillis-Steele in LDS)
__device__ unsigned long long pc_scan_excl(unsigned long long v, unsigned long long (*sh)[256])
{
    const int tid = threadIdx.x;
    int buf = 0;
    sh[0][tid] = v;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {
        unsigned long long a = sh[buf][tid];
        if (tid >= o) a += sh[buf][tid - o];
        sh[buf ^ 1][tid] = a;
        buf ^= 1;
        __syncthreads();
    }
    const unsigned long long r = tid ? sh[buf][tid - 1] : 0ull;
    __syncthreads();
    return r;
}

// pass A: q of the M measurements, per tile the sum of d and the first NaN measurement (~0 if none).  The e_k of k >= N are recomputed from x
// (measurement k - N is another thread's): one more strided 8-B read and atan2 per measurement, no ordering between threads.
__global__ __launch_bounds__(256) void pc_measure_kernel(const float2 *__restrict__ x, unsigned long long M, PcParams p, const PcState *__restrict__ si,
                                                         const unsigned long long *__restrict__ ring, unsigned long long *__restrict__ Q,
                                                         unsigned long long *__restrict__ t_sum, unsigned long long *__restrict__ t_nan)
{
    __shared__ unsigned long long sh[256];
    const unsigned long long off = si->off, g0 = si->g;
    const unsigned long long k0 = (unsigned long long)blockIdx.x * PC_TILE + (unsigned long long)threadIdx.x * PC_LC;
    unsigned long long sum = 0, first_nan = ~0ull;
#pragma unroll
    for (int u = 0; u < PC_LC; u++) {
        const unsigned long long k = k0 + u;
        if (k >= M) break;
        bool bad;
        const unsigned long long q = pc_quant(x[off + k * p.I], p, bad);
        if (bad && first_nan == ~0ull) first_nan = k;
        unsigned long long e;
        if (k >= p.N) {
            bool bad2;
            e = pc_quant(x[off + (k - p.N) * p.I], p, bad2);
        } else {
            unsigned long long slot = g0 + k;
            if (slot >= p.N) slot -= p.N;
            e = ring[slot];
        }
        Q[k] = q;
        sum += q - e;
    }
    sum = pc_block_sum(sum, sh);
    first_nan = pc_block_min(first_nan, sh);
    if (threadIdx.x == 0) { t_sum[blockIdx.x] = sum; t_nan[blockIdx.x] = first_nan; }
}

// pass B1, one workgroup: t_sum[t] <- S + the sums of the tiles before t; *nan_at = the call's first NaN measurement (0 if the carried state
// is already NaN, ~0 if none); the next call's state except its rotation (pc_window_kernel's last measurement writes that; with M = 0 it is copied)
__global__ __launch_bounds__(256) void pc_carry_kernel(unsigned long long *__restrict__ t_sum, const unsigned long long *__restrict__ t_nan, unsigned long long nt,
                                                       unsigned long long M, unsigned long long n, PcParams p, const PcState *__restrict__ si,
                                                       PcState *__restrict__ so, unsigned long long *__restrict__ nan_at)
{
    __shared__ unsigned long long sh[2][256];
    const unsigned long long per = (nt + 255) / 256, a = (unsigned long long)threadIdx.x * per, b = a + per < nt ? a + per : nt;
    unsigned long long s = 0, fn = ~0ull;
    for (unsigned long long t = a; t < b; t++) {
        s += t_sum[t];
        if (t_nan[t] < fn) fn = t_nan[t];
    }
    const unsigned long long tot_all = pc_block_sum(s, sh[0]);
    fn = pc_block_min(fn, sh[0]);
    unsigned long long base = si->S + pc_scan_excl(s, sh);
    for (unsigned long long t = a; t < b; t++) {
        const unsigned long long v = t_sum[t];
        t_sum[t] = base;
        base += v;
    }
    if (threadIdx.x == 0) {
        const int nan = si->nan || fn != ~0ull;
        *nan_at = si->nan ? 0ull : fn;
        so->S = si->S + tot_all;
        so->g = (si->g + M % p.N) % p.N;
        so->off = si->off + M * p.I - n;
        so->nan = nan;
        so->pad = 0;
        if (!M) { so->rot[0] = si->rot[0]; so->rot[1] = si->rot[1]; }
    }
}

// pass B2: window sums -> one float2 rotation per measurement (cos / sin in double, rounded to float: binaryphasecorrector.lua:69)
__global__ __launch_bounds__(256) void pc_window_kernel(const unsigned long long *__restrict__ Q, const unsigned long long *__restrict__ ring,
                                                        const unsigned long long *__restrict__ t_base, const unsigned long long *__restrict__ nan_at,
                                                        unsigned long long M, PcParams p, const PcState *__restrict__ si, PcState *__restrict__ so,
                                                        float2 *__restrict__ rot)
{
    __shared__ unsigned long long sh[2][256];
    const unsigned long long g0 = si->g, fn = *nan_at;
    const unsigned long long k0 = (unsigned long long)blockIdx.x * PC_TILE + (unsigned long long)threadIdx.x * PC_LC;
    unsigned long long d[PC_LC], s = 0;
#pragma unroll
    for (int u = 0; u < PC_LC; u++) {
        const unsigned long long k = k0 + u;
        d[u] = k < M ? Q[k] - pc_evicted(Q, ring, k, g0, p) : 0ull;
        s += d[u];
    }
    unsigned long long w = t_base[blockIdx.x] + pc_scan_excl(s, sh);
#pragma unroll
    for (int u = 0; u < PC_LC; u++) {
        const unsigned long long k = k0 + u;
        if (k >= M) break;
        w += d[u];
        float2 r;
        if (k >= fn) {
            r.x = r.y = __int_as_float(0x7fc00000);
        } else {
            const double avg = (double)(long long)w / p.den;
            r.x = (float)cos(-avg);
            r.y = (float)sin(-avg);
        }
        rot[k] = r;
        if (k == M - 1) { so->rot[0] = r.x; so->rot[1] = r.y; }
    }
}

// (double)a * (double)b is exact, so contraction into an fma does not change the once-rounded component
__device__ __forceinline__ float2 pc_mul(float2 v, float2 r)
{
    return make_float2((float)((double)v.x * (double)r.x - (double)v.y * (double)r.y), (float)((double)v.x * (double)r.y + (double)v.y * (double)r.x));
}

// index of the last measurement at or before sample off + j (32-bit division where it fits)
__device__ __forceinline__ unsigned long long pc_index(unsigned long long j, unsigned long long I)
{
    if ((j | I) >> 32) return j / I;
    return (unsigned long long)((unsigned)j / (unsigned)I);
}

// pass C: VEC samples per thread (2: one 16-B load, pointers 16-B aligned), `items` = ceil(n / VEC) threads.  First the call's last min(M, N) q
// go into the ring (every read of the ring is in the passes before).
template <int VEC, bool REAL>
__global__ __launch_bounds__(256) void pc_rotate_kernel(const float2 *__restrict__ x, void *__restrict__ y, unsigned long long n, unsigned long long items,
                                                        unsigned long long M, PcParams p, const PcState *__restrict__ si, const float2 *__restrict__ rot,
                                                        const unsigned long long *__restrict__ Q, unsigned long long *__restrict__ ring)
{
    const unsigned long long off = si->off, g0 = si->g, stride = (unsigned long long)gridDim.x * blockDim.x;
    const unsigned long long gid = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    const unsigned long long keep = M < p.N ? M : p.N;
    for (unsigned long long t = gid; t < keep; t += stride) {
        const unsigned long long k = M - keep + t;
        ring[(g0 + k) % p.N] = Q[k];
    }
    const float2 r0 = make_float2(si->rot[0], si->rot[1]);
    for (unsigned long long t = gid; t < items; t += stride) {
        const unsigned long long i0 = t * VEC;
        const bool full = VEC == 2 && i0 + 1 < n;
        float2 v[VEC], o[VEC];
        if (full) {
            const float4 w = *(const float4 *)(x + i0);
            v[0] = make_float2(w.x, w.y);
            v[VEC - 1] = make_float2(w.z, w.w);
        } else {
#pragma unroll
            for (int j = 0; j < VEC; j++) v[j] = i0 + j < n ? x[i0 + j] : make_float2(0.f, 0.f);
        }
#pragma unroll
        for (int j = 0; j < VEC; j++) {
            const unsigned long long i = i0 + j;
            const float2 r = i < off ? r0 : rot[pc_index(i - off, p.I)];
            o[j] = pc_mul(v[j], r);
        }
        if (REAL) {
            float *yr = (float *)y;
            if (full) *(float2 *)(yr + i0) = make_float2(o[0].x, o[VEC - 1].x);
            else
                for (int j = 0; j < VEC; j++)
                    if (i0 + j < n) yr[i0 + j] = o[j].x;
        } else {
            float2 *yc = (float2 *)y;
            if (full) *(float4 *)(yc + i0) = make_float4(o[0].x, o[0].y, o[VEC - 1].x, o[VEC - 1].y);
            else
                for (int j = 0; j < VEC; j++)
                    if (i0 + j < n) yc[i0 + j] = o[j];
        }
    }
}

}  // namespace lrhip
