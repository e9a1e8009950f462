// kernels_demodulator.h - PulseAmplitudeDemodulatorBlock / QuadratureAmplitudeDemodulatorBlock: Float32 / ComplexFloat32 -> Bit (1 B), or -> Float32
// max-log LLRs.  Symbol s of the stream is decided on input sample s P + offset against the 2^b entries of the (already scaled) symbol table.  All
// arithmetic is Float32, every operation rounded on its own (contract(off)): dr = x.re - c.re, di = x.im - c.im, d = fl(fl(dr dr) + fl(di di)); one axis
// (pam): d = fl(dr dr).
//   hard, general table: the first v with the smallest d (best = +inf; d < best takes v: a NaN or infinite sample decides 0).
//   hard, grid table (table[v] = (I[v >> qb], Q[v & (2^qb - 1)]); pam is the one-axis case): the same rule per axis on fl(dr dr) and fl(di di) alone, the
//     two indices joined.  Differs from the general rule only where two candidates differ before the final addition and coincide after it.
//   soft: llr_k = fl(fl(m1_k - m0_k) w), m0_k / m1_k the smallest d over the entries whose bit k is 0 / 1, from +inf and ignoring NaN (fminf returns its
//     other operand for a NaN one, which is what the explicit comparison does).  Rounding is monotone, so on a grid m = fl(min_i a_i + min_q b_q) with
//     the bit's axis restricted to its half: the same Float32 as the full search.
// One lane owns one symbol (the 16-byte-load form for P = 1: the 2 or 4 symbols of its vector, one after the other); a workgroup stages the table, or the
// axes of up to 2^12 entries, in LDS once and strides through the tiles of 256 lanes; every lane walks the table in the same order, so each LDS read is
// a broadcast.  The soft search walks the table in blocks of 16 entries: inside a block the minima are folded level by level (bit 0: even against odd
// entries, then pairs, ...), which costs 3 minimum operations per entry for the four low bits; each higher bit is the same on every lane for a whole
// block and takes the block's minimum once, 1/16 per entry and bit.  A naive search takes b per entry.
// A symbol's b bit bytes leave as one 2-, 4-, 8- or 16-byte store where b is that and the pointer allows; its LLRs (on a grid: the run of the I bits
// and the run of the Q bits) as 16- or 8-byte stores where the run's length and address allow, else one by one.
// (part of liblrhip.so; included by lrhip.hip in this order, one translation unit)
#pragma once

namespace lrhip {

constexpr int DEM_NT = 256;                  // lanes per workgroup
constexpr int DEM_GENERAL_MAX_BITS = 12;     // a general table is searched from LDS: 2^12 ComplexFloat32 entries are 32 KiB
constexpr int DEM_LDS_AXIS_BITS = 12;        // a grid axis of up to 2^12 entries is staged in LDS, a longer one is read through L2
constexpr int DEM_BLOCK = 16;                // entries per block of the soft search; tables and axes are padded with NaN to a multiple of it

struct DemodParams {
    unsigned P;                              // input samples per symbol
    int b, msb;                              // bits per symbol; 1: the first bit written is the most significant
    int ni, nq;                              // grid: entries of the I and the Q axis (pam: nq = 0); general: ni = 2^b entries
    int ibits, qbits;                        // grid: bits of the symbol value that index each axis (value = i << qbits | q)
    float w;                                 // soft: the LLR weight
    unsigned long first, nsym;               // input index of the call's first symbol; symbols of the call
};

__device__ __forceinline__ int dem_padded(int n) { return (n + DEM_BLOCK - 1) & ~(DEM_BLOCK - 1); }

__device__ __forceinline__ float dem_dist(float x, float c)
{
#pragma clang fp contract(off)
    const float dr = x - c;
    return dr * dr;
}
__device__ __forceinline__ float dem_dist(float2 x, float2 c)
{
#pragma clang fp contract(off)
    const float dr = x.x - c.x, di = x.y - c.y;
    const float a = dr * dr, q = di * di;
    return a + q;
}

// the first index with the smallest distance (0 when no distance is below +inf)
template <typename T>
__device__ __forceinline__ unsigned dem_nearest(const T *tab, int n, T x)
{
    float best = INFINITY;
    unsigned idx = 0;
    for (int v = 0; v < n; v++) {
        const float d = dem_dist(x, tab[v]);
        if (d < best) { best = d; idx = (unsigned)v; }
    }
    return idx;
}

// m0[k] / m1[k]: the smallest distance over the entries whose index has bit k clear / set, k < nbits <= NB (the others stay +inf or hold padding);
// npad >= 2^nbits a multiple of DEM_BLOCK (the padding is NaN)
template <int NB, typename T>
__device__ __forceinline__ void dem_minima(const T *tab, int npad, int nbits, T x, float (&m0)[NB], float (&m1)[NB])
{
    static_assert(NB >= 4 && DEM_BLOCK == 16, "the four low bits are folded inside a block of 16 entries");
#pragma unroll
    for (int k = 0; k < NB; k++) m0[k] = m1[k] = INFINITY;
    for (int base = 0; base < npad; base += DEM_BLOCK) {
        float c[DEM_BLOCK];
#pragma unroll
        for (int j = 0; j < DEM_BLOCK; j++) c[j] = dem_dist(x, tab[base + j]);
#pragma unroll
        for (int lv = 0; lv < 4; lv++) {
#pragma unroll
            for (int i = 0; i < (DEM_BLOCK >> lv); i += 2) {
                m0[lv] = fminf(m0[lv], c[i]);
                m1[lv] = fminf(m1[lv], c[i + 1]);
            }
#pragma unroll
            for (int i = 0; i < (DEM_BLOCK >> lv) / 2; i++) c[i] = fminf(c[2 * i], c[2 * i + 1]);
        }
        const unsigned blk = (unsigned)base / DEM_BLOCK;          // the bits above the block, the same on every lane
#pragma unroll
        for (int lv = 4; lv < NB; lv++) {
            if (lv < nbits) {
                const bool one = (blk >> (lv - 4)) & 1u;
                const float t = fminf(one ? m1[lv] : m0[lv], c[0]);
                m1[lv] = one ? t : m1[lv];
                m0[lv] = one ? m0[lv] : t;
            }
        }
    }
}

__device__ __forceinline__ float dem_llr(float m0, float m1, float w)
{
#pragma clang fp contract(off)
    const float t = m1 - m0;
    return t * w;
}

// the B LLRs of one symbol or of one axis of it, l[k] of bit k, to out[0 .. B): bits B-1 .. 0 with msb, else 0 .. B-1; 16- or 8-byte stores where B
// and the pointer allow
template <int B, int NB>
__device__ __forceinline__ void dem_store_llrs_fixed(float *__restrict__ out, const float (&l)[NB], int msb)
{
    float r[B];
#pragma unroll
    for (int t = 0; t < B; t++) r[t] = msb ? l[B - 1 - t] : l[t];
    const uintptr_t a = reinterpret_cast<uintptr_t>(out);
    if constexpr (B % 4 == 0) {
        if (!(a & 15)) {
#pragma unroll
            for (int j = 0; j < B / 4; j++) reinterpret_cast<float4 *>(out)[j] = make_float4(r[4 * j], r[4 * j + 1], r[4 * j + 2], r[4 * j + 3]);
            return;
        }
    }
    if constexpr (B % 2 == 0) {
        if (!(a & 7)) {
#pragma unroll
            for (int j = 0; j < B / 2; j++) reinterpret_cast<float2 *>(out)[j] = make_float2(r[2 * j], r[2 * j + 1]);
            return;
        }
    }
#pragma unroll
    for (int t = 0; t < B; t++) out[t] = r[t];
}
// (b is the same on every lane: one case runs, with every register index a constant)
template <int NB>
__device__ __forceinline__ void dem_store_llrs(float *__restrict__ out, const float (&l)[NB], int b, int msb)
{
#define DEM_LLR_CASE(B) case B: if constexpr (B <= NB) dem_store_llrs_fixed<B, NB>(out, l, msb); break;
    switch (b) {
        DEM_LLR_CASE(1) DEM_LLR_CASE(2) DEM_LLR_CASE(3) DEM_LLR_CASE(4) DEM_LLR_CASE(5) DEM_LLR_CASE(6) DEM_LLR_CASE(7) DEM_LLR_CASE(8)
        DEM_LLR_CASE(9) DEM_LLR_CASE(10) DEM_LLR_CASE(11) DEM_LLR_CASE(12) DEM_LLR_CASE(13) DEM_LLR_CASE(14) DEM_LLR_CASE(15) DEM_LLR_CASE(16)
    default: break;
    }
#undef DEM_LLR_CASE
}

// the b bytes of one symbol: positions b-1 .. 0 of the value with msb, else 0 .. b-1.  packed: b is 2, 4, 8 or 16 and y + sym b is aligned to it
__device__ __forceinline__ void dem_store_bits(uint8_t *__restrict__ y, unsigned long sym, unsigned v, int b, int msb, int packed)
{
    unsigned w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int t = 0; t < 16; t++)
        if (t < b) w[t >> 2] |= ((v >> (msb ? b - 1 - t : t)) & 1u) << (8 * (t & 3));
    uint8_t *p = y + sym * (unsigned long)b;
    if (packed && b == 2) *reinterpret_cast<uint16_t *>(p) = (uint16_t)w[0];
    else if (packed && b == 4) *reinterpret_cast<unsigned *>(p) = w[0];
    else if (packed && b == 8) *reinterpret_cast<uint2 *>(p) = make_uint2(w[0], w[1]);
    else if (packed && b == 16) *reinterpret_cast<uint4 *>(p) = make_uint4(w[0], w[1], w[2], w[3]);
    else {
#pragma unroll
        for (int t = 0; t < 16; t++)
            if (t < b) p[t] = (uint8_t)((w[t >> 2] >> (8 * (t & 3))) & 0xffu);
    }
}

__device__ __forceinline__ float dem_axis_sample(float x, int) { return x; }
__device__ __forceinline__ float dem_axis_sample(float2 x, int axis) { return axis ? x.y : x.x; }

// one symbol on a grid table: axI / axQ the axes where they are read (LDS or global memory)
template <typename T, bool SOFT>
__device__ __forceinline__ void dem_decide_grid(const float *axI, const float *axQ, T x, const DemodParams &p, void *__restrict__ y, unsigned long sym, int packed)
{
    constexpr bool CPLX = sizeof(T) == 8;
    const float xi = dem_axis_sample(x, 0), xq = dem_axis_sample(x, 1);
    if constexpr (!SOFT) {
        unsigned v = dem_nearest(axI, p.ni, xi);
        if (CPLX) v = (v << p.qbits) | dem_nearest(axQ, p.nq, xq);
        dem_store_bits((uint8_t *)y, sym, v, p.b, p.msb, packed);
    } else {
#pragma clang fp contract(off)
        constexpr int NB = MOD_MAX_BITS;
        float *out = (float *)y + sym * (unsigned long)p.b;
        float i0[NB], i1[NB], li[NB] = {};
        dem_minima<NB>(axI, dem_padded(p.ni), p.ibits, xi, i0, i1);
        if constexpr (CPLX) {
            // the symbol's bits are those of the I index above those of the Q index: two runs of consecutive outputs
            float q0[NB], q1[NB], lq[NB] = {};
            dem_minima<NB>(axQ, dem_padded(p.nq), p.qbits, xq, q0, q1);
            const float mi = fminf(i0[0], i1[0]), mq = fminf(q0[0], q1[0]);
#pragma unroll
            for (int k = 0; k < NB; k++) {
                if (k < p.qbits) lq[k] = dem_llr(mi + q0[k], mi + q1[k], p.w);
                if (k < p.ibits) li[k] = dem_llr(i0[k] + mq, i1[k] + mq, p.w);
            }
            dem_store_llrs<NB>(out + (p.msb ? 0 : p.qbits), li, p.ibits, p.msb);
            dem_store_llrs<NB>(out + (p.msb ? p.ibits : 0), lq, p.qbits, p.msb);
        } else {
#pragma unroll
            for (int k = 0; k < NB; k++)
                if (k < p.b) li[k] = dem_llr(i0[k], i1[k], p.w);
            dem_store_llrs<NB>(out, li, p.b, p.msb);
        }
    }
}

// one symbol on a general table (in LDS)
template <bool SOFT>
__device__ __forceinline__ void dem_decide_general(const float2 *tab, float2 x, const DemodParams &p, void *__restrict__ y, unsigned long sym, int packed)
{
    if constexpr (!SOFT) {
        dem_store_bits((uint8_t *)y, sym, dem_nearest(tab, p.ni, x), p.b, p.msb, packed);
    } else {
        constexpr int NB = DEM_GENERAL_MAX_BITS;
        float *out = (float *)y + sym * (unsigned long)p.b;
        float m0[NB], m1[NB], l[NB] = {};
        dem_minima<NB>(tab, dem_padded(p.ni), p.b, x, m0, m1);
#pragma unroll
        for (int k = 0; k < NB; k++)
            if (k < p.b) l[k] = dem_llr(m0[k], m1[k], p.w);
        dem_store_llrs<NB>(out, l, p.b, p.msb);
    }
}

template <typename T, int PER>
__device__ __forceinline__ T dem_pick(const float4 &v, int k)
{
    if constexpr (PER == 2) return k ? make_float2(v.z, v.w) : make_float2(v.x, v.y);
    else return k == 0 ? v.x : k == 1 ? v.y : k == 2 ? v.z : v.w;
}

// T: float (pam) or float2 (qam).  PER = 1: one symbol per lane, any P, any pointer.  PER = 16 / sizeof(T): P = 1 and x + first 16-byte aligned - a lane
// loads the 16 bytes of its PER symbols at once; the lane on the call's last, incomplete vector reads its samples one by one.
// gtab: GENERAL - the table, padded to a multiple of DEM_BLOCK entries; else the I axis, padded, then the Q axis, padded.  stage_i / stage_q: that axis
// is read from LDS.  Dynamic LDS: the staged floats.
template <typename T, bool GENERAL, bool SOFT, int PER>
__global__ __launch_bounds__(DEM_NT) void demod_kernel(const T *__restrict__ x, const float *__restrict__ gtab, void *__restrict__ y, DemodParams p,
                                                        int stage_i, int stage_q, int packed, unsigned long ntiles)
{
    extern __shared__ __attribute__((aligned(16))) float dem_lds[];
    const int npi = dem_padded(p.ni), npq = dem_padded(p.nq);
    const float *g_i = gtab, *g_q = gtab + npi;
    float *s_i = dem_lds, *s_q = dem_lds + (stage_i ? npi : 0);
    if (GENERAL) {
        for (int e = threadIdx.x; e < 2 * npi; e += DEM_NT) dem_lds[e] = gtab[e];
    } else {
        if (stage_i)
            for (int e = threadIdx.x; e < npi; e += DEM_NT) s_i[e] = g_i[e];
        if (stage_q)
            for (int e = threadIdx.x; e < npq; e += DEM_NT) s_q[e] = g_q[e];
    }
    __syncthreads();
    const bool all_lds = GENERAL || (stage_i && (stage_q || !p.nq));
    for (unsigned long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const unsigned long s0 = (tile * DEM_NT + threadIdx.x) * PER;
        if (s0 >= p.nsym) continue;
        const bool whole = PER > 1 && s0 + PER <= p.nsym;
        const int cnt = whole ? PER : (int)(p.nsym - s0 < (unsigned long)PER ? p.nsym - s0 : (unsigned long)PER);
        float4 vec = make_float4(0.f, 0.f, 0.f, 0.f);
        if (whole) vec = *reinterpret_cast<const float4 *>(x + p.first + s0);
#pragma unroll 1
        for (int k = 0; k < cnt; k++) {
            const unsigned long sym = s0 + (unsigned long)k;
            T xs;
            if constexpr (PER > 1) xs = whole ? dem_pick<T, PER>(vec, k) : x[p.first + sym];
            else xs = x[p.first + sym * p.P];
            if constexpr (GENERAL) dem_decide_general<SOFT>(reinterpret_cast<const float2 *>(dem_lds), xs, p, y, sym, packed);
            else if (all_lds) dem_decide_grid<T, SOFT>(s_i, s_q, xs, p, y, sym, packed);
            else dem_decide_grid<T, SOFT>(stage_i ? (const float *)s_i : g_i, stage_q ? (const float *)s_q : g_q, xs, p, y, sym, packed);
        }
    }
}

}  // namespace lrhip
