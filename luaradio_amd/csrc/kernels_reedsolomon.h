// kernels_reedsolomon.h - ReedSolomonEncoderBlock, ReedSolomonDecoderBlock, PackBitsBlock and UnpackBitsBlock: systematic Reed-Solomon codes over
// GF(2^8) with n <= 255 and 2 .. 64 parity bytes, symbol-interleaved I = 1 .. 8 deep, and the Bit <-> Byte stages that put them behind the Viterbi
// decoder.  Not blocks of the reference; the contract is the literal model of tests/helpers/reedsolomon_model.py, and the frame arithmetic and the
// construction of the field, the roots and the parity matrix are rs_plan.h.
//
// Frames.  A stage turns frames of FI input bytes into frames of FO output bytes (rs_plan.h).  The bytes of a call are the carried ones (fewer than
// FI, in a device buffer) followed by the call's vector: byte v of that virtual stream is carry[v] for v < c and x[v - c] behind.  frame_carry_kernel
// writes the bytes behind the last complete frame into the other carry buffer.
//
// Arithmetic.  Products go through logarithms: a b = exp[log a + log b] with log 0 = 511 and an exp table of 1024 bytes whose entries from 510 on are
// zero, so a zero factor needs no branch.  Both tables (and the encoder's parity matrix, as logarithms) are built on the host, sit in one device
// buffer and are copied into LDS by the workgroup before its single barrier.
//
// Shape.  One wave owns one frame: it loads the frame's bytes into its own piece of LDS with coalesced loads (a codeword of an interleaved frame is
// then a stride-I walk through LDS, not through memory), works through the frame's I codewords and stores the output frame coalesced.  The waves of a
// workgroup share the tables and nothing else: behind the table barrier there is no workgroup barrier, only wave-level fences around a wave's own
// LDS traffic.
//   Encoder: parity = message x matrix.  With W = the power of two at or above n - k, lane l holds parity byte l mod W for the message bytes
//   i = l / W (mod 64 / W): three LDS reads per byte (log of the message byte, matrix entry, exp), no dependence between steps, then an xor across
//   the 64 / W groups.  (An LFSR has the same reads on a serial chain of k steps; it was not measured.)
//   Decoder: lanes over positions, degree p = lane + 64 q, q < 4.  Syndrome i is the wave xor of r_p X_i^p; four syndromes travel in one dword
//   through the six xor-shuffles.  A ballot of non-zero syndromes decides the common case: none, and the message bytes leave as they came.
//   Otherwise Berlekamp-Massey (lane i holds Lambda_i and B_i, the discrepancy is a wave xor, 2 t serial steps, given up as soon as L > t), a Chien
//   search that evaluates Lambda(1 / X_p) in every lane's positions and keeps the odd-degree part on the side - in characteristic 2 that is
//   Lambda'(1 / X_p) / X_p -, Omega = S Lambda mod x^L with lane j holding Omega_j, and Forney in the lanes that found a root:
//   e = X^(-fcr) Omega(1 / X) / odd part.  Uncorrectable: L > t, not exactly L roots among the n real positions, or a zero magnitude.
// (part of liblrhip.so; included by lrhip.hip in this order, one translation unit)
#pragma once
#include "common.h"
#include "rs_plan.h"

namespace lrhip {

constexpr int RS_NT = 256;                   // four waves, four frames, per workgroup
constexpr int RS_TABLE_BYTES = rsplan::EXP_SIZE + 256 * 2;

struct RsParams {
    int n, k, p, t, I, fcr, prim, status;    // p = n - k = 2 t
    int w_log2;                              // the encoder's lane group: 2^w_log2 >= p
    int table_bytes;                         // exp + log (+ the matrix), a multiple of 16
};

// a wave's own LDS traffic: what its lanes wrote is what its lanes read behind this
__device__ __forceinline__ void rs_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
__device__ __forceinline__ int rs_wave_xor(int v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v ^= __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ int rs_mod255(int v) { return v >= 255 ? v - 255 : v; }      // v < 510
__device__ __forceinline__ uint8_t rs_fetch(const uint8_t *__restrict__ carry, const uint8_t *__restrict__ x, uint32_t c, uint64_t v)
{
    return v < c ? carry[v] : x[v - c];
}

// bytes v0 .. v0 + count - 1 of [carry | x] for the next call
__global__ __launch_bounds__(256) void frame_carry_kernel(const uint8_t *__restrict__ carry, const uint8_t *__restrict__ x, uint8_t *__restrict__ carry_out,
                                                          uint32_t c, uint64_t v0, unsigned count)
{
    const unsigned i = blockIdx.x * 256 + threadIdx.x;
    if (i < count) carry_out[i] = rs_fetch(carry, x, c, v0 + i);
}

// the tables into LDS, by the whole workgroup
__device__ __forceinline__ void rs_load_tables(uint32_t *lds, const uint32_t *__restrict__ tables, int bytes)
{
    for (int i = threadIdx.x; i < bytes / 4; i += blockDim.x) lds[i] = tables[i];
    __syncthreads();
}
// `bytes` bytes of the virtual stream from v0 on into a wave's LDS (16-byte aligned), four per lane where they come from the call's vector
__device__ __forceinline__ void rs_load_frame(uint8_t *dst, const uint8_t *__restrict__ carry, const uint8_t *__restrict__ x, uint32_t c, uint64_t v0, int bytes,
                                              int lane)
{
    if (v0 >= c) {
        const uint8_t *src = x + (v0 - c);
        for (int i = 4 * lane; i + 4 <= bytes; i += 256) {
            uint32_t w;
            __builtin_memcpy(&w, src + i, 4);
            *(uint32_t *)(dst + i) = w;
        }
        const int i = (bytes & ~3) + lane;
        if (i < bytes) dst[i] = src[i];
    } else {
        for (int i = lane; i < bytes; i += 64) dst[i] = rs_fetch(carry, x, c, v0 + (uint64_t)i);
    }
}
__device__ __forceinline__ void rs_store_frame(uint8_t *__restrict__ y, const uint8_t *src, int bytes, int lane)
{
    for (int i = 4 * lane; i + 4 <= bytes; i += 256) {
        const uint32_t w = *(const uint32_t *)(src + i);
        __builtin_memcpy(y + i, &w, 4);
    }
    const int i = (bytes & ~3) + lane;
    if (i < bytes) y[i] = src[i];
}

// ---- encoder ---------------------------------------------------------------------------------------------------------------------------------------
// frames 0 .. nf - 1 of the call, frame f to y + f I n.  Dynamic LDS: the tables and the matrix, then per wave the frame (I k bytes), the logarithms
// of its bytes (2 I k bytes) and its parity (I p bytes), each rounded up to 16
__global__ __launch_bounds__(RS_NT) void rsenc_kernel(const uint8_t *__restrict__ carry, const uint8_t *__restrict__ x, uint8_t *__restrict__ y,
                                                      const uint32_t *__restrict__ tables, RsParams P, uint32_t c, long nf, int wave_bytes)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t rs_lds[];
    rs_load_tables((uint32_t *)rs_lds, tables, P.table_bytes);
    const uint8_t *ex = rs_lds;
    const uint16_t *lg = (const uint16_t *)(rs_lds + rsplan::EXP_SIZE), *mat = (const uint16_t *)(rs_lds + RS_TABLE_BYTES);
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), waves = blockDim.x >> 6;
    const int fi = P.I * P.k, fo = P.I * P.n, par_bytes = P.I * P.p;
    uint8_t *frame = rs_lds + P.table_bytes + (size_t)wave * wave_bytes;
    uint16_t *mlog = (uint16_t *)(frame + ((fi + 15) & ~15));
    uint8_t *par = (uint8_t *)mlog + ((2 * fi + 15) & ~15);
    const int W = 1 << P.w_log2, G = 64 >> P.w_log2, j = lane & (W - 1), grp = lane >> P.w_log2, jj = j < P.p ? j : P.p - 1;
    for (long f = (long)blockIdx.x * waves + wave; f < nf; f += (long)gridDim.x * waves) {
        uint8_t *out = y + (uint64_t)f * fo;
        rs_load_frame(frame, carry, x, c, (uint64_t)f * fi, fi, lane);
        rs_wave_sync();
        rs_store_frame(out, frame, fi, lane);
        for (int i = lane; i < fi; i += 64) mlog[i] = lg[frame[i]];
        rs_wave_sync();
        for (int cw = 0; cw < P.I; cw++) {
            int acc = 0;
            for (int i = grp; i < P.k; i += G) acc ^= ex[mlog[i * P.I + cw] + mat[i * P.p + jj]];
            for (int o = W; o < 64; o <<= 1) acc ^= __shfl_xor(acc, o);
            if (grp == 0 && j < P.p) par[j * P.I + cw] = (uint8_t)acc;
        }
        rs_wave_sync();
        for (int i = lane; i < par_bytes; i += 64) out[fi + i] = par[i];
        rs_wave_sync();
    }
}

// ---- decoder ---------------------------------------------------------------------------------------------------------------------------------------
// one codeword of a frame in LDS, bytes fr[j I + cw]: corrects it in place and returns the symbols corrected, or 255.  Everything that steers the
// control flow is wave-uniform
__device__ __forceinline__ int rs_decode_codeword(uint8_t *fr, int cw, const uint8_t *ex, const uint16_t *lg, const RsParams &P, int lane)
{
    const int n = P.n, t = P.t, two_t = P.p, nq = (n + 63) >> 6;
    int addr[4], r[4], lr[4], step[4], e[4];
    const int first = (P.fcr * P.prim) % 255;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const int p = lane + 64 * q;
        const bool valid = q < nq && p < n;
        addr[q] = valid ? (n - 1 - p) * P.I + cw : -1;
        r[q] = valid ? fr[addr[q]] : 0;
        lr[q] = valid ? lg[r[q]] : rsplan::LOG_ZERO;
        step[q] = (P.prim * p) % 255;                                       // log X_p
        e[q] = (first * p) % 255;
    }
    // syndromes: S_i = sum_p r_p alpha^((fcr + i) prim p), lane i keeps S_i
    int S = 0;
    for (int i0 = 0; i0 < two_t; i0 += 4) {
        int word = 0;
#pragma unroll
        for (int b = 0; b < 4; b++) {
            int term = 0;
#pragma unroll
            for (int q = 0; q < 4; q++)
                if (q < nq) {
                    term ^= ex[lr[q] + e[q]];
                    e[q] = rs_mod255(e[q] + step[q]);
                }
            word |= term << (8 * b);                                        // (a syndrome at or above 2 t is computed and dropped)
        }
        word = rs_wave_xor(word);
        if ((lane >> 2) == (i0 >> 2) && lane < two_t) S = (word >> (8 * (lane & 3))) & 255;
    }
    if (__ballot(S != 0) == 0) return 0;
    const int logS = lg[S];
    // Berlekamp-Massey: lane i holds Lambda_i and B_i
    int lam = lane == 0, B = lam, L = 0, lb = 0;
    for (int rr = 0; rr < two_t; rr++) {
        B = __shfl_up(B, 1);
        if (lane == 0) B = 0;
        const int sv = __builtin_amdgcn_ds_bpermute(4 * ((rr - lane) & 63), logS);
        const int prod = lane <= L && lane <= rr ? ex[lg[lam] + sv] : 0;
        const int d = __builtin_amdgcn_readfirstlane(rs_wave_xor(prod));
        if (d) {
            const int ld = lg[d], coefficient = rs_mod255(ld + 255 - lb), old = lam;
            lam ^= ex[coefficient + lg[B]];
            if (2 * L <= rr) {
                L = rr + 1 - L;
                B = old;
                lb = ld;
                if (L > t) return 255;
            }
        }
    }
    const int loglam = lg[lam];
    // Chien: Lambda(1 / X_p) in every position of the lane, the odd-degree terms on the side
    int inv[4], sum[4], odd[4];
#pragma unroll
    for (int q = 0; q < 4; q++) {
        inv[q] = rs_mod255(255 - step[q]);                                  // log (1 / X_p)
        e[q] = 0; sum[q] = 0; odd[q] = 0;
    }
    for (int i = 0; i <= L; i++) {
        const int ll = __builtin_amdgcn_readlane(loglam, i);
#pragma unroll
        for (int q = 0; q < 4; q++)
            if (q < nq) {
                const int term = ex[ll + e[q]];
                sum[q] ^= term;
                if (i & 1) odd[q] ^= term;
                e[q] = rs_mod255(e[q] + inv[q]);
            }
    }
    int roots = 0;
    bool root[4];
#pragma unroll
    for (int q = 0; q < 4; q++) {
        root[q] = addr[q] >= 0 && sum[q] == 0;
        roots += __popcll(__ballot(root[q]));
    }
    if (roots != L) return 255;
    // Omega = S Lambda mod x^L, lane j holds Omega_j
    int om = 0;
    for (int i = 0; i < L; i++) {
        const int ll = __builtin_amdgcn_readlane(loglam, i);
        const int sv = __builtin_amdgcn_ds_bpermute(4 * ((lane - i) & 63), logS);
        if (lane >= i && lane < L) om ^= ex[ll + sv];
    }
    const int logom = lane < L ? lg[om] : rsplan::LOG_ZERO;
    int val[4];
#pragma unroll
    for (int q = 0; q < 4; q++) { e[q] = 0; val[q] = 0; }
    for (int i = 0; i < L; i++) {
        const int lo = __builtin_amdgcn_readlane(logom, i);
#pragma unroll
        for (int q = 0; q < 4; q++)
            if (q < nq) {
                val[q] ^= ex[lo + e[q]];
                e[q] = rs_mod255(e[q] + inv[q]);
            }
    }
    // Forney: e = X^(-fcr) Omega(1 / X) / (odd part), in the lanes that found a root
    int mag[4];
    bool bad = false;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        mag[q] = 0;
        if (root[q]) {
            if (val[q] && odd[q]) mag[q] = ex[rs_mod255((inv[q] * P.fcr) % 255 + 255 - lg[odd[q]]) + lg[val[q]]];
            bad = bad || mag[q] == 0;
        }
    }
    if (__ballot(bad) != 0) return 255;
#pragma unroll
    for (int q = 0; q < 4; q++)
        if (root[q]) fr[addr[q]] = (uint8_t)(r[q] ^ mag[q]);
    return L;
}

// frames 0 .. nf - 1 of the call, frame f to y + f I (k + status).  Dynamic LDS: the tables, then per wave the frame (I n bytes rounded up to 16)
__global__ __launch_bounds__(RS_NT) void rsdec_kernel(const uint8_t *__restrict__ carry, const uint8_t *__restrict__ x, uint8_t *__restrict__ y,
                                                      const uint32_t *__restrict__ tables, RsParams P, uint32_t c, long nf, int wave_bytes)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t rs_lds[];
    rs_load_tables((uint32_t *)rs_lds, tables, P.table_bytes);
    const uint8_t *ex = rs_lds;
    const uint16_t *lg = (const uint16_t *)(rs_lds + rsplan::EXP_SIZE);
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), waves = blockDim.x >> 6;
    const int fi = P.I * P.n, msg = P.I * P.k, fo = msg + (P.status ? P.I : 0);
    uint8_t *frame = rs_lds + P.table_bytes + (size_t)wave * wave_bytes;
    for (long f = (long)blockIdx.x * waves + wave; f < nf; f += (long)gridDim.x * waves) {
        uint8_t *out = y + (uint64_t)f * fo;
        rs_load_frame(frame, carry, x, c, (uint64_t)f * fi, fi, lane);
        rs_wave_sync();
        int status = 0;                                                     // lane cw keeps the status of codeword cw
        for (int cw = 0; cw < P.I; cw++) {
            const int s = rs_decode_codeword(frame, cw, ex, lg, P, lane);
            if (lane == cw) status = s;
        }
        rs_wave_sync();
        rs_store_frame(out, frame, msg, lane);
        if (P.status && lane < P.I) out[msg + lane] = (uint8_t)status;
        rs_wave_sync();
    }
}

// ---- bits <-> bytes --------------------------------------------------------------------------------------------------------------------------------
// PackBitsBlock: one lane per output byte, bit 0 of each of its eight input bytes
__global__ __launch_bounds__(256) void packbits_kernel(const uint8_t *__restrict__ carry, const uint8_t *__restrict__ x, uint8_t *__restrict__ y, uint32_t c,
                                                       unsigned long n_out, int msb)
{
    const unsigned long o = (unsigned long)blockIdx.x * 256 + threadIdx.x;
    if (o >= n_out) return;
    unsigned v = 0;
    for (int b = 0; b < 8; b++) v |= (unsigned)(rs_fetch(carry, x, c, 8 * (uint64_t)o + b) & 1u) << (msb ? 7 - b : b);
    y[o] = (uint8_t)v;
}
// UnpackBitsBlock: one lane per output bit
__global__ __launch_bounds__(256) void unpackbits_kernel(const uint8_t *__restrict__ x, uint8_t *__restrict__ y, unsigned long n_out, int msb)
{
    const unsigned long i = (unsigned long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_out) return;
    const int b = (int)(i & 7);
    y[i] = (uint8_t)((x[i >> 3] >> (msb ? 7 - b : b)) & 1u);
}

}  // namespace lrhip
