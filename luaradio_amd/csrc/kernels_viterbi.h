// kernels_viterbi.h - ConvolutionalEncoderBlock and ViterbiDecoderBlock: a rate-1/n convolutional code of constraint length K = 3 .. 9 and its
// sliding-window Viterbi decoder on soft (Float32 LLR, positive = 0) or hard (Bit) input.  Not blocks of the reference; the contract is the literal
// model of tests/helpers/viterbi_model.py, and the count arithmetic is viterbi_plan.h.
//
// Code.  Polynomials in the usual octal notation: bit K - 1 of g_j multiplies the current input bit.  The register after input u_t is
// r = (u_t << (K - 1)) | (r >> 1) from r = 0 at absolute bit 0, out[n t + j] = parity(r & g_j), the state is r >> 1.
//
// Decoder.  Each input is quantised ONCE, q = clamp(rintf(fl32(llr * scale)), -127, 127), NaN -> 0 (an erasure); a hard bit b is q = 127 (1 - 2 b).
// Everything behind that is int32 and exact: state s' has the predecessors p_b = ((s' << 1) | b) & (S - 1), S = 2^(K - 1), its input bit is
// u = s' >> (K - 2), the branch register is (u << (K - 1)) | p_b with code bits c_j, bm_b = sum_j (c_j ? -q_j : q_j), cand_b = m[p_b] + bm_b,
// d = cand_1 > cand_0 (a tie takes b = 0), m'[s'] = max.  |m| <= 4 * 127 * 2560 < 2^21: no normalisation.  Window w (viterbi_plan.h) starts from
// m = {0, -2^29, ...} at step 0 and from m = 0 elsewhere, and traces back from the best state (the lowest on a tie) behind its last step.
//
// Shape.  One wave owns one window; the waves of a workgroup share nothing, and there is no barrier anywhere.  A lane holds R = max(1, S / 64)
// metrics, state r * 64 + lane in slot r (S < 64: lane l runs state l mod S, so a state also sits in the lane of its own number).  The predecessors of
// every slot of a lane sit in ONE lane per b, (2 lane + b) mod 64, in slot (2 r + lane / 32) mod R: a step is 2 R ds_bpermute, R selects per b for
// R > 1, and per state two v_dot4_i32_i8 that add the branch metric - the lane's code bits as +-1 bytes against the step's n quantised bytes - onto
// the predecessor's metric, one compare, one max, and a select and an or that put the decision into bit j of the lane's own decision register.
// The steps of a window go in chunks of 64.  Lane j of a chunk loads and quantises the n inputs of step 64 c + j, coalesced, into one dword; the step
// loop reads it with v_readlane.  A lane keeps the 64 decisions of each of its states for the chunk in a register pair (no ballot: the word is indexed
// by step, the lane by state) and writes it to LDS once per chunk, one 8-byte write per lane and slot, to the address the SAME lane reads on the way
// back: LDS is the lane's private array here (no cross-lane traffic, hence no fence), and takes 8 R bytes per step and wave.  The traceback keeps the
// state wave-uniform: it reads the register of state s with v_readlane (lane s mod 64), takes bit j, and the 64 bits of a chunk leave as one byte
// store per lane.  An earlier form kept the __ballot word of a step in lane j (a select on lane == j per step and register): 1.05 ms against
// 0.75 ms for 2^24 bits at the default shape.
// (part of liblrhip.so; included by lrhip.hip in this order, one translation unit)
#pragma once
#include "common.h"
#include "viterbi_plan.h"

namespace lrhip {

constexpr int VIT_NT = 256;                  // at most four waves, four windows, per workgroup

struct VitCode {
    int K, n;
    unsigned g[4];
};

__device__ __forceinline__ int vit_quantise(float llr, float scale)
{
#pragma clang fp contract(off)
    const float r = rintf(llr * scale);
    if (!(r == r)) return 0;
    return (int)fminf(fmaxf(r, -(float)vitplan::Q_MAX), (float)vitplan::Q_MAX);
}
template <bool SOFT>
__device__ __forceinline__ int vit_input(const void *x, long i, float scale)
{
    if (SOFT) return vit_quantise(((const float *)x)[i], scale);
    return ((const uint8_t *)x)[i] & 1 ? -vitplan::Q_MAX : vitplan::Q_MAX;
}
// input number a (absolute) of the stream: behind Q it comes from the call's vector, in front of it from the carried, already quantised ones
template <bool SOFT>
__device__ __forceinline__ int vit_fetch(const int8_t *__restrict__ carry, const void *__restrict__ x, uint64_t a, uint64_t base, uint64_t Q, long n_in,
                                         float scale)
{
    if (a >= Q) {
        const uint64_t i = a - Q;
        return i < (uint64_t)n_in ? vit_input<SOFT>(x, (long)i, scale) : 0;
    }
    return a >= base ? (int)carry[a - base] : 0;
}

// the inputs from new_base on, quantised, for the next call: [carry | x] -> carry_out
template <bool SOFT>
__global__ __launch_bounds__(256) void viterbi_carry_kernel(const int8_t *__restrict__ carry, const void *__restrict__ x, int8_t *__restrict__ carry_out,
                                                            uint64_t base, uint64_t Q, long n_in, uint64_t new_base, unsigned count, float scale)
{
    const unsigned i = blockIdx.x * 256 + threadIdx.x;
    if (i < count) carry_out[i] = (int8_t)vit_fetch<SOFT>(carry, x, new_base + i, base, Q, n_in, scale);
}

// windows w_first .. w_first + nw - 1, window w to y + (w - w_first) D.  Dynamic LDS: 8 R bytes per step and wave, chunks * 64 steps per wave
template <int R, bool SOFT>
__global__ __launch_bounds__(VIT_NT) void viterbi_kernel(const int8_t *__restrict__ carry, const void *__restrict__ x, uint8_t *__restrict__ y, VitCode code,
                                                         vitplan::Shape shape, uint64_t base, uint64_t Q, long n_in, uint64_t w_first, long nw, int chunks_max,
                                                         float scale)
{
    extern __shared__ __attribute__((aligned(16))) uint64_t vit_lds[];
    // (the wave's number through v_readfirstlane: the compiler then knows that the window, its step counts and the loops below are wave-uniform)
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), waves = blockDim.x >> 6;
    const int K = code.K, n = code.n, S = 1 << (K - 1);
    uint64_t *dec = vit_lds + (size_t)wave * chunks_max * R * 64;                 // [chunk][slot][lane]
    // what a lane keeps for the whole launch: where its predecessors sit, and its code bits as +-1 bytes
    int src[2], sg[R][2];
    const bool upper = lane >= 32;
#pragma unroll
    for (int b = 0; b < 2; b++) src[b] = 4 * ((R > 1 ? 2 * lane + b : (2 * (lane & (S - 1)) + b) & (S - 1)) & 63);
#pragma unroll
    for (int r = 0; r < R; r++) {
        const int s = R > 1 ? r * 64 + lane : lane & (S - 1), u = s >> (K - 2);
#pragma unroll
        for (int b = 0; b < 2; b++) {
            const unsigned reg = ((unsigned)u << (K - 1)) | (unsigned)(((s << 1) | b) & (S - 1));
            unsigned pack = 0;
            for (int j = 0; j < n; j++) pack |= (__popc(reg & code.g[j]) & 1 ? 0xFFu : 0x01u) << (8 * j);
            sg[r][b] = (int)pack;
        }
    }
    for (long wi = (long)blockIdx.x * waves + wave; wi < nw; wi += (long)gridDim.x * waves) {
        const uint64_t w = w_first + (uint64_t)wi, t0 = vitplan::first_step(w, shape), wD = w * shape.D;
        const int nsteps = (int)vitplan::window_steps(w, shape), chunks = (nsteps + 63) >> 6;
        int m[R];
#pragma unroll
        for (int r = 0; r < R; r++) m[r] = t0 == 0 && (R > 1 ? r * 64 + lane : lane & (S - 1)) != 0 ? vitplan::START_PENALTY : 0;
        // the n quantised inputs of step 64 c + lane of the window, as bytes of one dword
        auto load_chunk = [&](int c) -> int {
            const int st = c * 64 + lane;
            unsigned pack = 0;
            if (st < nsteps) {
                const uint64_t a = (t0 + (uint64_t)st) * (uint64_t)n;
                for (int j = 0; j < n; j++) pack |= ((unsigned)vit_fetch<SOFT>(carry, x, a + j, base, Q, n_in, scale) & 0xFFu) << (8 * j);
            }
            return (int)pack;
        };
        int qnext = load_chunk(0);
        for (int c = 0; c < chunks; c++) {
            const int qw = qnext;
            if (c + 1 < chunks) qnext = load_chunk(c + 1);
            const int jn = nsteps - c * 64 < 64 ? nsteps - c * 64 : 64;
            unsigned d[2][R];                                                     // bit j & 31 of d[j / 32][r]: the decision of the lane's state r at step 64 c + j
#pragma unroll
            for (int half = 0; half < 2; half++) {
#pragma unroll
                for (int r = 0; r < R; r++) d[half][r] = 0;
                const int j1 = jn < 32 * half + 32 ? jn : 32 * half + 32;
                for (int j = 32 * half; j < j1; j++) {
                    const int q = __builtin_amdgcn_readlane(qw, j);
                    const unsigned bit = 1u << (j & 31);
                    int v[2][R];
#pragma unroll
                    for (int b = 0; b < 2; b++)
#pragma unroll
                        for (int k = 0; k < R; k++) v[b][k] = __builtin_amdgcn_ds_bpermute(src[b], m[k]);
#pragma unroll
                    for (int r = 0; r < R; r++) {
                        const int c0 = __builtin_amdgcn_sdot4(sg[r][0], q, upper ? v[0][(2 * r + 1) % R] : v[0][(2 * r) % R], false);
                        const int c1 = __builtin_amdgcn_sdot4(sg[r][1], q, upper ? v[1][(2 * r + 1) % R] : v[1][(2 * r) % R], false);
                        d[half][r] |= c1 > c0 ? bit : 0u;
                        m[r] = c1 > c0 ? c1 : c0;
                    }
                }
            }
#pragma unroll
            for (int r = 0; r < R; r++) dec[(c * R + r) * 64 + lane] = ((uint64_t)d[1][r] << 32) | d[0][r];
        }
        // the state of greatest metric, the lowest one on a tie
        int best = m[0], bs = R > 1 ? lane : lane & (S - 1);
#pragma unroll
        for (int r = 1; r < R; r++)
            if (m[r] > best) { best = m[r]; bs = r * 64 + lane; }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            const int om = __shfl_xor(best, o), os = __shfl_xor(bs, o);
            if (om > best || (om == best && os < bs)) { best = om; bs = os; }
        }
        unsigned s = (unsigned)__builtin_amdgcn_readfirstlane(bs);
        for (int c = chunks - 1; c >= 0; c--) {
            uint64_t dw[R];
#pragma unroll
            for (int r = 0; r < R; r++) dw[r] = dec[(c * R + r) * 64 + lane];
            const int jn = nsteps - c * 64 < 64 ? nsteps - c * 64 : 64;
            uint64_t bits = 0;
#pragma unroll
            for (int half = 1; half >= 0; half--) {
                int dh[R];
#pragma unroll
                for (int r = 0; r < R; r++) dh[r] = (int)(unsigned)(dw[r] >> (32 * half));
                const int j1 = jn < 32 * half + 32 ? jn : 32 * half + 32;
                for (int j = j1 - 1; j >= 32 * half; j--) {
                    // the decisions of state s: lane s mod 64 (a state below 64 also sits in the lane of its own number when S < 64), slot s / 64
                    unsigned word = (unsigned)__builtin_amdgcn_readlane(dh[0], (int)(s & 63));
#pragma unroll
                    for (int r = 1; r < R; r++) {
                        const unsigned wr = (unsigned)__builtin_amdgcn_readlane(dh[r], (int)(s & 63));
                        if ((s >> 6) == (unsigned)r) word = wr;
                    }
                    bits |= (uint64_t)(s >> (K - 2)) << j;
                    s = ((s << 1) | ((word >> (j & 31)) & 1u)) & (unsigned)(S - 1);
                }
            }
            const uint64_t t = t0 + (uint64_t)(c * 64 + lane);
            if (lane < jn && t >= wD && t - wD < shape.D) y[(uint64_t)wi * shape.D + (t - wD)] = (uint8_t)((bits >> lane) & 1);
        }
    }
}

// ConvolutionalEncoderBlock: one lane per input bit; it reads its bit and the K - 1 bits before it ([hist | x], hist = the last K - 1 bits of the call
// before) and writes its n code bits.  The lane of the last bit hands the next call's history on
__global__ __launch_bounds__(256) void convenc_kernel(const uint8_t *__restrict__ hist, const uint8_t *__restrict__ x, uint8_t *__restrict__ y, unsigned long n_in,
                                                      VitCode code, uint8_t *__restrict__ hist_out)
{
    const unsigned long t = (unsigned long)blockIdx.x * 256 + threadIdx.x;
    if (t >= n_in) return;
    const int K = code.K, H = K - 1;
    unsigned reg = 0;
    for (int i = 0; i < K; i++) {
        const long g = (long)t - i;
        const unsigned u = (g >= 0 ? x[g] : hist[g + H]) & 1u;
        reg |= u << (K - 1 - i);
    }
    for (int j = 0; j < code.n; j++) y[t * (unsigned long)code.n + j] = (uint8_t)(__popc(reg & code.g[j]) & 1);
    if (t == n_in - 1)
        for (int h = 0; h < H; h++) {
            const long g = (long)n_in - H + h;
            hist_out[h] = (g >= 0 ? x[g] : hist[g + H]) & 1u;
        }
}

}  // namespace lrhip
