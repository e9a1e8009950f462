// viterbi_plan.h - the count arithmetic of the windowed Viterbi decoder (ViterbiDecoderBlock): which steps a window runs, how many windows a stream of Q
// inputs has completed, where a seek lands, what a call can emit at most, which inputs are carried.  Shared by the stage (stage_viterbi.h), the kernels
// (kernels_viterbi.h) and a CPU checker (tools/host_viterbi_check.hip).  Host + device, plain integer C++: no HIP call, no header of the library.
//
// A rate-1/n code: trellis step t reads the inputs n t .. n t + n - 1 of the stream, counted from absolute input 0.  With the block D and the depth L,
// window w decodes the bits [w D, (w + 1) D) and runs the steps
//     t0(w) = max(0, w D - L)  ..  t1(w) = (w + 1) D + L - 1
// so it is complete once E = floor(Q / n) >= (w + 1) D + L whole steps have arrived: after Q inputs floor((E - L) / D) windows are complete (none while
// E < L).  Everything else follows from that count.  Q goes up to 2^64 - 1 and n >= 2, so E < 2^63 and no sum below leaves 64 bits.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define VIT_HD __host__ __device__
#else
#define VIT_HD
#endif

namespace vitplan {

constexpr int K_MIN = 3, K_MAX = 9, N_MIN = 2, N_MAX = 4;
constexpr int D_MIN = 64, D_MAX = 2048, L_MAX = 256;                   // depth: K - 1 .. 256
constexpr int DECISION_BYTES_MAX = 64 * 1024;                           // (D + 2 L) * 2^(K - 1) / 8, the decision words of one window
constexpr int Q_MAX = 127;                                              // |q| of a quantised input
constexpr int32_t START_PENALTY = -(1 << 29);                           // the metric of every state but 0 where the encoder's start state is known

struct Shape { uint32_t n, D, L; };

// the first and the last step of window w
VIT_HD inline uint64_t first_step(uint64_t w, Shape s) { const uint64_t b = w * s.D; return b > s.L ? b - s.L : 0; }
VIT_HD inline uint64_t last_step(uint64_t w, Shape s) { return (w + 1) * s.D + s.L - 1; }
// steps of a window, at most D + 2 L
VIT_HD inline uint32_t window_steps(uint64_t w, Shape s) { return (uint32_t)(last_step(w, s) - first_step(w, s) + 1); }

// windows complete after Q inputs
VIT_HD inline uint64_t windows_done(uint64_t Q, Shape s)
{
    const uint64_t E = Q / s.n;
    return E >= s.L ? (E - s.L) / s.D : 0;
}
// bits emitted after Q inputs, which is also where a seek to input n0 = Q lands in the output
VIT_HD inline uint64_t bits_done(uint64_t Q, Shape s) { return windows_done(Q, s) * s.D; }
// the first input the stage still needs once `done` windows are out: everything from there to Q is carried
VIT_HD inline uint64_t carry_base(uint64_t done, Shape s) { return first_step(done, s) * s.n; }
// inputs carried after any call: Q - carry_base < n (D + 2 L + 1), because E < (done + 1) D + L
VIT_HD inline uint32_t carry_capacity(Shape s) { return s.n * (s.D + 2 * s.L + 1); }

// An upper bound of the bits of ANY call of N inputs, whatever came before: N inputs complete at most ceil(N / n) steps, and e more steps at most
// ceil(e / D) more windows.  Saturates at 2^64 - 1
VIT_HD inline uint64_t max_output(uint64_t N, Shape s)
{
    const uint64_t e = N / s.n + (N % s.n ? 1 : 0), w = e / s.D + (e % s.D ? 1 : 0);
    return w > ~0ull / s.D ? ~0ull : w * s.D;
}

// Inputs after which a decoder started by a seek to ANY n0 emits what the uninterrupted stream would: a window is right when all its inputs lie at or
// behind n0, n (w D - L) >= n0.  The window that input number i completes has n ((w + 1) D + L) = i + 1 (i is the last input of its last step), so
// i >= n0 + n (D + 2 L) - 1 is enough, and one input less is not: n0 = n (w D - L) + 1 erases the window's first input
VIT_HD inline uint64_t memory(Shape s) { return (uint64_t)s.n * (s.D + 2 * s.L) - 1; }

}  // namespace vitplan
