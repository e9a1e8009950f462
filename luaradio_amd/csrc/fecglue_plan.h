// fecglue_plan.h - what the puncturing, interleaving and scrambling stages (stage_fecglue.h), their kernels (kernels_fecglue.h) and a CPU checker
// (tools/host_fecglue_check.hip) share: the limits, the frames of a puncturing pattern IN ELEMENTS (the frame / count / carry arithmetic itself is
// rs_plan.h's, which counts whatever unit it is handed), the index into a scrambler's table and the source index of the Forney interleaver.
// Host + device, plain C++: no HIP call, no header of the library but rs_plan.h.
//
// Puncture.  A pattern B of 2 .. 64 characters 0 / 1 with at least one 1: a frame is FI = len(B) elements in and FO = popcount(B) out, element j kept
// where B[j] == '1'.  Depuncture is the inverse framing, FI = popcount(B), FO = len(B).
// Scrambler.  out[i] = in[i] ^ table[(i + K) mod P], 1 <= P <= 8192, 0 <= K < P: i is reduced mod P BEFORE K is added, so no i < 2^64 wraps.
// Interleaver.  I branches, step M: with j = i mod I, out[i] = in[i - j M I]; the deinterleaver out[i] = in[i - (I - 1 - j) M I]; in[negative] = 0.
// The pair is a delay of D = (I - 1) M I <= 65536 bytes, which is also what either stage carries between calls.
#pragma once
#include <cstdint>

#include "rs_plan.h"

namespace fgplan {

constexpr int PATTERN_MIN = 2, PATTERN_MAX = 64;
constexpr int TABLE_MAX = 8192;                                         // bytes of a scrambler's table
constexpr int BRANCHES_MIN = 2, BRANCHES_MAX = 256, STEP_MIN = 1, STEP_MAX = 256;
constexpr uint32_t DEPTH_MAX = 65536;
constexpr uint8_t PUNCTURED = 0xFF;                                     // "no input element" in a depuncture map

// 0 if the n characters are a pattern; 1 its length, 2 a character that is neither 0 nor 1, 3 no 1 at all
RS_HD inline int check_pattern(const char *b, uint64_t n)
{
    if (n < (uint64_t)PATTERN_MIN || n > (uint64_t)PATTERN_MAX) return 1;
    int ones = 0;
    for (uint64_t j = 0; j < n; j++) {
        if (b[j] != '0' && b[j] != '1') return 2;
        ones += b[j] == '1';
    }
    return ones ? 0 : 3;
}
RS_HD inline uint32_t ones(const char *b, uint32_t n)
{
    uint32_t c = 0;
    for (uint32_t j = 0; j < n; j++) c += b[j] == '1';
    return c;
}
RS_HD inline rsplan::Frame puncture_frame(const char *b, uint32_t n) { return rsplan::Frame{n, ones(b, n)}; }
RS_HD inline rsplan::Frame depuncture_frame(const char *b, uint32_t n) { return rsplan::Frame{ones(b, n), n}; }
// map[k], k < popcount: the element of an input frame that output k of the puncturer is
RS_HD inline void puncture_map(const char *b, uint32_t n, uint8_t *map)
{
    uint32_t k = 0;
    for (uint32_t j = 0; j < n; j++)
        if (b[j] == '1') map[k++] = (uint8_t)j;
}
// map[j], j < len: the element of an input frame that output j of the depuncturer is, or PUNCTURED
RS_HD inline void depuncture_map(const char *b, uint32_t n, uint8_t *map)
{
    uint32_t k = 0;
    for (uint32_t j = 0; j < n; j++) map[j] = b[j] == '1' ? (uint8_t)k++ : PUNCTURED;
}

// ---- scrambler: the table entry of absolute byte i, and where a stream stands after n more bytes ------------------------------------------------
RS_HD inline uint32_t table_index(uint64_t i, uint32_t K, uint32_t P) { return (uint32_t)(((uint32_t)(i % P) + K) % P); }
RS_HD inline uint32_t table_advance(uint32_t index, uint64_t n, uint32_t P) { return (uint32_t)((index + (uint32_t)(n % P)) % P); }

// ---- interleaver --------------------------------------------------------------------------------------------------------------------------------
// 0 if the stages take the shape; 1 branches, 2 step, 3 the depth
RS_HD inline int check_interleaver(long branches, long step)
{
    if (branches < BRANCHES_MIN || branches > BRANCHES_MAX) return 1;
    if (step < STEP_MIN || step > STEP_MAX) return 2;
    return (uint64_t)(branches - 1) * (uint64_t)step * (uint64_t)branches > DEPTH_MAX ? 3 : 0;
}
RS_HD inline uint32_t depth(uint32_t I, uint32_t M) { return (I - 1) * M * I; }
// the delay of branch j = i mod I
RS_HD inline uint32_t branch_delay(uint32_t j, uint32_t I, uint32_t M, bool deinterleave) { return (deinterleave ? I - 1 - j : j) * M * I; }
// the absolute input that absolute output i is; false where it lies in front of the stream (a zero)
RS_HD inline bool source_index(uint64_t i, uint32_t I, uint32_t M, bool deinterleave, uint64_t *src)
{
    const uint32_t d = branch_delay((uint32_t)(i % I), I, M, deinterleave);
    if (i < d) return false;
    *src = i - d;
    return true;
}

}  // namespace fgplan
