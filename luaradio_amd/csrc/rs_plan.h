// rs_plan.h - what the Reed-Solomon and the bit-packing stages (stage_reedsolomon.h), their kernels (kernels_reedsolomon.h) and a CPU checker
// (tools/host_rs_check.hip) share: the limits, the frame / count / carry arithmetic of a stage that turns whole frames of FI input bytes into
// frames of FO output bytes, and the host-side construction of GF(2^8), the roots, the generator polynomial and the parity matrix of a code.
// Host + device, plain C++: no HIP call, no header of the library.
//
// Frames.  Frame f of a stream is the input bytes [f FI, (f + 1) FI), counted from absolute input 0, and leaves as the output bytes
// [f FO, (f + 1) FO).  After Q inputs floor(Q / FI) frames are out and Q mod FI bytes are carried; a call returns the frames its inputs complete.
//     rsenc       FI = I k        FO = I n
//     rsdec       FI = I n        FO = I k (+ I status bytes with status=1)
//     packbits    FI = 8          FO = 1
//     unpackbits  FI = 1          FO = 8
// Code.  GF(2^8) = GF(2)[x] / gfpoly in the polynomial basis, alpha = 2.  g(x) = prod_{i < n - k} (x - alpha^((fcr + i) prim)); byte j of a codeword
// is the coefficient of x^(n - 1 - j); the parity of a message is (m(x) x^(n - k)) mod g(x), a GF(2^8)-linear map, kept as a k x (n - k) matrix.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RS_HD __host__ __device__
#else
#define RS_HD
#endif

namespace rsplan {

constexpr int N_MAX = 255, PARITY_MIN = 2, PARITY_MAX = 64, I_MIN = 1, I_MAX = 8, FCR_MAX = 254, PRIM_MAX = 254;
constexpr int FRAME_MAX = I_MAX * N_MAX;                                // bytes of the largest frame, and more than any carry
constexpr int LOG_ZERO = 511;                                           // "log 0": any sum with it indexes a zero of the exp table
constexpr int EXP_SIZE = 1024;                                          // exp[0 .. 509] = alpha^(i mod 255), exp[510 .. 1023] = 0: 2 LOG_ZERO < 1024

struct Frame { uint32_t fi, fo; };

RS_HD inline uint64_t frames_done(uint64_t Q, Frame f) { return Q / f.fi; }
RS_HD inline uint32_t carried(uint64_t Q, Frame f) { return (uint32_t)(Q % f.fi); }
// the output position after Q inputs, which is where a seek to input Q lands; false if it lies at or behind 2^64
RS_HD inline bool out_position(uint64_t Q, Frame f, uint64_t *pos)
{
    const uint64_t frames = Q / f.fi;
    if (frames > ~0ull / f.fo) return false;
    *pos = frames * f.fo;
    return true;
}
// An upper bound of the output of ANY call of N inputs, whatever came before: with up to FI - 1 bytes carried, N inputs complete at most
// ceil(N / FI) frames, and a call of N = 1 does complete one.  Saturates at 2^64 - 1
RS_HD inline uint64_t max_output(uint64_t N, Frame f)
{
    const uint64_t frames = N / f.fi + (N % f.fi ? 1 : 0);
    return frames > ~0ull / f.fo ? ~0ull : frames * f.fo;
}
// inputs after which a stage started by a seek to ANY n0 emits what the uninterrupted stream would: the bytes of frame floor(n0 / FI) in front of
// n0 count as zeros, so the first frame that is right is the next one, complete FI - 1 inputs behind the worst n0 = f FI + 1
RS_HD inline uint64_t memory(Frame f) { return f.fi - 1; }

struct Code { int n, k, gfpoly, fcr, prim, interleave, status; };
RS_HD inline Frame encoder_frame(const Code &c) { return Frame{(uint32_t)(c.interleave * c.k), (uint32_t)(c.interleave * c.n)}; }
RS_HD inline Frame decoder_frame(const Code &c) { return Frame{(uint32_t)(c.interleave * c.n), (uint32_t)(c.interleave * (c.k + (c.status ? 1 : 0)))}; }

// ---- the field and the code, on the host -------------------------------------------------------------------------------------------------------
struct Field {
    uint8_t exp[EXP_SIZE];
    uint16_t log[256];                                                  // log[0] = LOG_ZERO
};

// the tables of GF(2)[x] / gfpoly by shift-and-reduce.  false unless gfpoly has degree 8 and alpha = 2 has order 255 (gfpoly is primitive)
inline bool build_field(int gfpoly, Field &f)
{
    if (gfpoly < 0x100 || gfpoly > 0x1ff) return false;
    bool seen[256] = {false};
    unsigned x = 1;
    for (int i = 0; i < 255; i++) {
        if (x == 0 || seen[x]) return false;
        seen[x] = true;
        f.exp[i] = f.exp[i + 255] = (uint8_t)x;
        f.log[x] = (uint16_t)i;
        x <<= 1;
        if (x & 0x100) x ^= (unsigned)gfpoly;
    }
    if (x != 1) return false;
    for (int i = 510; i < EXP_SIZE; i++) f.exp[i] = 0;
    f.log[0] = LOG_ZERO;
    return true;
}
inline uint8_t gf_mul(const Field &f, uint8_t a, uint8_t b) { return f.exp[f.log[a] + f.log[b]]; }
inline int gcd(int a, int b) { while (b) { const int r = a % b; a = b; b = r; } return a; }

// the index of the first refused parameter in the order n, k, gfpoly, fcr, prim, interleave (1 .. 6; n - k odd or out of range counts as k), 0 if
// the code is one the stages take
inline int check_code(const Code &c)
{
    Field f;
    if (c.n < PARITY_MIN + 1 || c.n > N_MAX) return 1;
    if (c.k < 1 || c.k >= c.n || (c.n - c.k) % 2 || c.n - c.k < PARITY_MIN || c.n - c.k > PARITY_MAX) return 2;
    if (!build_field(c.gfpoly, f)) return 3;
    if (c.fcr < 0 || c.fcr > FCR_MAX) return 4;
    if (c.prim < 1 || c.prim > PRIM_MAX || gcd(c.prim, 255) != 1) return 5;
    if (c.interleave < I_MIN || c.interleave > I_MAX) return 6;
    return 0;
}

// root[i] = alpha^((fcr + i) prim), i < n - k, as logarithms (0 .. 254)
inline void build_roots(const Code &c, uint8_t *root_log)
{
    for (int i = 0; i < c.n - c.k; i++) root_log[i] = (uint8_t)(((c.fcr + i) * c.prim) % 255);
}
// gen[j] = the coefficient of x^j of g(x), j = 0 .. n - k; gen[n - k] = 1
inline void build_generator(const Code &c, const Field &f, uint8_t *gen)
{
    uint8_t root_log[PARITY_MAX];
    build_roots(c, root_log);
    const int p = c.n - c.k;
    gen[0] = 1;
    for (int i = 0; i < p; i++) {
        const uint8_t r = f.exp[root_log[i]];
        gen[i + 1] = 0;
        for (int j = i + 1; j > 0; j--) gen[j] = (uint8_t)(gen[j - 1] ^ gf_mul(f, gen[j], r));     // (x + r) g: char 2, - is +
        gen[0] = gf_mul(f, gen[0], r);
    }
}
// matrix[i (n - k) + j] = the coefficient of x^(n - k - 1 - j) of x^(n - 1 - i) mod g(x): what message byte i adds to parity byte j
inline void build_parity_matrix(const Code &c, const Field &f, uint8_t *matrix)
{
    uint8_t gen[PARITY_MAX + 1], rem[PARITY_MAX];                       // rem[d] = the coefficient of x^d of x^e mod g, e = n - k at message byte k - 1
    build_generator(c, f, gen);
    const int p = c.n - c.k;
    for (int d = 0; d < p; d++) rem[d] = gen[d];                        // x^p mod g = g - x^p
    for (int i = c.k - 1; i >= 0; i--) {
        for (int j = 0; j < p; j++) matrix[i * p + j] = rem[p - 1 - j];
        const uint8_t top = rem[p - 1];                                 // times x, the x^p term reduced by g
        for (int d = p - 1; d > 0; d--) rem[d] = (uint8_t)(rem[d - 1] ^ gf_mul(f, top, gen[d]));
        rem[0] = gf_mul(f, top, gen[0]);
    }
}

}  // namespace rsplan
