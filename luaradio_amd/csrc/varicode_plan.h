// varicode_plan.h - the host-checkable logic of the Varicode decoder (kernels_varicode.h, VcStage in stage_preamble.h): the alphabet, the
// per-byte step of radio/blocks/protocol/varicodedecoder.lua:61-87, the map of its 21 segmentation states and the composition of such maps.
// Everything here compiles for the host as well (tools/host_varicode_check.hip plays the passes in a loop against the literal loop).
//
// The reference appends every input byte to `state`; when the last two entries are both 0 it looks the entries in front of them up and empties
// the state, else it empties the state once it holds more than 10 entries.  Write L for the length at such a delimiter (the two zeros
// included, 2 <= L <= 11).  What is looked up is the value of the L - 2 bytes in front of the two zeros, most significant first, a byte
// counting as a one only when it equals 1 (Bit.tonumber); the reference's `offset` only skips a leading byte that is not a one, and for L = 2
// the number is 0, which is no key.  So the emission is a function of the stream around the delimiter, and the automaton that decides where
// the delimiters are needs to know only the length of the state and whether its last byte equals 0:
//   state 0              empty
//   state 2 (L - 1) + 1  L bytes (1 .. 10), the last one not 0
//   state 2 (L - 1) + 2  L bytes, the last one 0
// The bytes themselves are not state: they are still in the stream ("the carried bytes, then the call's").  A byte is a delimiter zero only
// when it equals 0 and a one only when it equals 1; 2 or 255 is neither - it breaks a delimiter and counts as a 0 in the number.
//
// Codes of 10 bits (40 of the 128, `Z` and `?` among them) are never decoded: the state is emptied at length 11, before their delimiter is
// complete, and the code's first delimiter zero stays behind as a stray entry that costs the next character one bit of room.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define LR_VC_HD __host__ __device__
#else
#define LR_VC_HD
#endif

namespace lrhip {

constexpr int VC_STATES = 21, VC_MAX_LEN = 10;           // a state of more than 10 entries is emptied
constexpr int VC_NONE = 0xff;                            // "no character" in the lookup table

// The PSK31 Varicode alphabet by character: code[c] read most significant bit first is the code of character c, without the 00 behind it.
// No code contains 00, every code starts and ends with a 1.
struct VcAlphabet { uint16_t code[128]; };
constexpr VcAlphabet VC_ALPHABET = {{
    0x2ab, 0x2db, 0x2ed, 0x377, 0x2eb, 0x35f, 0x2ef, 0x2fd, 0x2ff, 0x0ef, 0x01d, 0x36f, 0x2dd, 0x01f, 0x375, 0x3ab,      // NUL .. SI
    0x2f7, 0x2f5, 0x3ad, 0x3af, 0x35b, 0x36b, 0x36d, 0x357, 0x37b, 0x37d, 0x3b7, 0x355, 0x35d, 0x3bb, 0x2fb, 0x37f,      // DLE .. US
    0x001, 0x1ff, 0x15f, 0x1f5, 0x1db, 0x2d5, 0x2bb, 0x17f, 0x0fb, 0x0f7, 0x16f, 0x1df, 0x075, 0x035, 0x057, 0x1af,      // space ! " # $ % & ' ( ) * + , - . /
    0x0b7, 0x0bd, 0x0ed, 0x0ff, 0x177, 0x15b, 0x16b, 0x1ad, 0x1ab, 0x1b7, 0x0f5, 0x1bd, 0x1ed, 0x055, 0x1d7, 0x2af,      // 0 .. 9 : ; < = > ?
    0x2bd, 0x07d, 0x0eb, 0x0ad, 0x0b5, 0x077, 0x0db, 0x0fd, 0x155, 0x07f, 0x1fd, 0x17d, 0x0d7, 0x0bb, 0x0dd, 0x0ab,      // @ A .. O
    0x0d5, 0x1dd, 0x0af, 0x06f, 0x06d, 0x157, 0x1b5, 0x15d, 0x175, 0x17b, 0x2ad, 0x1f7, 0x1ef, 0x1fb, 0x2bf, 0x16d,      // P .. Z [ \ ] ^ _
    0x2df, 0x00b, 0x05f, 0x02f, 0x02d, 0x003, 0x03d, 0x05b, 0x02b, 0x00d, 0x1eb, 0x0bf, 0x01b, 0x03b, 0x00f, 0x007,      // ` a .. o
    0x03f, 0x1bf, 0x015, 0x017, 0x005, 0x037, 0x07b, 0x06b, 0x0df, 0x05d, 0x1d5, 0x2b7, 0x1bb, 0x2b5, 0x2d7, 0x3b5}};    // p .. z { | } ~ DEL

// number -> character, VC_NONE where the number is no code.  512 entries: at most 9 bytes fit in front of a delimiter, so the codes of 10 bits
// have no entry - they can never be looked up.
struct VcTable { uint8_t ch[512]; };
constexpr VcTable vc_make_table()
{
    VcTable t{};
    for (int k = 0; k < 512; k++) t.ch[k] = (uint8_t)VC_NONE;
    for (int c = 0; c < 128; c++)
        if (VC_ALPHABET.code[c] < 512) t.ch[VC_ALPHABET.code[c]] = (uint8_t)c;
    return t;
}

LR_VC_HD inline int vc_state(int len, bool last_zero) { return len ? 2 * (len - 1) + 1 + (last_zero ? 1 : 0) : 0; }
LR_VC_HD inline int vc_len(int s) { return (s + 1) >> 1; }
LR_VC_HD inline bool vc_last_zero(int s) { return s && !(s & 1); }

// One byte from state s (varicodedecoder.lua:65-82); only whether the byte equals 0 matters.  Returns the new state; *L = the state's length
// at a delimiter (2 .. 11, the byte at hand being its last entry), else 0.
LR_VC_HD inline int vc_step(int s, bool zero, int *L)
{
    const int len = vc_len(s) + 1;
    *L = 0;
    if (zero && vc_last_zero(s)) { *L = len; return 0; }
    if (len > VC_MAX_LEN) return 0;
    return vc_state(len, zero);
}

// The exit state for each of the 21 entry states, 5 bits each: states 0 .. 11 in lo, 12 .. 20 in hi.
struct VcMap { unsigned long long lo, hi; };
LR_VC_HD inline int vc_map_to(const VcMap &m, int s) { return (int)((s < 12 ? m.lo >> (5 * s) : m.hi >> (5 * (s - 12))) & 31ull); }
LR_VC_HD inline void vc_map_set(VcMap &m, int s, int to)
{
    if (s < 12) m.lo |= (unsigned long long)to << (5 * s);
    else m.hi |= (unsigned long long)to << (5 * (s - 12));
}
LR_VC_HD inline VcMap vc_map_identity()
{
    VcMap m{0ull, 0ull};
    for (int s = 0; s < VC_STATES; s++) vc_map_set(m, s, s);
    return m;
}
// a, then b
LR_VC_HD inline VcMap vc_map_compose(const VcMap &a, const VcMap &b)
{
    VcMap r{0ull, 0ull};
    for (int s = 0; s < VC_STATES; s++) vc_map_set(r, s, vc_map_to(b, vc_map_to(a, s)));
    return r;
}
// The map of up to 16 bytes: bit q of `zeros` says that byte q equals 0.
LR_VC_HD inline VcMap vc_map_of(unsigned zeros, int count)
{
    VcMap r{0ull, 0ull};
    for (int s = 0; s < VC_STATES; s++) {
        int st = s, L;
        for (int q = 0; q < count; q++) st = vc_step(st, (zeros >> q) & 1u, &L);
        vc_map_set(r, s, st);
    }
    return r;
}

// The character of a delimiter of length L whose second zero is byte u of the stream `in` (in(v) = byte v), or VC_NONE.  u - (L - 1) >= 0 by
// construction - the state's entries are bytes of the stream - and the loop does not read in front of the stream whatever it is handed.
template <class Stream> LR_VC_HD inline int vc_lookup(const Stream &in, long long u, int L, const uint8_t *table)
{
    unsigned number = 0;
    for (long long v = u - (L - 1) > 0 ? u - (L - 1) : 0; v <= u - 2; v++) number = ((number << 1) | (in(v) == 1u ? 1u : 0u)) & 511u;
    return table[number];
}

// the most a call of n bytes emits: a character owns at least 3 bytes of its own (a code `1` and 00), of which the second zero lies in the
// call, and the state carries at most 10 bytes in
LR_VC_HD inline unsigned long vc_max_output(unsigned long n) { const unsigned long b = (n + VC_MAX_LEN) / 3; return n < b ? n : b; }

}  // namespace lrhip
