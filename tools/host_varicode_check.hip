// host_varicode_check.hip - the Varicode decoder's passes (luaradio_amd/csrc/varicode_plan.h, kernels_varicode.h) on the CPU: the threads and
// tiles are played in host loops with the very functions the kernels call - per-thread maps over 16-byte chunks, their composition per tile
// and over the tiles, the replay from the composed entry states - and compared with a plain copy of the loop of varicodedecoder.lua:61-87,
// characters and final state.
//   hipcc --offload-arch=gfx950 -O1 -std=c++17 -I luaradio_amd/csrc -I include -o /tmp/host_varicode_check tools/host_varicode_check.hip && /tmp/host_varicode_check
// Checked: random streams at one-probabilities 0.3, 0.5 and 0.7, with and without 2 % of bytes other than 0 and 1, cut into ragged calls; runs
// of ones of every length 0 .. 23 in front of a character (the character is emitted for some lengths and lost for others); every carried
// state length 0 .. 10; the bound of every call.
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>
#include "varicode_plan.h"
using namespace lrhip;

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { failures++; printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

static const VcTable TABLE = vc_make_table();
constexpr int CHUNK = 16, THREADS = 256, TILE = CHUNK * THREADS;     // DG_LC, the workgroup, DG_TILE

// varicodedecoder.lua:61-87, literally: the state is a list of bytes
struct Literal {
    std::vector<uint8_t> state;
    void process(const std::vector<uint8_t> &x, std::string &out)
    {
        for (uint8_t b : x) {
            state.push_back(b);
            const size_t len = state.size();
            if (len >= 2) {
                if (state[len - 2] == 0 && state[len - 1] == 0) {
                    const int offset = state[0] == 1 ? 0 : 1;
                    const int count = (int)len - offset - 2;
                    unsigned number = 0;                                 // Bit.tonumber(state, offset, count): nothing for count <= 0
                    for (int k = 0; k < count; k++) number = (number << 1) | (state[offset + k] == 1 ? 1u : 0u);
                    for (int c = 0; c < 128; c++)
                        if (VC_ALPHABET.code[c] == number) out.push_back((char)c);
                    state.clear();
                } else if (len > 10) {
                    state.clear();
                }
            }
        }
    }
};

// the device's carried state and one call of the stage, pass by pass
struct Played {
    std::vector<uint8_t> carried;                                        // the state's bytes (len = carried.size())
    unsigned long last_count = 0;
    void process(const std::vector<uint8_t> &x, std::string &out)
    {
        const unsigned long n = x.size();
        if (!n) return;
        const int carry = (int)carried.size();
        const std::vector<uint8_t> &cr = carried;
        auto in = [&](long long u) -> unsigned { return u < carry ? cr[(size_t)u] : x[(size_t)(u - carry)]; };
        const unsigned long nt = (n + TILE - 1) / TILE;
        // per-thread maps, and the summary pass: their composition per tile
        std::vector<unsigned> zeros(nt * THREADS, 0u);
        std::vector<int> counts(nt * THREADS, 0);
        std::vector<VcMap> maps(nt * THREADS), tiles(nt);
        for (unsigned long t = 0; t < nt; t++) {
            VcMap acc = vc_map_identity();
            for (int th = 0; th < THREADS; th++) {
                const unsigned long c0 = t * TILE + (unsigned long)th * CHUNK, id = t * THREADS + th;
                for (int k = 0; k < CHUNK && c0 + k < n; k++) { zeros[id] |= (x[c0 + k] == 0 ? 1u : 0u) << k; counts[id] = k + 1; }
                maps[id] = vc_map_of(zeros[id], counts[id]);
                acc = vc_map_compose(acc, maps[id]);
            }
            tiles[t] = acc;
        }
        // the carry pass: every tile's entry state, the next state
        const int s0 = vc_state(carry, carry > 0 && cr[carry - 1] == 0);
        std::vector<int> t_state(nt);
        VcMap run = vc_map_identity();
        for (unsigned long t = 0; t < nt; t++) { t_state[t] = vc_map_to(run, s0); run = vc_map_compose(run, tiles[t]); }
        const int len = vc_len(vc_map_to(run, s0));
        std::vector<uint8_t> next((size_t)len);
        for (int k = 0; k < len; k++) next[k] = (uint8_t)in((long long)carry + (long long)n - len + k);
        // count and final in one: each thread replays its chunk from its entry state (the tile's maps scanned, entered at the tile's state)
        unsigned long emitted = 0;
        for (unsigned long t = 0; t < nt; t++) {
            VcMap pre = vc_map_identity();
            for (int th = 0; th < THREADS; th++) {
                const unsigned long id = t * THREADS + th;
                int st = vc_map_to(pre, t_state[t]);
                for (int q = 0; q < counts[id]; q++) {
                    int L;
                    st = vc_step(st, (zeros[id] >> q) & 1u, &L);
                    if (L) {
                        const int ch = vc_lookup(in, (long long)carry + (long long)(t * TILE + (unsigned long)th * CHUNK + q), L, TABLE.ch);
                        if (ch != VC_NONE) { out.push_back((char)ch); emitted++; }
                    }
                }
                pre = vc_map_compose(pre, maps[id]);
                CHECK(st == vc_map_to(pre, t_state[t]), "replay and map disagree (tile %lu thread %d)", t, th);
            }
        }
        CHECK(emitted <= vc_max_output(n), "%lu characters from %lu bytes exceed the bound %lu", emitted, n, vc_max_output(n));
        last_count = emitted;
        carried = next;
    }
};

struct Rng {
    uint64_t s = 0x9E3779B97F4A7C15ull;
    uint64_t next() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; }
    double uni() { return ((next() >> 11) + 0.5) / 9007199254740992.0; }
};

static void append_char(std::vector<uint8_t> &x, int c)
{
    const unsigned code = VC_ALPHABET.code[c];
    int bits = 0;
    while ((code >> bits) != 0) bits++;
    for (int k = bits - 1; k >= 0; k--) x.push_back((uint8_t)((code >> k) & 1u));
    x.push_back(0); x.push_back(0);
}

// the stream under `cuts` (call lengths, the rest in a last call) against the literal loop fed the same calls
static void compare(const char *what, const std::vector<uint8_t> &x, const std::vector<unsigned long> &cuts, unsigned long *chars = nullptr)
{
    Literal lit;
    Played dev;
    std::string want, got;
    unsigned long at = 0;
    for (size_t k = 0; k <= cuts.size() && at < x.size(); k++) {
        unsigned long m = k < cuts.size() ? cuts[k] : x.size() - at;
        if (m > x.size() - at) m = x.size() - at;
        const std::vector<uint8_t> part(x.begin() + at, x.begin() + at + m);
        lit.process(part, want);
        dev.process(part, got);
        at += m;
        CHECK(dev.carried == lit.state, "%s: carried state differs after %lu bytes (%zu against %zu entries)", what, at, dev.carried.size(), lit.state.size());
    }
    CHECK(got == want, "%s: %zu characters, the literal loop gives %zu", what, got.size(), want.size());
    if (chars) *chars = want.size();
}

int main()
{
    Rng g;
    // ---- the table: 128 distinct codes, none 0, none with 00 inside, 40 of them of 10 bits
    {
        int ten = 0, hits = 0;
        for (int c = 0; c < 128; c++) {
            const unsigned code = VC_ALPHABET.code[c];
            CHECK(code >= 1 && code < 1024 && (code & 1u), "code of character %d", c);
            for (int k = 0; (code >> (k + 2)) != 0; k++) CHECK(((code >> k) & 3u) != 0, "00 inside the code of character %d", c);
            ten += code >= 512;
        }
        for (int k = 0; k < 512; k++) hits += TABLE.ch[k] != VC_NONE;
        CHECK(ten == 40 && hits == 88 && TABLE.ch[0] == VC_NONE && TABLE.ch[1] == ' ' && TABLE.ch[3] == 'e', "table: %d codes of 10 bits, %d entries", ten, hits);
    }
    // ---- maps: identity, and composition against stepping, over all 16-bit chunks' worth of random pairs
    {
        const VcMap id = vc_map_identity();
        for (int s = 0; s < VC_STATES; s++) CHECK(vc_map_to(id, s) == s && vc_state(vc_len(s), vc_last_zero(s)) == s, "identity / state coding at %d", s);
        for (int trial = 0; trial < 2000; trial++) {
            const unsigned za = (unsigned)(g.next() & 0xffff), zb = (unsigned)(g.next() & 0xffff);
            const int ca = (int)(g.next() % 17), cb = (int)(g.next() % 17);
            const VcMap ab = vc_map_compose(vc_map_of(za, ca), vc_map_of(zb, cb));
            for (int s = 0; s < VC_STATES; s++) {
                int st = s, L;
                for (int q = 0; q < ca; q++) st = vc_step(st, (za >> q) & 1u, &L);
                for (int q = 0; q < cb; q++) st = vc_step(st, (zb >> q) & 1u, &L);
                CHECK(vc_map_to(ab, s) == st, "composition at state %d", s);
            }
        }
    }
    // ---- random streams, whole and under ragged cuts
    const unsigned long lengths[] = {1, 2, 3, 10, 11, 12, 15, 16, 17, 4095, 4096, 4097, 2 * 4096 + 10, 5 * 4096 + 5};
    for (double p1 : {0.3, 0.5, 0.7})
        for (int other : {0, 1})
            for (unsigned long n : lengths) {
                std::vector<uint8_t> x(n);
                for (auto &b : x) {
                    b = g.uni() < p1 ? 1 : 0;
                    if (other && g.uni() < 0.02) { const uint8_t o[] = {2, 128, 255}; b = o[g.next() % 3]; }
                }
                char what[96];
                snprintf(what, sizeof(what), "random p1=%.1f other=%d n=%lu", p1, other, n);
                unsigned long chars = 0;
                compare(what, x, {}, &chars);
                if (n >= 4096 && p1 == 0.5 && !other) CHECK(chars >= n / 20, "%s: only %lu characters", what, chars);
                for (int trial = 0; trial < 3; trial++) {
                    std::vector<unsigned long> cuts;
                    unsigned long left = trial == 0 && n > 3ul * TILE ? 2ul * TILE + 10 : n;     // (few-byte calls over three tiles at the most, the rest in one)
                    while (left) { const unsigned long m = 1 + g.next() % (trial == 0 ? 7 : trial == 1 ? 5000 : 20000); cuts.push_back(m); left -= m < left ? m : left; }
                    compare(what, x, cuts);
                }
            }
    // ---- runs of ones of every length 0 .. 23 in front of a character, across a tile boundary and across a call cut
    {
        int emitted = 0, lost = 0;
        for (int R = 0; R <= 23; R++)
            for (int shift = 0; shift < 24; shift += 5) {
                std::vector<uint8_t> x((size_t)(TILE - 12 + shift - R > 0 ? TILE - 12 + shift - R : 0), 0);
                const size_t run_at = x.size();
                x.insert(x.end(), (size_t)R, 1);
                append_char(x, 'e');
                append_char(x, 't');
                Literal lit;
                std::string want;
                lit.process(x, want);
                if (shift == 0) { emitted += want == "et"; lost += want == "t"; }
                compare("run of ones over a tile boundary", x, {});
                compare("run of ones over a call cut", x, {(unsigned long)(run_at + R / 2)});
                compare("run of ones, cut behind it", x, {(unsigned long)(run_at + R)});
            }
        CHECK(emitted > 0 && lost > 0, "runs of ones: the character was emitted %d times and lost %d times", emitted, lost);
    }
    // ---- every carried state length 0 .. 10: a prefix that leaves that many entries, then a cut, then text
    for (int len = 0; len <= 10; len++)
        for (int last_zero = 0; last_zero < 2; last_zero++) {
            if (!len && last_zero) continue;
            std::vector<uint8_t> x = {0, 0};
            for (int k = 0; k < len; k++) x.push_back(k == len - 1 && last_zero ? 0 : 1);
            const unsigned long cut = x.size();
            for (int c : {'0', 'e', ' ', 'Z', 'x'}) append_char(x, c);
            Literal lit;
            std::string sink;
            lit.process(std::vector<uint8_t>(x.begin(), x.begin() + cut), sink);
            CHECK((int)lit.state.size() == len, "prefix leaves %zu entries, wanted %d", lit.state.size(), len);
            compare("carried state length", x, {cut});
            compare("carried state length, one byte per call", x, std::vector<unsigned long>(x.size(), 1ul));
        }
    // ---- the examples of a lost 10-bit code
    {
        std::vector<uint8_t> x = {0, 0};
        for (int c : {'!', 'Z', 'x'}) append_char(x, c);
        Played dev;
        std::string got;
        dev.process(x, got);
        CHECK(got == "!x", "\"!Zx\" decodes to \"%s\"", got.c_str());
    }
    if (failures) { printf("%d FAILED\n", failures); return 1; }
    printf("OK\n");
    return 0;
}
