// host_op_string_check.cpp - the op string reader (luaradio_amd/csrc/op_string.h: the header the creators use, not a copy) on the CPU, over a file of
// op strings, one per line (tests/test_op_strings_cpu.py writes the corpus of tests/helpers/op_string_corpus.py).  Every string and every prefix of
// it goes through split() and the getters its creator calls, three times: from a heap block of exactly its length (built with
// -fsanitize=address,undefined a read past the terminator stops the program), and from two blocks with different text behind the terminator, which
// must not change the answer.  A refusal must leave a message.  Of a string above 4096 characters only the prefixes near its end and every 4096th
// are read.
//   g++ -O1 -std=c++17 -I luaradio_amd/csrc -o /tmp/host_op_string_check tools/host_op_string_check.cpp && /tmp/host_op_string_check corpus.txt
#include <cstdarg>
#include <cstdio>
#include <fstream>
#include <memory>

static char g_error[512];
static int set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof g_error, fmt, ap);
    va_end(ap);
    return -1;
}
#include "op_string.h"

enum Kind { NUM, FIN, INT, FLAG, U64, WORD, BITS, LIST };
struct Field { const char *key, *def; Kind kind; long lo, hi; };
struct Head { const char *name, *who; bool echo; std::vector<Field> fields; };

// what each creator hands to split() and which getter it calls per key (stage_*.h)
static const std::vector<Head> kHeads = {
    {"zerocrossingclockrecovery", nullptr, true, {{"period", nullptr, NUM}, {"threshold", nullptr, NUM}}},
    {"clocksampler", nullptr, true, {{"period", nullptr, NUM}, {"threshold", nullptr, NUM}}},
    {"slicer", "slicer", true, {{"threshold", nullptr, NUM}}},
    {"differentialdecoder", "differentialdecoder", true, {{"invert", nullptr, FLAG}}},
    {"manchesterdecoder", "manchesterdecoder", true, {{"invert", nullptr, FLAG}}},
    {"binaryphasecorrector", "binaryphasecorrector", true, {{"num_samples", nullptr, NUM}, {"sample_interval", "32", NUM}}},
    {"pll", "pll", true, {{"alpha", nullptr, NUM}, {"beta", nullptr, NUM}, {"fmin", nullptr, NUM}, {"fmax", nullptr, NUM}, {"mult", "1", NUM},
                          {"port", "out", WORD}, {"segment", "", NUM}, {"warmup", "", NUM}, {"speculate", "1", FLAG}}},
    {"preamblesampler", "preamblesampler", true, {{"period", nullptr, INT, -0x7fffffffl, 0x7fffffffl}, {"num_samples", nullptr, INT, -0x7fffffffl, 0x7fffffffl},
                                                  {"preamble", nullptr, BITS}}},
    {"pam", nullptr, false, {{"period", nullptr, INT, LONG_MIN, LONG_MAX}, {"bits", nullptr, INT, LONG_MIN, LONG_MAX}, {"msb", nullptr, INT, LONG_MIN, LONG_MAX},
                             {"table", nullptr, LIST, 0}}},
    {"qam", nullptr, false, {{"period", nullptr, INT, LONG_MIN, LONG_MAX}, {"bits", nullptr, INT, LONG_MIN, LONG_MAX}, {"msb", nullptr, INT, LONG_MIN, LONG_MAX},
                             {"table", nullptr, LIST, 0}}},
    {"pfbsynthesizer", "pfb_synthesizer", false, {{"channels", nullptr, INT, 0, 1000000}, {"oversample", nullptr, INT, 0, 1000000}, {"taps", nullptr, LIST, 65536}}},
    {"interleave", nullptr, true, {{"channels", nullptr, NUM}, {"size", nullptr, NUM}}},
    {"deinterleave", nullptr, true, {{"channels", nullptr, NUM}, {"size", nullptr, NUM}}},
    {"wavpack", nullptr, true, {{"channels", nullptr, NUM}, {"bits", nullptr, NUM}}},
    {"wavunpack", nullptr, true, {{"channels", nullptr, NUM}, {"bits", nullptr, NUM}}},
    {"signalsource", nullptr, false, {{"signal", nullptr, WORD}, {"frequency", nullptr, FIN}, {"rate", nullptr, FIN}, {"amplitude", nullptr, FIN},
                                      {"phase", nullptr, FIN}, {"offset", nullptr, FIN}}},
    {"uniformrandomsource", nullptr, false, {{"type", nullptr, WORD}, {"lo", nullptr, FIN}, {"hi", nullptr, FIN}, {"seed", nullptr, U64}}},
};

// the answer to one string: refused or not, the message, and the values read, as text
struct Answer {
    bool ok = false;
    std::string message, values;
    bool operator==(const Answer &o) const { return ok == o.ok && message == o.message && values == o.values; }
};

static bool read_field(const OpFields &f, const Field &d, std::string &values)
{
    char text[64];
    text[0] = 0;
    if (d.kind == NUM || d.kind == FIN) {
        double v = 0.0;
        if (!f.has(d.key) && d.def && !*d.def) return true;              // an optional key without a default is read only when it was given
        if (!f.number(d.key, v, d.kind == FIN)) return false;
        snprintf(text, sizeof text, "%a;", v);
    } else if (d.kind == INT) {
        long v = 0;
        if (!f.integer(d.key, d.lo, d.hi, v)) return false;
        snprintf(text, sizeof text, "%ld;", v);
    } else if (d.kind == FLAG) {
        bool v = false;
        if (!f.flag(d.key, v)) return false;
        snprintf(text, sizeof text, "%d;", (int)v);
    } else if (d.kind == U64) {
        uint64_t v = 0;
        if (!f.u64(d.key, v)) return false;
        snprintf(text, sizeof text, "%llu;", (unsigned long long)v);
    } else if (d.kind == WORD) {
        const int v = f.word(d.key, {"out", "error", "sine", "cosine", "byte", "f32"}, "not a word: \"", "\"");
        if (v < 0) return false;
        snprintf(text, sizeof text, "%d;", v);
    } else if (d.kind == BITS) {
        std::string v;
        if (!f.bits(d.key, v)) return false;
        values += v + ";";
    } else {
        std::vector<float> v;
        if (!f.floats(d.key, v, (size_t)d.lo, "entry", "", "the list ends")) return false;
        for (float x : v) {
            snprintf(text, sizeof text, "%a,", (double)x);
            values += text;
        }
        text[0] = 0;
    }
    values += text;
    return true;
}

static Answer answer(const Head &h, const char *op)
{
    Answer a;
    g_error[0] = 0;
    OpFields f;
    std::vector<OpKey> keys;
    for (const Field &d : h.fields) keys.push_back(OpKey{d.key, d.def});
    bool ok = f.split(op, h.who, keys, h.echo);
    for (size_t i = 0; ok && i < h.fields.size(); i++) ok = read_field(f, h.fields[i], a.values);
    a.ok = ok;
    a.message = g_error;
    return a;
}

// the first n characters of s, terminated, in a block of its own with `behind` after the terminator (nullptr: the block ends with it)
static std::unique_ptr<char[]> block(const std::string &s, size_t n, const char *behind)
{
    const size_t extra = behind ? strlen(behind) + 1 : 0;
    std::unique_ptr<char[]> p(new char[n + 1 + extra]);
    memcpy(p.get(), s.data(), n);
    p[n] = 0;
    if (behind) memcpy(p.get() + n + 1, behind, extra);
    return p;
}

int main(int argc, char **argv)
{
    if (argc != 2) { printf("usage: host_op_string_check <file of op strings>\n"); return 2; }
    std::ifstream in(argv[1]);
    if (!in) { printf("cannot read %s\n", argv[1]); return 2; }
    std::string op;
    long strings = 0, runs = 0, refused = 0, failures = 0, unread = 0;
    while (std::getline(in, op)) {
        const size_t head_len = op.find(':') == std::string::npos ? op.size() : op.find(':');
        const Head *h = nullptr;
        for (const Head &c : kHeads)
            if (op.compare(0, head_len, c.name) == 0) h = &c;
        if (!h) { unread++; continue; }               // a head without parameters, or none the library knows: nothing for the reader
        strings++;
        for (size_t n = strlen(h->name); n <= op.size(); n++) {
            if (op.size() > 4096 && n + 64 < op.size() && n % 4096) continue;
            const Answer a = answer(*h, block(op, n, nullptr).get()), b = answer(*h, block(op, n, ":x=1,2:=").get()),
                         c = answer(*h, block(op, n, "=9e999:01").get());
            runs++;
            refused += !a.ok;
            const bool ok = a == b && a == c && (a.ok || !a.message.empty()) && (!a.ok || a.message.empty());
            if (!ok && failures++ < 20) printf("FAIL \"%.80s\" cut at %zu: %d \"%s\" [%.60s] / %d \"%s\" [%.60s] / %d \"%s\" [%.60s]\n", op.c_str(), n, a.ok,
                                               a.message.c_str(), a.values.c_str(), b.ok, b.message.c_str(), b.values.c_str(), c.ok, c.message.c_str(), c.values.c_str());
        }
    }
    if (failures || !strings) {
        printf("%ld of %ld runs FAILED (%ld strings)\n", failures, runs, strings);
        return 1;
    }
    printf("%ld strings (%ld without a reader), %ld prefixes, %ld refused: OK\n", strings, unread, runs, refused);
    return 0;
}
