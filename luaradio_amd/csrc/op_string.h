// op_string.h - the one reader of the op strings of lrhip_unary_create, "name:key=value:key=value" (include/lrhip.h).
// split() cuts the string against a list of keys, each required or optional with a default, and keeps the values as text; the typed getters read
// that text.  A refusal returns false (word(): -1) with the message in lrhip_strerror, prefixed by the name the caller hands in.  On a string with
// several defects the order is fixed: the fields from left to right (malformed, unknown key, key given twice), then the getters in the order the
// creator calls them, each refusing a required key that is absent before a value of the wrong kind.
// Plain host C++: the standard library and set_error (common.h; a stand-alone program brings its own, tools/host_op_string_check.cpp).
#pragma once
#include <cerrno>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <string>
#include <vector>

struct OpKey { const char *key, *def; };         // def: the text an absent key reads as; nullptr: the key is required

struct OpFields {
    std::string name;                            // the text in front of the first ':'

    // who: the prefix of every message (nullptr: the op's own name).  echo: a bad-value or missing-key message quotes the op string, cut at 96
    // characters as in the malformed-field message, which always quotes it.
    bool split(const char *op, const char *who_, const std::vector<OpKey> &list, bool echo)
    {
        const char *c = strchr(op, ':');
        name.assign(op, c ? (size_t)(c - op) : strlen(op));
        who = who_ ? std::string(who_) : name;
        keys = list;
        val.assign(keys.size(), std::string());
        given.assign(keys.size(), 0);
        quoted = echo ? " in \"" + std::string(op).substr(0, 96) + "\"" : std::string();
        while (c) {
            const char *k = c + 1, *eq = strchr(k, '='), *next = strchr(k, ':');
            if (!eq || (next && eq > next) || eq == k) { set_error("%s: malformed parameter in \"%.96s\" (expected key=value)", who.c_str(), op); return false; }
            const std::string key(k, (size_t)(eq - k));
            const int i = find(key.c_str());
            if (i < 0) { set_error("%s: unknown parameter \"%s\"", who.c_str(), key.c_str()); return false; }
            if (given[i]) { set_error("%s: parameter \"%s\" given twice", who.c_str(), key.c_str()); return false; }
            given[i] = 1;
            val[i].assign(eq + 1, next ? (size_t)(next - eq - 1) : strlen(eq + 1));
            c = next;
        }
        for (size_t i = 0; i < keys.size(); i++)
            if (!given[i] && keys[i].def) val[i] = keys[i].def;
        return true;
    }

    bool has(const char *key) const { const int i = find(key); return i >= 0 && given[i]; }
    const std::string &text(const char *key) const
    {
        static const std::string none;
        const int i = find(key);
        return i < 0 ? none : val[i];
    }

    // a double: strtod of the whole value, no ERANGE; `finite` refuses nan and inf as well
    bool number(const char *key, double &out, bool finite = false) const
    {
        if (missing(key)) return false;
        const std::string &v = text(key);
        char *end = nullptr;
        errno = 0;
        out = strtod(v.c_str(), &end);
        if (v.empty() || *end || errno == ERANGE || (finite && !std::isfinite(out))) return bad(key, finite ? " (a finite number)" : "");
        return true;
    }
    // a decimal integer in [lo, hi]
    bool integer(const char *key, long lo, long hi, long &out) const
    {
        if (missing(key)) return false;
        const std::string &v = text(key);
        char *end = nullptr;
        errno = 0;
        out = strtol(v.c_str(), &end, 10);
        if (v.empty() || *end || errno == ERANGE || out < lo || out > hi) return bad(key, " (an integer)");
        return true;
    }
    // a number that is 0 or 1
    bool flag(const char *key, bool &out) const
    {
        double d = 0.0;
        if (!number(key, d)) return false;
        if (d != 0.0 && d != 1.0) { set_error("%s: %s must be 0 or 1", who.c_str(), key); return false; }
        out = d != 0.0;
        return true;
    }
    // decimal digits only, below 2^64
    bool u64(const char *key, uint64_t &out) const
    {
        if (missing(key)) return false;
        const std::string &v = text(key);
        char *end = nullptr;
        errno = 0;
        out = strtoull(v.c_str(), &end, 10);
        if (v.empty() || v.find_first_not_of("0123456789") != std::string::npos || *end || errno == ERANGE) return bad(key, " (a decimal integer below 2^64)");
        return true;
    }
    // the index of the value in `words`; -1 if it is none of them, with the message <before><value><after>: each stage has its own wording
    int word(const char *key, std::initializer_list<const char *> words, const char *before, const char *after) const
    {
        if (missing(key)) return -1;
        int i = 0;
        for (const char *w : words) {
            if (text(key) == w) return i;
            i++;
        }
        set_error("%s%s%s", before, text(key).c_str(), after);
        return -1;
    }
    // a string of 0 / 1 characters, possibly empty
    bool bits(const char *key, std::string &out) const
    {
        if (missing(key)) return false;
        const std::string &v = text(key);
        if (v.find_first_not_of("01") != std::string::npos) { set_error("%s: %s must be a string of 0 / 1 characters, got \"%s\"", who.c_str(), key, v.c_str()); return false; }
        out = v;
        return true;
    }
    // an even number of hexadecimal digits, at least two: the bytes they spell, the first pair first
    bool hex(const char *key, std::vector<uint8_t> &out) const
    {
        if (missing(key)) return false;
        const std::string &v = text(key);
        if (v.empty() || v.size() % 2 || v.find_first_not_of("0123456789abcdefABCDEF") != std::string::npos) {
            set_error("%s: %s must be an even number of hexadecimal digits, at least two", who.c_str(), key);
            return false;
        }
        auto digit = [](char ch) { return ch <= '9' ? ch - '0' : (ch | 0x20) - 'a' + 10; };
        out.resize(v.size() / 2);
        for (size_t i = 0; i < out.size(); i++) out[i] = (uint8_t)(digit(v[2 * i]) << 4 | digit(v[2 * i + 1]));
        return true;
    }
    // a comma list of Float32 values, possibly empty: each strtod text (decimal or hexadecimal floating point) rounded to Float32, so %.9g and %a
    // give back the Float32 they were printed from.  No trailing comma; entry / hint / ends word the messages ("bad <entry> N<hint>", "<ends> with a
    // comma").  cap > 0: reading stops once more than cap values are out, for a caller that refuses the list by its count anyway.
    bool floats(const char *key, std::vector<float> &out, size_t cap, const char *entry, const char *hint, const char *ends) const
    {
        if (missing(key)) return false;
        const std::string &s = text(key);
        const char *v = s.c_str(), *vend = v + s.size();
        while (v < vend) {
            if (cap && out.size() > cap) break;
            char *end = nullptr;
            const double d = strtod(v, &end);
            if (end == v || (end < vend && *end != ',')) { set_error("%s: bad %s %zu%s", who.c_str(), entry, out.size(), hint); return false; }
            out.push_back((float)d);
            v = end < vend ? end + 1 : end;
            if (end < vend && v == vend) { set_error("%s: %s with a comma", who.c_str(), ends); return false; }
        }
        return true;
    }

private:
    std::string who, quoted;
    std::vector<OpKey> keys;
    std::vector<std::string> val;
    std::vector<char> given;
    int find(const char *key) const
    {
        for (size_t i = 0; i < keys.size(); i++)
            if (!strcmp(keys[i].key, key)) return (int)i;
        return -1;
    }
    // a required key that was not given: the message, and true
    bool missing(const char *key) const
    {
        const int i = find(key);
        if (i < 0 || given[i] || keys[i].def) return false;
        set_error("%s: missing parameter \"%s\"%s", who.c_str(), key, quoted.c_str());
        return true;
    }
    bool bad(const char *key, const char *hint) const
    {
        set_error("%s: bad value for \"%s\"%s%s", who.c_str(), key, quoted.c_str(), hint);
        return false;
    }
};
