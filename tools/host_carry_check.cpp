// host_carry_check.cpp - the two carried-state types of luaradio_amd/csrc/stage_carry.h (the header the stages include, not a copy) on the CPU,
// over buffers of exactly the requested size in host memory: in() and out() are the two slots, flip() swaps them, reset() returns to the first slot
// with both slots filled however many calls went before, the typed pair's slots are adjacent, and only fetch() allocates the read-back buffer.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -I luaradio_amd/csrc -o /tmp/host_carry_check tools/host_carry_check.cpp && /tmp/host_carry_check
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>

// ---- what the header takes from common.h and stage.h, on the heap (an exact-size allocation: the sanitizer sees one byte too many)
struct DeviceBuf {
    void *p = nullptr;
    size_t cap = 0;
    int reserve(size_t bytes)
    {
        if (bytes <= cap) return 0;
        free(p);
        p = malloc(bytes);
        cap = p ? bytes : 0;
        return p ? 0 : -1;
    }
    ~DeviceBuf() { free(p); }
};
using PinnedBuf = DeviceBuf;
static int upload(DeviceBuf &b, const void *src, size_t bytes)
{
    if (b.reserve(bytes ? bytes : 4)) return -1;
    memcpy(b.p, src, bytes);
    return 0;
}
static int zero_fill(DeviceBuf &b, size_t bytes)
{
    if (b.reserve(bytes ? bytes : 4)) return -1;
    memset(b.p, 0, bytes ? bytes : 4);
    return 0;
}
struct Ctx { int stream = 0; };
static Ctx &ctx() { static Ctx c; return c; }
enum { hipMemcpyDeviceToHost = 2 };
static int hipMemcpyAsync(void *dst, const void *src, size_t n, int, int) { memcpy(dst, src, n); return 0; }
static int hipStreamSynchronize(int) { return 0; }
#define LR_HIP(call) do { if ((call) != 0) return -1; } while (0)

#include "stage_carry.h"

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { failures++; printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); } } while (0)

static bool all_zero(const void *p, size_t n)
{
    for (size_t i = 0; i < n; i++) if (((const uint8_t *)p)[i]) return false;
    return true;
}

struct State { double a; uint64_t count; float r[2]; };

int main()
{
    for (size_t bytes : {(size_t)1, (size_t)7, (size_t)4096}) {
        TwoSlots t;
        CHECK(t.reset(bytes) == 0);
        for (int calls = 0; calls < 4; calls++) {
            void *in = t.in(), *out = t.out();
            CHECK(in != out && in == (void *)t.in<float>() && out == (void *)t.out<uint8_t>());
            memset(out, 0x5a + calls, bytes);                  // a call's kernels write the whole out() slot
            t.flip();
            CHECK(t.in() == out && t.out() == in && ((const uint8_t *)t.in())[bytes - 1] == 0x5a + calls);
            if (calls % 2 == 0) {                              // reset behind an odd number of calls: the first slot again, both zero
                TwoSlots u;
                CHECK(u.reset(bytes) == 0);
                memset(u.out(), 1, bytes);
                u.flip();
                CHECK(u.reset(bytes) == 0 && u.in() == u.slot[0].p && all_zero(u.in(), bytes) && all_zero(u.out(), bytes));
            }
        }
    }
    {
        Carried<State> c;
        State v{1.5, 7, {2.f, -0.f}};
        CHECK(c.reset(v) == 0 && c.host.p == nullptr);         // no read-back buffer before the first fetch()
        CHECK(c.out() == c.in() + 1 && !memcmp(c.in(), &v, sizeof(v)) && !memcmp(c.out(), &v, sizeof(v)));
        c.out()->count = 8;
        c.flip();
        CHECK(c.in()->count == 8 && c.out() == c.in() - 1 && c.out()->count == 7);
        State got{};
        CHECK(c.fetch(got) == 0 && got.count == 8 && c.host.p != nullptr);
        CHECK(c.reset() == 0 && c.out() == c.in() + 1 && all_zero(c.in(), 2 * sizeof(State)));
    }
    {
        Carried<uint8_t[8]> h;                                 // an array state: *in() is its first element
        CHECK(h.reset() == 0);
        const uint8_t *in = *h.in();
        uint8_t *out = *h.out();
        CHECK(out == in + 8 && all_zero(in, 16));
        memset(out, 3, 8);
        h.flip();
        CHECK(*h.in() == out && (*h.in())[7] == 3 && *h.out() == in);
        Carried<double[2]> d;
        CHECK(d.reset() == 0 && *d.out() == *d.in() + 2);
    }
    {
        Carried<State, 24> c;                                  // carried bytes beside the state
        CHECK(c.reset() == 0 && c.co() == c.ci() + 24 && all_zero(c.ci(), 48));
        memset(c.co(), 9, 24);
        c.flip();
        CHECK(c.ci()[23] == 9 && c.co() == c.ci() - 24);
        CHECK(c.reset() == 0 && all_zero(c.ci(), 48) && c.co() == c.ci() + 24);
    }
    if (failures) printf("%d FAILED\n", failures); else printf("OK\n");
    return failures ? 1 : 0;
}
