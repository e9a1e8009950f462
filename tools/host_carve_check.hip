// host_carve_check.hip - the scratch layouts of the nine counted stages (luaradio_amd/csrc/stage_counted.h: the structs the stages' run()
// use, not copies), on the CPU: for tile counts around 1 and 256 and frame bounds 1, 2 and an odd large value, the regions lie in the order
// they were taken and do not overlap, each starts on a multiple of its alignment, and the total covers them all.
//   hipcc --offload-arch=gfx950 -O1 -std=c++17 -I luaradio_amd/csrc -I include -o /tmp/host_carve_check tools/host_carve_check.hip && /tmp/host_carve_check
#include <cstdio>
#include <cstring>
#include <memory>
#include "lrhip.h"
#include "common.h"
#include "kernels_digital.h"
#include "kernels_bitscan.h"
#include "kernels_preamble.h"
#include "kernels_varicode.h"
using namespace lrhip;
#include "stage.h"
#include "stage_carry.h"
#include "stage_counted.h"

static int failures = 0;

// `want`: alignment of each region in order (0 ends the list)
static void check(const char *what, unsigned long nt, unsigned long bound, const Carve &c, const size_t *want)
{
    int expected = 0;
    while (want[expected]) expected++;
    bool ok = c.count == expected && c.count <= (int)(sizeof(c.spans) / sizeof(c.spans[0]));
    size_t end = 0, sum = 0;
    for (int k = 0; ok && k < c.count; k++) {
        const Carve::Span &s = c.spans[k];
        ok = s.align == want[k] && s.at % s.align == 0 && s.at >= end && s.bytes > 0;
        end = s.at + s.bytes;
        sum += s.bytes;
    }
    ok = ok && c.total >= end && c.total >= sum;
    if (!ok) {
        failures++;
        printf("FAIL %s nt=%lu bound=%lu: %d regions (want %d), total %zu\n", what, nt, bound, c.count, expected, c.total);
        for (int k = 0; k < c.count && k < 8; k++) printf("   [%d] at %zu, %zu bytes, align %zu\n", k, c.spans[k].at, c.spans[k].bytes, c.spans[k].align);
    }
}

int main()
{
    const unsigned long tiles[] = {1, 2, 3, 255, 256, 257}, bounds[] = {1, 2, 1000003};
    const size_t rf[] = {8, 4, 8, 0}, ef[] = {8, 8, 4, 8, 0}, ax[] = {8, 4, 8, 8, 1, 0}, pg[] = {8, 4, 0}, ps[] = {8, 8, 4, 4, 16, 0}, md[] = {8, 4, 8, 0},
                 zc[] = {8, 4, 8, 4, 8, 4, 4, 4, 0}, sm[] = {8, 4, 8, 0}, vc[] = {8, 8, 4, 4, 4, 0};
    int cases = 0;
    for (unsigned long nt : tiles)
        for (unsigned long b : bounds) {
            check("rdsframer", nt, b, RfScratch(nt, b), rf);
            check("ertframer", nt, b, EfScratch(nt, b), ef);
            // (the flag list of the AX.25 stage is sized by the call, as the tiles are: every combination with the frame bound)
            for (unsigned long flags : bounds) check("ax25framer", nt, b, AxScratch(nt, flags, b), ax);
            check("pocsagframer", nt, b, PgScratch(nt), pg);
            check("preamblesampler", nt, b, PsScratch(nt, b), ps);
            check("manchesterdecoder", nt, b, MdScratch(nt), md);
            check("clocksampler", nt, b, ZcScratch(nt), zc);
            check("sampler", nt, b, SamplerScratch(nt), sm);
            check("varicodedecoder", nt, b, VcScratch(nt), vc);
            cases += 11;
        }
    if (failures) {
        printf("%d of %d layouts FAILED\n", failures, cases);
        return 1;
    }
    printf("%d scratch layouts OK\n", cases);
    return 0;
}
