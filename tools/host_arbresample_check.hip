// host_arbresample_check.hip - the position arithmetic of the arbitrary-ratio resampler (luaradio_amd/csrc/arbresample_plan.h: the header the stage and the
// kernel use, not a copy) on the CPU.  Reads a file of lines and answers each on one line (tests/test_arbresample_cpu.py holds the answers to Python's
// big integers):
//     pos <step> <log2 P> <m>      ->  pos <i_hi> <i_lo> <p> <mu24>          i = i_hi * 2^64 + i_lo, mu = mu24 * 2^-24
//     count <step> <Q>             ->  count <hi> <lo>                       outputs that exist after Q inputs
//     seek <step> <n0>             ->  seek <hi> <lo>                        the first output of a stream that continues at input n0
//     max <step> <n>               ->  max <bound>                           the capacity bound of a call of n inputs
// No device code and no HIP call: it builds as plain C++ as well as with hipcc.
//   g++ -O1 -std=c++17 -x c++ -I luaradio_amd/csrc -o /tmp/host_arbresample_check tools/host_arbresample_check.hip && /tmp/host_arbresample_check cases.txt
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "arbresample_plan.h"

int main(int argc, char **argv)
{
    if (argc != 2) { printf("usage: host_arbresample_check <file of cases>\n"); return 2; }
    FILE *in = fopen(argv[1], "r");
    if (!in) { printf("cannot read %s\n", argv[1]); return 2; }
    char line[256], what[16];
    long lines = 0;
    while (fgets(line, sizeof line, in)) {
        uint64_t step = 0, a = 0, b = 0;
        const int got = sscanf(line, "%15s %" SCNu64 " %" SCNu64 " %" SCNu64, what, &step, &a, &b);
        if (got < 3 || step < arbplan::STEP_MIN || step > arbplan::STEP_MAX) { printf("bad line %ld: %s", lines + 1, line); fclose(in); return 1; }
        if (!strcmp(what, "pos") && got == 4 && a >= (uint64_t)arbplan::LOG2P_MIN && a <= (uint64_t)arbplan::LOG2P_MAX) {
            const arbplan::Pos q = arbplan::position(b, step, (int)a);
            printf("pos %" PRIu64 " %" PRIu64 " %u %u\n", q.i_hi, q.i_lo, q.p, q.mu24);
        } else if (!strcmp(what, "count") && got == 3) {
            const arbplan::Count c = arbplan::output_count(a, step);
            printf("count %" PRIu64 " %" PRIu64 "\n", c.hi, c.lo);
        } else if (!strcmp(what, "seek") && got == 3) {
            const arbplan::Count c = arbplan::seek_output(a, step);
            printf("seek %" PRIu64 " %" PRIu64 "\n", c.hi, c.lo);
        } else if (!strcmp(what, "max") && got == 3) {
            printf("max %" PRIu64 "\n", arbplan::max_output(a, step));
        } else {
            printf("bad line %ld: %s", lines + 1, line);
            fclose(in);
            return 1;
        }
        lines++;
    }
    fclose(in);
    return lines ? 0 : 1;
}
