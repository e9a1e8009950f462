// host_viterbi_check.hip - the count arithmetic of the windowed Viterbi decoder (luaradio_amd/csrc/viterbi_plan.h: the header the stage and the kernels
// use, not a copy) on the CPU.  Reads a file of lines and answers each on one line (tests/test_viterbi_cpu.py holds the answers to Python's integers):
//     done <n> <D> <L> <Q>      ->  done <windows> <bits>            windows complete and bits emitted after Q inputs (also where a seek to Q lands)
//     win <n> <D> <L> <w>       ->  win <first step> <last step> <steps>
//     base <n> <D> <L> <done>   ->  base <first carried input>
//     max <n> <D> <L> <N>       ->  max <bound>                      the capacity bound of a call of N inputs
//     shape <n> <D> <L>         ->  shape <memory> <carry capacity>
// No device code and no HIP call: it builds as plain C++ as well as with hipcc.
//   g++ -O1 -std=c++17 -x c++ -I luaradio_amd/csrc -o /tmp/host_viterbi_check tools/host_viterbi_check.hip && /tmp/host_viterbi_check cases.txt
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "viterbi_plan.h"

int main(int argc, char **argv)
{
    if (argc != 2) { printf("usage: host_viterbi_check <file of cases>\n"); return 2; }
    FILE *in = fopen(argv[1], "r");
    if (!in) { printf("cannot read %s\n", argv[1]); return 2; }
    char line[256], what[16];
    long lines = 0;
    while (fgets(line, sizeof line, in)) {
        uint64_t n = 0, D = 0, L = 0, a = 0;
        const int got = sscanf(line, "%15s %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64, what, &n, &D, &L, &a);
        if (got < 4 || n < (uint64_t)vitplan::N_MIN || n > (uint64_t)vitplan::N_MAX || D < (uint64_t)vitplan::D_MIN || D > (uint64_t)vitplan::D_MAX || L < 1 ||
            L > (uint64_t)vitplan::L_MAX) {
            printf("bad line %ld: %s", lines + 1, line);
            fclose(in);
            return 1;
        }
        const vitplan::Shape s{(uint32_t)n, (uint32_t)D, (uint32_t)L};
        if (!strcmp(what, "done") && got == 5) {
            printf("done %" PRIu64 " %" PRIu64 "\n", vitplan::windows_done(a, s), vitplan::bits_done(a, s));
        } else if (!strcmp(what, "win") && got == 5) {
            printf("win %" PRIu64 " %" PRIu64 " %u\n", vitplan::first_step(a, s), vitplan::last_step(a, s), vitplan::window_steps(a, s));
        } else if (!strcmp(what, "base") && got == 5) {
            printf("base %" PRIu64 "\n", vitplan::carry_base(a, s));
        } else if (!strcmp(what, "max") && got == 5) {
            printf("max %" PRIu64 "\n", vitplan::max_output(a, s));
        } else if (!strcmp(what, "shape") && got == 4) {
            printf("shape %" PRIu64 " %u\n", vitplan::memory(s), vitplan::carry_capacity(s));
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
