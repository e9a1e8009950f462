// host_fecglue_check.hip - the counting and index arithmetic of the puncturing, interleaving and scrambling stages (luaradio_amd/csrc/fecglue_plan.h
// and, for the frames, rs_plan.h: the headers the stages and the kernels use, not copies) on the CPU.  Reads a file of lines and answers each on one
// line (tests/test_fecglue_cpu.py holds the answers to Python's integers and to the models of tests/helpers/fecglue_model.py):
//     frames <B>              ->  frames <check> <puncture FI> <FO> <depuncture FI> <FO>   check: 0, or 1 length, 2 character, 3 no 1 (then zeros)
//     pmap <B>                ->  pmap <input element of output 0> ...                     the puncturer's map of a frame
//     dmap <B>                ->  dmap <input element of output 0, or 255> ...             the depuncturer's
//     done <FI> <FO> <Q>      ->  done <frames> <elements carried> <ok> <output position>  after Q input elements (ok = 0: at or behind 2^64, printed 0)
//     max <FI> <FO> <N>       ->  max <bound>                                              the capacity bound of a call of N elements
//     shape <FI> <FO>         ->  shape <memory>
//     table <i> <K> <P>       ->  table <index of the table entry of absolute byte i>
//     advance <t> <n> <P>     ->  advance <the index n bytes behind index t>
//     check <I> <M>           ->  check <0, or 1 branches, 2 step, 3 depth> <depth, 0 if refused>
//     source <i> <I> <M> <d>  ->  source <ok> <absolute input of absolute output i>        d = 1: the deinterleaver; ok = 0: in front of the stream
// All numbers are decimal.  No device code and no HIP call: it builds as plain C++ as well as with hipcc.
//   g++ -O1 -std=c++17 -x c++ -I luaradio_amd/csrc -o /tmp/host_fecglue_check tools/host_fecglue_check.hip && /tmp/host_fecglue_check cases.txt
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "fecglue_plan.h"

static int bad_line(FILE *in, long number, const char *line)
{
    printf("bad line %ld: %s", number, line);
    fclose(in);
    return 1;
}

int main(int argc, char **argv)
{
    if (argc != 2) { printf("usage: host_fecglue_check <file of cases>\n"); return 2; }
    FILE *in = fopen(argv[1], "r");
    if (!in) { printf("cannot read %s\n", argv[1]); return 2; }
    char line[512], what[16], text[256];
    long lines = 0;
    while (fgets(line, sizeof line, in)) {
        lines++;
        if (sscanf(line, "%15s", what) != 1) return bad_line(in, lines, line);
        if (!strcmp(what, "frames") || !strcmp(what, "pmap") || !strcmp(what, "dmap")) {
            text[0] = 0;
            (void)sscanf(line, "%*s %255s", text);                       // an empty pattern is a case
            const uint64_t n = strlen(text);
            const int check = fgplan::check_pattern(text, n);
            if (!strcmp(what, "frames")) {
                if (check) { printf("frames %d 0 0 0 0\n", check); continue; }
                const rsplan::Frame p = fgplan::puncture_frame(text, (uint32_t)n), d = fgplan::depuncture_frame(text, (uint32_t)n);
                printf("frames 0 %u %u %u %u\n", p.fi, p.fo, d.fi, d.fo);
                continue;
            }
            if (check) return bad_line(in, lines, line);
            uint8_t map[fgplan::PATTERN_MAX];
            const bool punct = !strcmp(what, "pmap");
            if (punct) fgplan::puncture_map(text, (uint32_t)n, map); else fgplan::depuncture_map(text, (uint32_t)n, map);
            printf("%s", what);
            const uint32_t count = punct ? fgplan::ones(text, (uint32_t)n) : (uint32_t)n;
            for (uint32_t i = 0; i < count; i++) printf(" %u", map[i]);
            printf("\n");
            continue;
        }
        uint64_t a[4] = {0, 0, 0, 0};
        const int got = sscanf(line, "%*s %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64, &a[0], &a[1], &a[2], &a[3]);
        if (!strcmp(what, "done") || !strcmp(what, "max") || !strcmp(what, "shape")) {
            if (got < 2 || a[0] < 1 || a[0] > 64 || a[1] < 1 || a[1] > 64) return bad_line(in, lines, line);
            const rsplan::Frame f{(uint32_t)a[0], (uint32_t)a[1]};
            if (!strcmp(what, "done") && got == 3) {
                uint64_t pos = 0;
                const bool ok = rsplan::out_position(a[2], f, &pos);
                printf("done %" PRIu64 " %u %d %" PRIu64 "\n", rsplan::frames_done(a[2], f), rsplan::carried(a[2], f), ok ? 1 : 0, ok ? pos : (uint64_t)0);
            } else if (!strcmp(what, "max") && got == 3) {
                printf("max %" PRIu64 "\n", rsplan::max_output(a[2], f));
            } else if (!strcmp(what, "shape") && got == 2) {
                printf("shape %" PRIu64 "\n", rsplan::memory(f));
            } else {
                return bad_line(in, lines, line);
            }
        } else if (!strcmp(what, "table") && got == 3 && a[2] >= 1 && a[2] <= (uint64_t)fgplan::TABLE_MAX && a[1] < a[2]) {
            printf("table %u\n", fgplan::table_index(a[0], (uint32_t)a[1], (uint32_t)a[2]));
        } else if (!strcmp(what, "advance") && got == 3 && a[2] >= 1 && a[2] <= (uint64_t)fgplan::TABLE_MAX && a[0] < a[2]) {
            printf("advance %u\n", fgplan::table_advance((uint32_t)a[0], a[1], (uint32_t)a[2]));
        } else if (!strcmp(what, "check") && got == 2 && a[0] <= 100000 && a[1] <= 100000) {
            const int check = fgplan::check_interleaver((long)a[0], (long)a[1]);
            printf("check %d %u\n", check, check ? 0u : fgplan::depth((uint32_t)a[0], (uint32_t)a[1]));
        } else if (!strcmp(what, "source") && got == 4 && !fgplan::check_interleaver((long)a[1], (long)a[2]) && a[3] <= 1) {
            uint64_t src = 0;
            const bool ok = fgplan::source_index(a[0], (uint32_t)a[1], (uint32_t)a[2], a[3] == 1, &src);
            printf("source %d %" PRIu64 "\n", ok ? 1 : 0, ok ? src : (uint64_t)0);
        } else {
            return bad_line(in, lines, line);
        }
    }
    fclose(in);
    return lines ? 0 : 1;
}
