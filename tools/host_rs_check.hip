// host_rs_check.hip - the frame arithmetic and the code construction of the Reed-Solomon and bit-packing stages (luaradio_amd/csrc/rs_plan.h: the
// header the stages and the kernels use, not a copy) on the CPU.  Reads a file of lines and answers each on one line (tests/test_reedsolomon_cpu.py
// holds the answers to Python's integers and to the model of tests/helpers/reedsolomon_model.py):
//     done <FI> <FO> <Q>      ->  done <frames> <bytes carried> <ok> <output position>    after Q inputs (also where a seek to Q lands; ok = 0: the
//                                                                                         position lies at or behind 2^64 and is printed as 0)
//     max <FI> <FO> <N>       ->  max <bound>                                            the capacity bound of a call of N inputs
//     shape <FI> <FO>         ->  shape <memory>
//     frames <n> <k> <I> <status>  ->  frames <encoder FI> <encoder FO> <decoder FI> <decoder FO>
//     check <n> <k> <gfpoly> <fcr> <prim> <I>  ->  check <0, or the number of the first refused parameter>
//     exp <n> <k> <gfpoly> <fcr> <prim>    ->  exp <alpha^0> ... <alpha^254>
//     roots <n> <k> <gfpoly> <fcr> <prim>  ->  roots <root 0> ... <root n - k - 1>
//     gen <n> <k> <gfpoly> <fcr> <prim>    ->  gen <coefficient of x^0> ... <coefficient of x^(n - k)>
//     parity <n> <k> <gfpoly> <fcr> <prim> <i>  ->  parity <the n - k parity bytes of the message whose byte i is 1 and whose other bytes are 0>
// All numbers are decimal.  No device code and no HIP call: it builds as plain C++ as well as with hipcc.
//   g++ -O1 -std=c++17 -x c++ -I luaradio_amd/csrc -o /tmp/host_rs_check tools/host_rs_check.hip && /tmp/host_rs_check cases.txt
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "rs_plan.h"

static int bad_line(FILE *in, long number, const char *line)
{
    printf("bad line %ld: %s", number, line);
    fclose(in);
    return 1;
}

int main(int argc, char **argv)
{
    if (argc != 2) { printf("usage: host_rs_check <file of cases>\n"); return 2; }
    FILE *in = fopen(argv[1], "r");
    if (!in) { printf("cannot read %s\n", argv[1]); return 2; }
    char line[256], what[16];
    long lines = 0;
    while (fgets(line, sizeof line, in)) {
        uint64_t a[6] = {0, 0, 0, 0, 0, 0};
        const int got = sscanf(line, "%15s %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64, what, &a[0], &a[1], &a[2], &a[3], &a[4], &a[5]);
        if (got < 3) return bad_line(in, lines + 1, line);
        const bool framed = !strcmp(what, "done") || !strcmp(what, "max") || !strcmp(what, "shape");
        if (framed) {
            if (a[0] < 1 || a[0] > (uint64_t)rsplan::FRAME_MAX || a[1] < 1 || a[1] > (uint64_t)rsplan::FRAME_MAX) return bad_line(in, lines + 1, line);
            const rsplan::Frame f{(uint32_t)a[0], (uint32_t)a[1]};
            if (!strcmp(what, "done") && got == 4) {
                uint64_t pos = 0;
                const bool ok = rsplan::out_position(a[2], f, &pos);
                printf("done %" PRIu64 " %u %d %" PRIu64 "\n", rsplan::frames_done(a[2], f), rsplan::carried(a[2], f), ok ? 1 : 0, ok ? pos : (uint64_t)0);
            } else if (!strcmp(what, "max") && got == 4) {
                printf("max %" PRIu64 "\n", rsplan::max_output(a[2], f));
            } else if (!strcmp(what, "shape") && got == 3) {
                printf("shape %" PRIu64 "\n", rsplan::memory(f));
            } else {
                return bad_line(in, lines + 1, line);
            }
            lines++;
            continue;
        }
        for (int i = 0; i < 6; i++)
            if (a[i] > 65536) return bad_line(in, lines + 1, line);
        if (!strcmp(what, "frames") && got == 5) {
            const rsplan::Code c{(int)a[0], (int)a[1], 0x11d, 0, 1, (int)a[2], (int)a[3]};
            if (rsplan::check_code(c)) return bad_line(in, lines + 1, line);
            const rsplan::Frame e = rsplan::encoder_frame(c), d = rsplan::decoder_frame(c);
            printf("frames %u %u %u %u\n", e.fi, e.fo, d.fi, d.fo);
            lines++;
            continue;
        }
        if (!strcmp(what, "check") && got == 7) {
            printf("check %d\n", rsplan::check_code(rsplan::Code{(int)a[0], (int)a[1], (int)a[2], (int)a[3], (int)a[4], (int)a[5], 0}));
            lines++;
            continue;
        }
        const rsplan::Code c{(int)a[0], (int)a[1], (int)a[2], (int)a[3], (int)a[4], 1, 0};
        if (got < 6 || rsplan::check_code(c)) return bad_line(in, lines + 1, line);
        rsplan::Field field;
        rsplan::build_field(c.gfpoly, field);
        const int p = c.n - c.k;
        if (!strcmp(what, "exp") && got == 6) {
            printf("exp");
            for (int i = 0; i < 255; i++) printf(" %d", field.exp[i]);
        } else if (!strcmp(what, "roots") && got == 6) {
            uint8_t root_log[rsplan::PARITY_MAX];
            rsplan::build_roots(c, root_log);
            printf("roots");
            for (int i = 0; i < p; i++) printf(" %d", field.exp[root_log[i]]);
        } else if (!strcmp(what, "gen") && got == 6) {
            uint8_t gen[rsplan::PARITY_MAX + 1];
            rsplan::build_generator(c, field, gen);
            printf("gen");
            for (int i = 0; i <= p; i++) printf(" %d", gen[i]);
        } else if (!strcmp(what, "parity") && got == 7 && a[5] < (uint64_t)c.k) {
            std::vector<uint8_t> matrix((size_t)c.k * p);
            rsplan::build_parity_matrix(c, field, matrix.data());
            printf("parity");
            for (int j = 0; j < p; j++) printf(" %d", matrix[(size_t)a[5] * p + j]);
        } else {
            return bad_line(in, lines + 1, line);
        }
        printf("\n");
        lines++;
    }
    fclose(in);
    return lines ? 0 : 1;
}
