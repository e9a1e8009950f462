// host_launch_prep_check.hip - the grid arithmetic of luaradio_amd/csrc/launch_prep.h (persistent_grid, persistent_rounds) against the expressions the launchers
// spelled out by hand before that header existed, COPIED here as they stood: a difference is a change of launch geometry, to be explained, not re-recorded.
//   hipcc --offload-arch=gfx950 -O1 -std=c++17 -I luaradio_amd/csrc -I include -o /tmp/host_launch_prep_check tools/host_launch_prep_check.hip && /tmp/host_launch_prep_check
// (plain host code: also clean as an executable built with -Xarch_host -fsanitize=address,undefined)
#include <cstdio>
#include "launch_prep.h"
using namespace lrhip;

// stage_fir.h (persistent Toeplitz, both lambdas of launch_decim_lds): the gate, then the grid
static int gate_a(long ntiles, long slots, int knob) { const int rounds = ntiles > slots && knob > 0 ? knob : 0; return rounds; }
static unsigned grid_a(long ntiles, long slots, int rounds) { unsigned grid = rounds > 0 ? (unsigned)((ntiles + rounds - 1) / rounds) : (unsigned)(ntiles < slots ? ntiles : slots); return grid; }
// stage_spectrum.h (LRHIP_SPEC_ROUNDS, -1 = unset); stage_fir.h launch_fft (LRHIP_FFT_ROUNDS) spelled it so as well
static int gate_b(long want, long slots, int knob)
{
    int rounds = knob >= 0 ? knob : 0;
    if (want <= slots) rounds = 0;
    return rounds;
}
static unsigned grid_b(long want, long slots, int rounds) { unsigned grid = rounds > 0 ? (unsigned)((want + rounds - 1) / rounds) : (unsigned)(want < slots ? want : slots); return grid; }
// stage_resample.h (both register-window kernels): resample_rounds() without LRHIP_RESAMPLE_ROUNDS, then the workgroup count
static int gate_c(long ntiles, long slots) { return ntiles <= slots ? 0 : 1; }
static unsigned grid_c(long ntiles, long slots, int rounds) { const long wgs = rounds > 0 ? (ntiles + rounds - 1) / rounds : (ntiles < slots ? ntiles : slots); return (unsigned)wgs; }
// stage_fir.h launch_fft4k_ng: no rounds
static unsigned grid_d(long nslots, long slots) { const unsigned grid = (unsigned)(nslots < slots ? nslots : slots); return grid; }

int main()
{
    const long slot_counts[] = {1, 255, 256, 768, 2048};
    const int knobs[] = {-1, 0, 1, 2, 4, 8};      // (-1: the unset value of the two environment knobs)
    const int round_counts[] = {0, 1, 2, 4, 8};
    long bad = 0, checked = 0;
    auto expect = [&](const char *what, long work, long slots, int r, long got, long want) {
        checked++;
        if (got != want && bad++ < 20) printf("MISMATCH %s: work %ld, slots %ld, rounds / knob %d: %ld (want %ld)\n", what, work, slots, r, got, want);
    };
    for (long slots : slot_counts)
        for (long work = 0; work <= 5000; work++) {
            for (int knob : knobs) {
                const int r = persistent_rounds(work, slots, knob);
                expect("gate, work > slots && knob > 0", work, slots, knob, r, gate_a(work, slots, knob));
                expect("gate, want <= slots", work, slots, knob, r, gate_b(work, slots, knob));
                // gate and grid together, as a launcher uses them
                expect("gated grid", work, slots, knob, persistent_grid(work, slots, r), grid_a(work, slots, gate_a(work, slots, knob)));
                expect("gated grid, want <= slots", work, slots, knob, persistent_grid(work, slots, r), grid_b(work, slots, gate_b(work, slots, knob)));
            }
            expect("gate, resampler", work, slots, 1, persistent_rounds(work, slots, 1), gate_c(work, slots));
            // every rounds value, gated or forced (LRHIP_RESAMPLE_ROUNDS forces a run length on launches that fit the slots too)
            for (int rounds : round_counts) {
                const unsigned g = persistent_grid(work, slots, rounds);
                expect("grid", work, slots, rounds, g, grid_a(work, slots, rounds));
                expect("grid, overlap-save / spectrum", work, slots, rounds, g, grid_b(work, slots, rounds));
                expect("grid, resampler", work, slots, rounds, g, grid_c(work, slots, rounds));
            }
            expect("grid, 4096-point workgroups", work, slots, 0, persistent_grid(work, slots, 0), grid_d(work, slots));
        }
    printf("%ld comparisons\n", checked);
    printf(bad ? "FAILED (%ld)\n" : "OK\n", bad);
    return bad ? 1 : 0;
}
