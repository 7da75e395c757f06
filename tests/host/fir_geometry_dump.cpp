// fir_geometry_dump.cpp -- prints the geometry of a periodic FIR launch (fir_geometry.cpp: periodic_geometry) and the
// kernel build chosen for it (split_build_for / periodic_slot_for) over a grid of rate pairs, tap counts, channel counts
// and kernel modes: one row per input.  tests/test_host_programs.py builds it as plain C++ under ASan + UBSan, runs it
// once per setting of the debug switches (they are read once per process) and compares the rows with
// tests/golden/fir_geometry.json, which was recorded from the commit before the rules left the kernel files
// (tests/golden/make_fir_geometry_fixture.py: this program with -DRSMP_GEOMETRY_ONLY linked against that commit's
// library, the build choice transcribed from its launchers).
#include <cstdint>
#include <cstdio>
#include <numeric>

#include "fir_periodic_plan.h"

int main() {
    static const uint32_t rates[10] = {22050, 16000, 32000, 44100, 48000, 88200, 96000, 176400, 192000, 384000};
    static const uint32_t taps_of[4] = {16, 32, 64, 128};                    // every Latency
    static const uint32_t channels_of[9] = {1, 2, 3, 4, 6, 8, 12, 16, 17};
    static const bool modes[3][2] = {{true, true}, {false, true}, {true, false}};   // (allow_matrix, allow_split): AUTO / PERIODIC, PERIODIC_VECTOR, PERIODIC_F32
    uint32_t pairs[91][2];
    int n_pairs = 0;
    for (int i = 0; i < 10; ++i)
        for (int o = 0; o < 10; ++o)
            if (i != o) {
                pairs[n_pairs][0] = rates[i];
                pairs[n_pairs++][1] = rates[o];
            }
    pairs[n_pairs][0] = 24000;
    pairs[n_pairs++][1] = 16000;
    for (uint32_t taps : taps_of)
        for (uint32_t ch : channels_of)
            for (int mode = 0; mode < 3; ++mode)
                for (int p = 0; p < n_pairs; ++p) {
                    const uint32_t g0 = std::gcd(pairs[p][0], pairs[p][1]);
                    const uint32_t num = pairs[p][0] / g0, den = pairs[p][1] / g0;
                    const rsmp::PeriodicGeometry g = rsmp::periodic_geometry(num, den, taps, ch, modes[mode][0], modes[mode][1]);
                    printf("%u %u %d %u/%u | %d %u %u %u %u %u %u %u %u %u %u %u %u %u %u %u %u %u %u %u %d", taps, ch, mode, num, den, g.ok ? 1 : 0,
                           g.a, g.b, g.den, g.taps, g.row_len, g.n_tiles, g.cg, g.lp, g.pw, g.row_stride, g.waves, g.producers, g.images, g.mfma,
                           g.planes, g.groups, g.rounds, g.n_units, g.lds_bytes, g.inline_wraps ? 1 : 0);
#ifndef RSMP_GEOMETRY_ONLY
                    // the build: split kernel plain / diagnostic / 16-bit PCM input; the others without and with RSMP_FIR_MFMA_DBG=1
                    if (!g.ok) {
                        printf(" | -");
                    } else if (g.mfma == 3) {
                        static const struct { bool diag; uint32_t bits; } asks[3] = {{false, 0}, {true, 0}, {false, 16}};
                        printf(" |");
                        for (const auto& q : asks) {
                            const rsmp::SplitChoice c = rsmp::split_build_for(g, q.diag, rsmp::FirFormat{q.bits, 0, 0, false});
                            if (c.error != rsmp::BuildError::kNone) printf(" split:%s", c.error == rsmp::BuildError::kInvalid ? "invalid" : "unsupported");
                            else printf(" split:%d,%d,%d,%d,%d,%d", c.build.nk, c.build.planes, c.build.diag ? 1 : 0, c.build.wide, c.build.rounds, c.build.bits);
                        }
                    } else {
                        printf(" | slot:%d slot:%d", rsmp::periodic_slot_for(g, 0, rsmp::mfma_ring_knob()), rsmp::periodic_slot_for(g, 1, rsmp::mfma_ring_knob()));
                    }
#endif
                    printf("\n");
                }
    return 0;
}
