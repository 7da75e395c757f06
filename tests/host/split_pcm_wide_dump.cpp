// split_pcm_wide_dump.cpp -- prints the split kernel's build choice (fir_geometry.cpp: split_build_for) for PCM input and
// output over channel counts: the periodic geometry of a 128-tap filter for 44.1 -> 48, 96 -> 44.1 and 96 -> 48 kHz at 2, 4,
// 6, 8, 12 and 16 channels and for 44.1 -> 48 kHz at 1, 3 and 5, each asked with pcm_bits 0 / 16, out_bits 0 / 16 / 24 / 32 / 8,
// dither 0 / 1 and statistics off / on: one row per question.  tests/test_pcm_out_wide_host.py builds it as plain C++ under
// ASan + UBSan and holds the rows to the rule (even counts of 4 .. 16 channels write PCM from the channel-pair builds) and, for
// two channels and for f32 output, to tests/golden/split_pcm_wide.json (tests/golden/make_split_pcm_wide_fixture.py: this
// program compiled against the sources of the commit before the rule changed -- as it was at ef8e494, before split_build_for
// came to take a FirFormat; the rows it prints are the same).
#include <cstdint>
#include <cstdio>
#include <numeric>

#include "fir_periodic_plan.h"

int main() {
    static const struct { uint32_t in_hz, out_hz; uint32_t channels[6]; } cases[4] = {
        {44100, 48000, {2, 4, 6, 8, 12, 16}}, {96000, 44100, {2, 4, 6, 8, 12, 16}}, {96000, 48000, {2, 4, 6, 8, 12, 16}},
        {44100, 48000, {1, 3, 5, 0, 0, 0}}};
    static const uint32_t pcm_of[2] = {0, 16}, out_of[5] = {0, 16, 24, 32, 8};
    for (const auto& c : cases)
        for (uint32_t ch : c.channels) {
            if (ch == 0) continue;
            const uint32_t g0 = std::gcd(c.in_hz, c.out_hz);
            const rsmp::PeriodicGeometry g = rsmp::periodic_geometry(c.in_hz / g0, c.out_hz / g0, 128, ch, true, true);
            for (uint32_t pcm_bits : pcm_of)
                for (uint32_t out_bits : out_of)
                    for (uint32_t dither = 0; dither < 2; ++dither)
                        for (int stats = 0; stats < 2; ++stats) {
                            printf("%u %u %u %u %u %u %d | %d %u %u %u %u %u %u |", c.in_hz, c.out_hz, ch, pcm_bits, out_bits, dither, stats,
                                   g.ok ? 1 : 0, g.mfma, g.planes, g.cg, g.lp, g.rounds, g.row_len);
                            if (!g.ok || g.mfma != 3) {
                                printf(" -\n");
                                continue;
                            }
                            const rsmp::SplitChoice s = rsmp::split_build_for(g, false, rsmp::FirFormat{pcm_bits, out_bits, dither, stats != 0});
                            if (s.error != rsmp::BuildError::kNone) printf(" %s\n", s.error == rsmp::BuildError::kInvalid ? "invalid" : "unsupported");
                            else printf(" split:%d,%d,%d,%d,%d,%d,%d,%d,%d\n", s.build.nk, s.build.planes, s.build.diag ? 1 : 0, s.build.wide, s.build.rounds,
                                        s.build.bits, s.build.pcm_out ? 1 : 0, s.build.dither ? 1 : 0, s.build.stats ? 1 : 0);
                        }
        }
    return 0;
}
