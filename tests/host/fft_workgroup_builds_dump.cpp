// fft_workgroup_builds_dump.cpp -- what fft_launch.cpp answers to every request of tests/test_fft_workgroup_builds_gpu.py, as JSON:
// the ordinary library, 256 CUs.  tests/test_host_programs.py builds it with ASan + UBSan and runs it twice -- the debug switches
// are read once per process --: `default` with no switch set and `switched` under RSMP_DEBUG=1 RSMP_FFT_WAVE=0; the two outputs,
// as the members "default" and "switched" of one object, are tests/golden/fft_workgroup_builds.json byte for byte.  The same test
// reads from it which builds of fft_kernels.hip the GPU module's launches name.
//
//   "rows":  per ordered rate pair of fft_cases::plans() one line per kind of case,
//            "in_hz out_hz fft_in fft_out | kind | launch | launch ...", a launch being
//            "n_streams max_blocks max_channels min_channels family pair=P block=B gridz=Z lds=L grant=G runs=r/x,r/x,r/x" for the
//            workgroup kernels -- runs: fft_choose_run's blocks per run / grid.x for an occupancy answer of 1, 2 and 4 -- and
//            "... family pair=P chm=C occ=O bits=B block=B lds=L" for the pair and wave kernels.
//   kinds:   "mixed"      streams of 1, 3 and 2 channels: n_chunks [9, 4, 0], then [4, 5] on streams 0 and 2 (default only);
//            "uniform C"  three streams of C channels, the same launches;
//            "twin C"     a handle of C channels alone: 9, 4 and 5 blocks -- the launches the streams of a case get when each runs
//                         on its own, and the four blocks that follow a case;
//            "percall 1"  one block of one channel: resample() (default only).
//            C = 1, 2, 3; switched: 1, 2.
#include <cstdio>
#include <cstring>
#include <string>

#include "fft_launch.h"
#include "fft_launch_cases.h"

namespace {

const char* kFamily[] = {"pair", "wave", "ct", "ct2", "generic", "big", "notsupported", "invalid"};
constexpr int kCus = 256;
const int kOcc[] = {1, 2, 4};

struct Launch { uint32_t n_streams, max_blocks, max_channels, min_channels; };

rsmp::FftShape shape_of(const fft_cases::Plan& p) {
    rsmp::FftShape s{};
    s.fft_in = p.fft_in; s.fft_out = p.fft_out;
    s.n_stages_f = p.n_stages_f; s.n_stages_i = p.n_stages_i;
    for (int i = 0; i < 8; ++i) { s.radix_f[i] = p.radix_f[i]; s.radix_i[i] = p.radix_i[i]; }
    s.n_rc_f = p.n_rc_f; s.n_rc_i = p.n_rc_i;
    s.new_length = p.new_length; s.lds_complex = p.lds_complex;
    s.chirps = true;
    return s;
}

bool is_workgroup(rsmp::FftFamily f) {
    return f == rsmp::FftFamily::kCt || f == rsmp::FftFamily::kCt2 || f == rsmp::FftFamily::kGeneric || f == rsmp::FftFamily::kBig;
}

std::string text_of(const fft_cases::Plan& p, Launch l) {
    const rsmp::FftRequest rq{l.n_streams, l.max_blocks, l.max_channels, l.min_channels, 0, false, kCus};
    const rsmp::FftLaunch c = rsmp::fft_choose(shape_of(p), rq);
    char buf[256];
    int n = snprintf(buf, sizeof buf, " | %u %u %u %u %s", l.n_streams, l.max_blocks, l.max_channels, l.min_channels,
                     kFamily[static_cast<int>(c.family)]);
    std::string out(buf, static_cast<size_t>(n));
    if (c.family >= rsmp::FftFamily::kNotSupported) return out;
    if (!is_workgroup(c.family)) {
        n = snprintf(buf, sizeof buf, " pair=%d chm=%d occ=%d bits=%d block=%u lds=%zu", c.pair, c.chm, c.occ, c.bits, c.block, c.lds);
        return out.append(buf, static_cast<size_t>(n));
    }
    n = snprintf(buf, sizeof buf, " pair=%d block=%u gridz=%u lds=%zu grant=%d runs=", c.pair, c.block, c.grid[2], c.lds, c.grant_lds ? 1 : 0);
    out.append(buf, static_cast<size_t>(n));
    for (size_t i = 0; i < sizeof kOcc / sizeof kOcc[0]; ++i) {
        rsmp::FftLaunch run = c;
        rsmp::fft_choose_run(&run, rq, kOcc[i]);
        n = snprintf(buf, sizeof buf, "%s%u/%u", i ? "," : "", run.args[0], run.grid[0]);
        out.append(buf, static_cast<size_t>(n));
    }
    return out;
}

template <size_t N>
std::string row_of(const fft_cases::Plan& p, const char* kind, uint32_t channels, const Launch (&launches)[N]) {
    char buf[128];
    const int n = channels ? snprintf(buf, sizeof buf, "%u %u %u %u | %s %u", p.in_hz, p.out_hz, p.fft_in, p.fft_out, kind, channels)
                           : snprintf(buf, sizeof buf, "%u %u %u %u | %s", p.in_hz, p.out_hz, p.fft_in, p.fft_out, kind);
    std::string out(buf, static_cast<size_t>(n));
    for (const Launch& l : launches) out += text_of(p, l);
    return out;
}

}  // namespace

int main(int argc, char** argv) {
    const bool switched = argc > 1 && strcmp(argv[1], "switched") == 0;
    if (argc != 2 || (!switched && strcmp(argv[1], "default") != 0)) {
        fprintf(stderr, "usage: fft_workgroup_builds_dump default|switched\n");
        return 2;
    }
    const std::vector<fft_cases::Plan> all = fft_cases::plans();
    // (the process must be what its argument says: 96 -> 48 kHz, two channels, is the pair kernel's unless the switch is set)
    for (const fft_cases::Plan& p : all)
        if (p.in_hz == 96000 && p.out_hz == 48000) {
            const rsmp::FftRequest rq{3, 9, 2, 2, 0, false, kCus};
            if (is_workgroup(rsmp::fft_choose(shape_of(p), rq).family) != switched) {
                fprintf(stderr, "fft_workgroup_builds_dump %s: RSMP_FFT_WAVE is %s\n", argv[1], switched ? "not seen (RSMP_DEBUG=1?)" : "set");
                return 3;
            }
        }
    printf("{\n\"cus\": %d,\n\"rows\": [\n", kCus);
    const uint32_t n_channels = switched ? 2 : 3;
    for (size_t i = 0; i < all.size(); ++i) {
        const fft_cases::Plan& p = all[i];
        const bool last_plan = i + 1 == all.size();
        if (!switched) {
            const Launch mixed[] = {{3, 9, 3, 1}, {2, 5, 2, 1}};
            printf("  \"%s\",\n", row_of(p, "mixed", 0, mixed).c_str());
        }
        for (uint32_t c = 1; c <= n_channels; ++c) {
            const Launch uniform[] = {{3, 9, c, c}, {2, 5, c, c}};
            printf("  \"%s\",\n", row_of(p, "uniform", c, uniform).c_str());
        }
        for (uint32_t c = 1; c <= n_channels; ++c) {
            const Launch twin[] = {{1, 9, c, c}, {1, 4, c, c}, {1, 5, c, c}};
            printf("  \"%s\"%s\n", row_of(p, "twin", c, twin).c_str(), switched && last_plan && c == n_channels ? "" : ",");
        }
        if (!switched) {
            const Launch percall[] = {{1, 1, 1, 1}};
            printf("  \"%s\"%s\n", row_of(p, "percall", 1, percall).c_str(), last_plan ? "" : ",");
        }
    }
    printf("]\n}\n");
    return 0;
}
