// fir_generic_builds_dump.cpp -- what generic_launch_choice (fir_geometry.cpp, fir_generic_plan.h) decides for the launches of
// tests/test_fir_generic_builds_gpu.py: reads requests `in_bits out_bits max_out min_channels max_channels min_taps max_taps ratio
// bulk_on` from stdin, one per line (ratio in C's %a or decimal form, as strtod reads it), and prints
//   <the request> | latency <reason> | tiled ch=<0|1|2> full=<0|1> tile=.. cap=.. | grid_x=.. lds=..
// as the "rows" of a JSON document.  For every tiled answer -- to these requests and to a sweep of 1 .. 16 channels x 16 / 32 / 64 /
// 128 taps x the ratios of the ten sample rates against the ten rates +- 1 Hz, either way round -- it checks the bound the tiled
// kernel's window clamp relies on, ceil(tile * ratio) + taps + 2 <= cap, that the tile is a multiple of 64 in 512 .. 4096 and that
// the LDS stays inside the opt-in; a violation exits with status 1.  tests/test_host_programs.py builds it as plain C++ under ASan +
// UBSan, feeds it the GPU module's requests and compares the output byte for byte with tests/golden/fir_generic_builds.json.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "fir_generic_plan.h"

namespace {

const char* const kReasons[] = {"none", "switched_off", "short", "no_tile", "format"};
int g_tiled = 0, g_checked = 0;

bool bound_holds(const rsmp::GenericLaunchRequest& rq, const rsmp::GenericLaunchChoice& c) {
    ++g_checked;
    if (c.kernel != rsmp::GenericKernel::kTiled) return c.tile == 0 && c.lds_bytes == 0 && c.window_cap_frames == 0;
    ++g_tiled;
    const double need = std::ceil(static_cast<double>(c.tile) * rq.max_ratio) + rq.max_taps + 2.0;
    const uint64_t window_bytes = static_cast<uint64_t>(c.window_cap_frames) * rq.max_channels * 4u;
    return need <= static_cast<double>(c.window_cap_frames) && c.tile % 64u == 0 && c.tile >= rsmp::kBulkTileMin && c.tile <= rsmp::kBulkTileMax &&
           window_bytes <= rsmp::kBulkWindowBytes && c.lds_bytes <= rsmp::kBulkLdsOptIn && c.grid_x == (rq.max_out + c.tile - 1) / c.tile &&
           c.tile <= 0xFFFFu && need <= 65535.0;   // (BulkMeta::rel and the sorted list are 16 bits wide)
}

std::string row_of(const rsmp::GenericLaunchRequest& rq, const char* ratio_text, int bulk_on, const rsmp::GenericLaunchChoice& c) {
    char buf[512];
    int n = snprintf(buf, sizeof buf, "%u %u %u %u %u %u %u %s %d | ", rq.format.in_bits, rq.format.out_bits, rq.max_out, rq.min_channels, rq.max_channels,
                     rq.min_taps, rq.max_taps, ratio_text, bulk_on);
    std::string out(buf, static_cast<size_t>(n));
    if (c.kernel == rsmp::GenericKernel::kTiled)
        n = snprintf(buf, sizeof buf, "tiled ch=%d full=%d tile=%u cap=%u | grid_x=%u lds=%u", c.ch_build, c.full ? 1 : 0, c.tile, c.window_cap_frames, c.grid_x, c.lds_bytes);
    else
        n = snprintf(buf, sizeof buf, "latency %s | grid_x=%u lds=%u", kReasons[static_cast<int>(c.reason)], c.grid_x, c.lds_bytes);
    out.append(buf, static_cast<size_t>(n));
    return out;
}

}  // namespace

int main() {
    std::vector<std::string> rows;
    char line[256];
    while (fgets(line, sizeof line, stdin)) {
        rsmp::GenericLaunchRequest rq;
        char ratio[64];
        int bulk_on = 1;
        if (sscanf(line, "%u %u %u %u %u %u %u %63s %d", &rq.format.in_bits, &rq.format.out_bits, &rq.max_out, &rq.min_channels, &rq.max_channels, &rq.min_taps,
                   &rq.max_taps, ratio, &bulk_on) != 9) {
            fprintf(stderr, "fir_generic_builds_dump: cannot read the request `%s`\n", line);
            return 2;
        }
        rq.max_ratio = strtod(ratio, nullptr);
        const rsmp::GenericLaunchChoice c = rsmp::generic_launch_choice(rq, bulk_on != 0);
        if (!bound_holds(rq, c)) {
            fprintf(stderr, "fir_generic_builds_dump: the window bound fails for the request `%s`\n", line);
            return 1;
        }
        rows.push_back(row_of(rq, ratio, bulk_on, c));
    }
    const int fixture_tiled = g_tiled;
    // ---- the sweep
    static const uint32_t rates[10] = {22050, 16000, 32000, 44100, 48000, 88200, 96000, 176400, 192000, 384000};
    static const uint32_t taps[4] = {16, 32, 64, 128};
    for (uint32_t ch = 1; ch <= 16; ++ch)
        for (uint32_t t : taps)
            for (uint32_t a : rates)
                for (uint32_t b : rates)
                    for (int k = 0; k < 4; ++k) {
                        rsmp::GenericLaunchRequest rq;
                        rq.max_out = 1u << 20;
                        rq.min_channels = rq.max_channels = ch;
                        rq.min_taps = rq.max_taps = t;
                        const double in_hz = k == 2 ? a + 1.0 : k == 3 ? a - 1.0 : a, out_hz = k == 0 ? b + 1.0 : k == 1 ? b - 1.0 : b;
                        rq.max_ratio = in_hz / out_hz;
                        const rsmp::GenericLaunchChoice c = rsmp::generic_launch_choice(rq, true);
                        if (c.kernel != rsmp::GenericKernel::kTiled && c.reason != rsmp::GenericLatencyReason::kNoTile) return 1;
                        if (!bound_holds(rq, c)) {
                            fprintf(stderr, "fir_generic_builds_dump: the window bound fails for %u channels, %u taps, %.0f -> %.0f Hz\n", ch, t, in_hz, out_hz);
                            return 1;
                        }
                    }
    printf("{\n\"rows\": [\n");
    for (size_t i = 0; i < rows.size(); ++i) printf("  \"%s\"%s\n", rows[i].c_str(), i + 1 < rows.size() ? "," : "");
    printf("],\n\"window_bound\": \"ceil(tile * ratio) + taps + 2 <= cap in all %d tiled answers above and in %d tiled of %d swept requests\"\n}\n", fixture_tiled,
           g_tiled - fixture_tiled, g_checked - static_cast<int>(rows.size()));
    return 0;
}
