// fir_lockstep_paths_dump.cpp -- what lockstep_geometry (fir_lockstep_geometry.cpp) decides for the cases of
// tests/test_fir_lockstep_paths_gpu.py: reads requests `taps channels num den ratio step` from stdin, one per line (ratio in
// C's %a or decimal form, as strtod reads it), and prints every field of LockstepGeometry and of its class-table view in the
// row format of fir_lockstep_dump.cpp's print_geometry, as the "rows" of a JSON document.  allow_split is 1: a handle left on
// its default kernel.  tests/test_host_programs.py builds it as plain C++ under ASan + UBSan, feeds it the GPU module's CASES
// and compares the output byte for byte with tests/golden/fir_lockstep_paths.json.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "fir_lockstep_plan.h"

namespace {

std::string row_of(uint32_t taps, uint32_t ch, uint64_t num, uint64_t den, double ratio, uint32_t step) {
    const rsmp::LockstepGeometry g = rsmp::lockstep_geometry(num, den, ratio, taps, ch, step, true);
    const rsmp::PeriodicGeometry v = rsmp::lockstep_class_geometry(g);
    char buf[1024];
    int n = snprintf(buf, sizeof buf, "case %u %u 1 %llu/%llu %u | %d %u %u %u %u %u %u %u %u %u %u %u %u %u %u %u %u %u %u %d %u %u", taps, ch,
                     (unsigned long long)num, (unsigned long long)den, step, g.periodic ? 1 : 0, g.num, g.den, g.r, g.a, g.b, g.taps, g.row_len, g.n_tiles,
                     g.guard_frames, g.span_frames, g.region_frames, g.max_out, g.cols_per_stream, g.slots, g.wrap_words, g.wrap_cap, g.max_cols, g.lds_bytes,
                     g.split ? 1 : 0, g.rows, g.row_bytes);
    std::string out(buf, static_cast<size_t>(n));
    n = snprintf(buf, sizeof buf, " | %d %u %u %u %u %u %u %u %u %u %u %u %u %u %u %u %u %u %u %u %d", v.ok ? 1 : 0, v.a, v.b, v.den, v.taps, v.row_len, v.n_tiles,
                 v.cg, v.lp, v.pw, v.row_stride, v.waves, v.producers, v.images, v.mfma, v.planes, v.groups, v.rounds, v.n_units, v.lds_bytes,
                 v.inline_wraps ? 1 : 0);
    out.append(buf, static_cast<size_t>(n));
    return out;
}

}  // namespace

int main() {
    std::vector<std::string> rows;
    char line[256];
    while (fgets(line, sizeof line, stdin)) {
        unsigned taps = 0, ch = 0, step = 0;
        unsigned long long num = 0, den = 0;
        char ratio[64];
        if (sscanf(line, "%u %u %llu %llu %63s %u", &taps, &ch, &num, &den, ratio, &step) != 6) {
            fprintf(stderr, "fir_lockstep_paths_dump: cannot read the request `%s`\n", line);
            return 2;
        }
        rows.push_back(row_of(taps, ch, num, den, strtod(ratio, nullptr), step));
    }
    printf("{\n\"rows\": [\n");
    for (size_t i = 0; i < rows.size(); ++i) printf("  \"%s\"%s\n", rows[i].c_str(), i + 1 < rows.size() ? "," : "");
    printf("]\n}\n");
    return 0;
}
