// fir_class_table_dump.cpp -- writes the class-table images (fir_class_table.cpp: build_class_table) of a few geometries
// to stdout, for the real polyphase table of filter_design.cpp and three drifts: per image a text line
// "<name> <drift> <part> <bytes>\n" and then the bytes.  tests/test_host_programs.py builds it with ROCm's clang++ as plain
// host C++ (_Float16: the split kernel's two-plane cut) under ASan + UBSan and compares the SHA-256 of every part with
// tests/golden/fir_geometry.json, recorded from the commit before build_class_table left the kernel file
// (tests/golden/make_fir_geometry_fixture.py: this program linked against that commit's library).
// argv[1] = "headline": the headline geometry only (the run with RSMP_FIR_SPLIT_PLANES=3; switches are read once per process).
// argv[1] = "lockstep": the step kernel's tables instead (lockstep_class_geometry of 44.1 -> 48 kHz at 512 frames per step: the split
// layout, mfma = 3 in two planes, and the exact-f32 layout, mfma = 1 -- the A-operand order no periodic_geometry asks for), held
// against tests/golden/fir_lockstep.json (tests/golden/make_fir_lockstep_fixture.py).
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "filter_design.h"
#include "fir_lockstep_plan.h"
#include "fir_periodic_plan.h"

namespace {
struct Case {
    const char* name;
    uint32_t in_hz, out_hz, num, den;
    bool allow_matrix, allow_split;
};
int dump(const Case& c, bool lockstep = false) {
    const uint32_t taps = 128, channels = 2;
    const rsmp::FirDesign d = rsmp::fir_design(c.in_hz, c.out_hz, taps, rsmp::attenuation_beta(RSMP_ATTENUATION_DB90));
    const auto table = rsmp::get_or_create_fir_coeffs(d.cutoff, taps, RSMP_ATTENUATION_DB90);
    const rsmp::PeriodicGeometry g =
        lockstep ? rsmp::lockstep_class_geometry(rsmp::lockstep_geometry(c.num, c.den, static_cast<double>(c.in_hz) / c.out_hz, taps, channels, 512, c.allow_split))
                 : rsmp::periodic_geometry(c.num, c.den, taps, channels, c.allow_matrix, c.allow_split);
    if (!g.ok) {
        fprintf(stderr, "%s: no geometry\n", c.name);
        return 1;
    }
    static const double drifts[3] = {0.0, 2e-9, -2e-9};
    for (double drift : drifts) {
        const rsmp::HostClassTable t = rsmp::build_class_table(*table, g, drift);
        const struct { const char* part; const void* p; size_t bytes; } parts[3] = {
            {"coef", t.coef.data(), t.coef.size() * sizeof(float)},
            {"wrap_coef", t.wrap_coef.data(), t.wrap_coef.size() * sizeof(float)},
            {"meta", t.meta.data(), t.meta.size() * sizeof(rsmp::TileMeta)}};
        for (const auto& p : parts) {
            printf("%s:mfma%u:planes%u:wraps%d %g %s %zu\n", c.name, g.mfma, g.planes, g.inline_wraps ? 1 : 0, drift, p.part, p.bytes);
            if (fwrite(p.p, 1, p.bytes, stdout) != p.bytes) return 1;
        }
    }
    return 0;
}
}  // namespace

int main(int argc, char** argv) {
    static const Case cases[] = {
        {"headline", 44100, 48000, 147, 160, true, true},          // (= config 4's first pair)
        {"c4_48000_44100", 48000, 44100, 160, 147, true, true},
        {"c4_44100_96000", 44100, 96000, 147, 320, true, true},
        {"c4_96000_44100", 96000, 44100, 320, 147, true, true},
        {"c4_48000_96000", 48000, 96000, 1, 2, true, true},
        {"c4_96000_48000", 96000, 48000, 2, 1, true, true},
        {"f32_matrix", 44100, 48000, 147, 160, true, false},       // the exact-f32 matrix-core kernel
        {"vector_inline_wraps", 44100, 48000, 147, 160, false, true},
        {"vector_fixup_wraps", 96000, 48000, 2, 1, false, true}};  // den < 8: no wrap variant in the table
    if (argc > 1 && std::strcmp(argv[1], "lockstep") == 0) {
        static const Case step[] = {{"lockstep_split", 44100, 48000, 147, 160, true, true}, {"lockstep_exact", 44100, 48000, 147, 160, true, false}};
        for (const Case& c : step)
            if (dump(c, true)) return 1;
        return 0;
    }
    const bool headline_only = argc > 1 && std::strcmp(argv[1], "headline") == 0;
    for (const Case& c : cases) {
        if (dump(c)) return 1;
        if (headline_only) break;
    }
    return 0;
}
