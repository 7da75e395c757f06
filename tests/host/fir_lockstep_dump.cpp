// fir_lockstep_dump.cpp -- prints what the host rules of the lock-step batch (fir_lockstep_geometry.cpp) decide, one row per
// input: argv[1] = "geometry" (lockstep_geometry and its class-table view over rate pairs, taps, channels, step sizes and
// allow_split), "layout" (the LDS byte offsets of config 4's six geometries), "groups" (config 4's classes cut into
// workgroups, and their order at three CU counts) or "shape" (the run planner's launches).  tests/test_host_programs.py
// builds it as plain C++ under ASan + UBSan, runs it once per setting of the debug switches (they are read once per
// process) and compares the rows with tests/golden/fir_lockstep.json, which was recorded from the commit before the rules
// left the kernel files (tests/golden/make_fir_lockstep_fixture.py: this program with -DRSMP_LS_PARENT linked against that
// commit's library for what it exported, the rest transcribed from its sources).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <numeric>
#include <vector>

#include "fir_lockstep_plan.h"

#ifdef RSMP_LS_PARENT
namespace rsmp {
uint32_t lockstep_replay_cus(size_t n_streams, uint32_t k);   // (the commit before the move exported these two rules of the plan shape)
}
#endif

namespace {

struct Pair { uint64_t num, den; double ratio; };
const Pair kC4[6] = {{147, 160, 44100.0 / 48000.0}, {160, 147, 48000.0 / 44100.0}, {147, 320, 44100.0 / 96000.0},
                     {320, 147, 96000.0 / 44100.0}, {1, 2, 48000.0 / 96000.0},     {2, 1, 96000.0 / 48000.0}};

void print_geometry(const char* key, const Pair& p, uint32_t taps, uint32_t ch, uint32_t step, bool allow_split) {
    const rsmp::LockstepGeometry g = rsmp::lockstep_geometry(p.num, p.den, p.ratio, taps, ch, step, allow_split);
    const rsmp::PeriodicGeometry v = rsmp::lockstep_class_geometry(g);
    printf("%s %u %u %d %llu/%llu %u | %d %u %u %u %u %u %u %u %u %u %u %u %u %u %u %u %u %u %u %d %u %u", key, taps, ch, allow_split ? 1 : 0,
           (unsigned long long)p.num, (unsigned long long)p.den, step, g.periodic ? 1 : 0, g.num, g.den, g.r, g.a, g.b, g.taps, g.row_len, g.n_tiles,
           g.guard_frames, g.span_frames, g.region_frames, g.max_out, g.cols_per_stream, g.slots, g.wrap_words, g.wrap_cap, g.max_cols, g.lds_bytes,
           g.split ? 1 : 0, g.rows, g.row_bytes);
    printf(" | %d %u %u %u %u %u %u %u %u %u %u %u %u %u %u %u %u %u %u %u %d\n", v.ok ? 1 : 0, v.a, v.b, v.den, v.taps, v.row_len, v.n_tiles, v.cg, v.lp,
           v.pw, v.row_stride, v.waves, v.producers, v.images, v.mfma, v.planes, v.groups, v.rounds, v.n_units, v.lds_bytes, v.inline_wraps ? 1 : 0);
}

int geometry() {
    static const uint32_t rates[10] = {22050, 16000, 32000, 44100, 48000, 88200, 96000, 176400, 192000, 384000};   // (fir_geometry_dump.cpp's)
    static const uint32_t taps_of[4] = {16, 32, 64, 128};
    static const uint32_t channels_of[8] = {1, 2, 3, 4, 6, 8, 16, 17};
    static const uint32_t steps_of[5] = {1, 64, 512, 1024, 4096};
    for (uint32_t taps : taps_of)
        for (uint32_t ch : channels_of)
            for (int allow = 0; allow < 2; ++allow)
                for (int i = 0; i < 10; ++i)
                    for (int o = 0; o < 10; ++o)
                        for (uint32_t step : steps_of) {
                            if (i == o) continue;
                            const uint32_t g0 = std::gcd(rates[i], rates[o]);
                            const Pair p{rates[i] / g0, rates[o] / g0, static_cast<double>(rates[i]) / static_cast<double>(rates[o])};
                            print_geometry("walk", p, taps, ch, step, allow != 0);
                        }
    // no rational form (the mirror reports num = den = 0), and one too long for class tables
    static const Pair odd[3] = {{0, 0, 3.14159265358979323846 / 3.0}, {0, 0, 1e-3}, {1048583, 1048576, 1048583.0 / 1048576.0}};
    for (const Pair& p : odd)
        for (uint32_t ch : {1u, 2u})
            for (int allow = 0; allow < 2; ++allow) print_geometry("odd", p, 128, ch, 512, allow != 0);
    return 0;
}

#ifndef RSMP_LS_PARENT
rsmp::LockstepGeometry c4_geometry(int p) { return rsmp::lockstep_geometry(kC4[p].num, kC4[p].den, kC4[p].ratio, 128, 2, 512, true); }

int layout() {
    for (int p = 0; p < 6; ++p) {
        const rsmp::LockstepGeometry g = c4_geometry(p);
        const rsmp::LsLayout l = rsmp::ls_layout(g.slots, g.max_cols, g.wrap_words, g.wrap_cap,
                                                 rsmp::ls_data_bytes(g.split, g.rows, g.row_bytes, g.slots, g.region_frames, 2));
        printf("%llu/%llu | %u %u %u %u %u %u %u %u | %u %u | %u\n", (unsigned long long)kC4[p].num, (unsigned long long)kC4[p].den, l.ptrs, l.colsrc,
               l.cols, l.segs, l.wbits, l.wlist, l.spans, l.total, rsmp::kLsPeakOff, rsmp::kLsPeak1Off, rsmp::lockstep_rec_stride(g.wrap_cap));
    }
    return 0;
}

// Config 4: stream i has pair i mod 6; the classes in the order of the pairs.  Table pointers that name their class, to see them travel.
int groups() {
    static float coef[6];
    static rsmp::TileMeta meta[6];
    for (size_t n : {size_t(1024), size_t(128)}) {
        std::vector<rsmp::LockstepGroup> cut;
        rsmp::LsCutMax most{0, 0};
        size_t first = 0;
        for (int p = 0; p < 6; ++p) {
            const size_t count = n / 6 + (static_cast<size_t>(p) < n % 6 ? 1 : 0);
            const rsmp::LsCutMax m = rsmp::lockstep_cut_groups(cut, c4_geometry(p), 2, first, first + count, &coef[p], &meta[p], static_cast<uint32_t>(p));
            if (m.lds_bytes > most.lds_bytes) most.lds_bytes = m.lds_bytes;
            if (m.rec_stride > most.rec_stride) most.rec_stride = m.rec_stride;
            first += count;
        }
        printf("cut %zu | %zu %u %u\n", n, cut.size(), most.lds_bytes, most.rec_stride);
        for (const rsmp::LockstepGroup& g : cut) {
            if (g.class_coef != &coef[g.pad0] || g.class_meta != &meta[g.pad0]) return 1;
            printf("group %zu | %u %u %u %u %u | %u %u %u %u %u %u %u %u %u %u %u %u %u %u %u %u %u %u %u\n", n, g.first, g.count, g.slots, g.lds_bytes, g.pad0,
                   g.channels, g.taps, g.periodic, g.num, g.den, g.a, g.b, g.row_len, g.n_tiles, g.guard_frames, g.span_frames, g.region_frames, g.max_out,
                   g.wrap_words, g.wrap_cap, g.max_cols, g.split, g.rows, g.row_bytes);
        }
        for (uint32_t cus : {256u, 64u, 32u}) {
            std::vector<rsmp::LockstepGroup> o = cut;
            rsmp::lockstep_order_groups(o, cus);
            printf("order %zu %u |", n, cus);
            for (const rsmp::LockstepGroup& g : o) printf(" %u", g.first);
            printf("\n");
        }
    }
    return 0;
}
#endif

int shape() {
    static const size_t streams_of[11] = {1, 3, 4, 5, 63, 64, 128, 255, 256, 257, 1024};
    static const uint32_t k_of[8] = {1, 63, 64, 65, 256, 1024, 1025, 4096};
    for (size_t n : streams_of)
        for (uint32_t k : k_of) {
#ifdef RSMP_LS_PARENT
            printf("%zu %u | %u %u\n", n, k, rsmp::lockstep_plan_pack(n), rsmp::lockstep_replay_cus(n, k));
#else
            const rsmp::LsPlanShape s = rsmp::lockstep_plan_shape(n, k);
            printf("%zu %u | %u %u | %u %u %u | %u | %u | %u %u\n", n, k, s.k1_blocks_per_stream, s.k1_grid, s.pack, s.k2_grid, s.k2_block, s.k3_waves,
                   s.parallel_chain, s.chain_cus, s.replay_cus);
#endif
        }
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    const char* what = argc > 1 ? argv[1] : "";
    if (!std::strcmp(what, "geometry")) return geometry();
    if (!std::strcmp(what, "shape")) return shape();
#ifndef RSMP_LS_PARENT
    if (!std::strcmp(what, "layout")) return layout();
    if (!std::strcmp(what, "groups")) return groups();
#endif
    fprintf(stderr, "usage: fir_lockstep_dump geometry | layout | groups | shape\n");
    return 2;
}
