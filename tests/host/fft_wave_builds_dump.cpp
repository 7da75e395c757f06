// fft_wave_builds_dump.cpp -- what fft_launch.cpp answers to every request of tests/test_fft_wave_builds_gpu.py, as JSON: the
// ordinary library, 256 CUs.  tests/test_host_programs.py builds it with ASan + UBSan, runs it and compares its output with
// tests/golden/fft_wave_builds.json, byte for byte; the same test reads from it which of the 144 builds of fft_wave.hip the GPU
// module's launches name.
//
//   "pairs":  per entry of WavePairs (fft_wave_plan.h), in its order: "index fft_in fft_out served occ_any occ_c2 wide in_pair_pairs"
//             -- the budget fft_wave.hip instantiates its three builds of the pair with, straight from the header.
//   "rows":   per ordered rate pair of fft_cases::plans() and per case (channels, bits of the PCM input or 0), one line
//             "in_hz out_hz fft_in fft_out | channels bits kind | launch | launch ...", a launch being
//             "n_streams max_blocks family pair=P chm=C occ=O block=B lds=L args=a,b,c,d" (or "... notsupported" / "... invalid").
//             kind: "short" where the case's first long launch (3 streams, 9 blocks) would go to the pair kernel -- the wave kernel
//             is reachable there only below four blocks --, else "long"; "refuse": the one request of
//             test_every_other_plan_refuses_pcm, then the f32 launch that follows it.
#include <cstdio>
#include <string>
#include <type_traits>

#include "fft_launch.h"
#include "fft_launch_cases.h"

namespace rsmp {
namespace {
#include "fft_wave_plan.h"

template <class P, class... Qs>
constexpr bool listed(PairList<Qs...>) { return (std::is_same_v<P, Qs> || ...); }

template <class... Ps>
void print_pairs(PairList<Ps...>) {
    const WaveBudget budgets[] = {wave_budget<typename Ps::Fwd, typename Ps::Inv>(false)...};
    const int sizes[][2] = {{Ps::Fwd::N, Ps::Inv::N}...};
    const bool in_pair[] = {listed<Ps>(PairPairs{})...};
    for (int i = 0; i < static_cast<int>(sizeof...(Ps)); ++i)
        printf("  \"%d %d %d %d %d %d %u %d\"%s\n", i, sizes[i][0], sizes[i][1], budgets[i].served ? 1 : 0, budgets[i].occ_any, budgets[i].occ_c2,
               budgets[i].wide, in_pair[i] ? 1 : 0, i + 1 < static_cast<int>(sizeof...(Ps)) ? "," : "");
}

}  // namespace
}  // namespace rsmp

namespace {

const char* kFamily[] = {"pair", "wave", "ct", "ct2", "generic", "big", "notsupported", "invalid"};
constexpr int kCus = 256;

struct Launch { uint32_t n_streams, max_blocks; };
const Launch kLong[] = {{3, 9}, {2, 5}};            // n_chunks [9, 4, 0], then [4, 5] on streams 0 and 2
const Launch kShort[] = {{3, 3}, {2, 3}, {1, 2}};   // [3, 2, 0], then [3, 3] on streams 0 and 2, then [2] on stream 0
const Launch kRefuse[] = {{1, 4}};
const uint32_t kCases[][2] = {{1, 0}, {3, 0}, {2, 0}, {2, 16}, {2, 24}, {2, 32}, {4, 0}, {6, 0}};   // (channels, PCM bits)

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

rsmp::FftLaunch choose(const fft_cases::Plan& p, uint32_t channels, uint32_t bits, Launch l) {
    const rsmp::FftRequest rq{l.n_streams, l.max_blocks, channels, channels, bits, false, kCus};
    return rsmp::fft_choose(shape_of(p), rq);
}

std::string text_of(const fft_cases::Plan& p, uint32_t channels, uint32_t bits, Launch l) {
    const rsmp::FftLaunch c = choose(p, channels, bits, l);
    char buf[256];
    int n = snprintf(buf, sizeof buf, " | %u %u %s", l.n_streams, l.max_blocks, kFamily[static_cast<int>(c.family)]);
    std::string out(buf, static_cast<size_t>(n));
    if (c.family >= rsmp::FftFamily::kNotSupported) return out;
    n = snprintf(buf, sizeof buf, " pair=%d chm=%d occ=%d block=%u lds=%zu args=", c.pair, c.chm, c.occ, c.block, c.lds);
    out.append(buf, static_cast<size_t>(n));
    for (int i = 0; i < c.n_args; ++i) out += (i ? "," : "") + std::to_string(c.args[i]);
    return out;
}

template <size_t N>
std::string row_of(const fft_cases::Plan& p, uint32_t channels, uint32_t bits, const char* kind, const Launch (&launches)[N]) {
    char buf[128];
    const int n = snprintf(buf, sizeof buf, "%u %u %u %u | %u %u %s", p.in_hz, p.out_hz, p.fft_in, p.fft_out, channels, bits, kind);
    std::string out(buf, static_cast<size_t>(n));
    for (const Launch& l : launches) out += text_of(p, channels, bits, l);
    return out;
}

}  // namespace

int main() {
    printf("{\n\"cus\": %d,\n\"pairs\": [\n", kCus);
    rsmp::print_pairs(rsmp::WavePairs{});
    printf("],\n\"rows\": [\n");
    const std::vector<fft_cases::Plan> all = fft_cases::plans();
    for (size_t i = 0; i < all.size(); ++i) {
        const fft_cases::Plan& p = all[i];
        for (const auto& c : kCases) {
            const bool is_short = choose(p, c[0], c[1], kLong[0]).family == rsmp::FftFamily::kPair;
            printf("  \"%s\",\n", (is_short ? row_of(p, c[0], c[1], "short", kShort) : row_of(p, c[0], c[1], "long", kLong)).c_str());
        }
        std::string refuse = row_of(p, 2, 16, "refuse", kRefuse);
        refuse += text_of(p, 2, 0, kRefuse[0]);
        printf("  \"%s\"%s\n", refuse.c_str(), i + 1 < all.size() ? "," : "");
    }
    printf("]\n}\n");
    return 0;
}
