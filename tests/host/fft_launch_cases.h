// fft_launch_cases.h -- the requests tests/golden/fft_launch.json pins, and the row each becomes.  Shared by
// fft_launch_dump.cpp (the launch rules of fft_launch.cpp) and by the recorder tests/golden/make_fft_launch_fixture.py builds
// around the kernel files of the commit before the move, so that both walk the same requests in the same order and print
// the same text.  Standard library + fft_plan.h only.
//
// Output: per group (exact build or not, max / min channels, pcm_bits) a line "# group <exact> <max> <min> <pcm>", then a
// row per request:
//   in_hz out_hz n_streams max_blocks cus occ | status kernel grid.x grid.y grid.z block lds grant args...
// occ: the occupancy answered to the workgroup kernels' query (1, 2, 4), "-" where the launch never asks.  status: ok,
// notsupported or invalid (nothing follows the latter two).  kernel: the ordinal of the build's first appearance in the
// process -- the recorder knows builds by their function pointer only.  grant: whether hipFuncSetAttribute was called.
// Then "# kernels" and a line "ordinal name" per build.
#pragma once

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <string>
#include <vector>

#include "fft_plan.h"

namespace fft_cases {

struct Plan {   // what fft_api.cpp puts into the FftPlanDev of a rate pair (every table pointer exists)
    uint32_t in_hz, out_hz;
    uint32_t fft_in, fft_out, n_stages_f, n_stages_i, radix_f[8], radix_i[8], n_rc_f, n_rc_i, new_length, lds_complex;
};
struct Request { uint32_t n_streams, max_blocks, max_channels, min_channels, pcm_bits; bool exact; int cus; };
struct Result {
    const char* status = "notsupported";
    std::string kernel;      // a name of the build, unique in the process
    bool asked_occupancy = false, grant = false;
    uint32_t grid[3] = {0, 0, 0}, block = 0;
    size_t lds = 0;
    std::vector<uint32_t> args;
};

inline std::vector<Plan> plans() {
    static const uint32_t kRates[] = {16000, 22050, 32000, 44100, 48000, 88200, 96000, 176400, 192000, 384000};   // RATES of tests/test_fft_gpu.py
    std::vector<Plan> out;
    for (uint32_t in_hz : kRates)
        for (uint32_t out_hz : kRates) {
            if (in_hz == out_hz) continue;
            const rsmp::FftResamplerPlan h = rsmp::make_fft_resampler_plan(in_hz, out_hz);
            if (!h.ok || h.forward.stages.size() > 8 || h.inverse.stages.size() > 8) { fprintf(stderr, "no plan for %u -> %u\n", in_hz, out_hz); exit(2); }
            Plan p{};
            p.in_hz = in_hz; p.out_hz = out_hz;
            p.fft_in = static_cast<uint32_t>(h.fft_in); p.fft_out = static_cast<uint32_t>(h.fft_out);
            p.n_stages_f = static_cast<uint32_t>(h.forward.stages.size()); p.n_stages_i = static_cast<uint32_t>(h.inverse.stages.size());
            for (size_t s = 0; s < h.forward.stages.size(); ++s) p.radix_f[s] = static_cast<uint32_t>(h.forward.stages[s]);
            for (size_t s = 0; s < h.inverse.stages.size(); ++s) p.radix_i[s] = static_cast<uint32_t>(h.inverse.stages[s]);
            p.n_rc_f = static_cast<uint32_t>(h.forward.rc_twiddles.size()); p.n_rc_i = static_cast<uint32_t>(h.inverse.rc_twiddles.size());
            p.new_length = static_cast<uint32_t>(h.new_length);
            p.lds_complex = static_cast<uint32_t>((h.fft_in > h.fft_out ? h.fft_in : h.fft_out) + 1);
            out.push_back(p);
        }
    return out;
}

// run(plan, request, occupancy) -> Result
template <class Run>
void walk(bool exact, Run run) {
    static const uint32_t kChannels[][3] = {{1, 1, 0}, {2, 2, 0}, {3, 3, 0}, {4, 4, 0}, {6, 6, 0}, {8, 8, 0}, {2, 1, 0},
                                            {2, 2, 16}, {2, 2, 24}, {2, 2, 32}, {1, 1, 16}, {1, 1, 24}, {1, 1, 32}};
    static const uint32_t kStreams[] = {1, 3, 64, 1024}, kBlocks[] = {1, 3, 4, 5, 16, 17, 100, 891, 4096};
    static const int kCus[] = {256, 64}, kOcc[] = {1, 2, 4};
    const std::vector<Plan> all = plans();
    std::map<std::string, int> ordinal;
    std::vector<std::string> names;
    for (const auto& ch : kChannels) {
        printf("# group %d %u %u %u\n", exact ? 1 : 0, ch[0], ch[1], ch[2]);
        for (const Plan& p : all)
            for (uint32_t n_streams : kStreams)
                for (uint32_t max_blocks : kBlocks)
                    for (int cus : kCus)
                        for (int occ : kOcc) {
                            const Request rq{n_streams, max_blocks, ch[0], ch[1], ch[2], exact, cus};
                            const Result r = run(p, rq, occ);
                            printf("%u %u %u %u %d %s | %s", p.in_hz, p.out_hz, n_streams, max_blocks, cus,
                                   r.asked_occupancy ? std::to_string(occ).c_str() : "-", r.status);
                            if (r.status[0] == 'o') {
                                auto it = ordinal.find(r.kernel);
                                if (it == ordinal.end()) {
                                    it = ordinal.emplace(r.kernel, static_cast<int>(names.size())).first;
                                    names.push_back(r.kernel);
                                }
                                printf(" %d %u %u %u %u %zu %d", it->second, r.grid[0], r.grid[1], r.grid[2], r.block, r.lds, r.grant ? 1 : 0);
                                for (uint32_t a : r.args) printf(" %u", a);
                            }
                            printf("\n");
                            if (!r.asked_occupancy) break;   // one row where the occupancy is never asked for
                        }
    }
    printf("# kernels\n");
    for (size_t i = 0; i < names.size(); ++i) printf("%zu %s\n", i, names[i].c_str());
}

}  // namespace fft_cases
