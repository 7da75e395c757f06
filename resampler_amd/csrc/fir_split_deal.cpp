// fir_split_deal.cpp -- split_deal: how one launch of the split kernel shares its workgroups among several jobs (rate
// pairs).  A pure function.  Plain C++: includes no HIP header.
#include <algorithm>

#include "fir_periodic_plan.h"
#include "fir_split_consts.h"

namespace rsmp {

bool split_deal(const DealJob* jobs, uint32_t n, uint32_t cus, uint32_t* share) {
    // (items x frames of a period.  Round 6 tried the items' costs measured job by job instead -- 2.46 .. 4.39 us per item,
    // profiles/r05/channels_bench.txt, by which this deal gives the two-round jobs 30 % too many workgroups: config 4 got
    // 2 % SLOWER, 3.48 against 3.41 us per step in one lease; inside the shared launch the jobs do not cost what they cost alone)
    double weight[kMaxSplitJobs], weight_sum = 0.0;
    uint64_t items_sum = 0;
    for (uint32_t b = 0; b < n; ++b) {
        weight[b] = static_cast<double>(jobs[b].total_items) * jobs[b].a;
        weight_sum += weight[b];
        items_sum += jobs[b].total_items;
    }
    const uint32_t wgs = static_cast<uint32_t>(std::min<uint64_t>(cus, items_sum));
    if (wgs < n) return false;   // (fewer items than jobs cannot be: every job has at least one)
    // at least one workgroup per job, no more than it has items; the rest by weight (largest remainder)
    uint32_t given = 0;
    double frac[kMaxSplitJobs];
    for (uint32_t b = 0; b < n; ++b) {
        const double ideal = weight[b] / weight_sum * wgs;
        uint32_t w = static_cast<uint32_t>(ideal);
        w = std::max<uint32_t>(1u, std::min<uint32_t>(w, jobs[b].total_items));
        share[b] = w;
        frac[b] = ideal - w;
        given += w;
    }
    // A job with two tile groups: its item order makes workgroups w and w + n / 2 stage the same frames at about the
    // same time (tiles 0 .. 9 / 10 .. 19 of the same blocks), and the second of them finds the frames in L2 only if
    // both sit on one XCD -- workgroups go round the eight XCDs, so n / 2 must be a multiple of 8.  (Without this the
    // two such pairs of config 4 read their input twice from HBM: 0.37 GB of 2.35 per run.)
    bool two_groups[kMaxSplitJobs];
    for (uint32_t b = 0; b < n; ++b) {
        two_groups[b] = jobs[b].groups > 1;
        if (two_groups[b] && wgs >= 16) {
            const uint32_t r16 = std::max<uint32_t>(16u, (share[b] + 8u) / 16u * 16u);
            given = given - share[b] + r16;
            frac[b] += static_cast<double>(share[b]) - static_cast<double>(r16);
            share[b] = r16;
        }
    }
    auto step_of = [&](uint32_t b) { return two_groups[b] && wgs >= 16 ? 16u : 1u; };
    while (given > wgs) {   // (over: take from the job with the most to spare, a plain one if there is one)
        int big = -1;
        for (uint32_t b = 0; b < n; ++b)
            if (share[b] > step_of(b) && !(two_groups[b] && wgs >= 16) && (big < 0 || share[b] > share[big])) big = static_cast<int>(b);
        if (big < 0)
            for (uint32_t b = 0; b < n; ++b)
                if (share[b] > step_of(b) && (big < 0 || share[b] > share[big])) big = static_cast<int>(b);
        if (big < 0) break;
        const uint32_t st = std::min(step_of(big), share[big] - 1);
        share[big] -= st;
        frac[big] += st;
        given -= st;
    }
    while (given < wgs) {
        int best = -1;
        for (uint32_t b = 0; b < n; ++b)
            if (step_of(b) == 1u && share[b] < jobs[b].total_items && (best < 0 || frac[b] > frac[best])) best = static_cast<int>(b);
        if (best < 0) break;   // (only jobs that move in sixteens are left: the odd workgroups stay away)
        ++share[best];
        frac[best] -= 1.0;
        ++given;
    }
    return true;
}

}  // namespace rsmp
