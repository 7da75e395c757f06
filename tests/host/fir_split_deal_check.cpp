// fir_split_deal_check.cpp -- split_deal (fir_split_deal.cpp: how a shared launch of the split kernel deals its workgroups
// to its jobs) under ASan + UBSan: a stand-alone program, built and run by tests/test_host_programs.py.
//
// 400 seeded random job sets (1 .. 8 jobs of 1 .. 5000 items, one or two tile groups, 8 .. 256 workgroups).  With
// wgs = min(workgroups, all items) and `least` = one workgroup per one-group job + sixteen (wgs >= 16; else one) per
// two-group job, the least the rules allow:
//   * every share >= 1; a one-group job's share <= its items;
//   * wgs >= 16: a two-group job's share is a multiple of 16, and at most its items rounded to the nearest sixteen (16 at
//     least) -- a multiple of sixteen cannot stay below an item count that is none;  wgs < 16: at most its items;
//   * wgs >= least: the shares sum to at most wgs, and to exactly wgs while a one-group job still has room;
//     wgs < least: every job stands at its least, the sum is `least`.
// The two exceptions (a two-group share above its items, a sum above wgs) need a two-group job beside fewer than sixteen
// workgroups' worth of room; the program counts the sets in which shares <= items and sum <= wgs hold as they stand and
// prints the count.
#include <cstdint>
#include <cstdio>

#include "fir_periodic_plan.h"
#include "fir_split_consts.h"

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: %s (set %d)\n", __FILE__, __LINE__, #cond, set); return 1; } } while (0)

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t lo, uint32_t hi) {   // splitmix64, lo .. hi inclusive
    uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return lo + static_cast<uint32_t>(z % (hi - lo + 1));
}

int main() {
    int plain_sets = 0, set = 0;
    for (; set < 400; ++set) {
        rsmp::DealJob jobs[rsmp::kMaxSplitJobs];
        const uint32_t n = rnd(1, 8), cus = rnd(8, 256);
        uint64_t items_sum = 0;
        uint32_t n2 = 0;
        for (uint32_t b = 0; b < n; ++b) {
            jobs[b] = rsmp::DealJob{rnd(1, 5000), rnd(16, 320), rnd(1, 2)};
            items_sum += jobs[b].total_items;
            n2 += jobs[b].groups > 1;
        }
        const uint32_t wgs = static_cast<uint32_t>(items_sum < cus ? items_sum : cus);
        uint32_t share[rsmp::kMaxSplitJobs];
        const bool dealt = rsmp::split_deal(jobs, n, cus, share);
        CHECK(dealt == (wgs >= n));
        if (!dealt) continue;
        const bool sixteens = wgs >= 16;
        const uint32_t least = (n - n2) + (sixteens ? 16u : 1u) * n2;
        uint32_t sum = 0;
        bool room = false, plain = true;
        for (uint32_t b = 0; b < n; ++b) {
            sum += share[b];
            CHECK(share[b] >= 1);
            if (jobs[b].groups == 1 || !sixteens) CHECK(share[b] <= jobs[b].total_items);
            else {
                CHECK(share[b] % 16 == 0);
                const uint32_t near16 = (jobs[b].total_items + 8) / 16 * 16;
                CHECK(share[b] <= (near16 < 16 ? 16u : near16));
            }
            room = room || (jobs[b].groups == 1 && share[b] < jobs[b].total_items);
            plain = plain && share[b] <= jobs[b].total_items;
        }
        if (wgs >= least) {
            CHECK(sum <= wgs);
            if (room) CHECK(sum == wgs);
        } else {
            CHECK(sum == least);
        }
        plain_sets += plain && sum <= wgs;
    }
    // one job: all the workgroups its items can use; two equal jobs: half each
    {
        uint32_t share[2];
        const rsmp::DealJob one[1] = {{5000, 147, 1}}, few[1] = {{40, 147, 1}}, twins[2] = {{3000, 160, 1}, {3000, 160, 1}};
        CHECK(rsmp::split_deal(one, 1, 256, share) && share[0] == 256);
        CHECK(rsmp::split_deal(few, 1, 256, share) && share[0] == 40);
        CHECK(rsmp::split_deal(twins, 2, 256, share) && share[0] == 128 && share[1] == 128);
    }
    // BASELINE config 4 (six rate pairs, 256 calls of 512 frames per run) as the commit before the move dealt it on an MI355X, from
    // its "[rsmp] split multi launch: job ... workgroups=..." lines: 1024 streams and a 128-stream shard, on all 256 CUs and on
    // the 220 the lock-step batch leaves a repeated run of a small batch (36 reserved for the run planner).
    // Jobs: 44.1 -> 48, 44.1 -> 96, 48 -> 96 (two tile groups each), 96 -> 48, 48 -> 44.1, 96 -> 44.1 kHz.
    {
        const rsmp::DealJob big[6] = {{9747, 147, 1}, {19494, 147, 2}, {18020, 160, 2}, {4590, 320, 1}, {9063, 160, 1}, {4617, 320, 1}};
        const rsmp::DealJob shard[6] = {{1254, 147, 1}, {2394, 147, 2}, {2226, 160, 2}, {567, 320, 1}, {1166, 160, 1}, {567, 320, 1}};
        static const uint32_t all_cus[6] = {32, 64, 64, 32, 32, 32}, reserved[6] = {31, 48, 48, 31, 31, 31};
        uint32_t share[6];
        CHECK(rsmp::split_deal(big, 6, 256, share));
        for (int b = 0; b < 6; ++b) CHECK(share[b] == all_cus[b]);
        CHECK(rsmp::split_deal(shard, 6, 256, share));
        for (int b = 0; b < 6; ++b) CHECK(share[b] == all_cus[b]);
        CHECK(rsmp::split_deal(shard, 6, 256 - 36, share));
        for (int b = 0; b < 6; ++b) CHECK(share[b] == reserved[b]);
    }
    printf("fir_split_deal_check: ok (%d of 400 sets with every share <= its items and the sum <= the workgroups)\n", plain_sets);
    return 0;
}
