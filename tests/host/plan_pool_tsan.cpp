// plan_pool_tsan.cpp -- PlanPool under ThreadSanitizer: a stand-alone program (tests/test_host_programs.py builds it with
// g++ -fsanitize=thread and runs it; it must exit 0 without a report).  Every item of a run is claimed exactly once, runs
// follow one another without a worker carrying one run's counter into the next, and two callers at once take turns.
#include <atomic>
#include <cstdio>
#include <thread>
#include <vector>

#include "plan_pool.h"

// One run of `items` items: every item bumps its own slot; afterwards every slot is exactly 1.
static bool one_run(rsmp::PlanPool& pool, size_t items) {
    std::vector<int> slots(items, 0);
    pool.run(items, [&](size_t m) { ++slots[m]; });
    for (size_t m = 0; m < items; ++m)
        if (slots[m] != 1) {
            fprintf(stderr, "run of %zu items: item %zu ran %d times\n", items, m, slots[m]);
            return false;
        }
    return true;
}

int main() {
    rsmp::PlanPool& pool = rsmp::plan_pool();
    const size_t counts[] = {0, 1, 2, 63, 64, 65, 1000};
    for (int k = 0; k < 200; ++k)
        if (!one_run(pool, counts[k % 7])) return 1;
    // two callers at once: run() admits one run at a time, each caller gets all of its own items and none of the other's
    std::atomic<int> bad{0};
    auto caller = [&](size_t items) {
        for (int k = 0; k < 20; ++k)
            if (!one_run(pool, items)) ++bad;
    };
    std::thread a(caller, 65), b(caller, 1000);
    a.join();
    b.join();
    if (bad.load() != 0) return 1;
    // a pool of its own goes away with its workers joined
    {
        rsmp::PlanPool local;
        if (!one_run(local, 64)) return 1;
    }
    printf("plan_pool_tsan: ok\n");
    return 0;
}
