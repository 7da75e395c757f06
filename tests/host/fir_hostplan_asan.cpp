// fir_hostplan_asan.cpp -- the host planner under AddressSanitizer + UBSan: a stand-alone program
// (tests/test_host_programs.py builds it with fir_hostplan.cpp, fir_plan.cpp, fir_geometry.cpp, filter_design.cpp and common.cpp,
// none of which includes a HIP header, and runs it).  The periodic_* rules the planner asks about are the library's own
// (fir_geometry.cpp): the rate pair and the length of the job pick the plan's kind.
#include <cstdio>
#include <memory>

#include "errors.h"
#include "fir_hostplan.h"
#include "fir_periodic_plan.h"

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); return 1; } } while (0)

// A 10-chunk bulk job of a fresh two-channel stream, planned twice: the second is the cached plan, with the same counts,
// and they are the counts of the loop run directly (what rsmp_fir_plan_bulk does).
static int plan_twice(uint32_t in_hz, uint32_t out_hz, size_t chunk_frames, bool periodic) {
    const size_t ch = 2, taps = 128, frames = 10 * chunk_frames;
    const rsmp::FirMirror fresh(in_hz, out_hz, taps);
    const rsmp::PlanRequest q{fresh, ch, taps, in_hz, out_hz, 0, frames * ch, 1u << 20, chunk_frames * ch};
    std::shared_ptr<rsmp::Plan> first, second;
    CHECK(rsmp::plan_job(q, &first) == RSMP_OK && first);
    CHECK(rsmp::plan_job(q, &second) == RSMP_OK && second.get() == first.get());   // (a cache hit: the very same plan)
    CHECK(first->periodic == periodic && first->segs.empty() == periodic);
    rsmp::FirMirror m(in_hz, out_hz, taps);
    const rsmp::BulkTotals t = rsmp::drive_bulk(m, frames, chunk_frames, 0, nullptr, nullptr, nullptr);
    CHECK(t.calls == 10 && first->calls.size() == 20 && !t.overflow);
    CHECK(first->accepted_frames == t.accepted && first->produced_frames == t.produced && first->consumed_frames == t.consumed);
    CHECK(first->planned.position() == m.position() && first->planned.available() == m.available());
    // no room for the output: refused with the cached plan as without it, and the error says so
    rsmp::PlanRequest tight = q;
    tight.out_cap = ch;
    std::shared_ptr<rsmp::Plan> none;
    CHECK(rsmp::plan_job(tight, &none) == RSMP_ERR_CAPACITY && !none);
    CHECK(rsmp::last_error_slot().find("bulk output needs") == 0);
    return 0;
}

int main() {
    // 44.1 -> 48 kHz has a periodic geometry: 5120 frames are too few outputs to be worth it (periodic_worthwhile), 20480 are
    // enough; 44100 / 48001 does not reduce to a period any kernel holds (periodic_supported)
    if (plan_twice(44100, 48000, 512, false) || plan_twice(44100, 48000, 2048, true) || plan_twice(44100, 48001, 512, false)) return 1;
    // more distinct requests than the cache holds: the oldest entries are overwritten in place
    for (size_t k = 1; k <= 80; ++k) {
        const rsmp::FirMirror fresh(48000, 44100, 128);
        const rsmp::PlanRequest q{fresh, 1, 128, 48000, 44100, 0, 100 * k, 1u << 20, 64};
        std::shared_ptr<rsmp::Plan> p;
        CHECK(rsmp::plan_job(q, &p) == RSMP_OK && p->accepted_frames == 100 * k);
    }
    printf("fir_hostplan_asan: ok\n");
    return 0;
}
