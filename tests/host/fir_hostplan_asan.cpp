// fir_hostplan_asan.cpp -- the host planner under AddressSanitizer + UBSan: a stand-alone program
// (tests/test_host_programs.py builds it with fir_hostplan.cpp, fir_plan.cpp, filter_design.cpp and common.cpp, none of which
// includes a HIP header, and runs it).  The four periodic_* rules the planner asks about live beside the kernels
// (fir_periodic.hip); this program answers them itself instead of linking a kernel file: `g_periodic` picks the plan's kind.
#include <cstdio>
#include <memory>

#include "errors.h"
#include "fir_hostplan.h"
#include "fir_periodic_plan.h"

static bool g_periodic = false;
namespace rsmp {
bool periodic_supported(const FirMirror&, size_t, size_t, int) { return g_periodic; }
bool periodic_worthwhile(const FirMirror&, size_t, int) { return true; }
size_t periodic_wrap_words(uint64_t, uint32_t n_out, uint64_t den) { return (n_out / den + 1 + 31) / 32; }
void periodic_fill_wrap_bits(const std::vector<uint32_t>&, uint64_t, uint64_t, uint32_t* words, size_t n_words) {
    for (size_t w = 0; w < n_words; ++w) words[w] = 0;
}
}  // namespace rsmp

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); return 1; } } while (0)

// A 10-chunk bulk job of a fresh two-channel stream (another chunk size per kind of plan: the kind is no part of the cache's key,
// in the library it follows from the key), planned twice: the second is the cached plan, with the same counts,
// and they are the counts of the loop run directly (what rsmp_fir_plan_bulk does).
static int plan_twice(uint32_t in_hz, uint32_t out_hz, size_t chunk_frames, bool periodic) {
    g_periodic = periodic;
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
    if (plan_twice(44100, 48000, 512, false) || plan_twice(44100, 48000, 256, true) || plan_twice(44100, 48001, 512, false)) return 1;
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
