// fir_hostplan.cpp -- see fir_hostplan.h.
#include "fir_hostplan.h"

#include <mutex>
#include <utility>

#include "errors.h"
#include "fir_periodic_plan.h"

namespace rsmp {

PlanKey make_key(const PlanRequest& q) {
    PlanKey k;
    std::memset(&k, 0, sizeof k);
    k.in_hz = q.in_hz;
    k.out_hz = q.out_hz;
    k.taps = q.taps;
    k.channels = q.channels;
    k.read_position = q.mirror.read_position();
    k.available = q.mirror.available();
    const double pos = q.mirror.position();
    std::memcpy(&k.position_bits, &pos, sizeof pos);
    k.abs_out = q.mirror.abs_out();
    k.abs_consumed = q.mirror.abs_consumed();
    k.in_len = q.in_len;
    k.out_cap_or_zero = q.chunk_len == 0 ? q.out_cap : 0;
    k.chunk_len = q.chunk_len;
    k.kernel_mode = q.kernel_mode;
    return k;
}

namespace {

// Process-wide plan cache.  A plan is a pure function of (configuration, stream state, amount of
// input, chunking) -- no sample values -- so, like an FFT plan, it is built once and reused: a
// service converting many files replays the same few plans over and over (every fresh stream
// of a given length starts in the same state).  Bounded; oldest entry evicted first.
struct PlanCache {
    std::mutex mu;
    std::vector<std::pair<PlanKey, std::shared_ptr<Plan>>> entries;
    size_t next_evict = 0;
    static constexpr size_t kMaxEntries = 64;

    std::shared_ptr<Plan> find(const PlanKey& k) {
        std::lock_guard<std::mutex> lock(mu);
        for (auto& e : entries) if (e.first == k) return e.second;
        return nullptr;
    }
    void insert(const PlanKey& k, const std::shared_ptr<Plan>& p) {
        std::lock_guard<std::mutex> lock(mu);
        if (entries.size() < kMaxEntries) { entries.emplace_back(k, p); return; }
        entries[next_evict] = std::make_pair(k, p);
        next_evict = (next_evict + 1) % kMaxEntries;
    }
};
PlanCache& plan_cache() {
    static PlanCache* c = new PlanCache;
    return *c;
}

// Replays the reference call sequence on a copy of the mirror (the caller commits it only on success).
int replay(const PlanRequest& q, bool with_segments, std::shared_ptr<Plan>* out) {
    const size_t ch = q.channels;
    if (q.in_len % ch != 0)
        return fail(RSMP_ERR_INVALID_INPUT_BUFFER_SIZE, "Input buffer size is invalid");
    auto plan = std::make_shared<Plan>(q.mirror);
    Plan& pl = *plan;
    pl.hist_frames = pl.planned.available();
    const bool want_periodic = !with_segments && periodic_supported(pl.planned, ch, q.taps, q.kernel_mode);
    std::vector<uint32_t>* wraps = want_periodic ? &pl.wraps : nullptr;
    std::vector<rsmp_fir_segment>* segs = want_periodic ? nullptr : &pl.segs;
    if (q.chunk_len == 0) {
        if (q.out_cap % ch != 0)
            return fail(RSMP_ERR_INVALID_OUTPUT_BUFFER_SIZE, "Output buffer size is invalid");
        const FirCallResult c = pl.planned.call(q.in_len / ch, q.out_cap / ch, 0, 0, segs, wraps);
        pl.accepted_frames = c.accepted;
        pl.produced_frames = c.produced;
        pl.consumed_frames = c.consumed;
        pl.calls.push_back(c.accepted);
        pl.calls.push_back(c.produced);
    } else {
        if (q.chunk_len % ch != 0)
            return fail(RSMP_ERR_INVALID_INPUT_BUFFER_SIZE,
                        "Input buffer size is invalid (chunk_len not a multiple of channels)");
        const BulkTotals t = drive_bulk(pl.planned, q.in_len / ch, q.chunk_len / ch, 0, segs, wraps, &pl.calls);
        if (t.overflow) return fail(RSMP_ERR_CAPACITY, "bulk launch exceeds 2^31 output frames");
        pl.accepted_frames = t.accepted;
        pl.produced_frames = t.produced;
        pl.consumed_frames = t.consumed;
        if (pl.produced_frames * ch > q.out_cap)
            return fail(RSMP_ERR_CAPACITY, "bulk output needs %zu values, room for %zu", pl.produced_frames * ch, q.out_cap);
    }
    if (want_periodic) {
        if (!pl.planned.periodic_ok() || !periodic_worthwhile(pl.planned, pl.produced_frames, q.kernel_mode))
            return replay(q, true, out);  // replay once more, keeping the position runs
        pl.periodic = true;
        // (one 64-bit division per wrapped output: on the planning worker, not on the thread that builds the launch)
        pl.wrap_bits.resize(periodic_wrap_words(q.mirror.abs_out(), static_cast<uint32_t>(pl.produced_frames), q.mirror.den()));
        periodic_fill_wrap_bits(pl.wraps, q.mirror.abs_out(), q.mirror.den(), pl.wrap_bits.data(), pl.wrap_bits.size());
    }
    *out = plan;
    return RSMP_OK;
}

}  // namespace

BulkTotals drive_bulk(FirMirror& m, size_t in_frames, size_t chunk_frames, size_t max_calls, std::vector<rsmp_fir_segment>* segs,
                      std::vector<uint32_t>* wraps, std::vector<size_t>* calls) {
    BulkTotals t;
    const size_t cap_frames = m.buffer_size_output_frames();
    while (t.accepted < in_frames && (max_calls == 0 || t.calls < max_calls)) {
        const size_t remaining = in_frames - t.accepted;
        if ((segs || wraps) && t.produced > 0x7FF00000ull - cap_frames) {
            t.overflow = true;
            break;
        }
        const FirCallResult c = m.call(remaining < chunk_frames ? remaining : chunk_frames, cap_frames, static_cast<int64_t>(t.consumed),
                                       static_cast<uint32_t>(t.produced), segs, wraps);
        if (calls) {
            calls->push_back(c.accepted);
            calls->push_back(c.produced);
        }
        t.produced += c.produced;
        t.consumed += c.consumed;
        t.accepted += c.accepted;
        ++t.calls;
        if (c.accepted == 0) break;
    }
    return t;
}

int plan_job(const PlanRequest& q, std::shared_ptr<Plan>* out) {
    if (q.chunk_len == 0) return replay(q, false, out);  // one call: cheaper than a lookup
    const PlanKey key = make_key(q);
    if (auto hit = plan_cache().find(key)) {
        if (hit->produced_frames * q.channels > q.out_cap)
            return fail(RSMP_ERR_CAPACITY, "bulk output needs %zu values, room for %zu", hit->produced_frames * q.channels, q.out_cap);
        *out = hit;
        return RSMP_OK;
    }
    const int rc = replay(q, false, out);
    if (rc == RSMP_OK) plan_cache().insert(key, *out);
    return rc;
}

}  // namespace rsmp
