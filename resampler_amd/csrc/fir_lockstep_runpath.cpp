// fir_lockstep_runpath.cpp -- rsmp_fir_lockstep_run: k consecutive calls per stream in one go, planned on the device
// (fir_lockstep_run.hip), the next run planned ahead on a stream beside the caller's; and the bulk entries on top of it.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>

#include "fir_lockstep_batch.h"

using rsmp::FirMirrorState;
using rsmp::LockstepStream;

namespace rsmp {

namespace {

// The run path's debug switches, read once per process (each only under RSMP_DEBUG=1, common.h; tests/test_knobs_gpu.py
// runs every one of them in a process of its own).
struct LsKnobs {
    static int num(const char* name, int unset) { const char* e = rsmp::knob(name); return e ? atoi(e) : unset; }
    bool ahead = num("RSMP_LS_AHEAD", 1) != 0;               // 0: every run plans on the caller's stream
    int commit_on_plan = num("RSMP_LS_COMMIT_ON_PLAN", 1);   // 0: commits on the caller's stream; 2: on the plan stream for big batches too
    bool fuse_commit = num("RSMP_LS_FUSE_COMMIT", 1) != 0;   // 0: the commit is always a launch of its own
    bool stop_event = num("RSMP_LS_STOP_EVENT", 1) != 0;     // 0: events are recorded behind the launches, never completed by them
    bool items_ahead = num("RSMP_LS_ITEMS_AHEAD", 1) != 0;   // 0: the split kernel's item tables are built where they are used
    int reserve = num("RSMP_LS_RESERVE", -1);                // the number of CUs a small batch's bulk kernels leave the planner, 0 = none
    bool early_wait = num("RSMP_LS_EARLY_WAIT", 1) != 0;     // 0: the wait for the plan where it is taken over
    bool lazy_done = num("RSMP_LS_LAZY_DONE", 1) != 0;       // 0: a slot's "computed" event is recorded always
};
const LsKnobs& ls_knobs() { static const LsKnobs knobs; return knobs; }

// From this many streams on a batch's period is its bulk kernels'; below, its planner's (profiles/r05/c4_shard_sweep*.txt).
constexpr size_t kLsBigBatch = 256;

// What one run decides from the batch's size, its shape and the switches -- once, at the top of lockstep_run.
struct RunPolicy {
    // Is the NEXT run worth planning ahead?  When this run repeats the previous one's shape (the loop of a caller that
    // feeds run after run): then the run after this one is guessed to repeat it again, its input offset moving on as it
    // did between the last two.  Its planner goes to the plan stream below and runs beside this run's bulk kernels (its
    // kernels use no LDS: the split kernel's ring of images fills a CU's).  What that buys depends on the batch: a small one
    // (128 streams: the bulk kernels leave most of a run's time to the chain's latency) runs 1.5x faster, config 4's 1024
    // streams the same -- the stagers of the split kernel and the chain compete for the same issue slots, and each is slowed
    // by what the other takes.  LsKnobs::ahead off (debug): every run plans on the caller's stream.
    bool repeats = false;
    // K1 of the next run -- eighteen 64-bit divisions per call, a kernel of CODE -- goes in front of this run's bulk
    // kernels on the caller's own stream: alone it takes 10-18 us, beside the split kernel (whose sixteen differently
    // programmed waves fill the instruction cache two CUs share) 72 us for a shard of 128 streams and 0.5 ms for the
    // whole batch, in front of a chain that takes 100-200.  It writes the next run's predictions and bitmaps only; the
    // chain and the replay follow on the plan stream, beside the bulk kernels.
    // (A small batch -- a shard of 128 streams -- is bound by the planner's own chain, not by the bulk kernels: there the
    // chain should not start beside the big single-round launch, where it runs 1.5x slower, and K1 on the plan stream
    // delays it by just about that launch: 0.96 against 1.21 us per step; from 256 streams up K1 in front wins, 1024
    // streams 3.56 -> 3.38 us per step.  profiles/r05/c4_shard_sweep*.txt.)
    bool k1_in_front = false;
    // A small batch's period is its PLANNER's (predict + chain + replay, ~150 us for 128 streams x 256 calls, against
    // ~130 us of bulk kernels), and with the commit on the caller's stream the planner's loop crossed queues twice per
    // run -- plan stream -> caller's stream (commit) -> plan stream (the next plan): two event hand-overs of ~12 us in a
    // 185 us period (profiles/r06/c4_run_timeline_128_ahead1.txt).  So the commit goes to the PLAN stream, right behind
    // the plan it commits, the next plan right behind it, and the caller's stream waits for the commit -- unless this
    // call put something on the caller's stream that the next plan must see (new class tables: rare), or unless the buffers
    // changed under this run (rsmp_fir_lockstep_rebind_buffers: the new stream table and the zeroed append positions are
    // still queued on the caller's stream -- behind whatever the caller enqueued there before -- and a commit on the plan
    // stream could land in front of the zeroing, which would then wipe the positions after this run, while the next plan
    // read the old buffers' pointers).
    bool commit_on_plan_stream_allowed = false;
    // (the commit of a run planned ahead: K1 of the next run does it where that is launched on this stream, in front of the bulk
    // kernels -- a launch of 5 us less between two split launches; LsKnobs::fuse_commit off, debug: always a launch of its own)
    bool fuse_commit = false;
    // A big batch's planner is through long before its split launch (profiles/r06/c4_run_timeline_1024_ahead1.txt): the wait for
    // it goes behind the split launch, where the queue's processor handles the cross-queue dependency while the launch
    // drains -- in front of the next run's first kernel it was 11 us of idle chip between two split launches.
    // (LsKnobs::early_wait off, debug: the wait where the plan is taken over.)
    bool early_wait = false;
    // (the slot's "computed" event: a small batch's plan stream waits for it before it plans into the slot again; a big batch's K1 runs
    // on this very stream and needs none -- LsKnobs::lazy_done off, debug: recorded always)
    bool lazy_done = false;
    // A workgroup of the split kernel fills its CU (512 vector registers per SIMD lane, 136 KB of LDS): the planner of the
    // NEXT run, on the plan stream, does not run beside it but behind it, CU by CU as the launch drains -- for a small
    // batch, whose period is the planner's, that was the bulk launch's length added to every run (K1 "72 us beside the
    // split kernel, 10 alone").  A batch of fewer than kLsBigBatch streams planned ahead leaves the planner a wave's worth of CUs
    // per stream (one chain wave per stream, four SIMDs per CU); its bulk kernels lose an eighth of the chip they do not
    // need.  LsKnobs::reserve (debug): the number of CUs, 0 = none.
    uint32_t reserve_cus = 0;
    // The split kernel's item tables of the run planned ahead (one record per item: which frames, which outputs -- from the descriptors
    // the planner has just written) are built behind the plan on the plan stream: in front of the run's own kernels
    // the table launch was 6 us between two split launches.  (LsKnobs::items_ahead off, debug: built where they are used.)
    bool items_ahead = false;
    // (an event may be completed by a launch itself where that is on a stream of the caller's own -- not the legacy handle,
    // which an event must not carry, common.h)
    bool launch_completes_events = false;
};

RunPolicy run_policy(size_t n, uint32_t k, bool repeats, bool legacy_stream) {
    const LsKnobs& kn = ls_knobs();
    const bool big = n >= kLsBigBatch;
    RunPolicy p;
    p.repeats = repeats;
    p.k1_in_front = big;
    p.commit_on_plan_stream_allowed = kn.commit_on_plan != 0 && (!big || kn.commit_on_plan == 2);
    p.fuse_commit = kn.fuse_commit && big;
    p.early_wait = kn.early_wait && big;
    p.lazy_done = kn.lazy_done && big;
    // (the planner's packed workgroups take lockstep_plan_shape(n, k).chain_cus CUs -- 32 for 128 streams --, + 4 for its one-wave kernels; the
    // replay behind the chain a wave per chunk: a bulk launch of 64 streams x 4096 calls has 1024 of them, 64 CUs' worth, and with
    // 20 CUs left to it every fourth launch took 0.78 instead of 0.56 ms -- profiles/r06/bulk_distinct_reserve.txt)
    if (repeats && !big) {
        const rsmp::LsPlanShape shape = rsmp::lockstep_plan_shape(n, k);
        p.reserve_cus = kn.reserve >= 0 ? static_cast<uint32_t>(kn.reserve) : std::min<uint32_t>(64u, std::max(shape.chain_cus, shape.replay_cus) + 4u);
    }
    p.items_ahead = kn.items_ahead;
    p.launch_completes_events = kn.stop_event && !legacy_stream;
    return p;
}

// One call of lockstep_run: its arguments, its policy, and what its phases hand to each other.
struct RunCall {
    rsmp_fir_lockstep* ls;
    hipStream_t s;
    void* stream;   // as the caller gave it (rsmp_fir_lockstep_step takes it again)
    size_t n, in_frames, in_offset;
    uint32_t k;
    int append;
    const uint32_t* d_totals;   // non-null: a ragged run
    RunPolicy pol;
    RunKey key;
    int sl = 0;
    bool repeat = false;            // the next run is planned ahead
    bool commit_on_q = false;       // this run's states were committed on the plan stream
    bool plan_taken_over = false;
    bool commit_pending = false;    // ... are still to be committed on the caller's stream: by K1 of the next run, or a launch of its own
    rsmp::LsCommitArgs c{};
};

// What a run of k calls can need of one run group at most: outputs per stream, blocks of the bulk kernels, chunks and
// words of the non-finite marks, words of the wrapped outputs' bitmap.
struct RunGroupBounds { uint64_t n_out_max; uint32_t max_blocks, nf_chunks, nf_words, wrap_words; };
RunGroupBounds run_group_bounds(const RunGroup& g, uint32_t k) {
    RunGroupBounds b;
    b.n_out_max = static_cast<uint64_t>(k) * g.max_out_step;
    b.max_blocks = static_cast<uint32_t>((b.n_out_max / g.geo.b + 1) / g.geo.pw + 1);
    b.nf_chunks = static_cast<uint32_t>(b.n_out_max >> rsmp::kNfChunkShift) + 1;
    b.nf_words = 1 + static_cast<uint32_t>((g.count * static_cast<uint64_t>(b.nf_chunks) + 31) / 32);
    b.wrap_words = static_cast<uint32_t>(b.n_out_max / g.geo.den / 32 + 2);
    return b;
}

// The split kernel's jobs of a run of k calls over the descriptors `descs`: the rate pairs it takes, with their marks
// (`nf`, one per run group) or, for the item tables alone, without.
std::vector<rsmp::SplitJob> split_jobs(const rsmp_fir_lockstep* ls, const rsmp::FirStreamDesc* descs, uint32_t k, const rsmp::NfArgs* nf) {
    std::vector<rsmp::SplitJob> jobs;
    for (size_t gi = 0; gi < ls->run.groups.size(); ++gi) {
        const RunGroup& g = ls->run.groups[gi];
        if (g.geo.mfma != 3) continue;
        jobs.push_back(rsmp::SplitJob{descs + g.first, static_cast<uint32_t>(g.count), &g.geo, run_group_bounds(g, k).max_blocks,
                                      nf ? nf[gi] : rsmp::NfArgs{}});
    }
    return jobs;
}

// The plan stream of a caller's stream: one that runs BESIDE it.  HIP deals a handful of hardware queues to its streams in
// turn, and two streams on one queue run their kernels one after the other (the bench's torch stream and the batch's plan
// stream met on one: planned ahead, nothing overlapped).  Nothing tells which queue a stream has, so it is tried out, once per
// caller's stream, by a probe the DEVICE decides (launch_fir_lockstep_probe_wait: a wave on the caller's stream waits up to
// 1 ms for a word that a kernel on the candidate stores; behind it on one queue that kernel cannot start in time) and whose
// result the host looks at when its event has passed -- no host clock, no host wait: round 4's version timed the pair with
// the host's clock against 200 us around a hipStreamSynchronize, which a busy host fails for both candidates, and the batch
// then silently ran without plan-ahead.  Two candidates created one after the other sit on different queues, so at most one of
// them shares the caller's; a candidate that fails is tried once more after the other one (a host descheduled for a
// millisecond between the two launches reads like a shared queue).  Until a stream's answer is in, its runs plan on the
// stream itself.  (A stream of higher priority has a queue of its own for certain -- and starves the short kernels between
// the bulk launches: a run of 16 calls took 2.7x as long.)
int pick_plan_stream(PlanStreamPick& pk, hipStream_t s) {
    // (a caller with a stream per launch would grow the map by one entry per launch: its answers are dropped beyond 64
    // streams -- except the one whose probe is in flight -- and such a stream is probed again)
    if (pk.by_stream.size() >= 64 && pk.by_stream.find(s) == pk.by_stream.end())
        for (auto it = pk.by_stream.begin(); it != pk.by_stream.end();)
            it = it->first == pk.probe_owner ? std::next(it) : pk.by_stream.erase(it);
    PlanStreamPick::Pick& pp = pk.by_stream[s];
    if (!pp.decided) {
        if (pp.probing && pk.probe_owner == s) pk.take_probe_answer();
        if (!pp.decided && !pp.probing && pk.probe_owner == nullptr) {
            const uint32_t token = ++pk.probe_token ? pk.probe_token : ++pk.probe_token;
            *pk.h_probe.as<volatile uint32_t>() = 0u;
            RSMP_HIP_CHECK(rsmp::launch_fir_lockstep_probe_wait(pk.d_probe.as<uint32_t>(), token, 100000u, pk.h_probe.as<uint32_t>(), s));
            RSMP_HIP_CHECK(rsmp::launch_fir_lockstep_probe_set(pk.d_probe.as<uint32_t>(), token, pk.candidates[pp.cand]));
            RSMP_HIP_CHECK(rsmp::event_record(pk.probe_ev, s));
            pp.probing = true;
            pk.probe_owner = s;
            ++pk.probes;
        }
    }
    pk.stream = pp.decided && pp.pick >= 0 ? static_cast<hipStream_t>(pk.candidates[pp.pick]) : nullptr;
    return RSMP_OK;
}

// The bulk kernels' side of a batch: one geometry + class table per rate pair, the constant half of every
// stream's descriptor, the planner's waves.  Done once, at the first run.
int prepare_run(rsmp_fir_lockstep* ls) {
    RunSlots& run = ls->run;
    if (run.state != 0) return RSMP_OK;
    const size_t n = ls->rs.size();
    std::vector<rsmp::FirStreamDesc> descs(n);
    std::vector<rsmp::LsRunStream> rstreams(n);
    std::memset(descs.data(), 0, n * sizeof(rsmp::FirStreamDesc));
    run.groups.clear();
    for (size_t c = 0; c < ls->drift.classes.size(); ++c) {   // one group of streams per drift class (key + drift: rsmp_fir_lockstep_new)
        DriftClass& cl = ls->drift.classes[c];
        const size_t k = cl.first, e = cl.first + cl.count;
        const rsmp_fir* r0 = cl.r0;
        const int mode = r0->kernel_mode;
        rsmp::PeriodicGeometry geo;
        if (mode != RSMP_FIR_KERNEL_GENERIC && r0->mirror.periodic_ok())
            geo = rsmp::periodic_geometry(r0->mirror.num(), r0->mirror.den(), static_cast<uint32_t>(r0->taps),
                                          static_cast<uint32_t>(r0->channels), mode != RSMP_FIR_KERNEL_PERIODIC_VECTOR,
                                          mode != RSMP_FIR_KERNEL_PERIODIC_F32);
        const uint64_t den = r0->mirror.den();
        // (a geometry without the wrap variant in the kernel wants a list of wrapped outputs, which the device
        // planner does not keep -- unless the ratio is exact in f64 and no output ever wraps)
        if (!geo.ok || (!geo.inline_wraps && (den & (den - 1)) != 0)) {
            // runs are loops of steps; their per-call counts are gathered with the streams' caller indices
            for (auto& x : ls->drift.classes) x.has_run = false;
            for (size_t i = 0; i < n; ++i) rstreams[i].caller = ls->order[i];
            if (run.d_rs.reserve(n * sizeof(rsmp::LsRunStream)) != hipSuccess)
                return rsmp::fail(RSMP_ERR_HIP, "lock-step run: cannot allocate device state");
            RSMP_HIP_CHECK(hipMemcpy(run.d_rs.get(), rstreams.data(), n * sizeof(rsmp::LsRunStream), hipMemcpyHostToDevice));
            run.state = -1;
            return RSMP_OK;
        }
        rsmp::ClassTable ct;
        if (rsmp::class_table_for(ls->device, *r0->table, geo, cl.table_drift, &ct) != RSMP_OK) return RSMP_ERR_HIP;
        cl.has_run = true;
        cl.run_geo = geo;
        cl.run_table = ct;
        if (!cl.run_next) cl.run_next = ls->drift.refresher->add_table(geo, r0->table);
        if (!cl.run_next) return rsmp::fail(RSMP_ERR_HIP, "lock-step run: cannot create an event");
        RunGroup g;
        g.geo = geo;
        g.first = k;
        g.count = e - k;
        g.max_out_step = static_cast<uint32_t>(std::ceil(static_cast<double>(ls->step_frames + 8) / r0->mirror.ratio())) + 2;
        run.groups.push_back(g);
        for (size_t i = k; i < e; ++i) {
            const rsmp_fir* r = ls->rs[ls->order[i]];
            rsmp::FirStreamDesc& d = descs[i];
            d.coeffs = r->d_coeffs;
            d.class_coef = ct.d_coef;
            d.class_wrap_coef = ct.d_wrap_coef;
            d.class_meta = ct.d_meta;
            d.channels = static_cast<uint32_t>(r->channels);
            d.taps = static_cast<uint32_t>(r->taps);
            d.num = static_cast<uint32_t>(r->mirror.num());
            d.den = static_cast<uint32_t>(den);
            d.drift = cl.table_drift;
            rstreams[i].wrap_unit = geo.mfma == 3 ? geo.b : geo.den;
            rstreams[i].den = static_cast<uint32_t>(den);
            rstreams[i].channels = static_cast<uint32_t>(r->channels);
            rstreams[i].caller = ls->order[i];
            rstreams[i].class_coef = ct.d_coef;          // (the planner writes these into the run's descriptor: they follow the drift)
            rstreams[i].class_wrap_coef = ct.d_wrap_coef;
            rstreams[i].class_meta = ct.d_meta;
            rstreams[i].drift = cl.table_drift;
        }
    }
    run.h_rs = rstreams;
    // (a failure below leaves what was created to the batch's holders: the next attempt, or the batch's end, finds it there)
    if (run.slot[0].descs.reserve(n * sizeof(rsmp::FirStreamDesc)) != hipSuccess ||
        run.slot[1].descs.reserve(n * sizeof(rsmp::FirStreamDesc)) != hipSuccess ||
        run.sp_states.reserve(n * sizeof(FirMirrorState)) != hipSuccess ||
        run.sp_cursor.reserve(n * sizeof(uint64_t)) != hipSuccess ||
        run.sp_last.reserve(2 * n * sizeof(uint64_t)) != hipSuccess ||
        run.sp_status.reserve(n * sizeof(uint32_t)) != hipSuccess ||
        ls->pick.candidates[0].create(hipStreamNonBlocking) != hipSuccess ||
        ls->pick.candidates[1].create(hipStreamNonBlocking) != hipSuccess ||
        ls->plan.ev_ready.create(hipEventDisableTiming) != hipSuccess ||
        ls->plan.done.create(hipEventDisableTiming) != hipSuccess ||
        ls->plan.ev_commit.create(hipEventDisableTiming) != hipSuccess ||
        run.slot[0].compute_done.create(hipEventDisableTiming) != hipSuccess ||
        run.slot[1].compute_done.create(hipEventDisableTiming) != hipSuccess ||
        run.d_rs.reserve(n * sizeof(rsmp::LsRunStream)) != hipSuccess ||
        run.d_states0.reserve(n * sizeof(FirMirrorState)) != hipSuccess ||
        run.d_work.reserve(std::max<size_t>(64, run.groups.size()) * sizeof(unsigned long long)) != hipSuccess)
        return rsmp::fail(RSMP_ERR_HIP, "lock-step run: cannot allocate device state");
    for (auto& sl : run.slot)
        RSMP_HIP_CHECK(hipMemcpy(sl.descs.get(), descs.data(), n * sizeof(rsmp::FirStreamDesc), hipMemcpyHostToDevice));
    RSMP_HIP_CHECK(hipMemcpy(run.d_rs.get(), rstreams.data(), n * sizeof(rsmp::LsRunStream), hipMemcpyHostToDevice));
    // (one work counter per run group: a batch of many drift classes on a non-split geometry has more than 64)
    RSMP_HIP_CHECK(hipMemset(run.d_work.get(), 0, std::max<size_t>(64, run.groups.size()) * sizeof(unsigned long long)));
    run.state = 1;
    return RSMP_OK;
}

// workspaces that grow with k: the per-call counts and records, the predictions, the bitmaps of wrapped outputs.
// (A reallocation waits for both streams: kernels planned ahead may still use the old buffers.)
int grow_run_workspaces(RunCall& rc, uint32_t wrap_words, bool loop_of_steps) {
    rsmp_fir_lockstep* ls = rc.ls;
    RunSlots& run = ls->run;
    const size_t n = rc.n;
    if (!(rc.k > run.k || (!loop_of_steps && wrap_words > run.wrap_words))) return RSMP_OK;
    RSMP_HIP_CHECK(hipStreamSynchronize(rc.s));
    if (int e = drop_plan_ahead(ls, nullptr)) return e;
    const uint32_t kk = std::max(rc.k, run.k), ww = std::max(wrap_words, run.wrap_words);
    for (auto& sl : run.slot)
        if (sl.counts.reserve(2 * n * static_cast<size_t>(kk) * sizeof(uint32_t)) != hipSuccess ||
            sl.recs.reserve(n * static_cast<size_t>(kk) * 24) != hipSuccess ||
            sl.bits.reserve(n * static_cast<size_t>(ww) * sizeof(uint32_t)) != hipSuccess)
            return rsmp::fail(RSMP_ERR_HIP, "lock-step run: cannot allocate the plan of %u calls", rc.k);
    if (run.d_preds.reserve(n * static_cast<size_t>(kk) * sizeof(rsmp::MirrorPred)) != hipSuccess)
        return rsmp::fail(RSMP_ERR_HIP, "lock-step run: cannot allocate the plan of %u calls", rc.k);
    run.k = kk;
    run.wrap_words = ww;
    return RSMP_OK;
}

// The fallback: a run as a loop of k steps, each with a small kernel behind it that keeps its counts.
int run_as_steps(RunCall& rc) {
    rsmp_fir_lockstep* ls = rc.ls;
    hipStream_t s = rc.s;
    const size_t n = rc.n, in_frames = rc.in_frames;
    const bool ragged = rc.d_totals != nullptr;
    RSMP_HIP_CHECK(ls->order_behind_last(s));   // (in front of the memset below)
    if (int e = drop_plan_ahead(ls, s)) return e;
    ls->plan.prev.valid = false;
    if (!rc.append && !ragged)   // (the device planner starts a run at the front itself: no launch for it; ragged: the first step's offer kernel)
        RSMP_HIP_CHECK(hipMemsetAsync(ls->d_cursor.get(), 0, n * sizeof(uint64_t), s));
    const int sl = ls->run.next_slot;
    for (uint32_t i = 0; i < rc.k; ++i) {
        const size_t offset = rc.in_offset + static_cast<size_t>(i) * in_frames;
        uint32_t* row = ls->run.slot[sl].counts.as<uint32_t>() + 2 * n * static_cast<size_t>(i);
        const rsmp::LsRunStream* rs = ls->run.d_rs.as<rsmp::LsRunStream>();
        const uint32_t nn = static_cast<uint32_t>(n), chunk = static_cast<uint32_t>(in_frames);
        if (ragged) {
            // step i offers every stream what is left of its buffer, at most in_frames frames.  A stream that is through takes an
            // EMPTY call, which the driver loop never makes: state-neutral behind a call that was not stopped by its output room
            // (src/resampler_fir.rs:542-602: the loop breaks at once, nothing is retired), and kept out of the stream's counts.
            RaggedTotals& t = ls->totals;
            RSMP_HIP_CHECK(rsmp::launch_fir_lockstep_ragged_offer(rc.d_totals, rs, t.d_offer.as<uint32_t>(), ls->d_counts.as<uint64_t>(),
                                                                  t.d_keep.as<uint64_t>(),
                                                                  i == 0 && !rc.append ? ls->d_cursor.as<uint64_t>() : nullptr, i, chunk, nn, s));
            if (int e = rsmp_fir_lockstep_step(ls, in_frames, offset, t.d_offer.as<uint32_t>(), 1, rc.stream)) return e;
            RSMP_HIP_CHECK(rsmp::launch_fir_lockstep_ragged_gather(rc.d_totals, rs, ls->d_counts.as<uint64_t>(), t.d_keep.as<uint64_t>(), row, i,
                                                                   chunk, nn, s));
        } else {
            if (int e = rsmp_fir_lockstep_step(ls, in_frames, offset, nullptr, 1, rc.stream)) return e;
            RSMP_HIP_CHECK(rsmp::launch_fir_lockstep_gather_counts(ls->d_counts.as<uint64_t>(), rs, row, nn, s));
        }
    }
    ls->run.last_slot = sl;
    ls->run.counts_k = rc.k;
    ls->run.planned = false;
    return RSMP_OK;
}

bool same_key(const RunKey& x, const RunKey& y) {
    return x.valid && y.valid && x.k == y.k && x.in_frames == y.in_frames && x.append == y.append && x.parity == y.parity &&
           x.in_offset == y.in_offset && x.seq == y.seq && x.slot == y.slot;
}

// The planner's arguments for the run `kk`: into the batch's own states, or (`scratch`: planned ahead) into the copies.
rsmp::LsRunArgs plan_args(const RunCall& rc, const RunKey& kk, bool scratch) {
    rsmp_fir_lockstep* ls = rc.ls;
    RunSlots& run = ls->run;
    rsmp::LsRunArgs a;
    RunSlot& t = run.slot[kk.slot];
    a.streams = ls->d_streams.as<LockstepStream>();
    a.rs = run.d_rs.as<rsmp::LsRunStream>();
    a.states_in = ls->d_states.as<FirMirrorState>();
    a.states_out = scratch ? run.sp_states.as<FirMirrorState>() : ls->d_states.as<FirMirrorState>();
    a.states_before = run.d_states0.as<FirMirrorState>();
    a.preds = run.d_preds.as<rsmp::MirrorPred>();
    a.call_recs = t.recs.get();
    a.cursor_in = ls->d_cursor.as<uint64_t>();
    a.cursor_out = scratch ? run.sp_cursor.as<uint64_t>() : ls->d_cursor.as<uint64_t>();
    a.descs = t.descs.as<rsmp::FirStreamDesc>();
    a.wrap_bits = t.bits.as<uint32_t>();
    a.counts = t.counts.as<uint32_t>();
    a.last_counts = scratch ? run.sp_last.as<uint64_t>() : ls->d_counts.as<uint64_t>();
    a.status = scratch ? run.sp_status.as<uint32_t>() : ls->d_status.as<uint32_t>();
    a.zero_status = scratch ? run.sp_status.as<uint32_t>() : nullptr;
    a.in_offset = kk.in_offset;
    a.n_streams = static_cast<uint32_t>(rc.n);
    a.k = kk.k;
    a.in_frames = kk.in_frames;
    a.wrap_words = run.wrap_words;
    a.append = kk.append;
    a.hist_parity = kk.parity;
    a.totals = scratch ? nullptr : rc.d_totals;   // (a ragged run is planned here and now; what is planned ahead is a uniform run)
    return a;
}

// This very run was planned ahead while the previous run computed: wait for it (an event, no host block) and take its results
// over (a big batch's caller stream has waited already, behind the previous run's split launch -- RunPolicy::early_wait).
// Where the commit goes: RunPolicy::commit_on_plan_stream_allowed.
int take_over_plan(RunCall& rc) {
    rsmp_fir_lockstep* ls = rc.ls;
    PlanAhead& plan = ls->plan;
    hipStream_t s = rc.s;
    if (!(plan.waited && plan.waited_on == s)) RSMP_HIP_CHECK(rsmp::stream_wait_event(s, plan.done));
    plan.waited = false;
    plan.inflight = false;
    rc.plan_taken_over = true;
    ++plan.hits;
    const bool rebased = plan.rebased;
    if (plan.rebased) {   // (planned when the batch was bound to other buffers: the two pointers of every descriptor again)
        RSMP_HIP_CHECK(rsmp::launch_fir_lockstep_rebase(ls->run.slot[rc.sl].descs.as<rsmp::FirStreamDesc>(), ls->d_streams.as<LockstepStream>(),
                                                        ls->run.d_rs.as<rsmp::LsRunStream>(), rc.key.in_offset, static_cast<uint32_t>(rc.n), s));
        plan.rebased = false;
    }
    // (new tables: from the next plan on; this run was planned with the old ones, whose images nobody overwrites
    // before this run's kernels are through -- TableRefresher's guard event.  Behind the wait: the planner read
    // the stream table this may patch.)
    const uint64_t table_ops0 = ls->drift.table_ops;
    if (int e = poll_drift(ls, s)) return e;
    if (int e = flush_tables(ls, s)) return e;
    rc.commit_on_q = rc.pol.commit_on_plan_stream_allowed && plan.q != nullptr && ls->drift.table_ops == table_ops0 && !rebased;
    hipStream_t cs = rc.commit_on_q ? plan.q : s;
    if (rc.commit_on_q && ls->drift.inflight)   // (a reading of the states on the caller's stream: in front of what changes them)
        RSMP_HIP_CHECK(rsmp::stream_wait_event(cs, ls->drift.ev));
    rsmp::LsCommitArgs& c = rc.c;
    c.states = ls->d_states.as<FirMirrorState>();
    c.sp_states = ls->run.sp_states.as<FirMirrorState>();
    c.cursor = ls->d_cursor.as<uint64_t>();
    c.sp_cursor = ls->run.sp_cursor.as<uint64_t>();
    c.last_counts = ls->d_counts.as<uint64_t>();
    c.sp_last_counts = ls->run.sp_last.as<uint64_t>();
    c.status = ls->d_status.as<uint32_t>();
    c.sp_status = ls->run.sp_status.as<uint32_t>();
    c.n_streams = static_cast<uint32_t>(rc.n);
    if (!rc.commit_on_q) {
        rc.commit_pending = true;
        return RSMP_OK;
    }
    RSMP_HIP_CHECK(rsmp::launch_fir_lockstep_commit(c, cs));
    RSMP_HIP_CHECK(rsmp::event_record(plan.ev_commit, cs));
    RSMP_HIP_CHECK(rsmp::stream_wait_event(s, plan.ev_commit));
    ++plan.commits_on_plan_stream;
    return RSMP_OK;
}

// The plan: taken from the plan stream if this very run was planned ahead there, made here otherwise.
int obtain_plan(RunCall& rc) {
    rsmp_fir_lockstep* ls = rc.ls;
    if (!rc.d_totals && same_key(ls->plan.ahead, rc.key)) {
        if (int e = take_over_plan(rc)) return e;
    } else {
        ls->plan.waited = false;
        ls->plan.rebased = false;   // (planned here, behind the new table)
        if (ls->plan.ahead.valid) ++ls->plan.misses;
        if (int e = drop_plan_ahead(ls, rc.s)) return e;   // (whatever the plan stream still does: finished before this stream goes on)
        if (int e = poll_drift(ls, rc.s)) return e;
        if (int e = flush_tables(ls, rc.s)) return e;
        RSMP_HIP_CHECK(rsmp::launch_fir_lockstep_plan(plan_args(rc, rc.key, false), rc.s));
    }
    ls->plan.ahead.valid = false;
    return RSMP_OK;
}

// The item tables of the run `nx` planned ahead, behind its plan on the plan stream `q` (RunPolicy::items_ahead).
int build_items_ahead(RunCall& rc, const RunKey& nx, hipStream_t q) {
    RunSlot& ns = rc.ls->run.slot[nx.slot];
    const std::vector<rsmp::SplitJob> jobs = split_jobs(rc.ls, ns.descs.as<rsmp::FirStreamDesc>(), rc.k, nullptr);
    const size_t bytes = rsmp::fir_split_multi_item_words(jobs.data(), jobs.size()) * sizeof(uint32_t);
    bool room = bytes <= ns.items.capacity();
    if (!room && bytes != 0) {   // (once per shape of run: nothing in flight reads a table that is about to be built for the first time)
        RSMP_HIP_CHECK(hipStreamSynchronize(q));
        RSMP_HIP_CHECK(hipStreamSynchronize(rc.s));
        RSMP_HIP_CHECK(ns.items.reserve(bytes + bytes / 2));
        room = true;
    }
    if (room && bytes != 0) {
        RSMP_HIP_CHECK(rsmp::launch_fir_split_multi(jobs.data(), jobs.size(), q, 0, ns.items.as<uint32_t>(), q));
        ns.items_seq = nx.seq;
        ns.items_ops = rc.ls->drift.table_ops;
        ns.items_valid = true;
    }
    return RSMP_OK;
}

// The next run is planned ahead (before this run's bulk kernels are launched: the planner starts as soon as the states
// are there): K1 where RunPolicy::k1_in_front says, the chain and the replay on the plan stream.
int plan_next_ahead(RunCall& rc) {
    rsmp_fir_lockstep* ls = rc.ls;
    PlanAhead& plan = ls->plan;
    hipStream_t s = rc.s;
    RunKey nx = rc.key;
    nx.in_offset = rc.key.in_offset + (rc.key.in_offset - plan.prev.in_offset);
    nx.parity = ls->hist_parity ^ 1u;
    nx.seq = ls->run.seq + 1;
    nx.slot = rc.sl ^ 1;
    hipStream_t q = ls->pick.stream;
    const bool k1_in_front = rc.pol.k1_in_front;
    // its buffers are free (long since); K1 on the very stream that computed on them is behind that anyway, and a big batch
    // does not even record the event (below) -- every event operation is a packet of its own that costs the queue 4-6 us
    // between two kernels (profiles/r06/c4_between_split_launches.txt).  Whoever needs it after all records it now: on the
    // stream that computed, behind everything enqueued there since.
    auto& nslot = ls->run.slot[nx.slot];
    if (nslot.used && !(k1_in_front && nslot.compute_stream == s)) {
        if (!nslot.compute_recorded) {
            RSMP_HIP_CHECK(rsmp::event_record(nslot.compute_done, nslot.compute_stream));
            nslot.compute_recorded = true;
        }
        RSMP_HIP_CHECK(rsmp::stream_wait_event(k1_in_front ? s : q, nslot.compute_done));
    }
    // (ev_ready below: completed by the K1 launch itself where RunPolicy::launch_completes_events allows)
    const bool k1_completes_ready = k1_in_front && rc.pol.launch_completes_events;
    if (k1_in_front)
        RSMP_HIP_CHECK(rsmp::launch_fir_lockstep_plan(plan_args(rc, nx, true), s, 1, rc.commit_pending ? &rc.c : nullptr, k1_completes_ready ? static_cast<hipEvent_t>(plan.ev_ready) : nullptr));
    if (rc.commit_on_q && !k1_in_front) {
        // (the states after this run are in place on the plan stream itself: nothing to wait for, unless the probe has
        // just moved the planner to the other candidate)
        if (q != plan.q) RSMP_HIP_CHECK(rsmp::stream_wait_event(q, plan.ev_commit));
    } else {
        if (!k1_completes_ready) RSMP_HIP_CHECK(rsmp::event_record(plan.ev_ready, s));   // the states after this run are in place (and the next run's predictions made)
        RSMP_HIP_CHECK(rsmp::stream_wait_event(q, plan.ev_ready));
    }
    RSMP_HIP_CHECK(rsmp::launch_fir_lockstep_plan(plan_args(rc, nx, true), q, k1_in_front ? 2 : 3));
    nslot.items_valid = false;
    if (rc.pol.items_ahead)
        if (int e = build_items_ahead(rc, nx, q)) return e;
    RSMP_HIP_CHECK(rsmp::event_record(plan.done, q));
    plan.q = q;
    plan.ahead = nx;
    plan.inflight = true;
    return RSMP_OK;
}

// The bulk kernels over the run's descriptors.  The rate pairs the split kernel takes go into launches shared by as
// many of them as have the same kernel build (launch_fir_split_multi), with one item-table launch in front and one
// repair launch behind for all of them: six rate pairs one after the other were 18 launches, most of a run of 16 calls.
// (Measured and dropped before that: the rate pairs' launches side by side on streams of their own, each with its share
// of the compute units -- a run of 16 calls was then bound by the host's ~40 stream / event / launch calls.)
int launch_bulk(RunCall& rc) {
    rsmp_fir_lockstep* ls = rc.ls;
    RunSlots& run = ls->run;
    hipStream_t s = rc.s;
    RunSlot& cslot = run.slot[rc.sl];
    const rsmp::FirStreamDesc* d_descs = cslot.descs.as<rsmp::FirStreamDesc>();
    const size_t n_groups = run.groups.size();
    uint32_t nf_off = 0, max_tail_values = 0;
    std::vector<rsmp::NfArgs> nfs(n_groups);
    std::vector<rsmp::RepairJob> repair_jobs;
    for (size_t gi = 0; gi < n_groups; ++gi) {
        const auto& g = run.groups[gi];
        const RunGroupBounds b = run_group_bounds(g, rc.k);
        rsmp::NfArgs& nf = nfs[gi];
        nf.chunks = b.nf_chunks;
        nf.words = run.d_nf.as<uint32_t>() + nf_off;
        if (++run.nf_tag == 0) run.nf_tag = 1;
        nf.tag = run.nf_tag;
        nf_off += b.nf_words;
        if (g.geo.mfma != 3)
            RSMP_HIP_CHECK(rsmp::launch_fir_periodic(d_descs + g.first, static_cast<uint32_t>(g.count), g.geo, b.max_blocks,
                                                     run.d_work.as<unsigned long long>() + gi, nf, s));
        repair_jobs.push_back(rsmp::RepairJob{d_descs + g.first, static_cast<uint32_t>(g.count), nf});
        const rsmp_fir* r0 = ls->rs[ls->order[g.first]];
        max_tail_values = std::max<uint32_t>(max_tail_values, static_cast<uint32_t>((r0->taps + 8) * r0->channels));
    }
    const std::vector<rsmp::SplitJob> jobs = split_jobs(ls, d_descs, rc.k, nfs.data());
    // (the item tables: built on the plan stream behind this run's plan, if it was planned ahead and no table has changed since)
    const uint32_t* items_prebuilt = rc.plan_taken_over && cslot.items_valid && cslot.items_seq == rc.key.seq && cslot.items_ops == ls->drift.table_ops
                                         ? cslot.items.as<uint32_t>() : nullptr;
    if (!jobs.empty()) RSMP_HIP_CHECK(rsmp::launch_fir_split_multi(jobs.data(), jobs.size(), s, rc.repeat ? rc.pol.reserve_cus : 0u, items_prebuilt));
    if (rc.pol.early_wait && rc.repeat && ls->plan.inflight) {   // (behind the split launch: RunPolicy::early_wait)
        RSMP_HIP_CHECK(rsmp::stream_wait_event(s, ls->plan.done));
        ls->plan.waited = true;
        ls->plan.waited_on = s;
    }
    // (the repair launch copies the streams' tails as well: one launch and its gap less per run)
    const bool record_done = !rc.pol.lazy_done;
    bool done_attached = false;
    const bool attach = record_done && rc.pol.launch_completes_events;
    RSMP_HIP_CHECK(rsmp::launch_fir_repair_multi(repair_jobs.data(), repair_jobs.size(), s, d_descs, static_cast<uint32_t>(rc.n), max_tail_values,
                                                 attach ? static_cast<hipEvent_t>(cslot.compute_done) : nullptr, &done_attached));
    if (record_done && !done_attached) RSMP_HIP_CHECK(rsmp::event_record(cslot.compute_done, s));
    cslot.compute_recorded = record_done;
    cslot.compute_stream = s;
    cslot.used = true;
    return RSMP_OK;
}

// The run is enqueued: the slots rotate, the next run is guessed from this one, the drifts are asked for now and then.
int finish_run(RunCall& rc) {
    rsmp_fir_lockstep* ls = rc.ls;
    RSMP_HIP_CHECK(ls->prof.end(rc.s));
    ls->hist_parity ^= 1u;
    ls->step += rc.k;
    ++ls->epoch;   // plans the one-call kernel made ahead belong to the states before the run
    ++ls->run.seq;
    ls->run.counts_k = rc.k;
    ls->run.planned = true;
    ls->last_stream = rc.s;
    ls->run.last_slot = rc.sl;
    ls->run.next_slot = rc.sl ^ 1;
    ls->plan.prev = rc.key;
    if (rc.d_totals) ls->plan.prev.valid = false;   // (nothing is guessed from a ragged run, and nothing planned ahead survives one)
    return request_drift(ls, rc.s, static_cast<uint64_t>(rc.k) * rc.in_frames);
}

}  // namespace

// The answer of the plan-stream probe in flight (pick_plan_stream), once the device has given it: kept for the caller's stream
// it was made for.
void PlanStreamPick::take_probe_answer() {
    if (!probe_owner) return;
    if (hipEventQuery(probe_ev) != hipSuccess) {
        (void)hipGetLastError();
        return;
    }
    Pick& pp = by_stream[probe_owner];
    pp.probing = false;
    if (*h_probe.as<volatile uint32_t>() == 1u) {
        pp.pick = pp.cand;
        pp.decided = true;
    } else if (++pp.tries >= 4) {
        pp.pick = -1;
        pp.decided = true;
    } else {
        pp.cand ^= 1;
    }
    if (ls_verbose() && pp.decided)
        fprintf(stderr, "[rsmp] lock-step run: plan stream candidate %d runs beside stream %p (%d probes)\n", pp.pick,
                static_cast<void*>(probe_owner), pp.tries + 1);
    probe_owner = nullptr;
}

// A probe in flight on the caller's stream is through as well: it is forgotten (that stream is probed again if it comes back), so
// the next stream's probe is not held up by a stream that may no longer exist.
void PlanStreamPick::forget_caller_streams() {
    if (!probe_owner) return;
    take_probe_answer();
    if (probe_owner) {   // (no answer although its stream is through: that stream is probed again if it comes back)
        auto it = by_stream.find(probe_owner);
        if (it != by_stream.end()) it->second.probing = false;
        probe_owner = nullptr;
    }
}

// Whatever the plan stream was asked to plan ahead is dropped: the caller did something else than repeat its run.  Its
// kernels only WRITE scratch copies and the other slot, but they READ the batch's states, append positions and bound
// pointers: before those change, the plan stream must have finished (`s`: that stream waits; null: the host does).
int drop_plan_ahead(rsmp_fir_lockstep* ls, hipStream_t s) {
    PlanAhead& plan = ls->plan;
    if (plan.inflight && plan.done) {
        if (s) RSMP_HIP_CHECK(rsmp::stream_wait_event(s, plan.done));
        else RSMP_HIP_CHECK(hipEventSynchronize(plan.done));
    }
    plan.inflight = false;
    plan.waited = false;
    plan.ahead.valid = false;
    return RSMP_OK;
}

// k_steps calls of in_frames frames per stream -- or, d_totals != null (rsmp_fir_lockstep_run_bulk_v), a RAGGED run: d_totals[gs]
// frames for stream gs (device array, internal order, in place on `stream`) in calls of in_frames frames, the last one shorter;
// k_steps is then the largest number of calls a stream makes.
int lockstep_run(rsmp_fir_lockstep* ls, size_t k_steps, size_t in_frames, size_t in_offset_frames, int append, void* stream,
                 const uint32_t* d_totals) {
    const bool ragged = d_totals != nullptr;
    if (!ls || !ls->bound)
        return rsmp::fail(RSMP_ERR_INVALID_ARGUMENT, "rsmp_fir_lockstep_run: bind buffers first");
    if (k_steps == 0) return RSMP_OK;
    if (in_frames > ls->step_frames)
        return rsmp::fail(RSMP_ERR_INVALID_INPUT_BUFFER_SIZE,
                          "lock-step batch: %zu frames offered, created for %u per step", in_frames, ls->step_frames);
    DeviceGuard guard(ls->device);
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : static_cast<hipStream_t>(ls->own_stream);
    if (int e = prepare_run(ls)) return e;
    RunSlots& run = ls->run;
    // A run is defined as k steps.  The bulk kernels read a stream's accepted frames as ONE span of its input, which
    // they are as long as every call accepts all it is offered (resampler_fir.rs:524-528: always, unless the step is
    // nearly as long as the reference's 4096-frame input buffer).
    const bool whole_accept = ls->accepts_whole(in_frames);
    // The outputs of a run's calls follow each other in `out`: behind what earlier steps / runs appended, or -- without
    // `append` -- from the front of the buffer (the append position starts again there).
    // (the planner's counters of a run -- outputs, frames, bitmap bits -- are 32-bit: a run whose inputs or whose outputs of
    // any rate pair could pass 2^27 / 2^31 is a loop of steps; 8 -> 384 kHz makes 48 outputs per frame)
    uint64_t max_out_run = 0;
    for (const auto& g : run.groups) max_out_run = std::max<uint64_t>(max_out_run, k_steps * static_cast<uint64_t>(g.max_out_step));
    const bool loop_of_steps = run.state < 0 || k_steps == 1 || !whole_accept ||
                               k_steps * static_cast<uint64_t>(ls->step_frames) > (1u << 27) || max_out_run >= (1ull << 31);
    if (k_steps > (1u << 20)) return rsmp::fail(RSMP_ERR_INVALID_ARGUMENT, "rsmp_fir_lockstep_run: at most 2^20 calls per run");
    RunCall rc{ls, s, stream, ls->rs.size(), in_frames, in_offset_frames, static_cast<uint32_t>(k_steps), append, d_totals, {}, {}};
    uint32_t wrap_words = 1, nf_words = 0;   // (the bitmaps of wrapped outputs, the non-finite marks)
    for (const auto& g : run.groups) {
        const RunGroupBounds b = run_group_bounds(g, rc.k);
        wrap_words = std::max(wrap_words, b.wrap_words);
        nf_words += b.nf_words;
    }
    if (int e = grow_run_workspaces(rc, wrap_words, loop_of_steps)) return e;
    if (loop_of_steps) return run_as_steps(rc);
    RSMP_HIP_CHECK(ls->order_behind_last(s));
    if (nf_words * sizeof(uint32_t) > run.d_nf.capacity()) {
        RSMP_HIP_CHECK(hipStreamSynchronize(s));
        RSMP_HIP_CHECK(run.d_nf.reserve(nf_words * sizeof(uint32_t)));
        RSMP_HIP_CHECK(hipMemsetAsync(run.d_nf.get(), 0, run.d_nf.capacity(), s));
    }
    rc.sl = run.next_slot;
    RunKey& key = rc.key;
    key.k = rc.k;
    key.in_frames = static_cast<uint32_t>(in_frames);
    key.append = append ? 1u : 0u;
    key.parity = ls->hist_parity;
    key.in_offset = in_offset_frames;
    key.seq = run.seq;
    key.slot = rc.sl;
    key.valid = true;
    const RunKey& prev = ls->plan.prev;
    rc.pol = run_policy(rc.n, rc.k, !ragged && ls_knobs().ahead && prev.valid && prev.k == key.k && prev.in_frames == key.in_frames && prev.append == key.append,
                        s == reinterpret_cast<hipStream_t>(RSMP_STREAM_LEGACY));
    RSMP_HIP_CHECK(ls->prof.begin(s));
    if (int e = obtain_plan(rc)) return e;
    rc.repeat = rc.pol.repeats;
    if (rc.repeat) {
        if (int e = pick_plan_stream(ls->pick, s)) return e;
        rc.repeat = ls->pick.stream != nullptr;
    }
    if (rc.commit_pending && !(rc.pol.fuse_commit && rc.repeat)) {   // (RunPolicy::fuse_commit: otherwise K1 of the next run commits)
        RSMP_HIP_CHECK(rsmp::launch_fir_lockstep_commit(rc.c, s));
        rc.commit_pending = false;
    }
    if (rc.repeat)
        if (int e = plan_next_ahead(rc)) return e;
    if (int e = launch_bulk(rc)) return e;
    return finish_run(rc);
}

}  // namespace rsmp

extern "C" int rsmp_fir_lockstep_run(rsmp_fir_lockstep* ls, size_t k_steps, size_t in_frames, size_t in_offset_frames,
                                     int append, void* stream) {
    return rsmp::lockstep_run(ls, k_steps, in_frames, in_offset_frames, append, stream, nullptr);
}

// A whole buffer per stream, fed as the reference's driver loop feeds it (resample/src/main.rs:226-254: calls of
// `chunk_frames` frames until the input is used up, the last one shorter): floor(total / chunk) equal calls through the
// device planner (rsmp_fir_lockstep_run) and, where total is no multiple of chunk, one more call of the remaining frames
// (rsmp_fir_lockstep_step), their outputs appended behind the run's.  Whatever states the streams are in, nothing is
// planned on the host and nothing waits: the calls' counts are device data (rsmp_fir_lockstep_run_counts for the equal
// calls, rsmp_fir_lockstep_counts for the last one), the streams' states stay on the device (rsmp_fir_lockstep_sync).
// This is the bulk entry point for BATCHES IN DISTINCT STATES: rsmp_fir_batch_resample_bulk_device
// replays every stream's control flow on the host's planning workers -- 0.7-1.0 ms for 64 streams x 4096 calls on a
// free 256-thread host, 19-26 ms where the workers have to be woken on a busy one.
extern "C" int rsmp_fir_lockstep_run_bulk(rsmp_fir_lockstep* ls, size_t total_frames, size_t chunk_frames, size_t in_offset_frames,
                                          int append, void* stream) {
    if (!ls || chunk_frames == 0) return rsmp::fail(RSMP_ERR_INVALID_ARGUMENT, "rsmp_fir_lockstep_run_bulk: null batch or zero chunk");
    if (chunk_frames > ls->step_frames)
        return rsmp::fail(RSMP_ERR_INVALID_INPUT_BUFFER_SIZE, "lock-step batch: calls of %zu frames, created for %u per step", chunk_frames,
                          ls->step_frames);
    // The driver loop this stands for offers a call's remainder again when the call accepts less than its offer (resample/src/main.rs:
    // 226-254); a run's calls read their input at fixed offsets.  So the calls must be ones every stream accepts whole: a stream buffers at
    // most INPUT_CAPACITY = 4096 frames (resampler_fir.rs:18, :524-528) and keeps up to taps + 1 of them between calls.
    if (!ls->accepts_whole(chunk_frames))
        return rsmp::fail(RSMP_ERR_INVALID_INPUT_BUFFER_SIZE,
                          "rsmp_fir_lockstep_run_bulk: calls of %zu frames are not accepted whole by a stream of %zu taps (at most %zu)", chunk_frames,
                          ls->max_taps, static_cast<size_t>(rsmp::kMirrorInputCapacity) - ls->max_taps - 8);
    const size_t k = total_frames / chunk_frames, tail = total_frames - k * chunk_frames;
    if (k > 0)
        if (int rc = rsmp_fir_lockstep_run(ls, k, chunk_frames, in_offset_frames, append, stream)) return rc;
    if (tail > 0) {
        const size_t run_k = ls->run.counts_k;
        if (int rc = rsmp_fir_lockstep_step(ls, tail, in_offset_frames + k * chunk_frames, nullptr, (k > 0 || append) ? 1 : 0, stream)) return rc;
        if (k > 0) ls->run.counts_k = run_k;   // (the run's counts stay readable: the last call's are rsmp_fir_lockstep_counts')
    }
    return RSMP_OK;
}

// rsmp_fir_lockstep_run_bulk with a buffer length per stream: every stream makes the calls the driver loop makes for ITS buffer
// (resample/src/main.rs:226-254), all of them -- the short last one included -- planned on the device in one run
// (fir_lockstep_run.hip: the RAGGED instantiations of the planner's kernels), the bulk kernels launched once over descriptors
// whose lengths differ from stream to stream as they always have.
extern "C" int rsmp_fir_lockstep_run_bulk_v(rsmp_fir_lockstep* ls, const size_t* total_frames, size_t chunk_frames, size_t in_offset_frames,
                                            int append, void* stream) {
    if (!ls || !total_frames || chunk_frames == 0)
        return rsmp::fail(RSMP_ERR_INVALID_ARGUMENT, "rsmp_fir_lockstep_run_bulk_v: null batch, null lengths or zero chunk");
    if (chunk_frames > ls->step_frames)
        return rsmp::fail(RSMP_ERR_INVALID_INPUT_BUFFER_SIZE, "lock-step batch: calls of %zu frames, created for %u per step", chunk_frames,
                          ls->step_frames);
    if (!ls->accepts_whole(chunk_frames))   // (calls every stream accepts whole: rsmp_fir_lockstep_run_bulk)
        return rsmp::fail(RSMP_ERR_INVALID_INPUT_BUFFER_SIZE,
                          "rsmp_fir_lockstep_run_bulk_v: calls of %zu frames are not accepted whole by a stream of %zu taps (at most %zu)", chunk_frames,
                          ls->max_taps, static_cast<size_t>(rsmp::kMirrorInputCapacity) - ls->max_taps - 8);
    if (!ls->bound) return rsmp::fail(RSMP_ERR_INVALID_ARGUMENT, "rsmp_fir_lockstep_run_bulk_v: bind buffers first");
    const size_t n = ls->rs.size();
    size_t longest = 0;
    for (size_t i = 0; i < n; ++i) longest = std::max(longest, total_frames[i]);
    if (longest == 0) return RSMP_OK;
    if (longest > (1u << 27)) return rsmp::fail(RSMP_ERR_INVALID_ARGUMENT, "rsmp_fir_lockstep_run_bulk_v: at most 2^27 frames per stream and run");
    const size_t k = (longest + chunk_frames - 1) / chunk_frames;   // rows of the run's tables: the longest stream's calls
    rsmp::DeviceGuard guard(ls->device);
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : static_cast<hipStream_t>(ls->own_stream);
    RSMP_HIP_CHECK(ls->order_behind_last(s));   // (in front of the upload below)
    if (int rc = rsmp::prepare_run(ls)) return rc;
    rsmp::RaggedTotals& t = ls->totals;
    if (t.d_totals.capacity() < n * sizeof(uint32_t) || !t.ev[rsmp::RaggedTotals::kRing - 1]) {   // (the batch's first ragged run)
        if (t.d_totals.reserve(n * sizeof(uint32_t)) != hipSuccess || t.d_offer.reserve(n * sizeof(uint32_t)) != hipSuccess ||
            t.d_keep.reserve(2 * n * sizeof(uint64_t)) != hipSuccess)
            return rsmp::fail(RSMP_ERR_HIP, "rsmp_fir_lockstep_run_bulk_v: cannot allocate device state");
        for (int j = 0; j < rsmp::RaggedTotals::kRing; ++j)
            if (t.h[j].reserve(n * sizeof(uint32_t)) != hipSuccess || t.ev[j].create(hipEventDisableTiming) != hipSuccess)
                return rsmp::fail(RSMP_ERR_HIP, "rsmp_fir_lockstep_run_bulk_v: cannot allocate staging memory");
    }
    const int j = t.next;
    t.next = (j + 1) % rsmp::RaggedTotals::kRing;
    if (t.inflight[j]) RSMP_HIP_CHECK(hipEventSynchronize(t.ev[j]));   // (the upload four ragged runs ago)
    uint32_t* h = t.h[j].as<uint32_t>();
    for (size_t gs = 0; gs < n; ++gs) h[gs] = static_cast<uint32_t>(total_frames[ls->order[gs]]);
    RSMP_HIP_CHECK(hipMemcpyAsync(t.d_totals.get(), h, n * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    RSMP_HIP_CHECK(rsmp::event_record(t.ev[j], s));
    t.inflight[j] = true;
    ls->last_stream = s;
    return rsmp::lockstep_run(ls, k, chunk_frames, in_offset_frames, append, stream, t.d_totals.as<uint32_t>());
}
