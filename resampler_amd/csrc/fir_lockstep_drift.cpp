// fir_lockstep_drift.cpp -- the lock-step batch's drift classes: reading the streams' f64 drift back from the device and
// replacing a class's tables when it has moved too far (struct Drift, fir_lockstep_batch.h).
#include <cmath>
#include <cstdio>
#include <cstring>

#include "fir_lockstep_batch.h"

using rsmp::FirMirrorState;
using rsmp::LockstepGroup;

namespace rsmp {

namespace {

constexpr double kLsDriftQuantum = 1e-8;      // tables are built for drifts on this grid (frames)
constexpr double kLsDriftClass = 2e-8;        // streams of one key whose drifts round to the same multiple share a class
// A class's tables are replaced when its drift is further from theirs than this: 2e-7 of a full-scale sample at worst,
// a fifth of the 1e-6 the path is allowed.  (Tighter costs: a replacement is a table built on the host per class, ~0.5 ms;
// config 4 on one GPU runs 0.13 M frames of every stream per millisecond, and at 4e-8 its six classes were rebuilt every
// 35 ms -- 10 % of the bench's step.  A real-time stream crosses 1.2e-7 every five minutes.)
constexpr double kLsDriftTolerance = 1.2e-7;
constexpr uint64_t kLsDriftCheckFrames = 1u << 19;   // input frames per stream between two looks at the drifts (~5e-9 of drift)

// Class `c` takes `step` / `run` as its tables (either may be null: not replaced), built for drift `t`: the host copies
// of the group and stream tables are changed; the caller moves them to the device (flush_tables, or a patch kernel).
void bind_class_tables(rsmp_fir_lockstep* ls, size_t c, const rsmp::ClassTable* step, const rsmp::ClassTable* run, double t) {
    DriftClass& cl = ls->drift.classes[c];
    if (step) {
        if (cl.step_table.hold) cl.holds.push_back(cl.step_table.hold);   // (a run planned ahead may still name it)
        cl.step_table = *step;
        for (LockstepGroup& g : ls->groups)
            if (g.periodic && g.pad0 == c) {
                g.class_coef = step->d_coef;
                g.class_meta = step->d_meta;
            }
    }
    if (run) {
        if (cl.run_table.hold) cl.holds.push_back(cl.run_table.hold);
        cl.run_table = *run;
        for (size_t i = cl.first; i < cl.first + cl.count; ++i) {
            ls->run.h_rs[i].class_coef = run->d_coef;
            ls->run.h_rs[i].class_wrap_coef = run->d_wrap_coef;
            ls->run.h_rs[i].class_meta = run->d_meta;
            ls->run.h_rs[i].drift = t;
        }
    }
    cl.table_drift = t;
    ++ls->drift.table_rebinds;
}

// Images unbound by a replacement may be overwritten behind everything enqueued on `s` so far.  An image whose guard
// could not be recorded stays in the list (the next call tries again before it asks for anything).
int record_due_guards(Drift& dr, hipStream_t s) {
    while (!dr.guards_due.empty()) {
        if (int rc = dr.refresher->record_guard(dr.guards_due.back(), s)) return rc;
        dr.guards_due.pop_back();
    }
    return RSMP_OK;
}

// A reading of the drifts that has come back from the device is taken in: every class's drift and its rate.
bool take_drift_reading(Drift& dr) {
    if (!dr.inflight) return false;
    if (hipEventQuery(dr.ev) != hipSuccess) {
        (void)hipGetLastError();   // (hipErrorNotReady is not an error here)
        return false;
    }
    dr.inflight = false;
    const double* d = dr.h_drift.as<double>();
    const bool rate_ok = dr.have_seen && dr.frames_at_inflight > dr.frames_at_seen;
    const double span = rate_ok ? static_cast<double>(dr.frames_at_inflight - dr.frames_at_seen) : 1.0;
    for (size_t c = 0; c < dr.classes.size(); ++c) {
        DriftClass& cl = dr.classes[c];
        if (rate_ok) cl.rate = (d[c] - cl.seen_drift) / span;
        cl.seen_drift = d[c];
    }
    dr.frames_at_seen = dr.frames_at_inflight;
    dr.have_seen = true;
    return true;
}

// The patches of one look at the classes: one patch kernel on `s` for up to kLsMaxPatches replacements.
struct TablePatches {
    rsmp_fir_lockstep* ls;
    hipStream_t s;
    rsmp::LsPatchArgs pa;
    int flush() {
        if (pa.n_patches) {
            RSMP_HIP_CHECK(rsmp::launch_fir_lockstep_patch_tables(pa, s));
            ++ls->drift.table_ops;
        }
        pa.n_patches = 0;
        return RSMP_OK;
    }
};

using TR = rsmp::TableRefresher;
int state_of(TR::Table* t) { return t ? t->state.load(std::memory_order_acquire) : static_cast<int>(TR::kReady); }

int ask_next_tables(Drift& dr, DriftClass& cl, bool want_step, bool want_run, double nd) {
    cl.next_drift = nd;
    if (want_step) if (int rc = dr.refresher->request(cl.step_next, nd)) return rc;
    if (want_run) if (int rc = dr.refresher->request(cl.run_next, nd)) return rc;
    cl.next_pending = true;
    return RSMP_OK;
}

// Class `c` takes the tables the worker has left for it: pointer swaps and a patch for the device's copies.
int take_next_tables(rsmp_fir_lockstep* ls, size_t c, bool want_step, bool want_run, TablePatches& tp) {
    Drift& dr = ls->drift;
    DriftClass& cl = dr.classes[c];
    rsmp::ClassTable stt, rtt;
    if (want_step) { stt = dr.refresher->take(cl.step_next); dr.guards_due.push_back(cl.step_next); }
    if (want_run) { rtt = dr.refresher->take(cl.run_next); dr.guards_due.push_back(cl.run_next); }
    cl.next_pending = false;
    bind_class_tables(ls, c, want_step ? &stt : nullptr, want_run ? &rtt : nullptr, cl.next_drift);
    cl.late = false;
    --dr.n_late;
    rsmp::LsTablePatch& q = tp.pa.p[tp.pa.n_patches++];
    q.cls = static_cast<uint32_t>(c);
    q.first = static_cast<uint32_t>(cl.first);
    q.count = static_cast<uint32_t>(cl.count);
    q.flags = (want_step ? 1u : 0u) | (want_run ? 2u : 0u);
    q.step_coef = stt.d_coef;
    q.step_meta = stt.d_meta;
    q.run_coef = rtt.d_coef;
    q.run_wrap_coef = rtt.d_wrap_coef;
    q.run_meta = rtt.d_meta;
    q.drift = cl.next_drift;
    return tp.pa.n_patches == rsmp::kLsMaxPatches ? tp.flush() : RSMP_OK;
}

// One class's decision for the drift `now_drift` a launch enqueued now will see: ask for its next tables, wait for them,
// take them, or discard what was prepared for another drift.
int poll_class(rsmp_fir_lockstep* ls, size_t c, double now_drift, TablePatches& tp) {
    Drift& dr = ls->drift;
    DriftClass& cl = dr.classes[c];
    const double tol = dr.tolerance, off = now_drift - cl.table_drift;
    const bool want_step = cl.has_step, want_run = cl.has_run && ls->run.state == 1;
    if (!want_step && !want_run) return RSMP_OK;
    if (std::fabs(off) <= tol) {
        if (cl.late) { cl.late = false; --dr.n_late; }   // (the extrapolation came back inside the tolerance: no more polling on its account)
        if (std::fabs(off) > 0.6 * tol && !cl.next_pending) {
            // most of the way: the tables the class will want at the crossing are made now, beside everything else
            return ask_next_tables(dr, cl, want_step, want_run, quantized_drift(cl.table_drift + (off > 0.0 ? tol : -tol)));
        }
        return RSMP_OK;
    }
    if (!cl.late) { cl.late = true; ++dr.n_late; }
    int st = want_step ? state_of(cl.step_next) : TR::kReady, rt = want_run ? state_of(cl.run_next) : TR::kReady;
    if (cl.next_pending && (st == TR::kRequested || rt == TR::kRequested) && std::fabs(off) > 3.0 * tol) {
        if (want_step) dr.refresher->wait(cl.step_next);
        if (want_run) dr.refresher->wait(cl.run_next);
        ++dr.table_waits;
        st = want_step ? state_of(cl.step_next) : TR::kReady;
        rt = want_run ? state_of(cl.run_next) : TR::kReady;
    }
    if (cl.next_pending && (st == TR::kRequested || rt == TR::kRequested)) {
        if (ls_verbose()) fprintf(stderr, "[rsmp] class %zu: drift %.3g past its tables' %.3g, the next ones (%.3g) on their way\n", c, now_drift, cl.table_drift, cl.next_drift);
        ++dr.late_polls;   // on their way: the old tables serve a little longer (a fifth of the bound per tolerance)
        return RSMP_OK;
    }
    if (cl.next_pending && (st == TR::kFailed || rt == TR::kFailed))
        return rsmp::fail(RSMP_ERR_HIP, "lock-step batch: the replacement class tables could not be made");
    if (cl.next_pending && std::fabs(now_drift - cl.next_drift) <= 0.5 * tol) {
        if (ls_verbose()) fprintf(stderr, "[rsmp] class %zu: drift %.3g (read %.3g + lead), tables %.3g -> %.3g\n", c, now_drift, cl.seen_drift, cl.table_drift, cl.next_drift);
        return take_next_tables(ls, c, want_step, want_run, tp);
    }
    // nothing asked for yet, or what was prepared is for another drift (a jump): ask now
    if (cl.next_pending) {   // (both results are in: drop them, the images are free again)
        if (want_step) dr.refresher->discard(cl.step_next);
        if (want_run) dr.refresher->discard(cl.run_next);
        cl.next_pending = false;
    }
    ++dr.late_polls;
    if (ls_verbose()) fprintf(stderr, "[rsmp] class %zu: drift %.3g past its tables' %.3g with nothing asked for\n", c, now_drift, cl.table_drift);
    return ask_next_tables(dr, cl, want_step, want_run, quantized_drift(now_drift));
}

}  // namespace

double quantized_drift(double d) { return std::round(d / kLsDriftQuantum) * kLsDriftQuantum; }
long long drift_class_of(double drift) { return std::llround(drift / kLsDriftClass); }

void init_drift(rsmp_fir_lockstep* ls) {
    ls->drift.tolerance = kLsDriftTolerance;
    ls->drift.check_frames = kLsDriftCheckFrames;
    ls->drift.refresher.reset(new rsmp::TableRefresher(ls->device));   // (its thread starts with the batch's first request)
}

int set_drift_policy(rsmp_fir_lockstep* ls, double tolerance_frames, size_t check_frames) {
    if (!ls || !(tolerance_frames >= 2.0 * kLsDriftQuantum) || tolerance_frames > 1e-6 || check_frames == 0)
        return rsmp::fail(RSMP_ERR_INVALID_ARGUMENT, "rsmp_fir_lockstep_set_drift_policy: tolerance in [2e-8, 1e-6] frames, check_frames > 0");
    ls->drift.tolerance = tolerance_frames;
    ls->drift.check_frames = check_frames;
    return RSMP_OK;
}

// New tables for class `c` from the process-wide cache, built for drift `d` -- where the HOST knows the states and may
// wait (creation, reset): class_table_for builds on this thread, allocates and copies synchronously.
int rebind_class_blocking(rsmp_fir_lockstep* ls, size_t c, double d) {
    DriftClass& cl = ls->drift.classes[c];
    const double t = quantized_drift(d);
    rsmp::ClassTable st, rt;
    const bool want_run = cl.has_run && ls->run.state == 1;
    if (cl.has_step)
        if (int rc = rsmp::class_table_for(ls->device, *cl.r0->table, cl.step_geo, t, &st)) return rc;
    if (want_run)
        if (int rc = rsmp::class_table_for(ls->device, *cl.r0->table, cl.run_geo, t, &rt)) return rc;
    bind_class_tables(ls, c, cl.has_step ? &st : nullptr, want_run ? &rt : nullptr, t);
    if (cl.has_step) ls->drift.groups_dirty = true;
    if (want_run) ls->drift.rs_dirty = true;
    if (cl.late) { cl.late = false; --ls->drift.n_late; }
    return RSMP_OK;
}

// The launch path's side of a replacement.  Where the drifts that have come back from the device say so, a class's next
// tables are ASKED FOR (most of the way to the tolerance: one event record), and a class past the tolerance TAKES the
// tables the worker has left for it (pointer swaps + one patch kernel for all classes of this look).  Nothing here
// builds, allocates or copies.  It WAITS for the worker only where a class is three tolerances past its tables without new
// ones: back-pressure on a caller that enqueues without ever waiting -- the image a replacement overwrites was bound
// until the replacement before it, and the device must have passed that point (TableRefresher's guard), so the host
// can be about two table generations ahead of the device and no more (tools/soak_lockstep.py --hours 24 at ~25 k
// launches per second of host time: 374 waits in 29 k runs, none in the bench's 64 launches or behind a caller that
// synchronises now and then; counted in Drift::table_waits).
int poll_drift(rsmp_fir_lockstep* ls, hipStream_t s) {
    Drift& dr = ls->drift;
    // Guards a previous call took but did not get to record (it failed between its replacement and request_drift): the
    // images it unbound must not be refilled before everything enqueued so far has passed -- recorded here, in front of
    // any request() below, they are later than needed and never stale.
    if (int rc = record_due_guards(dr, s)) return rc;
    const bool fresh = take_drift_reading(dr);
    // (looked at when a reading has come in, while a class is late, and every 2^17 frames in between: the host's lead grows)
    if (!fresh && dr.n_late == 0 && dr.frames_total - dr.frames_at_eval < (1u << 17)) return RSMP_OK;
    dr.frames_at_eval = dr.frames_total;
    const double lead = dr.have_seen ? static_cast<double>(dr.frames_total - dr.frames_at_seen) : 0.0;
    TablePatches tp{ls, s, {}};
    tp.pa.groups = ls->d_groups.as<LockstepGroup>();
    tp.pa.rs = ls->run.state == 1 ? ls->run.d_rs.as<rsmp::LsRunStream>() : nullptr;
    tp.pa.n_groups = static_cast<uint32_t>(ls->groups.size());
    tp.pa.n_streams = static_cast<uint32_t>(ls->rs.size());
    tp.pa.n_patches = 0;
    tp.pa.pad = 0;
    for (size_t c = 0; c < dr.classes.size(); ++c) {
        const DriftClass& cl = dr.classes[c];
        // (what a launch enqueued now will see)
        if (int rc = poll_class(ls, c, cl.seen_drift + cl.rate * lead, tp)) return rc;
    }
    return tp.flush();
}

// Changed group / stream tables go to the device as a whole, in stream order in front of what is enqueued next: the
// blocking paths' way (reset, the first run).  (Called where no planner of the batch is running: the plan stream has
// been waited for.)
int flush_tables(rsmp_fir_lockstep* ls, hipStream_t s) {
    Drift& dr = ls->drift;
    if (!dr.groups_dirty && !dr.rs_dirty) return RSMP_OK;
    ++dr.table_ops;
    const size_t gb = ls->groups.size() * sizeof(LockstepGroup), rb = ls->run.h_rs.size() * sizeof(rsmp::LsRunStream);
    if (dr.stage_inflight) {   // (the staging memory of the previous change: long since read)
        RSMP_HIP_CHECK(hipEventSynchronize(dr.stage_ev));
        dr.stage_inflight = false;
    }
    RSMP_HIP_CHECK(dr.h_stage.reserve(gb + rb));
    char* h = dr.h_stage.as<char>();
    if (dr.groups_dirty) {
        std::memcpy(h, ls->groups.data(), gb);
        RSMP_HIP_CHECK(hipMemcpyAsync(ls->d_groups.get(), h, gb, hipMemcpyHostToDevice, s));
    }
    if (dr.rs_dirty && ls->run.state == 1) {
        std::memcpy(h + gb, ls->run.h_rs.data(), rb);
        RSMP_HIP_CHECK(hipMemcpyAsync(ls->run.d_rs.get(), h + gb, rb, hipMemcpyHostToDevice, s));
    }
    RSMP_HIP_CHECK(rsmp::event_record(dr.stage_ev, s));
    dr.stage_inflight = true;
    dr.groups_dirty = dr.rs_dirty = false;
    return RSMP_OK;
}

// After a step or run of `frames` input frames per stream: now and then the classes' drifts start their way to the host.
// Images this call's replacements have unbound may be overwritten behind everything enqueued so far.
int request_drift(rsmp_fir_lockstep* ls, hipStream_t s, uint64_t frames) {
    Drift& dr = ls->drift;
    if (int rc = record_due_guards(dr, s)) return rc;
    dr.frames_since += frames;
    dr.frames_total += frames;
    if (dr.inflight || dr.frames_since < dr.check_frames || dr.classes.empty()) return RSMP_OK;
    const uint32_t nc = static_cast<uint32_t>(dr.classes.size());
    // (the kernel stores straight into the mapped, coherent host buffer: a copy-engine operation in the stream costs the
    // stream ~0.1 ms of cross-queue synchronisation, 6-9 % of config 4's step when done every fourth run)
    RSMP_HIP_CHECK(rsmp::launch_fir_lockstep_gather_drift(ls->d_states.as<FirMirrorState>(), dr.d_reps.as<uint32_t>(),
                                                          dr.h_drift.as<double>(), nc, s));
    RSMP_HIP_CHECK(rsmp::event_record(dr.ev, s));
    dr.inflight = true;
    dr.frames_at_inflight = dr.frames_total;
    dr.frames_since = 0;
    return RSMP_OK;
}

// The host knows the states (creation, reset): every class gets the tables of its first stream's drift at once.  What
// the worker was asked for belongs to the old states: waited for and dropped.
int rebind_from_host_states(rsmp_fir_lockstep* ls) {
    Drift& dr = ls->drift;
    if (dr.inflight) {   // (what is on its way belongs to the old states)
        RSMP_HIP_CHECK(hipEventSynchronize(dr.ev));
        dr.inflight = false;
    }
    dr.frames_since = 0;
    dr.have_seen = false;
    dr.frames_at_seen = dr.frames_at_inflight = dr.frames_at_eval = dr.frames_total;
    for (size_t c = 0; c < dr.classes.size(); ++c) {
        DriftClass& cl = dr.classes[c];
        if (cl.next_pending) {
            for (rsmp::TableRefresher::Table* t : {cl.step_next, cl.run_next})
                if (t && t->state.load(std::memory_order_acquire) != rsmp::TableRefresher::kIdle) {
                    dr.refresher->wait(t);
                    dr.refresher->discard(t);   // (nobody bound the image: it is the next to be filled again)
                }
            cl.next_pending = false;
        }
        const double d = ls->rs[ls->order[cl.rep]]->mirror.drift();
        cl.seen_drift = d;
        cl.rate = 0.0;
        if (std::fabs(d - cl.table_drift) > kLsDriftQuantum || cl.late)
            if (int rc = rebind_class_blocking(ls, c, d)) return rc;
    }
    return RSMP_OK;
}

}  // namespace rsmp
