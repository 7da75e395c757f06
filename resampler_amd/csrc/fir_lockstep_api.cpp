// fir_lockstep_api.cpp -- C ABI of the lock-step batch (rsmp_fir_lockstep_*): BASELINE config 4's
// shape, a fixed set of ResamplerFir instances (src/resampler_fir.rs:179-643) that are each fed one
// chunk per step.  Creation sorts the streams by rate pair / table, builds the per-workgroup groups
// and moves the streams' reference state to HBM; a step is one launch of fir_lockstep_kernel with
// constant arguments -- no per-stream host work, no upload, no host-side state machine.
// The batch itself is fir_lockstep_batch.h; drift classes and their tables are fir_lockstep_drift.cpp, runs of several calls
// and the bulk entries fir_lockstep_runpath.cpp.
#include <algorithm>
#include <cstring>
#include <tuple>

#include "fir_kernel_launch.h"
#include "fir_lockstep_batch.h"

using rsmp::DeviceGuard;
using rsmp::FirMirrorState;
using rsmp::LockstepGroup;
using rsmp::LockstepStream;
using rsmp::drop_plan_ahead;
using rsmp::flush_tables;
using rsmp::poll_drift;
using rsmp::quantized_drift;
using rsmp::request_drift;

namespace {

// A stream's buffered frames alternate between its two history buffers (fir_lockstep.h, LockstepStream):
// the next step (index ls->step) reads `hist` when its index is even.  After any number of steps the handle's
// `cur` is made to name the buffer that holds the frames.
void refresh_history_index(rsmp_fir_lockstep* ls) {
    if (!ls->bound) return;
    for (size_t k = 0; k < ls->rs.size(); ++k) {
        rsmp_fir* r = ls->rs[ls->order[k]];
        const float* live = ls->hist_parity ? ls->streams[k].hist_alt : ls->streams[k].hist;
        r->cur = live == r->d_hist[0] ? 0 : 1;
    }
}

int upload_states(rsmp_fir_lockstep* ls) {
    const size_t n = ls->rs.size();
    ls->h_states.resize(n);
    for (size_t k = 0; k < n; ++k) ls->h_states[k] = ls->rs[ls->order[k]]->mirror.state();
    RSMP_HIP_CHECK(hipMemcpy(ls->d_states.get(), ls->h_states.data(), n * sizeof(FirMirrorState),
                             hipMemcpyHostToDevice));
    return RSMP_OK;
}

// Creation, first half: the streams sorted into drift classes, the classes cut into the step kernel's workgroups.
bool build_classes_and_groups(rsmp_fir_lockstep* ls) {
    rsmp_fir* const* rs = ls->rs.data();
    const size_t n = ls->rs.size(), step_frames = ls->step_frames;
    // Streams that share a polyphase table, a rate pair and a channel count share a class table and
    // a geometry: they become neighbours, then workgroups of `slots` streams.
    // (a stream set to RSMP_FIR_KERNEL_PERIODIC_F32 keeps every product in f32: its own groups)
    // (... and whose f64 drifts lie together: DriftClass)
    typedef std::tuple<const void*, uint32_t, uint32_t, size_t, size_t, bool, long long> Key;
    auto exact_of = [](const rsmp_fir* r) { return r->kernel_mode != RSMP_FIR_KERNEL_AUTO; };
    auto key_of = [&](const rsmp_fir* r) {
        return Key(static_cast<const void*>(r->table.get()), r->in_hz, r->out_hz, r->channels, r->taps, exact_of(r),
                   rsmp::drift_class_of(r->mirror.drift()));
    };
    ls->order.resize(n);
    for (size_t i = 0; i < n; ++i) ls->order[i] = static_cast<uint32_t>(i);
    std::stable_sort(ls->order.begin(), ls->order.end(),
                     [&](uint32_t x, uint32_t y) { return key_of(rs[x]) < key_of(rs[y]); });
    ls->streams.resize(n);
    ls->channels.resize(n);
    size_t k = 0;
    while (k < n) {
        const rsmp_fir* r0 = rs[ls->order[k]];
        size_t e = k;
        while (e < n && key_of(rs[ls->order[e]]) == key_of(r0)) ++e;
        const rsmp::LockstepGeometry geo =
            rsmp::lockstep_geometry(r0->mirror.num(), r0->mirror.den(), r0->mirror.ratio(),
                                    static_cast<uint32_t>(r0->taps), static_cast<uint32_t>(r0->channels),
                                    ls->step_frames, !exact_of(r0));
        if (geo.lds_bytes == 0) {
            rsmp::fail(RSMP_ERR_INVALID_ARGUMENT,
                       "lock-step batch: %zu channels x %zu frames per step do not fit the LDS", r0->channels,
                       step_frames);
            return false;
        }
        rsmp::ClassTable ct;
        rsmp::DriftClass cl;
        cl.rep = static_cast<uint32_t>(k);
        cl.first = k;
        cl.count = e - k;
        cl.r0 = r0;
        cl.table_drift = quantized_drift(r0->mirror.drift());
        cl.has_step = geo.periodic;
        if (geo.periodic) {
            cl.step_geo = rsmp::lockstep_class_geometry(geo);
            if (rsmp::class_table_for(ls->device, *r0->table, cl.step_geo, cl.table_drift, &ct) != RSMP_OK)
                return false;
            cl.step_table = ct;
            cl.step_next = ls->drift.refresher->add_table(cl.step_geo, r0->table);
            if (!cl.step_next) {
                rsmp::fail(RSMP_ERR_HIP, "lock-step batch: cannot create an event");
                return false;
            }
        }
        cl.seen_drift = cl.table_drift;
        const uint32_t class_index = static_cast<uint32_t>(ls->drift.classes.size());
        ls->drift.classes.push_back(std::move(cl));
        const rsmp::LsCutMax most = rsmp::lockstep_cut_groups(ls->groups, geo, static_cast<uint32_t>(r0->channels), k, e, ct.d_coef, ct.d_meta, class_index);
        ls->max_lds = std::max(ls->max_lds, most.lds_bytes);
        ls->rec_stride = std::max(ls->rec_stride, most.rec_stride);
        for (size_t i = k; i < e; ++i) {
            const rsmp_fir* r = rs[ls->order[i]];
            if (r->mirror.available() >= r->taps + 8) {
                rsmp::fail(RSMP_ERR_INVALID_ARGUMENT,
                           "lock-step batch: stream %u holds %zu buffered frames (an output-capped call left "
                           "them); drain it first", ls->order[i], r->mirror.available());
                return false;
            }
            ls->channels[i] = static_cast<uint32_t>(r->channels);
        }
        k = e;
    }
    return true;
}

// Creation, second half: the batch's device state.  (What a failure leaves behind goes with the batch: its members own it.)
bool init_device_state(rsmp_fir_lockstep* ls) {
    rsmp_fir* const* rs = ls->rs.data();
    const size_t n = ls->rs.size();
    if (ls->d_groups.reserve(ls->groups.size() * sizeof(LockstepGroup)) != hipSuccess ||
        ls->d_streams.reserve(n * sizeof(LockstepStream)) != hipSuccess ||
        ls->d_states.reserve(n * sizeof(FirMirrorState)) != hipSuccess ||
        ls->d_cursor.reserve(n * sizeof(uint64_t)) != hipSuccess ||
        ls->d_counts.reserve(2 * n * sizeof(uint64_t)) != hipSuccess ||
        ls->d_status.reserve(n * sizeof(uint32_t)) != hipSuccess ||
        ls->d_order.reserve(n * sizeof(uint32_t)) != hipSuccess ||
        ls->d_recs.reserve(2 * n * static_cast<size_t>(ls->rec_stride)) != hipSuccess ||
        ls->d_peaks.reserve(n * 16) != hipSuccess ||
        ls->drift.d_reps.reserve(ls->drift.classes.size() * sizeof(uint32_t)) != hipSuccess ||
        ls->drift.h_drift.reserve(ls->drift.classes.size() * sizeof(double)) != hipSuccess ||
        ls->drift.ev.create(hipEventDisableTiming) != hipSuccess ||
        ls->drift.stage_ev.create(hipEventDisableTiming) != hipSuccess ||
        ls->pick.probe_ev.create(hipEventDisableTiming) != hipSuccess ||
        ls->pick.d_probe.reserve(sizeof(uint32_t)) != hipSuccess ||
        ls->pick.h_probe.reserve(sizeof(uint32_t)) != hipSuccess ||
        hipMemset(ls->pick.d_probe.get(), 0, sizeof(uint32_t)) != hipSuccess ||
        ls->own_stream.create(hipStreamNonBlocking) != hipSuccess) {
        rsmp::fail(RSMP_ERR_HIP, "lock-step batch: cannot allocate device state");
        return false;
    }
    // every stream's earlier launches (which wrote its buffered frames) must be complete
    for (size_t i = 0; i < n; ++i) {
        (void)hipStreamSynchronize(rs[i]->stream);
        if (rs[i]->last_launch) (void)hipEventSynchronize(rs[i]->last_launch->ev);   // (not the stream: it may be gone)
    }
    if (hipMemcpy(ls->d_groups.get(), ls->groups.data(), ls->groups.size() * sizeof(LockstepGroup),
                  hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(ls->d_order.get(), ls->order.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice) != hipSuccess ||
        [&] {
            std::vector<uint32_t> reps;
            for (const auto& cl : ls->drift.classes) reps.push_back(cl.rep);
            return hipMemcpy(ls->drift.d_reps.get(), reps.data(), reps.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
        }() != hipSuccess ||
        hipMemset(ls->d_recs.get(), 0, 2 * n * static_cast<size_t>(ls->rec_stride)) != hipSuccess ||
        hipMemset(ls->d_peaks.get(), 0, n * 16) != hipSuccess ||
        hipMemset(ls->d_cursor.get(), 0, n * sizeof(uint64_t)) != hipSuccess ||
        hipMemset(ls->d_counts.get(), 0, 2 * n * sizeof(uint64_t)) != hipSuccess ||
        hipMemset(ls->d_status.get(), 0, n * sizeof(uint32_t)) != hipSuccess ||
        upload_states(ls) != RSMP_OK) {
        rsmp::fail(RSMP_ERR_HIP, "lock-step batch: cannot initialise device state");
        return false;
    }
    return true;
}

}  // namespace

extern "C" rsmp_fir_lockstep* rsmp_fir_lockstep_new(rsmp_fir* const* rs, size_t n, size_t step_frames) {
    if (!rs || n == 0 || step_frames == 0 || step_frames > rsmp::kMirrorInputCapacity) {
        rsmp::fail(RSMP_ERR_INVALID_ARGUMENT, "rsmp_fir_lockstep_new: need streams and 1..4096 frames per step");
        return nullptr;
    }
    for (size_t i = 0; i < n; ++i)
        if (!rs[i] || rs[i]->device != rs[0]->device) {
            rsmp::fail(RSMP_ERR_INVALID_ARGUMENT, "lock-step streams must share one device");
            return nullptr;
        }
    {
        std::vector<rsmp_fir*> sorted(rs, rs + n);
        std::sort(sorted.begin(), sorted.end());
        if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) {
            rsmp::fail(RSMP_ERR_INVALID_ARGUMENT, "lock-step batch lists the same stream twice");
            return nullptr;
        }
    }
    DeviceGuard guard(rs[0]->device);
    std::unique_ptr<rsmp_fir_lockstep> ls(new rsmp_fir_lockstep);
    ls->device = rs[0]->device;
    ls->step_frames = static_cast<uint32_t>(step_frames);
    ls->rs.assign(rs, rs + n);
    for (size_t i = 0; i < n; ++i) ls->max_taps = std::max<size_t>(ls->max_taps, rs[i]->taps);
    rsmp::init_drift(ls.get());
    if (!build_classes_and_groups(ls.get())) return nullptr;
    rsmp::lockstep_order_groups(ls->groups, rsmp::device_cus(ls->device));
    if (!init_device_state(ls.get())) return nullptr;
    return ls.release();
}

static void lockstep_destroy(rsmp_fir_lockstep* ls, bool write_back);
extern "C" void rsmp_fir_lockstep_free(rsmp_fir_lockstep* ls) { lockstep_destroy(ls, true); }
extern "C" void rsmp_fir_lockstep_discard(rsmp_fir_lockstep* ls) { lockstep_destroy(ls, false); }
// The waits, in this order, then the members' holders free what they own.  What must not outlive something else is reset
// here by name: the order of the members' declarations decides nothing.
static void lockstep_destroy(rsmp_fir_lockstep* ls, bool write_back) {
    if (!ls) return;
    DeviceGuard guard(ls->device);
    if (write_back) (void)rsmp_fir_lockstep_sync(ls);
    else (void)ls->wait_last_launch();
    if (ls->pick.probe_ev) (void)hipEventSynchronize(ls->pick.probe_ev);   // (a probe's kernels name d_probe / h_probe)
    for (rsmp::StreamHolder& q : ls->pick.candidates) {
        if (q) (void)hipStreamSynchronize(q);
        q.reset();
    }
    if (ls->own_stream) rsmp::split_release_stream(ls->device, ls->own_stream);
    ls->own_stream.reset();
    ls->drift.refresher.reset();   // (joins its thread, frees the images: every kernel that read them has been waited for above)
    delete ls;
}

extern "C" size_t rsmp_fir_lockstep_size(const rsmp_fir_lockstep* ls) { return ls ? ls->rs.size() : 0; }
extern "C" size_t rsmp_fir_lockstep_workgroups(const rsmp_fir_lockstep* ls) { return ls ? ls->groups.size() : 0; }
extern "C" size_t rsmp_fir_lockstep_split_workgroups(const rsmp_fir_lockstep* ls) {
    size_t n = 0;
    if (ls) for (const LockstepGroup& g : ls->groups) n += g.split ? 1 : 0;
    return n;
}

extern "C" int rsmp_fir_lockstep_bind(rsmp_fir_lockstep* ls, const float* const* d_in, float* const* d_out,
                                      const size_t* out_caps) {
    if (!ls || !d_in || !d_out || !out_caps)
        return rsmp::fail(RSMP_ERR_INVALID_ARGUMENT, "rsmp_fir_lockstep_bind: null argument");
    DeviceGuard guard(ls->device);
    const size_t n = ls->rs.size();
    RSMP_HIP_CHECK(ls->wait_last_launch());
    if (int rc = drop_plan_ahead(ls, nullptr)) return rc;
    ls->plan.prev.valid = false;
    for (auto& cl : ls->drift.classes) cl.holds.clear();   // (nothing enqueued or planned ahead names a replaced cache table any more)
    refresh_history_index(ls);
    bool aligned8 = true;
    for (size_t k = 0; k < n; ++k) {
        const uint32_t i = ls->order[k];
        const rsmp_fir* r = ls->rs[i];
        if (out_caps[i] % r->channels != 0)
            return rsmp::fail(RSMP_ERR_INVALID_OUTPUT_BUFFER_SIZE, "Output buffer size is invalid");
        // the reference's documented sizing (resampler_fir.rs:456-465); with it a step never leaves more
        // than taps - 1 frames buffered, which is what bounds a stream's LDS span
        if (out_caps[i] < rsmp_fir_buffer_size_output(r))
            return rsmp::fail(RSMP_ERR_INVALID_OUTPUT_BUFFER_SIZE,
                              "lock-step batch: stream %u needs room for buffer_size_output() = %zu values per step",
                              i, rsmp_fir_buffer_size_output(r));
        LockstepStream& s = ls->streams[k];
        if (reinterpret_cast<uintptr_t>(d_in[i]) % 8 != 0) aligned8 = false;
        s.in = d_in[i];
        s.out = d_out[i];
        s.hist = r->d_hist[ls->hist_parity ? r->cur ^ 1 : r->cur];       // the next step reads the handle's current buffer
        s.hist_alt = r->d_hist[ls->hist_parity ? r->cur : r->cur ^ 1];
        s.coeffs = r->d_coeffs;
        s.out_cap_frames = out_caps[i] / r->channels;
    }
    RSMP_HIP_CHECK(ls->wait_last_launch());
    RSMP_HIP_CHECK(hipMemcpy(ls->d_streams.get(), ls->streams.data(), n * sizeof(LockstepStream),
                             hipMemcpyHostToDevice));
    RSMP_HIP_CHECK(hipMemset(ls->d_cursor.get(), 0, n * sizeof(uint64_t)));   // nothing has been appended to the new buffers
    ls->bound = true;
    ls->in_aligned8 = aligned8;
    ++ls->epoch;   // plans made ahead assumed the previous output capacities
    return RSMP_OK;
}

extern "C" int rsmp_fir_lockstep_rebind_buffers(rsmp_fir_lockstep* ls, const float* const* d_in, float* const* d_out, void* stream) {
    if (!ls || !d_in || !d_out) return rsmp::fail(RSMP_ERR_INVALID_ARGUMENT, "rsmp_fir_lockstep_rebind_buffers: null argument");
    if (!ls->bound) return rsmp::fail(RSMP_ERR_INVALID_ARGUMENT, "rsmp_fir_lockstep_rebind_buffers: the batch has not been bound yet");
    DeviceGuard guard(ls->device);
    const size_t n = ls->rs.size();
    bool aligned8 = true;
    for (size_t i = 0; i < n; ++i)
        if (reinterpret_cast<uintptr_t>(d_in[i]) % 8 != 0) aligned8 = false;
    if (aligned8 != ls->in_aligned8) {   // (another build of the step kernel's loads: a bind proper, with the capacities as they are)
        std::vector<size_t> caps(n);
        for (size_t k = 0; k < n; ++k) caps[ls->order[k]] = static_cast<size_t>(ls->streams[k].out_cap_frames) * ls->rs[ls->order[k]]->channels;
        return rsmp_fir_lockstep_bind(ls, d_in, d_out, caps.data());
    }
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : static_cast<hipStream_t>(ls->own_stream);
    RSMP_HIP_CHECK(ls->order_behind_last(s));
    // A run planned ahead survives if it starts at the front of `out` (nothing it computed depends on the buffers but the two pointers
    // in its descriptors); one that appends behind what the old buffers hold does not.
    const bool keep = ls->plan.inflight && ls->plan.ahead.valid && ls->plan.ahead.append == 0;
    if (!keep) {
        if (int rc = drop_plan_ahead(ls, s)) return rc;
    }
    for (size_t k = 0; k < n; ++k) {
        const uint32_t i = ls->order[k];
        ls->streams[k].in = d_in[i];
        ls->streams[k].out = d_out[i];
    }
    // (in stream order: steps and runs enqueued before this read the old table, those behind it the new one.  A planner already running
    // on the plan stream may see either -- its descriptors are patched when the run is taken over.)
    RSMP_HIP_CHECK(hipMemcpyAsync(ls->d_streams.get(), ls->streams.data(), n * sizeof(LockstepStream), hipMemcpyHostToDevice, s));
    RSMP_HIP_CHECK(hipMemsetAsync(ls->d_cursor.get(), 0, n * sizeof(uint64_t), s));   // nothing has been appended to the new buffers
    ls->plan.rebased = keep;
    ls->last_stream = s;
    return RSMP_OK;
}

extern "C" int rsmp_fir_lockstep_step(rsmp_fir_lockstep* ls, size_t in_frames, size_t in_offset_frames,
                                      const uint32_t* d_in_frames, int append, void* stream) {
    if (!ls || !ls->bound)
        return rsmp::fail(RSMP_ERR_INVALID_ARGUMENT, "rsmp_fir_lockstep_step: bind buffers first");
    if (in_frames > ls->step_frames)
        return rsmp::fail(RSMP_ERR_INVALID_INPUT_BUFFER_SIZE,
                          "lock-step batch: %zu frames offered, created for %u per step", in_frames,
                          ls->step_frames);
    DeviceGuard guard(ls->device);
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : static_cast<hipStream_t>(ls->own_stream);
    RSMP_HIP_CHECK(ls->order_behind_last(s));
    if (int rc = drop_plan_ahead(ls, s)) return rc;   // (a run planned ahead read the states this step is about to change)
    ls->plan.prev.valid = false;
    if (int rc = poll_drift(ls, s)) return rc;
    if (int rc = flush_tables(ls, s)) return rc;
    rsmp::LockstepArgs a;
    a.groups = ls->d_groups.as<LockstepGroup>();
    a.streams = ls->d_streams.as<LockstepStream>();
    a.states = ls->d_states.as<FirMirrorState>();
    a.out_cursor = ls->d_cursor.as<uint64_t>();
    a.counts = ls->d_counts.as<uint64_t>();
    a.status = ls->d_status.as<uint32_t>();
    a.order = ls->d_order.as<uint32_t>();
    a.in_frames_per_stream = d_in_frames;
    a.in_offset = in_offset_frames;
    a.in_frames = static_cast<uint32_t>(in_frames);
    a.append = append ? 1u : 0u;
    a.in_aligned8 = ls->in_aligned8 ? 1u : 0u;
    a.trace = nullptr;
    a.recs = ls->d_recs.as<char>();
    a.peaks = ls->d_peaks.as<uint32_t>();
    a.rec_stride = ls->rec_stride;
    a.n_streams = static_cast<uint32_t>(ls->rs.size());
    a.epoch = ls->epoch;
    a.step = ls->step++;
    a.hist_parity = ls->hist_parity;
    ls->hist_parity ^= 1u;
    ls->run.counts_k = 0;
    RSMP_HIP_CHECK(ls->prof.begin(s));
    RSMP_HIP_CHECK(rsmp::launch_fir_lockstep(a, static_cast<uint32_t>(ls->groups.size()), ls->max_lds, s));
    RSMP_HIP_CHECK(ls->prof.end(s));
    ls->last_stream = s;
    return request_drift(ls, s, in_frames);
}

extern "C" int rsmp_fir_lockstep_counts(rsmp_fir_lockstep* ls, size_t* consumed, size_t* produced) {
    if (!ls) return rsmp::fail(RSMP_ERR_INVALID_ARGUMENT, "rsmp_fir_lockstep_counts: null batch");
    DeviceGuard guard(ls->device);
    const size_t n = ls->rs.size();
    RSMP_HIP_CHECK(ls->wait_last_launch());
    ls->h_counts.resize(2 * n);
    RSMP_HIP_CHECK(hipMemcpy(ls->h_counts.data(), ls->d_counts.get(), 2 * n * sizeof(uint64_t),
                             hipMemcpyDeviceToHost));
    for (size_t k = 0; k < n; ++k) {
        const uint32_t i = ls->order[k];
        if (consumed) consumed[i] = static_cast<size_t>(ls->h_counts[2 * k]);
        if (produced) produced[i] = static_cast<size_t>(ls->h_counts[2 * k + 1]);
    }
    return RSMP_OK;
}

extern "C" int rsmp_fir_lockstep_status(rsmp_fir_lockstep* ls, uint32_t* status) {
    if (!ls || !status) return rsmp::fail(RSMP_ERR_INVALID_ARGUMENT, "rsmp_fir_lockstep_status: null argument");
    DeviceGuard guard(ls->device);
    const size_t n = ls->rs.size();
    RSMP_HIP_CHECK(ls->wait_last_launch());
    std::vector<uint32_t> h(n);
    RSMP_HIP_CHECK(hipMemcpy(h.data(), ls->d_status.get(), n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    for (size_t k = 0; k < n; ++k) status[ls->order[k]] = h[k];
    return RSMP_OK;
}

// Everything the batch enqueued on a caller's stream is complete (that stream has just been synchronized; a change of streams
// synchronized the one before): the batch keeps no handle of the caller's streams beyond this point, so the caller may destroy
// them (a stream per launch: the routed bulk entry syncs through here before it returns).  The slots' computations are
// through, a run planned ahead is waited for through its event, and a stream seen again is only compared, never used.  A probe
// in flight on the caller's stream is through as well: it is forgotten (that stream is probed again if it comes back), so the
// next stream's probe is not held up by a stream that may no longer exist.
static void forget_caller_streams(rsmp_fir_lockstep* ls) {
    ls->last_stream = nullptr;
    ls->pick.forget_caller_streams();
    ls->run.forget_caller_streams(ls->own_stream);
    ls->plan.forget_caller_streams();
}

extern "C" int rsmp_fir_lockstep_sync(rsmp_fir_lockstep* ls) {
    if (!ls) return rsmp::fail(RSMP_ERR_INVALID_ARGUMENT, "rsmp_fir_lockstep_sync: null batch");
    DeviceGuard guard(ls->device);
    const size_t n = ls->rs.size();
    RSMP_HIP_CHECK(ls->wait_last_launch());
    forget_caller_streams(ls);
    ls->h_states.resize(n);
    RSMP_HIP_CHECK(hipMemcpy(ls->h_states.data(), ls->d_states.get(), n * sizeof(FirMirrorState),
                             hipMemcpyDeviceToHost));
    for (size_t k = 0; k < n; ++k) ls->rs[ls->order[k]]->mirror.set_state(ls->h_states[k]);
    refresh_history_index(ls);
    return RSMP_OK;
}

extern "C" int rsmp_fir_lockstep_sync_totals(rsmp_fir_lockstep* ls, size_t* accepted, size_t* produced, uint32_t* status_or) {
    if (!ls) return rsmp::fail(RSMP_ERR_INVALID_ARGUMENT, "rsmp_fir_lockstep_sync_totals: null batch");
    const size_t n = ls->rs.size();
    const std::vector<FirMirrorState> before = ls->h_states;   // (internal order: what was last exchanged with the handles)
    if (before.size() != n) return rsmp::fail(RSMP_ERR_INVALID_ARGUMENT, "rsmp_fir_lockstep_sync_totals: the batch has no states yet");
    if (int rc = rsmp_fir_lockstep_sync(ls)) return rc;
    for (size_t k = 0; k < n; ++k) {
        const uint32_t i = ls->order[k];
        const size_t ch = ls->rs[i]->channels;
        const FirMirrorState &a = before[k], &b = ls->h_states[k];
        if (accepted) accepted[i] = static_cast<size_t>((b.abs_consumed + b.available) - (a.abs_consumed + a.available)) * ch;
        if (produced) produced[i] = static_cast<size_t>(b.abs_out - a.abs_out) * ch;
    }
    if (status_or) {
        std::vector<uint32_t> st(n);
        RSMP_HIP_CHECK(hipMemcpy(st.data(), ls->d_status.get(), n * sizeof(uint32_t), hipMemcpyDeviceToHost));
        uint32_t v = 0;
        for (uint32_t f : st) v |= f;
        *status_or = v;
    }
    return RSMP_OK;
}

extern "C" int rsmp_fir_lockstep_in_sync(const rsmp_fir_lockstep* ls, int* in_sync) {
    if (!ls || !in_sync) return rsmp::fail(RSMP_ERR_INVALID_ARGUMENT, "rsmp_fir_lockstep_in_sync: null argument");
    const size_t n = ls->rs.size();
    *in_sync = 0;
    if (ls->h_states.size() != n) return RSMP_OK;
    for (size_t k = 0; k < n; ++k) {
        const rsmp_fir* r = ls->rs[ls->order[k]];
        const FirMirrorState now = r->mirror.state();
        if (memcmp(&now, &ls->h_states[k], sizeof now) != 0) return RSMP_OK;
        // (the frames the stream has buffered: in the buffer the batch's next step reads)
        const float* live = ls->hist_parity ? ls->streams[k].hist_alt : ls->streams[k].hist;
        if (ls->bound && live != r->d_hist[r->cur]) return RSMP_OK;
    }
    *in_sync = 1;
    return RSMP_OK;
}

extern "C" int rsmp_fir_batch_distinct_states(rsmp_fir* const* rs, size_t n, size_t* distinct) {
    if (!rs || !distinct) return rsmp::fail(RSMP_ERR_INVALID_ARGUMENT, "rsmp_fir_batch_distinct_states: null argument");
    std::vector<FirMirrorState> seen;
    for (size_t i = 0; i < n; ++i) {
        if (!rs[i]) return rsmp::fail(RSMP_ERR_INVALID_ARGUMENT, "rsmp_fir_batch_distinct_states: null stream");
        const FirMirrorState s = rs[i]->mirror.state();
        bool found = false;
        for (const FirMirrorState& t : seen)
            if (memcmp(&s, &t, sizeof s) == 0) { found = true; break; }
        if (!found) seen.push_back(s);
    }
    *distinct = seen.size();
    return RSMP_OK;
}

extern "C" int rsmp_fir_lockstep_reset(rsmp_fir_lockstep* ls) {
    if (!ls) return rsmp::fail(RSMP_ERR_INVALID_ARGUMENT, "rsmp_fir_lockstep_reset: null batch");
    DeviceGuard guard(ls->device);
    const size_t n = ls->rs.size();
    RSMP_HIP_CHECK(ls->wait_last_launch());
    if (int rc = drop_plan_ahead(ls, nullptr)) return rc;
    ls->plan.prev.valid = false;
    for (auto& cl : ls->drift.classes) cl.holds.clear();
    for (rsmp_fir* r : ls->rs) r->mirror.reset();   // resampler_fir.rs:638-642
    RSMP_HIP_CHECK(hipMemset(ls->d_cursor.get(), 0, n * sizeof(uint64_t)));
    RSMP_HIP_CHECK(hipMemset(ls->d_status.get(), 0, n * sizeof(uint32_t)));
    ++ls->epoch;   // plans made ahead belong to the old states
    if (int rc = upload_states(ls)) return rc;
    if (int rc = rsmp::rebind_from_host_states(ls)) return rc;   // (fresh streams: drift 0)
    if (int rc = flush_tables(ls, ls->own_stream)) return rc;
    RSMP_HIP_CHECK(hipStreamSynchronize(ls->own_stream));
    return RSMP_OK;
}

extern "C" int rsmp_fir_lockstep_set_profiling(rsmp_fir_lockstep* ls, int enable) {
    if (!ls) return rsmp::fail(RSMP_ERR_INVALID_ARGUMENT, "rsmp_fir_lockstep_set_profiling: null batch");
    DeviceGuard guard(ls->device);
    if (enable && !ls->prof.start[0])
        for (int i = 0; i < rsmp::StepProfiler::kRing; ++i) {
            RSMP_HIP_CHECK(ls->prof.start[i].create());
            RSMP_HIP_CHECK(ls->prof.stop[i].create());
        }
    ls->prof.on = enable != 0;
    ls->prof.count = 0;
    return RSMP_OK;
}

extern "C" int rsmp_fir_lockstep_mean_kernel_ms(rsmp_fir_lockstep* ls, float* ms, size_t* launches) {
    if (!ls || !ms || ls->prof.count == 0)
        return rsmp::fail(RSMP_ERR_INVALID_ARGUMENT, "rsmp_fir_lockstep_mean_kernel_ms: no profiled step");
    DeviceGuard guard(ls->device);
    const size_t ring = rsmp::StepProfiler::kRing;
    const size_t n = ls->prof.count < ring ? ls->prof.count : ring;
    RSMP_HIP_CHECK(hipEventSynchronize(ls->prof.stop[(ls->prof.count - 1) % ring]));
    double sum = 0.0;
    for (size_t k = 0; k < n; ++k) {
        const size_t i = (ls->prof.count - 1 - k) % ring;
        float t = 0.f;
        RSMP_HIP_CHECK(hipEventElapsedTime(&t, ls->prof.start[i], ls->prof.stop[i]));
        sum += t;
    }
    *ms = static_cast<float>(sum / static_cast<double>(n));
    if (launches) *launches = n;
    return RSMP_OK;
}

extern "C" int rsmp_fir_lockstep_kernel_ms(rsmp_fir_lockstep* ls, float* ms, size_t cap, size_t* launches) {
    if (!ls || !ms || !launches) return rsmp::fail(RSMP_ERR_INVALID_ARGUMENT, "rsmp_fir_lockstep_kernel_ms: null argument");
    DeviceGuard guard(ls->device);
    const size_t ring = rsmp::StepProfiler::kRing;
    const size_t n = std::min(cap, std::min(ls->prof.count, ring));
    *launches = n;
    if (n == 0) return RSMP_OK;
    RSMP_HIP_CHECK(hipEventSynchronize(ls->prof.stop[(ls->prof.count - 1) % ring]));
    for (size_t k = 0; k < n; ++k) {   // oldest first
        const size_t i = (ls->prof.count - n + k) % ring;
        RSMP_HIP_CHECK(hipEventElapsedTime(&ms[k], ls->prof.start[i], ls->prof.stop[i]));
    }
    return RSMP_OK;
}

extern "C" int rsmp_fir_lockstep_run_counts(rsmp_fir_lockstep* ls, size_t* consumed, size_t* produced, size_t max_steps) {
    if (!ls) return rsmp::fail(RSMP_ERR_INVALID_ARGUMENT, "rsmp_fir_lockstep_run_counts: null batch");
    if (ls->run.counts_k == 0)
        return rsmp::fail(RSMP_ERR_INVALID_ARGUMENT, "rsmp_fir_lockstep_run_counts: the last launch was not a run of several calls");
    DeviceGuard guard(ls->device);
    const size_t n = ls->rs.size(), k = std::min(ls->run.counts_k, max_steps);
    RSMP_HIP_CHECK(ls->wait_last_launch());
    ls->run.h_counts.resize(2 * n * k);
    RSMP_HIP_CHECK(hipMemcpy(ls->run.h_counts.data(), ls->run.slot[ls->run.last_slot].counts.get(), 2 * n * k * sizeof(uint32_t), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n * k; ++i) {
        if (consumed) consumed[i] = ls->run.h_counts[2 * i];
        if (produced) produced[i] = ls->run.h_counts[2 * i + 1];
    }
    return RSMP_OK;
}

extern "C" int rsmp_fir_lockstep_table_rebinds(const rsmp_fir_lockstep* ls, size_t* rebinds) {
    if (!ls || !rebinds) return rsmp::fail(RSMP_ERR_INVALID_ARGUMENT, "rsmp_fir_lockstep_table_rebinds: null argument");
    *rebinds = ls->drift.table_rebinds;
    return RSMP_OK;
}

extern "C" int rsmp_fir_lockstep_run_slow_calls(rsmp_fir_lockstep* ls, size_t* slow_calls) {
    if (!ls || !slow_calls) return rsmp::fail(RSMP_ERR_INVALID_ARGUMENT, "rsmp_fir_lockstep_run_slow_calls: null argument");
    *slow_calls = 0;
    if (ls->run.counts_k <= 1 || ls->run.state <= 0 || !ls->run.planned) return RSMP_OK;   // (a loop of steps)
    DeviceGuard guard(ls->device);
    RSMP_HIP_CHECK(ls->wait_last_launch());
    struct Rec { double pos, drift; uint32_t flags, pad; };
    std::vector<Rec> h(ls->rs.size() * ls->run.counts_k);
    RSMP_HIP_CHECK(hipMemcpy(h.data(), ls->run.slot[ls->run.last_slot].recs.get(), h.size() * sizeof(Rec), hipMemcpyDeviceToHost));
    for (const Rec& r : h) *slow_calls += r.flags & 1u;
    return RSMP_OK;
}

extern "C" int rsmp_fir_lockstep_stats(const rsmp_fir_lockstep* ls, uint64_t* out, size_t n) {
    if (!ls || !out) return rsmp::fail(RSMP_ERR_INVALID_ARGUMENT, "rsmp_fir_lockstep_stats: null argument");
    const rsmp::Drift& dr = ls->drift;
    const uint64_t v[RSMP_LS_STAT_COUNT] = {dr.table_rebinds, ls->plan.hits, ls->plan.misses, dr.late_polls, dr.table_waits, ls->pick.probes,
                                            ls->pick.stream ? 1u : 0u, dr.classes.size(), ls->plan.commits_on_plan_stream};
    for (size_t i = 0; i < n && i < sizeof v / sizeof v[0]; ++i) out[i] = v[i];
    return RSMP_OK;
}

extern "C" int rsmp_fir_lockstep_set_drift_policy(rsmp_fir_lockstep* ls, double tolerance_frames, size_t check_frames) {
    return rsmp::set_drift_policy(ls, tolerance_frames, check_frames);
}
