// fir_api.cpp -- ResamplerFir front-end on the GPU: handles, device tables, the C ABI.
//
// Mirrors src/resampler_fir.rs of the reference: construction (:295-404), buffer_size_output
// (:456-465), resample (:509-621), delay (:630-632), reset (:638-642).  The per-call control
// flow (how many frames are accepted / produced / retired) runs on the host in FirMirror (planned by
// fir_hostplan.cpp); the arithmetic runs in one launch of fir_generic / fir_periodic per call, bulk
// buffer or batch (assembled by fir_launch.cpp).  DESIGN.md 4.3b says which file owns what.
//
// Device-side stream state: instead of the reference's planar double-size ring
// (input_buffers, :187, :329) each stream keeps only the frames still buffered
// (available_frames <= 4096) as an interleaved `hist` array, ping-ponged between two HBM
// buffers; a launch reads the virtual concatenation [hist | new input] and a small tail-copy
// kernel writes the next hist.  There is no CPU fallback anywhere in this file.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "common.h"
#include "device_util.h"
#include "filter_design.h"
#include "fir_handle.h"
#include "fir_hostplan.h"
#include "fir_launch.h"
#include "fir_routed.h"
#include "plan_pool.h"

using rsmp::DeviceGuard;
using rsmp::FirJob;
using rsmp::Plan;
using rsmp::PlanKey;
using rsmp::launch_jobs;
using rsmp::plan_pool;

namespace {

// Per-device cache of uploaded polyphase tables (the device-side half of the reference's
// FIR_CACHE, resampler_fir.rs:164-166): key = (device, host table identity).
struct DeviceTableCache {
    std::mutex mu;
    std::map<std::pair<int, const void*>, float*> tables;
    // Keeps host tables alive for as long as their device copies are cached.
    std::vector<std::shared_ptr<const std::vector<float>>> pins;
};
DeviceTableCache& table_cache() {
    static DeviceTableCache* c = new DeviceTableCache;  // leaked on purpose (process lifetime)
    return *c;
}

int upload_table(int device, const std::shared_ptr<const std::vector<float>>& host, float** out) {
    DeviceTableCache& c = table_cache();
    std::lock_guard<std::mutex> lock(c.mu);
    const auto key = std::make_pair(device, static_cast<const void*>(host.get()));
    auto it = c.tables.find(key);
    if (it != c.tables.end()) { *out = it->second; return RSMP_OK; }
    float* d = nullptr;
    RSMP_HIP_CHECK(hipMalloc(&d, host->size() * sizeof(float)));
    RSMP_HIP_CHECK(hipMemcpy(d, host->data(), host->size() * sizeof(float), hipMemcpyHostToDevice));
    c.tables.emplace(key, d);
    c.pins.push_back(host);
    *out = d;
    return RSMP_OK;
}


// Releases everything a (possibly half-built) handle owns.
void fir_destroy(rsmp_fir* r) {
    if (!r) return;
    rsmp::routed_forget(r);
    DeviceGuard guard(r->device);
    if (r->stream) (void)hipStreamSynchronize(r->stream);
    (void)hipDeviceSynchronize();
    for (int i = 0; i < 2; ++i) if (r->d_hist[i]) (void)hipFree(r->d_hist[i]);
    if (r->d_work_counter) (void)hipFree(r->d_work_counter);
    // (before the stream goes, as ever; the holders would let go of them with the handle)
    for (rsmp::EventHolder& e : r->plan_copied) e.reset();
    for (rsmp::EventHolder& e : r->prof_start) e.reset();
    for (rsmp::EventHolder& e : r->prof_stop) e.reset();
    if (r->stream) {
        rsmp::split_release_stream(r->device, r->stream);
        (void)hipStreamDestroy(r->stream);
    }
    delete r;
}

rsmp_fir* fir_create(size_t channels, uint32_t in_hz, uint32_t out_hz, int latency,
                     int attenuation, int device) {
    const size_t taps = rsmp::latency_taps(latency);
    const double beta = rsmp::attenuation_beta(attenuation);
    if (channels == 0 || channels > 4096 || taps == 0 || beta < 0.0) {
        rsmp::fail(RSMP_ERR_INVALID_ARGUMENT, "ResamplerFir: invalid channels/latency/attenuation");
        return nullptr;
    }
    if (in_hz == 0) {  // resampler_fir.rs:302-305 panics
        rsmp::fail(RSMP_ERR_INVALID_ARGUMENT, "input sample rate must be greater than zero");
        return nullptr;
    }
    if (out_hz == 0) {  // resampler_fir.rs:306-309 panics
        rsmp::fail(RSMP_ERR_INVALID_ARGUMENT, "output sample rate must be greater than zero");
        return nullptr;
    }
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) {
        rsmp::fail(RSMP_ERR_NO_DEVICE, "ResamplerFir: no HIP device (this engine has no CPU path)");
        return nullptr;
    }
    if (device < 0 || device >= n_dev) {
        rsmp::fail(RSMP_ERR_INVALID_ARGUMENT, "ResamplerFir: device %d out of range (%d devices)",
                   device, n_dev);
        return nullptr;
    }
    DeviceGuard guard(device);
    std::unique_ptr<rsmp_fir> r(new rsmp_fir(in_hz, out_hz, taps));
    r->device = device;
    r->channels = channels;
    r->taps = taps;
    r->attenuation = attenuation;
    r->in_hz = in_hz;
    r->out_hz = out_hz;
    const rsmp::FirDesign design = rsmp::fir_design(in_hz, out_hz, taps, beta);
    r->table = rsmp::get_or_create_fir_coeffs(design.cutoff, taps, attenuation);
    if (upload_table(device, r->table, &r->d_coeffs) != RSMP_OK) return nullptr;
    const size_t hist_bytes = rsmp::kInputCapacity * channels * sizeof(float);
    for (int i = 0; i < 2; ++i) {
        if (hipMalloc(&r->d_hist[i], hist_bytes) != hipSuccess ||
            hipMemset(r->d_hist[i], 0, hist_bytes) != hipSuccess ||
            hipStreamSynchronize(nullptr) != hipSuccess) {   // (the handle's stream is non-blocking: no implicit order)
            rsmp::fail(RSMP_ERR_HIP, "ResamplerFir: cannot allocate stream state");
            fir_destroy(r.release());
            return nullptr;
        }
    }
    if (hipStreamCreateWithFlags(&r->stream, hipStreamNonBlocking) != hipSuccess ||
        r->plan_copied[0].create(hipEventDisableTiming) != hipSuccess ||
        r->plan_copied[1].create(hipEventDisableTiming) != hipSuccess ||
        r->plan_copied[2].create(hipEventDisableTiming) != hipSuccess ||
        r->plan_copied[3].create(hipEventDisableTiming) != hipSuccess) {
        rsmp::fail(RSMP_ERR_HIP, "ResamplerFir: cannot create stream/event");
        fir_destroy(r.release());
        return nullptr;
    }
    return r.release();
}

void report_calls(const FirJob& j, size_t* calls, size_t max_calls, size_t* n_calls) {
    const Plan& pl = *j.plan;
    const size_t nc = pl.calls.size() / 2;
    if (n_calls) *n_calls = nc;
    if (calls)
        for (size_t i = 0; i < 2 * nc && i < 2 * max_calls; ++i) calls[i] = pl.calls[i] * j.r->channels;
}

int run_single_piece(rsmp_fir* r, const float* d_in, size_t in_len, float* d_out, size_t out_cap,
                     size_t chunk_len, size_t* consumed, size_t* produced, size_t* calls,
                     size_t max_calls, size_t* n_calls, hipStream_t stream) {
    std::vector<FirJob> jobs;
    jobs.push_back(FirJob{r, d_in, in_len, d_out, out_cap, chunk_len, nullptr});
    int rc = rsmp::plan_job(jobs[0].request(), &jobs[0].plan);
    if (rc != RSMP_OK) return rc;
    rc = launch_jobs(r, jobs, stream);
    if (rc != RSMP_OK) return rc;
    if (consumed) *consumed = jobs[0].consumed();
    if (produced) *produced = jobs[0].produced();
    report_calls(jobs[0], calls, max_calls, n_calls);
    return RSMP_OK;
}

// A bulk call of more than one launch's worth of input (rsmp::kMaxLaunchOutputs, fir_hostplan.h) is cut into launches.
// (The batch entry has the same loop over a list of streams -- rsmp_fir_batch_resample_bulk_device_ex: its pieces are
// planned through the memo and the pool and report no calls, this one's neither; one loop for both came out longer.)
int run_single(rsmp_fir* r, const float* d_in, size_t in_len, float* d_out, size_t out_cap,
               size_t chunk_len, size_t* consumed, size_t* produced, size_t* calls,
               size_t max_calls, size_t* n_calls, hipStream_t stream) {
    const size_t ch = r->channels;
    if (chunk_len == 0 || chunk_len % ch != 0 || in_len % ch != 0)
        return run_single_piece(r, d_in, in_len, d_out, out_cap, chunk_len, consumed, produced, calls, max_calls, n_calls, stream);
    const size_t piece_len = rsmp::launch_input_values(r->mirror.ratio(), ch, chunk_len);
    if (in_len <= piece_len)
        return run_single_piece(r, d_in, in_len, d_out, out_cap, chunk_len, consumed, produced, calls, max_calls, n_calls, stream);
    size_t off = 0, made = 0, n_total = 0;
    while (off < in_len) {
        const size_t take = std::min(piece_len, in_len - off);
        size_t c = 0, p = 0, nc = 0;
        const size_t room = n_total < max_calls ? max_calls - n_total : 0;
        if (int rc = run_single_piece(r, d_in + off, take, d_out + made, out_cap - made, chunk_len, &c, &p,
                                      calls && room ? calls + 2 * n_total : nullptr, room, &nc, stream))
            return rc;
        off += c;
        made += p;
        n_total += nc;
        if (c != take) break;   // (cannot happen in a bulk call: every call accepts what it is offered)
    }
    if (consumed) *consumed = off;
    if (produced) *produced = made;
    if (n_calls) *n_calls = n_total;
    return RSMP_OK;
}

// The host-pointer entries: the caller's slices are staged (in mapped host memory if `zero_copy`, else in HBM through the copy
// engine), the call runs on the handle's own stream, and the caller's buffers are free on return.
int run_staged(rsmp_fir* r, const float* in, size_t in_len, float* out, size_t out_cap, size_t chunk_len, bool zero_copy,
               size_t* consumed, size_t* produced, size_t* calls, size_t max_calls, size_t* n_calls) {
    RSMP_HIP_CHECK(hipStreamSynchronize(r->stream));
    float* d_in_stage = nullptr;
    float* d_out_stage = nullptr;
    if (zero_copy) {
        RSMP_HIP_CHECK(r->h_stage_in.reserve((in_len + 4) * sizeof(float), false));
        RSMP_HIP_CHECK(r->h_stage_out.reserve((out_cap + 4) * sizeof(float), false));
        if (in_len) std::memcpy(r->h_stage_in.get(), in, in_len * sizeof(float));
        RSMP_HIP_CHECK(hipHostGetDevicePointer(reinterpret_cast<void**>(&d_in_stage), r->h_stage_in.get(), 0));
        RSMP_HIP_CHECK(hipHostGetDevicePointer(reinterpret_cast<void**>(&d_out_stage), r->h_stage_out.get(), 0));
    } else {
        RSMP_HIP_CHECK(r->d_stage_in.reserve((in_len + 4) * sizeof(float)));
        RSMP_HIP_CHECK(r->d_stage_out.reserve((out_cap + 4) * sizeof(float)));
        if (in_len)
            RSMP_HIP_CHECK(hipMemcpyAsync(r->d_stage_in.get(), in, in_len * sizeof(float), hipMemcpyHostToDevice, r->stream));
        d_in_stage = r->d_stage_in.as<float>();
        d_out_stage = r->d_stage_out.as<float>();
    }
    size_t c = 0, p = 0;
    const int rc = run_single(r, d_in_stage, in_len, d_out_stage, out_cap, chunk_len, &c, &p, calls, max_calls, n_calls, r->stream);
    if (rc != RSMP_OK) return rc;
    if (p && !zero_copy)
        RSMP_HIP_CHECK(hipMemcpyAsync(out, r->d_stage_out.get(), p * sizeof(float), hipMemcpyDeviceToHost, r->stream));
    RSMP_HIP_CHECK(hipStreamSynchronize(r->stream));
    if (p && zero_copy) std::memcpy(out, r->h_stage_out.get(), p * sizeof(float));
    if (consumed) *consumed = c;
    if (produced) *produced = p;
    return RSMP_OK;
}

// One launch of a list of streams: a plan per distinct (state, amount of input), then launch_jobs led by the first handle.
int batch_bulk_piece(rsmp_fir* const* rs, size_t n, const float* const* d_in, const size_t* in_lens, size_t chunk_len,
                     float* const* d_out, const size_t* out_caps, size_t* consumed, size_t* produced, void* stream, const rsmp::FirFormat& format = {}) {
    switch (rsmp::batch_handles_fault(rs, n)) {
        case rsmp::BatchFault::NullOrOtherDevice: return rsmp::fail(RSMP_ERR_INVALID_ARGUMENT, "batch streams must share one device");
        case rsmp::BatchFault::Duplicate: return rsmp::fail(RSMP_ERR_INVALID_ARGUMENT, "batch lists the same stream twice");
        case rsmp::BatchFault::None: break;
    }
    DeviceGuard guard(rs[0]->device);
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : rs[0]->stream;
    static const bool verbose_t = rsmp::knob("RSMP_FIR_VERBOSE") != nullptr;
    const auto t_begin = std::chrono::steady_clock::now();
    std::vector<FirJob> jobs;
    jobs.reserve(n);
    // Streams in the same state that are fed the same amount share one replay of the reference
    // call sequence (the control flow does not depend on the sample values).
    std::vector<std::pair<PlanKey, std::shared_ptr<Plan>>> memo;
    std::vector<size_t> rep;        // per job: index into memo
    std::vector<size_t> memo_job;   // per memo entry: the first job with that key
    for (size_t i = 0; i < n; ++i) {
        jobs.push_back(FirJob{rs[i], d_in[i], in_lens[i], d_out[i], out_caps[i], chunk_len, nullptr});
        const PlanKey key = rsmp::make_key(jobs.back().request());
        size_t m = 0;
        while (m < memo.size() && !(memo[m].first == key)) ++m;
        if (m == memo.size()) {
            memo.emplace_back(key, nullptr);
            memo_job.push_back(i);
        }
        rep.push_back(m);
    }
    // Distinct keys are planned in parallel: replaying a long stream's control flow is ~0.5 ms of serial
    // f64 arithmetic on one core, and a batch of streams in different states has one replay per stream.  The
    // workers are a process-wide pool (creating a thread costs as much as a tenth of a replay).
    {
        const size_t todo = memo.size();
        std::vector<int> rcs(todo, RSMP_OK);
        std::vector<std::string> msgs(todo);
        auto work = [&](size_t m) {
            FirJob& j = jobs[memo_job[m]];
            rcs[m] = rsmp::plan_job(j.request(), &j.plan);
            if (rcs[m] != RSMP_OK) msgs[m] = rsmp::last_error_slot();   // (the slot is thread local)
            memo[m].second = j.plan;
        };
        if (todo <= 1) {
            if (todo == 1) work(0);
        } else {
            plan_pool().run(todo, work);
        }
        for (size_t m = 0; m < todo; ++m)
            if (rcs[m] != RSMP_OK) {
                rsmp::last_error_slot() = msgs[m];
                return rcs[m];
            }
    }
    for (size_t i = 0; i < n; ++i) {
        FirJob& j = jobs[i];
        j.plan = memo[rep[i]].second;
        if (j.plan->produced_frames * rs[i]->channels > out_caps[i])
            return rsmp::fail(RSMP_ERR_CAPACITY, "bulk output needs %zu values, room for %zu",
                              j.plan->produced_frames * rs[i]->channels, out_caps[i]);
    }
    const auto t_planned = std::chrono::steady_clock::now();
    const int rc = launch_jobs(rs[0], jobs, s, format);
    if (rc != RSMP_OK) return rc;
    if (verbose_t) {
        const auto t_end = std::chrono::steady_clock::now();
        fprintf(stderr, "[rsmp] bulk batch of %zu streams (%zu distinct plans): planning %.3f ms, building and enqueueing the launch %.3f ms\n", n,
                memo.size(), std::chrono::duration<double, std::milli>(t_planned - t_begin).count(),
                std::chrono::duration<double, std::milli>(t_end - t_planned).count());
    }
    for (size_t i = 0; i < n; ++i) {
        if (consumed) consumed[i] = jobs[i].consumed();
        if (produced) produced[i] = jobs[i].produced();
    }
    return RSMP_OK;
}

// Both PCM entries.  Before anything is planned: the arguments (required_bits: the entry's own width, which may not be 0), the format -- the
// widths and the handles' settings as one FirFormat -- against every stream (format_stream_fault; the periodic groups' part of the rule is
// launch_jobs'), one dither mode and statistics for all or none, the PCM buffers' alignment, and at most one launch's worth of input per
// stream.  Then one launch, the buffers under the types of the f32 path (the kernels read the descriptors' in_bits / out_bits).
template <class Out>
int pcm_call(const char* entry, rsmp_fir* const* rs, size_t n, const void* const* d_in, int in_bits, const size_t* in_lens, size_t chunk_len,
             Out* const* d_out, int out_bits, const size_t* out_caps, int required_bits, size_t* consumed, size_t* produced, void* stream) {
    if (n == 0) return RSMP_OK;
    if (!rs || !rs[0] || !d_in || !in_lens || !d_out || !out_caps || chunk_len == 0 || required_bits == 0)
        return rsmp::fail(RSMP_ERR_INVALID_ARGUMENT, "%s: null / zero argument", entry);
    const rsmp::FirFormat f{static_cast<uint32_t>(in_bits), static_cast<uint32_t>(out_bits),   // (the handles' settings: read only where PCM is written)
                            out_bits != 0 ? static_cast<uint32_t>(rs[0]->pcm_dither) : 0u, out_bits != 0 && rs[0]->pcm_stats,
                            out_bits != 0 && rs[0]->pcm_dither == RSMP_DITHER_TPDF ? static_cast<uint32_t>(rs[0]->pcm_dither_shape) : 0u};
    std::vector<const float*> in(n);
    std::vector<float*> out(n);
    for (size_t i = 0; i < n; ++i) {
        if (!rs[i]) return rsmp::fail(RSMP_ERR_INVALID_ARGUMENT, "%s: null stream", entry);
        const size_t ch = rs[i]->channels;
        if (const rsmp::FormatFault fault = rsmp::format_stream_fault(f, ch); fault != rsmp::FormatFault::kNone)
            return rsmp::fail(RSMP_ERR_INVALID_ARGUMENT, "%s", rsmp::format_fault_text(fault));
        if (out_bits != 0 && static_cast<uint32_t>(rs[i]->pcm_dither) != f.dither)
            return rsmp::fail(RSMP_ERR_INVALID_ARGUMENT, "PCM output: one dither mode for all the streams of a batch (rsmp_fir_set_pcm_dither; the seeds may differ)");
        if (out_bits != 0 && f.dither == RSMP_DITHER_TPDF && static_cast<uint32_t>(rs[i]->pcm_dither_shape) != f.dither_shape)
            return rsmp::fail(RSMP_ERR_INVALID_ARGUMENT, "PCM output: one dither shape for all the streams of a batch (rsmp_fir_set_pcm_dither_shape; the seeds may differ)");
        if (out_bits != 0 && rs[i]->pcm_stats != f.stats)
            return rsmp::fail(RSMP_ERR_INVALID_ARGUMENT, "PCM output: statistics for all the streams of a batch or for none (rsmp_fir_set_pcm_stats)");
        if ((in_bits != 0 && reinterpret_cast<uintptr_t>(d_in[i]) % 4 != 0) || (out_bits != 0 && reinterpret_cast<uintptr_t>(d_out[i]) % 4 != 0))
            return rsmp::fail(RSMP_ERR_INVALID_ARGUMENT, "PCM input and output must be 4-byte aligned");
        // (a launch's coefficient rows are mixed for one drift: more input -- 16 minutes of audio -- goes through the f32 entry point, which cuts it)
        if (chunk_len % ch == 0 && in_lens[i] % ch == 0 && in_lens[i] > rsmp::launch_input_values(rs[i]->mirror.ratio(), ch, chunk_len))
            return rsmp::fail(RSMP_ERR_INVALID_ARGUMENT, "%s: more than one launch's worth of input (46 M outputs)", entry);
        in[i] = static_cast<const float*>(d_in[i]);
        out[i] = static_cast<float*>(d_out[i]);
    }
    return batch_bulk_piece(rs, n, in.data(), in_lens, chunk_len, out.data(), out_caps, consumed, produced, stream, f);
}

}  // namespace

// ================================ C ABI ==========================================================
extern "C" int rsmp_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

extern "C" rsmp_fir* rsmp_fir_new_from_hz(size_t channels, uint32_t input_rate_hz,
                                          uint32_t output_rate_hz, int latency, int attenuation,
                                          int device) {
    (void)plan_pool();   // (the planning workers exist from the process's first ResamplerFir on: see PlanPool)
    return fir_create(channels, input_rate_hz, output_rate_hz, latency, attenuation, device);
}

extern "C" rsmp_fir* rsmp_fir_new(size_t channels, int input_rate, int output_rate, int latency,
                                  int attenuation, int device) {
    const uint32_t in_hz = rsmp_sample_rate_hz(input_rate);
    const uint32_t out_hz = rsmp_sample_rate_hz(output_rate);
    if (!in_hz || !out_hz) {
        rsmp::fail(RSMP_ERR_INVALID_ARGUMENT, "ResamplerFir::new: invalid SampleRate value");
        return nullptr;
    }
    (void)plan_pool();
    return fir_create(channels, in_hz, out_hz, latency, attenuation, device);
}

extern "C" void rsmp_fir_free(rsmp_fir* r) { fir_destroy(r); }

extern "C" size_t rsmp_fir_buffer_size_output(const rsmp_fir* r) {
    return r->mirror.buffer_size_output_frames() * r->channels;
}
extern "C" size_t rsmp_fir_delay(const rsmp_fir* r) { return r->taps / 2; }
extern "C" size_t rsmp_fir_channels(const rsmp_fir* r) { return r->channels; }
extern "C" size_t rsmp_fir_taps(const rsmp_fir* r) { return r->taps; }
extern "C" size_t rsmp_fir_phases(const rsmp_fir* r) { (void)r; return rsmp::kPhases; }

extern "C" void rsmp_fir_state(const rsmp_fir* r, size_t* read_position, size_t* available_frames,
                               double* position) {
    if (read_position) *read_position = r->mirror.read_position();
    if (available_frames) *available_frames = r->mirror.available();
    if (position) *position = r->mirror.position();
}

// Puts the stream where a host-only plan stands: the plan's state becomes the handle's and the frames the
// reference would hold buffered at that point (available_frames of them) are taken from the END of
// `history`, the input that precedes the point.  With rsmp_fir_plan_bulk this starts a resampler in the
// middle of a stream -- a long stream is cut at call boundaries and each piece runs on its own GPU with
// the results of the unsharded run (exact position state from the host mirror plus a halo).
extern "C" int rsmp_fir_seek(rsmp_fir* r, const rsmp_fir_plan* p, const float* history, size_t history_len,
                             int history_on_device, void* stream_v) {
    if (!r || !p) return rsmp::fail(RSMP_ERR_INVALID_ARGUMENT, "rsmp_fir_seek: null argument");
    const rsmp::FirMirrorState& s = p->mirror.state();
    if (s.num != r->mirror.num() || s.den != r->mirror.den() || s.taps != r->mirror.taps())
        return rsmp::fail(RSMP_ERR_INVALID_ARGUMENT, "rsmp_fir_seek: the plan is for another rate pair or latency");
    const size_t need = static_cast<size_t>(s.available) * r->channels;
    if (history_len < need || (need && !history))
        return rsmp::fail(RSMP_ERR_INVALID_INPUT_BUFFER_SIZE, "rsmp_fir_seek: %zu values buffered at this point, history holds %zu",
                          need, history_len);
    DeviceGuard guard(r->device);
    hipStream_t stream = stream_v ? static_cast<hipStream_t>(stream_v) : r->stream;
    const FirLaunchEvent* waited = nullptr;
    if (int rc = rsmp::order_behind_handle(r, stream, waited)) return rc;
    if (need) {
        RSMP_HIP_CHECK(hipMemcpyAsync(r->d_hist[r->cur], history + (history_len - need), need * sizeof(float),
                                      history_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, stream));
        if (!history_on_device) RSMP_HIP_CHECK(hipStreamSynchronize(stream));   // the caller's buffer is free on return
    }
    if (int rc = rsmp::record_launch(r, stream)) return rc;
    r->mirror.set_state(s);
    return RSMP_OK;
}

extern "C" void rsmp_fir_reset(rsmp_fir* r) {
    // resampler_fir.rs:638-642: only the three scalars; stale frames are unreachable.
    r->mirror.reset();
    r->pcm_stats_cleared = true;   // (a new stream: its PCM statistics start again -- a flag, nothing is enqueued)
}

extern "C" void rsmp_fir_batch_reset(rsmp_fir* const* rs, size_t n) {
    for (size_t i = 0; i < n; ++i) {
        rs[i]->mirror.reset();
        rs[i]->pcm_stats_cleared = true;
    }
}

extern "C" int rsmp_fir_set_kernel(rsmp_fir* r, int kernel) {
    if (kernel < RSMP_FIR_KERNEL_AUTO || kernel > RSMP_FIR_KERNEL_PERIODIC_F32)
        return rsmp::fail(RSMP_ERR_INVALID_ARGUMENT, "rsmp_fir_set_kernel: unknown kernel %d", kernel);
    r->kernel_mode = kernel;
    return RSMP_OK;
}

// PCM output's dither: a setting of the handle (reset and seek leave it), read when a PCM-output launch is made.
extern "C" int rsmp_fir_set_pcm_dither(rsmp_fir* r, int dither, uint64_t seed) {
    if (!r || (dither != RSMP_DITHER_NONE && dither != RSMP_DITHER_TPDF))
        return rsmp::fail(RSMP_ERR_INVALID_ARGUMENT, "rsmp_fir_set_pcm_dither: null handle or unknown dither mode %d", dither);
    r->pcm_dither = dither;
    r->pcm_dither_seed = seed;
    return RSMP_OK;
}

// ... and its shape: a setting like the mode, read only by a launch whose mode is TPDF.
extern "C" int rsmp_fir_set_pcm_dither_shape(rsmp_fir* r, int shape) {
    if (!r || (shape != RSMP_DITHER_SHAPE_WHITE && shape != RSMP_DITHER_SHAPE_HIGHPASS))
        return rsmp::fail(RSMP_ERR_INVALID_ARGUMENT, "rsmp_fir_set_pcm_dither_shape: null handle or unknown dither shape %d", shape);
    r->pcm_dither_shape = shape;
    return RSMP_OK;
}

extern "C" int rsmp_fir_pcm_dither_shape(const rsmp_fir* r, int* shape) {
    if (!r || !shape) return rsmp::fail(RSMP_ERR_INVALID_ARGUMENT, "rsmp_fir_pcm_dither_shape: null argument");
    *shape = r->pcm_dither_shape;
    return RSMP_OK;
}

// PCM output's gain: a setting like the dither (reset and seek leave it alone), per stream -- the streams of a batch may differ.
// fill_descriptors reads it at every PCM-output launch.
extern "C" int rsmp_fir_set_pcm_gain(rsmp_fir* r, float gain) {
    if (!r || !rsmp::fir_pcm_gain_ok(gain))
        return rsmp::fail(RSMP_ERR_INVALID_ARGUMENT, "rsmp_fir_set_pcm_gain: null handle, or gain not finite with 2^-32 <= |gain| <= 2^32");
    r->pcm_gain = gain;
    return RSMP_OK;
}

extern "C" int rsmp_fir_pcm_gain(const rsmp_fir* r, float* gain) {
    if (!r || !gain) return rsmp::fail(RSMP_ERR_INVALID_ARGUMENT, "rsmp_fir_pcm_gain: null argument");
    *gain = r->pcm_gain;
    return RSMP_OK;
}

extern "C" int rsmp_fir_pcm_dither(const rsmp_fir* r, int* dither, uint64_t* seed) {
    if (!r) return rsmp::fail(RSMP_ERR_INVALID_ARGUMENT, "rsmp_fir_pcm_dither: null handle");
    if (dither) *dither = r->pcm_dither;
    if (seed) *seed = r->pcm_dither_seed;
    return RSMP_OK;
}

// PCM output's statistics: a setting of the handle like the dither; the totals live in device memory (fir_handle.h).
extern "C" int rsmp_fir_set_pcm_stats(rsmp_fir* r, int enable) {
    if (!r) return rsmp::fail(RSMP_ERR_INVALID_ARGUMENT, "rsmp_fir_set_pcm_stats: null handle");
    if (enable && !r->d_pcm_stats.get()) {
        DeviceGuard guard(r->device);
        RSMP_HIP_CHECK(r->d_pcm_stats.reserve(sizeof(rsmp_pcm_stats)));
        r->pcm_stats_cleared = true;   // (the first counting launch writes the totals: no memset)
    }
    r->pcm_stats = enable != 0;
    return RSMP_OK;
}

extern "C" int rsmp_fir_pcm_stats(rsmp_fir* r, rsmp_pcm_stats* stats) {
    if (!r || !stats) return rsmp::fail(RSMP_ERR_INVALID_ARGUMENT, "rsmp_fir_pcm_stats: null argument");
    rsmp_pcm_stats t{};
    if (r->pcm_stats && !r->pcm_stats_cleared && r->d_pcm_stats.get()) {
        DeviceGuard guard(r->device);
        if (r->last_launch) RSMP_HIP_CHECK(hipEventSynchronize(r->last_launch->ev));
        RSMP_HIP_CHECK(hipMemcpy(&t, r->d_pcm_stats.get(), sizeof t, hipMemcpyDeviceToHost));
    }
    *stats = t;
    return RSMP_OK;
}

extern "C" int rsmp_fir_pcm_stats_clear(rsmp_fir* r) {
    if (!r) return rsmp::fail(RSMP_ERR_INVALID_ARGUMENT, "rsmp_fir_pcm_stats_clear: null handle");
    r->pcm_stats_cleared = true;
    return RSMP_OK;
}

extern "C" int rsmp_fir_set_profiling(rsmp_fir* r, int enable) {
    DeviceGuard guard(r->device);
    if (enable && !r->prof_start[0])
        for (int i = 0; i < rsmp_fir::kProfRing; ++i) {
            RSMP_HIP_CHECK(r->prof_start[i].create());
            RSMP_HIP_CHECK(r->prof_stop[i].create());
        }
    r->profiling = enable != 0;
    r->prof_count = 0;
    return RSMP_OK;
}

extern "C" int rsmp_fir_last_kernel_ms(rsmp_fir* r, float* ms) {
    DeviceGuard guard(r->device);
    if (r->prof_count == 0 || !ms)
        return rsmp::fail(RSMP_ERR_INVALID_ARGUMENT, "rsmp_fir_last_kernel_ms: no profiled launch");
    const size_t i = (r->prof_count - 1) % rsmp_fir::kProfRing;
    RSMP_HIP_CHECK(hipEventSynchronize(r->prof_stop[i]));
    RSMP_HIP_CHECK(hipEventElapsedTime(ms, r->prof_start[i], r->prof_stop[i]));
    return RSMP_OK;
}

extern "C" int rsmp_fir_kernel_variant(const rsmp_fir* r) {
    if (!r) return -1;
    if (!r->last_periodic || !r->periodic.geo_valid || !r->periodic.geo.ok) return 0;
    const rsmp::PeriodicGeometry& g = r->periodic.geo;
    return g.mfma == 3 ? (g.planes == 3 ? 4 : 5) : (g.mfma ? 3 : 1);   // (2 is no longer returned)
}

extern "C" int rsmp_fir_mean_kernel_ms(rsmp_fir* r, float* ms, size_t* launches) {
    DeviceGuard guard(r->device);
    if (r->prof_count == 0 || !ms)
        return rsmp::fail(RSMP_ERR_INVALID_ARGUMENT, "rsmp_fir_mean_kernel_ms: no profiled launch");
    const size_t n = r->prof_count < static_cast<size_t>(rsmp_fir::kProfRing) ? r->prof_count : rsmp_fir::kProfRing;
    RSMP_HIP_CHECK(hipEventSynchronize(r->prof_stop[(r->prof_count - 1) % rsmp_fir::kProfRing]));
    double sum = 0.0;
    for (size_t k = 0; k < n; ++k) {
        const size_t i = (r->prof_count - 1 - k) % rsmp_fir::kProfRing;
        float t = 0.f;
        RSMP_HIP_CHECK(hipEventElapsedTime(&t, r->prof_start[i], r->prof_stop[i]));
        sum += t;
    }
    *ms = static_cast<float>(sum / static_cast<double>(n));
    if (launches) *launches = n;
    return RSMP_OK;
}

extern "C" int rsmp_fir_resample_device(rsmp_fir* r, const float* d_in, size_t in_len, float* d_out,
                                        size_t out_len, size_t* consumed, size_t* produced,
                                        void* stream) {
    DeviceGuard guard(r->device);
    // resampler_fir.rs:514-519: input is validated before output.
    if (in_len % r->channels != 0)
        return rsmp::fail(RSMP_ERR_INVALID_INPUT_BUFFER_SIZE, "Input buffer size is invalid");
    if (out_len % r->channels != 0)
        return rsmp::fail(RSMP_ERR_INVALID_OUTPUT_BUFFER_SIZE, "Output buffer size is invalid");
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : r->stream;
    return run_single(r, d_in, in_len, d_out, out_len, 0, consumed, produced, nullptr, 0, nullptr, s);
}

extern "C" int rsmp_fir_resample(rsmp_fir* r, const float* in, size_t in_len, float* out,
                                 size_t out_len, size_t* consumed, size_t* produced) {
    DeviceGuard guard(r->device);
    if (in_len % r->channels != 0)
        return rsmp::fail(RSMP_ERR_INVALID_INPUT_BUFFER_SIZE, "Input buffer size is invalid");
    if (out_len % r->channels != 0)
        return rsmp::fail(RSMP_ERR_INVALID_OUTPUT_BUFFER_SIZE, "Output buffer size is invalid");
    // At most INPUT_CAPACITY frames can be accepted and buffer_size_output-ish produced per
    // call, so the staging buffers are bounded no matter how large the caller's slices are.
    const size_t max_in = rsmp::kInputCapacity * r->channels;
    const size_t stage_in = in_len < max_in ? in_len : max_in;
    const size_t max_out =
        (static_cast<size_t>(static_cast<double>(rsmp::kInputCapacity) / r->mirror.ratio()) + 8) *
        r->channels;
    const size_t stage_out = out_len < max_out ? out_len : max_out;
    // A streaming call is a few kilobytes: two copy-engine transfers and their synchronisation cost more than
    // the kernel.  Small calls therefore go through mapped host memory (cached on the device, visible at kernel
    // boundaries): the CPU copies the caller's slice in, the kernel reads it over the link (once: re-reads hit
    // L2) and writes the output back the same way.
    static const size_t zero_copy_max = [] {
        const char* e = getenv("RSMP_FIR_ZEROCOPY_MAX");   // bytes per direction; 0 disables
        return e ? static_cast<size_t>(atoll(e)) : static_cast<size_t>(256 * 1024);
    }();
    const bool zero_copy = (stage_in + 4) * sizeof(float) <= zero_copy_max && (stage_out + 4) * sizeof(float) <= zero_copy_max;
    return run_staged(r, in, stage_in, out, stage_out, 0, zero_copy, consumed, produced, nullptr, 0, nullptr);
}

extern "C" size_t rsmp_fir_bulk_output_bound(const rsmp_fir* r, size_t in_len, size_t chunk_len) {
    (void)chunk_len;
    // Everything buffered plus everything offered, resampled, plus one frame of slack per call
    // boundary effect; generous but O(in_len).
    const size_t frames = in_len / r->channels + r->mirror.available();
    const size_t out_frames = static_cast<size_t>(static_cast<double>(frames) / r->mirror.ratio()) + 8;
    return out_frames * r->channels;
}

extern "C" int rsmp_fir_resample_bulk_device(rsmp_fir* r, const float* d_in, size_t in_len,
                                             size_t chunk_len, float* d_out, size_t out_cap,
                                             size_t* consumed, size_t* produced, size_t* calls,
                                             size_t max_calls, size_t* n_calls, void* stream) {
    DeviceGuard guard(r->device);
    if (chunk_len == 0)
        return rsmp::fail(RSMP_ERR_INVALID_ARGUMENT, "rsmp_fir_resample_bulk: chunk_len must be > 0");
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : r->stream;
    return run_single(r, d_in, in_len, d_out, out_cap, chunk_len, consumed, produced, calls,
                      max_calls, n_calls, s);
}

extern "C" int rsmp_fir_resample_bulk(rsmp_fir* r, const float* in, size_t in_len, size_t chunk_len,
                                      float* out, size_t out_cap, size_t* consumed, size_t* produced,
                                      size_t* calls, size_t max_calls, size_t* n_calls) {
    DeviceGuard guard(r->device);
    if (chunk_len == 0)
        return rsmp::fail(RSMP_ERR_INVALID_ARGUMENT, "rsmp_fir_resample_bulk: chunk_len must be > 0");
    return run_staged(r, in, in_len, out, out_cap, chunk_len, false, consumed, produced, calls, max_calls, n_calls);
}

extern "C" int rsmp_fir_batch_resample_bulk_device(rsmp_fir* const* rs, size_t n,
                                                   const float* const* d_in, const size_t* in_lens,
                                                   size_t chunk_len, float* const* d_out,
                                                   const size_t* out_caps, size_t* consumed,
                                                   size_t* produced, void* stream) {
    return rsmp_fir_batch_resample_bulk_device_ex(rs, n, d_in, in_lens, chunk_len, d_out, out_caps, consumed, produced, stream, -1, nullptr);
}

extern "C" int rsmp_fir_batch_resample_bulk_device_ex(rsmp_fir* const* rs, size_t n,
                                                      const float* const* d_in, const size_t* in_lens,
                                                      size_t chunk_len, float* const* d_out,
                                                      const size_t* out_caps, size_t* consumed,
                                                      size_t* produced, void* stream, int planner, int* planned_on_device) {
    if (planned_on_device) *planned_on_device = 0;
    if (n == 0) return RSMP_OK;
    if (!rs || !d_in || !in_lens || !d_out || !out_caps || chunk_len == 0)
        return rsmp::fail(RSMP_ERR_INVALID_ARGUMENT, "rsmp_fir_batch_resample_bulk_device: null/zero argument");
    {
        bool any_null = false;
        for (size_t i = 0; i < n; ++i) any_null = any_null || !rs[i];
        int took = 0;
        if (!any_null) {
            const int rc = rsmp::batch_bulk_routed(rs, n, d_in, in_lens, chunk_len, d_out, out_caps, consumed, produced, stream, planner, &took);
            if (took) {
                if (planned_on_device) *planned_on_device = 1;
                return rc;
            }
        }
    }
    // A launch's coefficient rows are mixed for one drift (fir_hostplan.h): a stream offered more than kMaxLaunchOutputs outputs'
    // worth of input takes part in several launches, cut at call boundaries; the others are through after the first.
    std::vector<size_t> piece(n, 0);
    bool cut = false;
    for (size_t i = 0; i < n; ++i) {
        if (!rs[i]) return rsmp::fail(RSMP_ERR_INVALID_ARGUMENT, "rsmp_fir_batch_resample_bulk_device: null stream");
        const size_t ch = rs[i]->channels;
        piece[i] = in_lens[i];
        if (chunk_len % ch != 0 || in_lens[i] % ch != 0) continue;
        const size_t worth = rsmp::launch_input_values(rs[i]->mirror.ratio(), ch, chunk_len);
        if (in_lens[i] > worth) {
            piece[i] = worth;
            cut = true;
        }
    }
    if (!cut) return batch_bulk_piece(rs, n, d_in, in_lens, chunk_len, d_out, out_caps, consumed, produced, stream);
    std::vector<size_t> off(n, 0), made(n, 0);
    std::vector<char> stopped(n, 0);
    for (;;) {
        std::vector<rsmp_fir*> sub_rs;
        std::vector<const float*> sub_in;
        std::vector<float*> sub_out;
        std::vector<size_t> sub_len, sub_cap, idx;
        for (size_t i = 0; i < n; ++i) {
            if (stopped[i] || off[i] >= in_lens[i]) continue;   // (through; a stream offered nothing takes part in no launch)
            idx.push_back(i);
            sub_rs.push_back(rs[i]);
            sub_in.push_back(d_in[i] + off[i]);
            sub_len.push_back(std::min(piece[i], in_lens[i] - off[i]));
            sub_out.push_back(d_out[i] + made[i]);
            sub_cap.push_back(out_caps[i] - made[i]);
        }
        if (idx.empty()) break;
        std::vector<size_t> c(idx.size(), 0), p(idx.size(), 0);
        if (int rc = batch_bulk_piece(sub_rs.data(), idx.size(), sub_in.data(), sub_len.data(), chunk_len, sub_out.data(),
                                      sub_cap.data(), c.data(), p.data(), stream))
            return rc;
        bool progress = false;
        for (size_t k = 0; k < idx.size(); ++k) {
            off[idx[k]] += c[k];
            made[idx[k]] += p[k];
            if (c[k] != sub_len[k]) stopped[idx[k]] = 1;   // (cannot happen in a bulk call; the rest is not offered again)
            progress = progress || c[k] != 0;
        }
        if (!progress) break;
    }
    for (size_t i = 0; i < n; ++i) {
        if (consumed) consumed[i] = off[i];
        if (produced) produced[i] = made[i];
    }
    return RSMP_OK;
}

// The bulk driver loop over a WAV file's samples as they are in the file (resample/src/main.rs:128-137 + :226-254):
// d_pcm[i] = little-endian PCM of `bits` (16 / 24 / 32) per sample, two channels a frame, in_lens[i] SAMPLES; the
// conversion happens where the kernels read their input -- the split kernel's prefetch loads, its edge and wrap-window
// paths, the tail copy, the repair pass -- so the launch reads the PCM alone: rsmp_pcm_to_stereo_f32_device + the f32
// entry point give the same samples with one more pass over HBM (PCM read, f32 written, f32 read).
extern "C" int rsmp_fir_batch_resample_bulk_pcm_device(rsmp_fir* const* rs, size_t n, const void* const* d_pcm, int bits,
                                                       const size_t* in_lens, size_t chunk_len, float* const* d_out,
                                                       const size_t* out_caps, size_t* consumed, size_t* produced, void* stream) {
    return pcm_call("rsmp_fir_batch_resample_bulk_pcm_device", rs, n, d_pcm, bits, in_lens, chunk_len, d_out, 0, out_caps, bits, consumed, produced, stream);
}

// The same with the output as a WAV file stores it: d_out_pcm[i] receives little-endian PCM of `out_bits` (16 / 24 / 32; 24-bit
// packed), every sum quantised where the kernels store it (fir_pcm_quantise_gain with the stream's own gain -- rsmp_fir_set_pcm_gain, 1 by default --, fir_kernels.h) -- the split kernel's pending, full and
// per-frame stores, the generic kernels, the repair pass.  Input: interleaved f32 (in_bits = 0) or PCM as above.  Counts, end states
// and buffered frames (f32) are those of rsmp_fir_batch_resample_bulk_device; the bytes are rsmp_f32_to_pcm_device's of that
// entry's output, without the f32 ever reaching HBM (f32 written, f32 read, PCM written: two passes less).
// Handles set to RSMP_DITHER_TPDF (rsmp_fir_set_pcm_dither; all of a batch or none: the entry refuses a mix) add their noise at
// the same sites, value (frame n of the launch, channel c) with index (abs_out + n) * channels + c -- rsmp_f32_to_pcm_dither_device's
// bytes with the handle's seed and first_index = abs_out * channels.  With rsmp_fir_set_pcm_dither_shape(RSMP_DITHER_SHAPE_HIGHPASS) -- one
// shape for a batch under TPDF -- the noise is the high-pass form: rsmp_f32_to_pcm_shaped_device's bytes with the stream's channels.
// Handles set to count (rsmp_fir_set_pcm_stats; all of a batch or none) take the kernels' counting builds: the same bytes, and
// rsmp_f32_to_pcm_stats's statistics of them in the handles' totals.
// Which streams and launches: format_stream_fault and format_group_fault (fir_geometry.cpp).  Even counts of 4 .. 16 channels are written by the
// split kernel's channel-pair builds a frame of a pair at a time; streams that are planned generic go to the latency kernel at any length.
extern "C" int rsmp_fir_batch_resample_bulk_pcm_out_device(rsmp_fir* const* rs, size_t n, const void* const* d_in, int in_bits,
                                                           const size_t* in_lens, size_t chunk_len, void* const* d_out_pcm, int out_bits,
                                                           const size_t* out_caps, size_t* consumed, size_t* produced, void* stream) {
    return pcm_call("rsmp_fir_batch_resample_bulk_pcm_out_device", rs, n, d_in, in_bits, in_lens, chunk_len, d_out_pcm, out_bits, out_caps, out_bits,
                    consumed, produced, stream);
}
