// fir_launch.cpp -- see fir_launch.h.  launch_jobs at the end of the file reads as the list of its phases; each phase
// works on the launch-local state below.  There is no CPU fallback anywhere in this file.
#include "fir_launch.h"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <map>

#include "common.h"
#include "fir_kernels.h"
#include "fir_periodic.h"

namespace rsmp {

int launch_event(rsmp_fir* leader) {
    if (!leader->launch_ev) {
        auto ev = std::make_shared<FirLaunchEvent>();
        RSMP_HIP_CHECK(hipEventCreateWithFlags(&ev->ev, hipEventDisableTiming));
        leader->launch_ev = std::move(ev);
    }
    return RSMP_OK;
}

int record_launch(rsmp_fir* leader, hipStream_t stream, bool attached) {
    if (int rc = launch_event(leader)) return rc;
    if (!attached) RSMP_HIP_CHECK(event_record(leader->launch_ev->ev, stream));
    if (leader->last_launch != leader->launch_ev) leader->last_launch = leader->launch_ev;
    return RSMP_OK;
}

int order_behind_handle(rsmp_fir* h, hipStream_t stream, const FirLaunchEvent*& waited) {
    if (h->last_stream_valid && h->last_stream != stream && h->last_launch && h->last_launch.get() != waited) {
        RSMP_HIP_CHECK(stream_wait_event(stream, h->last_launch->ev));
        waited = h->last_launch.get();
    }
    h->last_stream = stream;
    h->last_stream_valid = true;
    return RSMP_OK;
}

namespace {

size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// Words of one launch group's non-finite mark region (fir_nonfinite.h): the tag word, then one bit per stream and chunk.
size_t nf_region_words(uint32_t streams, uint32_t chunks) { return 1 + (static_cast<size_t>(streams) * chunks + 31) / 32; }

// Plans are shared, immutable once built; where a plan's arrays sit in THIS launch's workspace is
// launch-local (streams of a batch that share a plan share its arrays too).
struct Placement { size_t seg_off = 0, tile_off = 0, wrap_off = 0; bool written = false; };
struct Group { PeriodicGeometry geo; std::vector<size_t> members; };
// Where the periodic launches mark non-finite sums: one bit per stream and 1024-frame chunk
// (fir_nonfinite.h), one region of the buffer per launch; the repair launches follow the timed ones.
struct Repair { size_t first; uint32_t count; NfArgs nf; };

struct Launch {
    rsmp_fir* const leader;
    std::vector<FirJob>& jobs;
    const hipStream_t stream;
    const FirFormat format;   // (one for the launch: the entry has held every handle to it)
    // A counting launch (format.stats).  st: the launch's table in the leader's d_stat_table, a row of st.chunks entries per stream
    // in launch order; targets_off: the FirStatTarget of every stream, in the workspace behind the plans' arrays.
    FirStatArgs st{nullptr, 0};
    size_t targets_off = 0;
    // (the table from stream `first` of the launch on; none: not counting)
    FirStatArgs stat_rows(size_t first) const { return format.stats ? FirStatArgs{st.table + first * st.chunks * 4, st.chunks} : FirStatArgs{}; }
    const size_t n;
    // launch order: generic jobs, then periodic jobs grouped by geometry (one launch per geometry)
    std::vector<size_t> order;
    size_t n_generic = 0;
    std::vector<Group> groups;
    // workspace: [descs] then per distinct plan: [runs][tile index] or [wraps]
    std::map<const Plan*, Placement> place;
    size_t bytes = 0;
    int slot = 0;
    bool direct = false;   // read by the kernels from mapped host memory, not uploaded
    char* h = nullptr;     // the image as it is assembled, in ordinary host memory
    char* d = nullptr;     // where the kernels will read it
    const FirStreamDesc* d_descs = nullptr;
    uint32_t max_out_generic = 0, max_ch_generic = 0, max_tail_values = 0, max_wraps = 0, max_taps_generic = 0,
             min_ch_generic = 0xFFFFFFFFu, min_taps_generic = 0xFFFFFFFFu;
    double max_ratio_generic = 0.0;
    std::vector<Repair> repairs;
    bool tail_fused = false;   // the last main kernel copies the tails as well: no tail-copy launch
    hipEvent_t done = nullptr;
    bool done_attached = false;
    Launch(rsmp_fir* l, std::vector<FirJob>& j, hipStream_t s, const FirFormat& f) : leader(l), jobs(j), stream(s), format(f), n(j.size()) {}
};

int order_streams(Launch& L) {
    const FirLaunchEvent* waited = nullptr;
    if (int rc = order_behind_handle(L.leader, L.stream, waited)) return rc;
    for (FirJob& j : L.jobs)
        if (int rc = order_behind_handle(j.r, L.stream, waited)) return rc;
    return RSMP_OK;
}

// Bind class tables first (may upload), then order: generic jobs, then periodic jobs grouped
// by geometry (one launch per geometry).
int bind_and_group(Launch& L) {
    std::vector<FirJob>& jobs = L.jobs;
    for (size_t i = 0; i < L.n; ++i)
        if (!jobs[i].plan->periodic) { L.order.push_back(i); ++L.n_generic; }
    for (size_t i = 0; i < L.n; ++i) {
        FirJob& j = jobs[i];
        if (!j.plan->periodic) continue;
        const int rc = periodic_bind(j.r->periodic, j.r->device, *j.r->table, j.r->kernel_mode, j.plan->planned,
                                     0.5 * (j.r->mirror.drift() + j.plan->planned.drift()),
                                     static_cast<uint32_t>(j.r->channels), L.stream);
        if (rc != RSMP_OK) return rc;
        bool found = false;
        for (Group& g : L.groups)
            if (g.geo == j.r->periodic.geo) { g.members.push_back(i); found = true; break; }
        if (!found) L.groups.push_back(Group{j.r->periodic.geo, {i}});
    }
    for (const Group& g : L.groups) for (size_t i : g.members) L.order.push_back(i);
    // PCM in or out: every periodic group needs a build of the split kernel for it (the streams' part of the rule: the entry)
    for (const Group& g : L.groups)
        if (const FormatFault f = format_group_fault(L.format, g.geo); f != FormatFault::kNone)
            return fail(RSMP_ERR_INVALID_ARGUMENT, "%s", format_fault_text(f));
    return RSMP_OK;
}

// Workspace layout: [descs] then per distinct plan: [runs][tile index] or [wraps].
void lay_out_workspace(Launch& L) {
    size_t bytes = align_up(L.n * sizeof(FirStreamDesc), 256);
    for (FirJob& j : L.jobs) {
        const Plan& pl = *j.plan;
        if (L.place.count(&pl)) continue;
        Placement& pp = L.place[&pl];
        if (!pl.periodic) {
            pp.seg_off = bytes;
            bytes = align_up(bytes + pl.segs.size() * sizeof(rsmp_fir_segment), 256);
            pp.tile_off = bytes;
            const size_t tiles = (pl.produced_frames + kFirTile - 1) / kFirTile;
            bytes = align_up(bytes + tiles * sizeof(uint32_t), 256);
        } else {
            pp.wrap_off = bytes;
            const PeriodicGeometry& geo = j.r->periodic.geo;
            const size_t words = geo.inline_wraps
                                     ? periodic_wrap_words(j.r->mirror.abs_out(), static_cast<uint32_t>(pl.produced_frames), geo.den)
                                     : pl.wraps.size();
            bytes = align_up(bytes + words * sizeof(uint32_t), 256);
        }
    }
    if (L.format.stats) {
        L.targets_off = bytes;
        bytes = align_up(bytes + L.n * sizeof(FirStatTarget), 256);
    }
    L.bytes = bytes;
}

// Takes the next slot of the leader's ring and makes room in it; the image is assembled (fill_descriptors) for the
// address the kernels will read it at.
int claim_slot(Launch& L) {
    rsmp_fir* leader = L.leader;
    const int slot = L.slot = leader->plan_slot;
    leader->plan_slot = (slot + 1) % rsmp_fir::kPlanSlots;
    // Small plans (a single call, a handful of streams) are not uploaded at all: the kernels read
    // them from mapped, coherent host memory.  That removes a copy-engine operation and its
    // cross-queue synchronisation (~50 us) from every streaming call.
    L.direct = L.bytes <= 16 * 1024;
    if (L.direct) {
        if (leader->plan_pending[slot]) {  // kernels of the slot's previous launch are done with it
            RSMP_HIP_CHECK(hipEventSynchronize(leader->plan_copied[slot]));
            leader->plan_pending[slot] = false;
        }
        RSMP_HIP_CHECK(leader->h_plan[slot].reserve(16 * 1024));
    } else if (L.bytes > leader->d_plan[slot].capacity()) {
        RSMP_HIP_CHECK(hipStreamSynchronize(L.stream));
        RSMP_HIP_CHECK(leader->d_plan[slot].reserve(L.bytes));
        leader->plan_image[slot].clear();
    }
    // The image is assembled in ordinary host memory first: a launch that repeats an earlier one
    // of this slot (same streams, buffers and state -- e.g. a service resampling batch after batch
    // of equally long files) finds its image already in HBM and skips the upload.
    leader->plan_scratch.assign(L.bytes, 0);
    L.h = leader->plan_scratch.data();
    L.d = L.direct ? leader->h_plan[slot].as<char>() : leader->d_plan[slot].as<char>();
    L.d_descs = reinterpret_cast<const FirStreamDesc*>(L.d);
    return RSMP_OK;
}

// A generic stream's position runs and the index of the run each output tile starts in.
void write_runs(const Plan& pl, const Placement& pp, char* h) {
    std::memcpy(h + pp.seg_off, pl.segs.data(), pl.segs.size() * sizeof(rsmp_fir_segment));
    uint32_t* ts = reinterpret_cast<uint32_t*>(h + pp.tile_off);
    size_t s = 0;
    for (size_t t = 0; t * kFirTile < pl.produced_frames; ++t) {
        const size_t first = t * kFirTile;
        while (first >= static_cast<size_t>(pl.segs[s].out_start) + pl.segs[s].count) ++s;
        ts[t] = static_cast<uint32_t>(s);
    }
}

// A periodic stream's class table and wrapped outputs (bitmap for the kernels with inline wraps, list for the fix-up kernel).
int fill_periodic(Launch& L, const FirJob& j, const Placement& pp, FirStreamDesc& ds) {
    const Plan& pl = *j.plan;
    const rsmp_fir* r = j.r;
    const PeriodicGeometry& geo = r->periodic.geo;
    ds.drift = r->periodic.table_drift;
    ds.class_coef = r->periodic.table.d_coef;
    ds.class_wrap_coef = r->periodic.table.d_wrap_coef;
    ds.class_meta = r->periodic.table.d_meta;
    if (geo.inline_wraps) {
        ds.wrap_bits = reinterpret_cast<const uint32_t*>(L.d + pp.wrap_off);
        // (the split kernel counts periods of b outputs; b = den unless its super period spans several true
        // periods -- exact ratios only, whose streams have no wrapped outputs: an all-zero bitmap, any indexing)
        ds.wrap_k0 = r->mirror.abs_out() / (geo.mfma == 3 ? geo.b : geo.den);
        if (geo.mfma == 3 && geo.b != geo.den && !pl.wraps.empty())
            return fail(RSMP_ERR_INVALID_ARGUMENT, "split kernel: a stream of an exact ratio has wrapped outputs");
        if (!pp.written) {
            const size_t words = periodic_wrap_words(r->mirror.abs_out(), ds.n_out, geo.den);
            if (pl.wrap_bits.size() == words && geo.den == r->mirror.den())
                std::memcpy(L.h + pp.wrap_off, pl.wrap_bits.data(), words * sizeof(uint32_t));
            else
                periodic_fill_wrap_bits(pl.wraps, r->mirror.abs_out(), geo.den, reinterpret_cast<uint32_t*>(L.h + pp.wrap_off), words);
        }
    } else {
        ds.wraps = reinterpret_cast<const uint32_t*>(L.d + pp.wrap_off);
        ds.n_wraps = static_cast<uint32_t>(pl.wraps.size());
        if (!pp.written) std::memcpy(L.h + pp.wrap_off, pl.wraps.data(), pl.wraps.size() * sizeof(uint32_t));
        if (ds.n_wraps > L.max_wraps) L.max_wraps = ds.n_wraps;
    }
    return RSMP_OK;
}

// One descriptor per stream, in launch order, and each distinct plan's arrays once.
int fill_descriptors(Launch& L) {
    FirStreamDesc* descs = reinterpret_cast<FirStreamDesc*>(L.h);
    for (size_t slot = 0; slot < L.n; ++slot) {
        FirJob& j = L.jobs[L.order[slot]];
        const Plan& pl = *j.plan;
        Placement& pp = L.place[&pl];
        rsmp_fir* r = j.r;
        const uint32_t ch = static_cast<uint32_t>(r->channels);
        FirStreamDesc& ds = descs[slot];
        std::memset(&ds, 0, sizeof ds);
        ds.in = j.d_in;
        ds.hist = r->d_hist[r->cur];
        ds.hist_next = r->d_hist[r->cur ^ 1];
        ds.out = j.d_out;
        ds.coeffs = r->d_coeffs;
        ds.n_out = static_cast<uint32_t>(pl.produced_frames);
        ds.hist_frames = static_cast<uint32_t>(pl.hist_frames);
        ds.in_frames = static_cast<uint32_t>(pl.accepted_frames);
        ds.tail_start = static_cast<uint32_t>(pl.consumed_frames);
        ds.tail_frames = static_cast<uint32_t>(pl.planned.available());
        ds.channels = ch;
        ds.taps = static_cast<uint32_t>(r->taps);
        ds.num = static_cast<uint32_t>(r->mirror.num());
        ds.den = static_cast<uint32_t>(r->mirror.den());
        ds.abs_out = r->mirror.abs_out();
        ds.abs_consumed = r->mirror.abs_consumed();
        ds.in_bits = L.format.in_bits;
        ds.out_bits = L.format.out_bits;
        ds.dither = L.format.dither;
        ds.dither_shape = L.format.out_bits != 0 && L.format.dither == RSMP_DITHER_TPDF ? L.format.dither_shape : 0;
        ds.dither_seed = L.format.out_bits != 0 ? r->pcm_dither_seed : 0;
        // (written for every PCM-output launch, whatever was cached: the descriptors are this launch's own, and publish() compares the image)
        ds.pcm_k = L.format.out_bits != 0 ? fir_pcm_gain_scale(r->pcm_gain, L.format.out_bits) : 0.0f;
        if (ds.tail_frames * ch > L.max_tail_values) L.max_tail_values = ds.tail_frames * ch;
        if (!pl.periodic) {
            ds.segs = reinterpret_cast<const rsmp_fir_segment*>(L.d + pp.seg_off);
            ds.n_segs = static_cast<uint32_t>(pl.segs.size());
            ds.tile_seg = reinterpret_cast<const uint32_t*>(L.d + pp.tile_off);
            if (!pp.written) write_runs(pl, pp, L.h);
            if (ds.n_out > L.max_out_generic) L.max_out_generic = ds.n_out;
            if (ch > L.max_ch_generic) L.max_ch_generic = ch;
            if (ch < L.min_ch_generic) L.min_ch_generic = ch;
            if (ds.taps > L.max_taps_generic) L.max_taps_generic = ds.taps;
            if (ds.taps < L.min_taps_generic) L.min_taps_generic = ds.taps;
            L.max_ratio_generic = std::max(L.max_ratio_generic, static_cast<double>(r->in_hz) / static_cast<double>(r->out_hz));
        } else if (int rc = fill_periodic(L, j, pp, ds)) {
            return rc;
        }
        pp.written = true;
        if (L.format.stats) reinterpret_cast<FirStatTarget*>(L.h + L.targets_off)[slot] = FirStatTarget{r->d_pcm_stats.as<rsmp_pcm_stats>(), r->pcm_stats_cleared ? 1u : 0u, 0u};
    }
    return RSMP_OK;
}

// A counting launch's table: a row of chunks per stream, zero before the main kernels (on the launch stream).
int reserve_stat_table(Launch& L) {
    if (!L.format.stats) return RSMP_OK;
    rsmp_fir* leader = L.leader;
    uint32_t max_out = 0;
    for (const FirJob& j : L.jobs)
        if (j.plan->produced_frames > max_out) max_out = static_cast<uint32_t>(j.plan->produced_frames);
    L.st.chunks = (max_out >> kNfChunkShift) + 1;
    const size_t bytes = L.n * L.st.chunks * 4 * sizeof(uint32_t);
    if (bytes > leader->d_stat_table.capacity()) {
        // (as reserve_mark_regions grows d_nf: the leader's earlier launches on ANOTHER stream are ahead of this one already --
        // order_streams made L.stream wait for the handle's launch event --, so L.stream's end is the end of all of them)
        RSMP_HIP_CHECK(hipStreamSynchronize(L.stream));
        RSMP_HIP_CHECK(leader->d_stat_table.reserve(bytes));
    }
    L.st.table = leader->d_stat_table.as<uint32_t>();
    RSMP_HIP_CHECK(hipMemsetAsync(L.st.table, 0, bytes, L.stream));
    return RSMP_OK;
}

// The image reaches the kernels: copied into the mapped slot, uploaded, or -- the slot's HBM holds it already -- neither.
int publish(Launch& L) {
    rsmp_fir* leader = L.leader;
    const int slot = L.slot;
    if (L.direct) {
        std::memcpy(L.d, L.h, L.bytes);
    } else if (leader->plan_image[slot] != leader->plan_scratch) {
        if (leader->plan_pending[slot]) {  // this slot's previous upload must have left pinned memory
            RSMP_HIP_CHECK(hipEventSynchronize(leader->plan_copied[slot]));
            leader->plan_pending[slot] = false;
        }
        RSMP_HIP_CHECK(leader->h_plan[slot].reserve(L.bytes));
        std::memcpy(leader->h_plan[slot].get(), L.h, L.bytes);
        RSMP_HIP_CHECK(hipMemcpyAsync(L.d, leader->h_plan[slot].get(), L.bytes, hipMemcpyHostToDevice, L.stream));
        RSMP_HIP_CHECK(event_record(leader->plan_copied[slot], L.stream));
        leader->plan_pending[slot] = true;
        leader->plan_image[slot].swap(leader->plan_scratch);
    }
    return RSMP_OK;
}

int launch_generic(Launch& L) {
    // a launch made of generic-kernel streams only (a streaming call, a batch of them) lets that kernel copy
    // the tails as well: one launch per call instead of two
    L.tail_fused = L.n_generic == L.n && L.max_out_generic != 0;
    // Latency kernel or tiled kernel, and which build of it: generic_launch_choice (fir_generic_plan.h, fir_geometry.cpp).
    // (RSMP_FIR_GENERIC_BULK=0, debug: the latency kernel for everything.)
    static const bool bulk_on = [] { const char* e = knob("RSMP_FIR_GENERIC_BULK"); return !e || atoi(e) != 0; }();
    if (L.n_generic == 0) return RSMP_OK;
    GenericLaunchRequest rq;
    rq.format = L.format;
    rq.max_out = L.max_out_generic;
    rq.min_channels = L.min_ch_generic;
    rq.max_channels = L.max_ch_generic;
    rq.min_taps = L.min_taps_generic;
    rq.max_taps = L.max_taps_generic;
    rq.max_ratio = L.max_ratio_generic;
    const GenericLaunchChoice choice = generic_launch_choice(rq, bulk_on);
    const FirStatArgs st = L.stat_rows(0);   // (the generic streams are the launch's first)
    if (choice.kernel == GenericKernel::kTiled) {
        L.tail_fused = false;
        RSMP_HIP_CHECK(launch_fir_generic_bulk(L.d_descs, static_cast<uint32_t>(L.n_generic), choice, L.stream, L.format, st));
    } else
        RSMP_HIP_CHECK(launch_fir_generic(L.d_descs, static_cast<uint32_t>(L.n_generic), L.max_out_generic, L.max_ch_generic, L.stream,
                                          L.tail_fused, L.format, st));
    return RSMP_OK;
}

// A region of the leader's mark buffer per group (grown first if need be).
int reserve_mark_regions(Launch& L) {
    rsmp_fir* leader = L.leader;
    size_t nf_words_total = 0;
    for (const Group& g : L.groups) {
        uint32_t max_out = 0;
        for (size_t i : g.members)
            if (L.jobs[i].plan->produced_frames > max_out) max_out = static_cast<uint32_t>(L.jobs[i].plan->produced_frames);
        Repair rp;
        rp.first = 0;
        rp.count = static_cast<uint32_t>(g.members.size());
        rp.nf.chunks = (max_out >> kNfChunkShift) + 1;
        rp.nf.words = reinterpret_cast<uint32_t*>(nf_words_total * sizeof(uint32_t));   // offset for now
        rp.nf.tag = 0;
        nf_words_total += nf_region_words(rp.count, rp.nf.chunks);
        L.repairs.push_back(rp);
    }
    if (nf_words_total * sizeof(uint32_t) > leader->d_nf.capacity()) {
        RSMP_HIP_CHECK(hipStreamSynchronize(L.stream));
        RSMP_HIP_CHECK(leader->d_nf.reserve(nf_words_total * sizeof(uint32_t)));
        RSMP_HIP_CHECK(hipMemsetAsync(leader->d_nf.get(), 0, leader->d_nf.capacity(), L.stream));
    }
    return RSMP_OK;
}

// What the split kernel's item table is a function of (fir_split.hip, split_items_kernel): FNV-1a over it.
uint64_t items_key(const Launch& L, const Group& g, uint32_t max_blocks) {
    uint64_t key = 1469598103934665603ull;
    auto mix = [&](uint64_t v) { for (int b = 0; b < 8; ++b) { key ^= (v >> (8 * b)) & 0xFFu; key *= 1099511628211ull; } };
    mix(g.geo.a); mix(g.geo.b); mix(g.geo.lp); mix(g.geo.groups); mix(max_blocks); mix(g.members.size());
    for (size_t i : g.members) {
        const FirJob& j = L.jobs[i];
        mix(j.r->mirror.abs_out()); mix(j.r->mirror.abs_consumed()); mix(j.plan->produced_frames);
        mix(j.plan->hist_frames); mix(j.plan->accepted_frames); mix(j.r->channels);
    }
    return key ? key : 1;
}

// One launch per geometry -- or, for several rate pairs of the split kernel in one batch, launches they share.
int launch_periodic_groups(Launch& L) {
    rsmp_fir* leader = L.leader;
    if (int rc = reserve_mark_regions(L)) return rc;
    size_t first = L.n_generic, gi = 0;
    std::vector<SplitJob> split_jobs;
    for (const Group& g : L.groups) {
        uint32_t max_blocks = 0;
        for (size_t i : g.members) {
            const uint32_t b = periodic_blocks(g.geo, L.jobs[i].r->mirror.abs_out(), static_cast<uint32_t>(L.jobs[i].plan->produced_frames));
            if (b > max_blocks) max_blocks = b;
        }
        if (!leader->d_work_counter) {
            RSMP_HIP_CHECK(hipMalloc(&leader->d_work_counter, sizeof(unsigned long long)));
            // on the launch stream: a null-stream memset is not ordered with a non-blocking stream and
            // could land after the first kernel had started claiming
            RSMP_HIP_CHECK(hipMemsetAsync(leader->d_work_counter, 0, sizeof(unsigned long long), L.stream));
        }
        // a launch made of split-kernel streams only lets that kernel copy the tails as well
        L.tail_fused = L.n_generic == 0 && L.groups.size() == 1 && g.geo.mfma == 3 && max_blocks != 0;
        Repair& rp = L.repairs[gi++];
        rp.first = first;
        rp.nf.words = leader->d_nf.as<uint32_t>() + reinterpret_cast<size_t>(rp.nf.words) / sizeof(uint32_t);
        if (++leader->nf_tag == 0) leader->nf_tag = 1;
        rp.nf.tag = leader->nf_tag;
        const uint64_t key = items_key(L, g, max_blocks);
        if (L.groups.size() > 1 && g.geo.mfma == 3 && split_groups_may_share(L.format)) {
            // several rate pairs in one batch: those of the split kernel share launches (launch_fir_split_multi: one item
            // table launch, one kernel launch per kernel build among them), as in rsmp_fir_lockstep_run
            split_jobs.push_back(SplitJob{L.d_descs + first, static_cast<uint32_t>(g.members.size()), &g.geo, max_blocks, rp.nf});
        } else {
            RSMP_HIP_CHECK(launch_fir_periodic(L.d_descs + first, static_cast<uint32_t>(g.members.size()), g.geo, max_blocks,
                                               leader->d_work_counter, rp.nf, L.stream, L.tail_fused, key, L.format, L.stat_rows(first)));
        }
        first += g.members.size();
    }
    if (!split_jobs.empty()) RSMP_HIP_CHECK(launch_fir_split_multi(split_jobs.data(), split_jobs.size(), L.stream));
    return RSMP_OK;
}

// The main kernels: generic or generic-bulk, then the periodic groups; timed as one where the leader is profiling.
int launch_main_kernels(Launch& L) {
    rsmp_fir* leader = L.leader;
    if (int rc = reserve_stat_table(L)) return rc;
    if (leader->profiling)
        RSMP_HIP_CHECK(event_record(leader->prof_start[leader->prof_count % rsmp_fir::kProfRing], L.stream));
    if (int rc = launch_generic(L)) return rc;
    if (int rc = launch_periodic_groups(L)) return rc;
    if (leader->profiling) {
        RSMP_HIP_CHECK(event_record(leader->prof_stop[leader->prof_count % rsmp_fir::kProfRing], L.stream));
        ++leader->prof_count;
    }
    return RSMP_OK;
}

// (RSMP_FIR_COUNT_MARKS, debug: how many chunks the launch marked, per launch group)
int dump_marks(const Launch& L) {
    RSMP_HIP_CHECK(hipStreamSynchronize(L.stream));
    for (const Repair& rp : L.repairs) {
        const size_t words = nf_region_words(rp.count, rp.nf.chunks);
        std::vector<uint32_t> h(words);
        RSMP_HIP_CHECK(hipMemcpy(h.data(), rp.nf.words, words * sizeof(uint32_t), hipMemcpyDeviceToHost));
        size_t bits = 0;
        for (size_t w = 1; w < words; ++w) bits += static_cast<size_t>(__builtin_popcount(h[w]));
        fprintf(stderr, "[rsmp] launch group of %u streams x %u chunks: tag word %u (this launch's %u), %zu chunks marked\n", rp.count, rp.nf.chunks,
                h[0], rp.nf.tag, bits);
        for (uint32_t st = 0; st < rp.count && st < 3; ++st) {   // (which: the first streams' chunk numbers)
            fprintf(stderr, "[rsmp]   stream %u:", st);
            for (uint32_t c = 0; c < rp.nf.chunks; ++c) {
                const size_t bit = static_cast<size_t>(st) * rp.nf.chunks + c;
                if (h[1 + (bit >> 5)] >> (bit & 31) & 1u) fprintf(stderr, " %u", c);
            }
            fprintf(stderr, "\n");
        }
    }
    return RSMP_OK;
}

// Repair, wrap fix-up, tail copy -- and the leader's launch event, completed by whichever comes last.
int launch_followups(Launch& L) {
    rsmp_fir* leader = L.leader;
    const size_t n = L.n, n_generic = L.n_generic;
    // (RSMP_FIR_NO_REPAIR, debug: what the periodic kernels wrote, without the repair pass -- tools/repair_probe.py)
    static const bool no_repair = knob("RSMP_FIR_NO_REPAIR") != nullptr;
    static const bool count_marks = knob("RSMP_FIR_COUNT_MARKS") != nullptr;
    if (count_marks)
        if (int rc = dump_marks(L)) return rc;
    if (no_repair) L.repairs.clear();
    // The handle's launch event (a later call on another stream waits for it) is completed by the LAST of the launches below
    // itself -- hipExtLaunchKernel's stop event: an event record of its own between two launches of 64 streams cost their
    // step 2-4 % --; where there is no such launch, or the stream is the legacy handle (which an event must not carry,
    // common.h), it is recorded behind them.
    if (int rc = launch_event(leader)) return rc;
    const bool wrap_last = n > n_generic && L.max_wraps > 0 && L.tail_fused;
    // (a counting launch: the fold behind the repair pass takes the repair pass's place as the last launch)
    const bool fold_last = L.format.stats && L.tail_fused && !wrap_last;
    const bool repair_last = L.tail_fused && !wrap_last && !L.format.stats;
    L.done = L.stream != reinterpret_cast<hipStream_t>(RSMP_STREAM_LEGACY) ? leader->launch_ev->ev : nullptr;
    if (L.repairs.size() > 1) {
        std::vector<RepairJob> rj;
        for (const Repair& rp : L.repairs) rj.push_back(RepairJob{L.d_descs + rp.first, rp.count, rp.nf, static_cast<uint32_t>(rp.first)});
        RSMP_HIP_CHECK(launch_fir_repair_multi(rj.data(), rj.size(), L.stream, nullptr, 0, 0, repair_last ? L.done : nullptr,
                                               &L.done_attached, L.format, L.st));
    } else {
        for (const Repair& rp : L.repairs)
            RSMP_HIP_CHECK(launch_fir_repair(L.d_descs + rp.first, rp.count, rp.nf, L.stream, repair_last ? L.done : nullptr,
                                             &L.done_attached, L.format, L.stat_rows(rp.first)));
    }
    if (L.format.stats)
        RSMP_HIP_CHECK(launch_fir_pcm_stats_fold(L.st, static_cast<uint32_t>(n), reinterpret_cast<const FirStatTarget*>(L.d + L.targets_off),
                                                 L.stream, fold_last ? L.done : nullptr, &L.done_attached));
    if (n > n_generic && L.max_wraps > 0)
        RSMP_HIP_CHECK(launch_fir_wrap_fixup(L.d_descs + n_generic, static_cast<uint32_t>(n - n_generic), L.max_wraps, L.stream,
                                             wrap_last ? L.done : nullptr, &L.done_attached));
    if (!L.tail_fused)
        RSMP_HIP_CHECK(launch_fir_tail_copy(L.d_descs, static_cast<uint32_t>(n), L.max_tail_values, L.stream, L.done, &L.done_attached));
    if (L.direct) {   // the slot may be rewritten once these kernels have read it
        RSMP_HIP_CHECK(event_record(leader->plan_copied[L.slot], L.stream));
        leader->plan_pending[L.slot] = true;
        leader->plan_image[L.slot].clear();
    }
    return record_launch(leader, L.stream, L.done_attached);
}

// Commit: the mirrors advance, the hist buffers swap.
void commit(Launch& L) {
    for (FirJob& j : L.jobs) {
        j.r->last_periodic = j.plan->periodic;
        j.r->mirror = j.plan->planned;
        j.r->cur ^= 1;
        if (L.format.stats) j.r->pcm_stats_cleared = false;   // (the fold has written the handle's totals)
        if (j.r->last_launch != L.leader->launch_ev) j.r->last_launch = L.leader->launch_ev;   // (no reference count traffic per launch)
    }
}

}  // namespace

int launch_jobs(rsmp_fir* leader, std::vector<FirJob>& jobs, hipStream_t stream, const FirFormat& format) {
    Launch L(leader, jobs, stream, format);
    if (int rc = order_streams(L)) return rc;
    if (int rc = bind_and_group(L)) return rc;
    lay_out_workspace(L);
    if (int rc = claim_slot(L)) return rc;
    if (int rc = fill_descriptors(L)) return rc;
    if (int rc = publish(L)) return rc;
    if (int rc = launch_main_kernels(L)) return rc;
    if (int rc = launch_followups(L)) return rc;
    commit(L);
    return RSMP_OK;
}

}  // namespace rsmp
