// fir_lockstep_geometry.cpp -- the host rules of the lock-step batch (fir_lockstep_plan.h): the geometry of a step, the cut
// of a class into workgroups and their order, and what the run planner's kernels are launched with.  Pure functions of
// their arguments and of debug switches read once.  Plain C++: no runtime header, compiled by a host compiler for the
// stand-alone tests (tests/host).
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "errors.h"
#include "fir_lockstep_plan.h"

namespace rsmp {

LockstepGeometry lockstep_geometry(uint64_t num, uint64_t den, double ratio, uint32_t taps,
                                   uint32_t channels, uint32_t step_frames, bool allow_split) {
    static const bool exact_knob = [] { const char* e = rsmp::knob("RSMP_LS_EXACT"); return e && atoi(e) != 0; }();
    LockstepGeometry g;
    g.taps = taps;
    g.num = static_cast<uint32_t>(num);
    g.den = static_cast<uint32_t>(den);
    // With out_cap >= buffer_size_output a step never leaves more than taps - 1 frames buffered, and
    // it produces at most (buffered + new - taps + 1) / ratio + 1 frames.
    g.span_frames = taps + step_frames + 8;
    g.max_out = static_cast<uint32_t>(std::ceil(static_cast<double>(step_frames + 8) / ratio)) + 2;
    g.wrap_words = (g.max_out + 31) / 32;
    auto finish = [&](bool periodic) -> bool {
        g.periodic = periodic;
        if (!periodic) {
            g.r = g.a = 0;
            g.b = 1;
            g.row_len = g.n_tiles = 0;
            g.guard_frames = 0;
            g.region_frames = g.span_frames + 64;   // (the last staging piece may run 63 dwords past the span)
            g.cols_per_stream = 1;
            g.wrap_cap = 1;
        }
        const uint32_t want = periodic ? std::max(1u, 16u / g.cols_per_stream) : 4u;
        for (uint32_t s = std::min(want, kLsMaxSlots); s >= 1; --s) {
            const uint32_t bytes = ls_layout(s, s * g.cols_per_stream, g.wrap_words, g.wrap_cap,
                                             ls_data_bytes(g.split, g.rows, g.row_bytes, s, g.region_frames, channels)).total;
            // Two workgroups per CU: 80 KB each.  One dynamic LDS size serves the whole launch, so a group above
            // that would halve the occupancy of every group: a split image that does not fit makes way for the
            // exact-f32 layout (which drops to one stream per workgroup before it gives up on that).
            if (g.split && s * g.cols_per_stream > 16) continue;   // one image = 16 columns (a long step of a high ratio has more: f32 layout)
            if (bytes <= (s > 1 || g.split ? kLsLdsPerWorkgroup : kLsLdsLimit)) {
                g.slots = s;
                g.max_cols = s * g.cols_per_stream;
                g.lds_bytes = bytes;
                return true;
            }
        }
        return false;
    };
    if (num != 0 && den != 0 && num <= (1u << 20) && den <= (1u << 20)) {
        const uint32_t shift = static_cast<uint32_t>((15 * num + den - 1) / den);
        g.split = allow_split && !exact_knob && channels == 2;
        g.row_len = g.split ? (taps + shift + 31) / 32 * 32 : (taps + shift + 15) / 16 * 16;
        uint64_t r = (96 + den - 1) / den;
        if (r == 0) r = 1;
        const uint64_t a = num * r, b = den * r;
        if (a <= 8192 && b <= 65536 && g.row_len <= 16 * kLsMaxBlk) {
            g.r = static_cast<uint32_t>(r);
            g.a = static_cast<uint32_t>(a);
            g.b = static_cast<uint32_t>(b);
            g.n_tiles = (g.b + 15) / 16;
            g.guard_frames = g.a + (g.a & 1u);
            g.region_frames = g.guard_frames + g.span_frames + g.a + g.row_len;
            g.region_frames += g.region_frames & 1u;
            g.cols_per_stream = (g.max_out - 1) / g.b + 2;
            g.wrap_cap = g.max_out / g.den + 2;
            g.rows = static_cast<uint32_t>((static_cast<uint64_t>(g.n_tiles - 1) * 16 * g.a) / g.b) + g.row_len;
            g.row_bytes = kLsImageRowBytes;
            if (finish(true)) return g;
            if (g.split) {   // without the rows' padding (transposed reads then meet on banks: 2-4x the LDS time of a unit, still far below f32 products)
                g.row_bytes = kLsImageRowBytesPacked;
                if (finish(true)) return g;
            }
            if (g.split) {   // the image does not fit: exact-f32 layout
                g.split = false;
                g.row_len = (taps + shift + 15) / 16 * 16;
                if (g.row_len <= 16 * kLsMaxBlk && finish(true)) return g;
            }
        }
    }
    g.split = false;
    if (!finish(false)) g.lds_bytes = 0;   // caller reports the failure
    return g;
}

PeriodicGeometry lockstep_class_geometry(const LockstepGeometry& g) {
    PeriodicGeometry p;
    p.ok = g.periodic;
    p.a = g.a;
    p.b = g.b;
    p.den = g.den;
    p.taps = g.taps;
    p.row_len = g.row_len;
    p.n_tiles = g.n_tiles;
    p.mfma = g.split ? 3 : 1;   // A-operand order of v_mfma_f32_16x16x4_f32, or the split table of fir_split.hip
    p.planes = g.split ? 2 : 0;
    p.inline_wraps = false;
    return p;
}

LsCutMax lockstep_cut_groups(std::vector<LockstepGroup>& groups, const LockstepGeometry& geo, uint32_t channels, size_t first, size_t end,
                             const float* class_coef, const TileMeta* class_meta, uint32_t class_index) {
    LsCutMax most{0, 0};
    for (; first < end; first += geo.slots) {
        LockstepGroup g;
        std::memset(&g, 0, sizeof g);
        g.first = static_cast<uint32_t>(first);
        g.count = static_cast<uint32_t>(std::min<size_t>(geo.slots, end - first));
        g.channels = channels;
        g.taps = geo.taps;
        g.periodic = geo.periodic ? 1u : 0u;
        g.num = geo.num;
        g.den = geo.den ? geo.den : 1u;
        g.a = geo.a;
        g.b = geo.b ? geo.b : 1u;
        g.row_len = geo.row_len;
        g.n_tiles = geo.n_tiles;
        g.guard_frames = geo.guard_frames;
        g.span_frames = geo.span_frames;
        g.region_frames = geo.region_frames;
        g.max_out = geo.max_out;
        g.wrap_words = geo.wrap_words;
        g.wrap_cap = geo.wrap_cap;
        g.max_cols = geo.max_cols;
        g.class_coef = class_coef;
        g.class_meta = class_meta;
        g.lds_bytes = geo.lds_bytes;
        g.slots = geo.slots;
        g.split = geo.split ? 1u : 0u;
        g.rows = geo.rows;
        g.row_bytes = geo.row_bytes;
        g.pad0 = class_index;
        groups.push_back(g);
        most.lds_bytes = std::max(most.lds_bytes, geo.lds_bytes);
        most.rec_stride = std::max(most.rec_stride, lockstep_rec_stride(geo.wrap_cap));
    }
    return most;
}

// With more workgroups than CUs (two fit a CU) number k + CUs becomes the second tenant of the CU that took number k.  The
// slow geometries first and the quick ones last pairs each slow workgroup with a quick one (or leaves it alone, see below)
// instead of with its own kind -- a step ends with its slowest workgroup, and two slow tenants slow each other
// (`tools/ls_trace.py`: the 20-tile and the 505-row images end at 46-52 k cycles, the one-stream 48 -> 96 kHz ones at 27 k).
// Cost: matrix units + rows to stage, a packed image's bank conflicts on top.
void lockstep_order_groups(std::vector<LockstepGroup>& groups, uint32_t cus) {
    auto cost = [](const LockstepGroup& g) {
        const double units = static_cast<double>(g.n_tiles) * ((g.max_cols + 15) / 16);
        return units + g.count * (g.split ? g.rows : g.region_frames) / 64.0 + (g.split && g.row_bytes == kLsImageRowBytesPacked ? 10.0 : 0.0);
    };
    std::stable_sort(groups.begin(), groups.end(), [&](const LockstepGroup& x, const LockstepGroup& y) { return cost(x) > cost(y); });
    // ... and the slowest of all ALONE: with n workgroups on c CUs the indices n - c .. c - 1 get no second tenant, so the
    // order is [next slowest: first tenants][slowest: alone][quickest: second tenants] (0.0184 -> 0.0181 ms per step)
    const size_t n = groups.size(), c = cus;
    if (n > c && n < 2 * c) {
        const size_t second = n - c, alone = c - second;
        std::vector<LockstepGroup> o;
        o.insert(o.end(), groups.begin() + alone, groups.begin() + alone + second);
        o.insert(o.end(), groups.begin(), groups.begin() + alone);
        o.insert(o.end(), groups.begin() + alone + second, groups.end());
        groups.swap(o);
    }
}

uint32_t lockstep_plan_pack(size_t n_streams) {
    static const uint32_t knob = [] { const char* e = rsmp::knob("RSMP_LS_PACK"); const int v = e ? atoi(e) : 0; return v == 1 || v == 2 || v == 4 ? static_cast<uint32_t>(v) : 0u; }();
    if (n_streams >= kLsPlanPackBelow) return 1u;
    return knob ? knob : kLsPlanPack;
}

LsPlanShape lockstep_plan_shape(size_t n_streams, uint32_t k) {
    static const bool pchain = [] { const char* e = rsmp::knob("RSMP_LS_PCHAIN"); return !e || atoi(e) != 0; }();
    const uint32_t n = static_cast<uint32_t>(n_streams);
    LsPlanShape s;
    s.k1_blocks_per_stream = (k + 255) / 256;
    s.k1_grid = s.k1_blocks_per_stream * n;
    s.pack = lockstep_plan_pack(n_streams);
    s.k2_grid = (n + s.pack - 1) / s.pack;
    s.k2_block = 64 * s.pack;
    // (the replay: a wave per chunk of 64 calls for small batches, one wave per stream otherwise)
    s.k3_waves = s.pack > 1 ? std::min<uint32_t>(kLsWrapWaves, (k + 63) / 64) : 1u;
    s.parallel_chain = pchain ? 1u : 0u;
    s.chain_cus = s.pack > 1 ? s.k2_grid : static_cast<uint32_t>((n_streams + 3) / 4);
    s.replay_cus = s.pack > 1 ? static_cast<uint32_t>((n_streams * s.k3_waves + 15) / 16) : 0u;
    return s;
}

}  // namespace rsmp
