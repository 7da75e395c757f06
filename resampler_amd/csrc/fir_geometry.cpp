// fir_geometry.cpp -- the geometry of a periodic FIR launch for a rate pair (which kernel family, how its LDS is laid
// out), the rules the host planner asks about, and which build of a kernel runs a geometry.  Pure functions of their
// arguments and of debug switches read once.  Plain C++: includes no HIP header and is compiled by a host compiler for
// the stand-alone tests (tests/host); the numbers it shares with the kernels come from the two *_consts.h headers and
// fir_generic_plan.h.
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "errors.h"
#include "fir_generic_plan.h"
#include "fir_periodic_consts.h"
#include "fir_periodic_plan.h"
#include "fir_split_consts.h"

namespace rsmp {

namespace {
// RSMP_FIR_MFMA: 0 = vector kernels only; 1 / 2 / 4 = exact-f32 matrix-core kernel with that many 16-period
// groups per work unit; 3 (default) = split-bf16 matrix kernel (fir_split.hip) where its geometry exists,
// else as 2.  Two interleaved channels only.
int mfma_knob() {
    static const int knob = [] {
        const char* e = rsmp::knob("RSMP_FIR_MFMA");
        return e ? atoi(e) : 3;
    }();
    return knob;
}
// RSMP_FIR_SPLIT_PLANES = 3 selects the three-plane bf16 split (every f32 operand exactly), default 2: two
// fp16 planes per operand, three matrix products instead of six.
uint32_t split_planes_knob() {
    static const uint32_t v = [] {
        const char* e = rsmp::knob("RSMP_FIR_SPLIT_PLANES");
        return e && atoi(e) == 3 ? 3u : 2u;
    }();
    return v;
}
}  // namespace

bool mfma_ring_knob() {
    static const bool forced = rsmp::knob("RSMP_FIR_MFMA_RING") != nullptr;
    return forced;
}

// Geometry of the split kernel for num/den, or !ok.  A super period of a = r num input frames and b = r den outputs:
// r = 1 for 16 .. 320 classes; a ratio with a power-of-two denominator below 16 (48 <-> 96 kHz: exact in f64, so no
// output ever takes the row-1023 variant and every class of the super period is an ordinary one) takes the largest r
// with a, b <= 320.  Up to ten class tiles per tile group (one tile per consumer wave), up to two groups; periods of up
// to 160 frames in one round of lane tasks, up to 320 in two (two-channel streams); window of <= 160 taps (192 with
// two rounds); two to four images within the LDS.
PeriodicGeometry split_geometry(uint64_t num, uint64_t den, uint32_t taps, uint32_t channels) {
    PeriodicGeometry g;
    // (three planes: the two-channel kernel only -- the channel-pair, one-channel and odd-count builds keep two)
    const uint32_t planes = channels == 2 ? split_planes_knob() : 2u;
    const uint32_t kRowBytes = row_bytes(static_cast<int>(planes));
    // two channels, or (RSMP_FIR_SPLIT_WIDE=0 turns it off) an even number up to 16 taken as channel pairs, two pairs per
    // 16-byte load (6, 10, 14 channels: the last pair alone -- its load reaches 8 bytes into the next frame)
    static const bool wide_ok = [] { const char* e = rsmp::knob("RSMP_FIR_SPLIT_WIDE"); return !e || atoi(e) != 0; }();
    static const bool long_ok = [] { const char* e = rsmp::knob("RSMP_FIR_SPLIT_LONG"); return !e || atoi(e) != 0; }();   // 0: round 2's geometries only
    if (channels != 2 && (channels > 16 || !wide_ok)) return g;
    constexpr uint32_t kMaxAB = kSplitMaxAB;
    if (num == 0 || den == 0 || num > kMaxAB || den > kMaxAB) return g;
    uint32_t r = 1;
    if (den < 16) {
        if ((den & (den - 1)) != 0) return g;   // (the wrap variant exists for class 0 only: exact ratios need none)
        r = static_cast<uint32_t>(std::min(kMaxAB / num, kMaxAB / den));
        r -= r % (16 / static_cast<uint32_t>(den));   // whole tiles
        if (r == 0) return g;
    }
    const uint32_t a = static_cast<uint32_t>(num) * r, b = static_cast<uint32_t>(den) * r;
    if (b < 16) return g;
    const uint32_t n_tiles = (b + 15) / 16;
    const uint32_t groups = (n_tiles + kConsumers - 1) / kConsumers;
    const uint32_t rounds = split_lane_tasks(a) > split_task_room(1) ? 2u : 1u;
    if (!long_ok && (groups > 1 || rounds > 1 || r > 1)) return g;
    if (groups > 2 || (rounds == 2 && (channels % 2 != 0 || planes != 2))) return g;   // (two rounds: channel pairs, fp16 planes)
    uint32_t shift = 0, ob_max = 0;
    for (uint32_t t = 0; t < n_tiles; ++t) {
        const uint32_t ob = class_offset(a, b, 16 * t);
        if (ob > ob_max) ob_max = ob;
        for (uint32_t i = 0; i < 16 && 16 * t + i < b; ++i) {
            const uint32_t s = class_offset(a, b, 16 * t + i) - ob;
            if (s > shift) shift = s;
        }
    }
    const uint32_t kpad = (taps + shift + 31) / 32 * 32;
    if (kpad / 32 < 1 || kpad / 32 > (rounds == 2 ? 6u : 5u) || taps > 16 * kWrapTaps) return g;
    if (rounds == 2 && kpad / 32 < 5) return g;   // (the two-round kernels exist for windows of 160 and 192 taps: 128-tap filters)
    // Rows a plane really needs: the last tile's window ends at ob_max + taps + shift.  The MFMA steps read
    // on to ob_max + kpad with zero coefficients -- into the rows that follow in LDS (the next plane, the next
    // image, the pad after the last image: always finite values, the whole LDS is zeroed at the start).
    const uint32_t rows = ob_max + taps + shift;
    if (split_lane_tasks(a) > split_task_room(rounds) || rows < a || rows > 2 * a) return g;   // (rows beyond a repeat the next period)
    const uint32_t pad = (kpad - (taps + shift)) * kRowBytes;
    uint32_t slots = (kLdsLimit - kImageBase - pad) / (rows * kRowBytes);   // ring of images: slack between producers and consumers
    if (slots > 4) slots = 4;
    if (slots < 2) return g;
    const uint32_t lds = kImageBase + slots * rows * kRowBytes + pad;
    g.a = a;
    g.b = b;
    g.den = static_cast<uint32_t>(den);   // the true period of the phase pattern (b = r den)
    g.taps = taps;
    g.row_len = kpad;
    g.n_tiles = n_tiles;
    g.n_units = n_tiles;
    g.cg = channels == 1 ? 1 : (channels % 2 ? 3 : 2);   // (1: one channel, a pair with a phantom second channel; 3: odd count, the last pair likewise)
    g.lp = (channels + 1) / 2;      // channel pairs of a frame (an item of the launch = one pair of a block)
    g.pw = 16;
    g.row_stride = rows;       // rows of an image (frames of a period + window reach)
    g.waves = kWaves;
    g.producers = kProducers;
    g.images = slots;
    g.mfma = 3;
    g.planes = planes;
    g.groups = groups;
    g.rounds = rounds;
    g.lds_bytes = lds;
    g.inline_wraps = true;
    g.ok = true;
    return g;
}

namespace {
PeriodicGeometry geometry_for(uint64_t num, uint64_t den, uint32_t taps, uint32_t channels,
                              bool want_mfma) {
    PeriodicGeometry g;
    if (num == 0 || den == 0 || channels == 0 || channels > 64) return g;
    if (num > (1u << 20) || den > (1u << 20)) return g;
    const int knob_mfma = mfma_knob() == 3 ? 2 : mfma_knob();   // 3: this is the fallback of the split kernel
    const uint32_t ct = want_mfma ? kMfmaClassTile : kClassTile;
    // max in-tile shift: off(j) = floor(j*num/den); tiles start at multiples of the class tile.
    const uint32_t shift = static_cast<uint32_t>(((ct - 1) * num + den - 1) / den);
    g.taps = taps;
    g.den = static_cast<uint32_t>(den);
    // whole 8-tap chunks (fir_periodic_kernel) / three blocks of four 4-tap MFMA steps
    g.row_len = want_mfma ? (taps + shift + 47) / 48 * 48 : (taps + shift + 7) / 8 * 8;
    // super period: a >= row_len (a window spans at most two rows) and b >= one class tile
    uint64_t r = (g.row_len + num - 1) / num;
    if (den * r < ct) r = (ct + den - 1) / den;
    const uint64_t a = num * r, b = den * r;
    if (a > 4096 || b > (1u << 16)) return g;
    g.a = static_cast<uint32_t>(a);
    g.b = static_cast<uint32_t>(b);
    g.n_tiles = (g.b + ct - 1) / ct;
    g.n_units = g.n_tiles;
    // wrap variant inside the kernel: vector kernels den >= 8 (one wrap class per 8-class tile at
    // most); matrix-core path den >= 16 and at most kMfmaWrapMax wrap classes per super period
    // (only the register-resident variant picks the results up: windows <= 144 taps, 1-2 groups/unit)
    // (144 taps at most: with a 192-tap tile in registers the register-resident build spilled)
    const bool mfma_regs = want_mfma && knob_mfma <= 2 && g.row_len <= 144 && !mfma_ring_knob();
    g.inline_wraps = want_mfma ? (mfma_regs && den >= kMfmaClassTile && r <= kMfmaWrapMax) : den >= kClassTile;

    bool two_per_cu = false;   // set by fit(): the single-image vector kernel with two workgroups per CU
    auto fit = [&](uint32_t cg) -> bool {
        two_per_cu = false;
        if (channels % cg != 0) return false;
        const uint32_t lp = channels / cg;
        if (lp > 64) return false;
        const uint32_t pw_max = 64 / lp;
        // odd number of frames per row: the lane stride then hits every LDS bank once (and with two
        // channels per lane, 2 * odd dwords keeps every lane's ds_read_b64 8-byte aligned)
        const uint32_t stride = (g.a | 1u) * channels;
        const uint32_t stride_bytes = stride * 4;
        const uint32_t fixed = (64 * channels + 16) * 4;  // xprev
        auto rows_in = [&](uint32_t budget) -> uint32_t {
            if (budget <= fixed + 2 * stride_bytes) return 0;
            return (budget - fixed) / stride_bytes - 1;
        };
        g.cg = cg;
        g.lp = lp;
        g.row_stride = stride;
        if (want_mfma) {
            // Two images in one workgroup (fir_periodic_db_kernel), if that keeps >= 75 % of the lanes
            // busy; else periodic_geometry() retries with the vector kernels.  Per image: + 96 floats of
            // read-ahead padding + the wrap results.  (A ring of four 32-period images, one per producer,
            // measured equal: the doubled per-item work ate what the extra slack gained.  The same
            // workgroup around the vector tile code measured slower than two single-image workgroups
            // per CU: 12 consumer waves cannot hide the scalar-cache latency that 24 can.)
            auto db_bytes = [&](uint32_t pw) -> uint32_t {
                return (kDbCtrlWords + 2 * (db_image_len(xprev_len_of(pw, channels), pw, stride) + mfma_wrap_words(pw))) * 4;
            };
            uint32_t pw = pw_max;
            while (pw * 4 >= pw_max * 3 && db_bytes(pw) > kLdsMax) --pw;
            if (pw * 4 < pw_max * 3) return false;
            g.images = 2;
            g.pw = pw;
            g.producers = 4;
            g.lds_bytes = db_bytes(pw);
            g.mfma = static_cast<uint32_t>(knob_mfma);
            // a work unit spans knob_mfma groups of 16 periods
            const uint32_t groups = (pw + 15) / 16;
            g.n_units = g.n_tiles * ((groups + g.mfma - 1) / g.mfma);
            // 4 producers + 8 consumers: two consumer waves per SIMD keep the matrix pipe busy, more only
            // add arbitration (and 12 waves are the __launch_bounds__(768) of the kernel)
            g.waves = 12;
            return true;
        }
        uint32_t pw = rows_in(kLdsTwoPerCu);
        two_per_cu = pw * 4 >= pw_max * 3;
        if (!two_per_cu) pw = rows_in(kLdsMax);  // < 75% of the lanes: use the whole LDS
        if (pw > pw_max) pw = pw_max;
        if (pw * 2 < pw_max || pw == 0) return false;
        g.pw = pw;
        g.producers = 0;
        g.lds_bytes = (xprev_len_of(pw, channels) + (pw + 1) * stride) * 4;
        // waves per workgroup: a multiple of the 4 SIMDs, at most 12 (__launch_bounds__(768, 6));
        // tiles are claimed dynamically, so the count need not divide n_tiles
        g.waves = g.n_tiles >= 12 ? 12u : (g.n_tiles >= 8 ? 8u : 4u);
        return true;
    };
    if (want_mfma) {   // the matrix-core kernel is written for two channels per lane group
        if (!fit(2)) return g;
    } else {
        // Two channels per lane make every v_pk_fma_f32 count twice, but with many channels a period row is long
        // and only one single-image workgroup fits a CU -- staging and arithmetic then take turns.  One channel per
        // lane halves the periods per image: where that is what lets two workgroups share a CU it is faster
        // (8 channels 96 -> 44.1 kHz: 0.73 -> 0.62 ms per 20 M frames).
        const bool ok2 = fit(2);
        if (!ok2 || !two_per_cu) {
            const PeriodicGeometry g2 = g;
            if (!(fit(1) && (two_per_cu || !ok2))) {
                if (!ok2) return g;
                g = g2;
            }
        }
    }
    g.ok = true;
    return g;
}
}  // namespace

PeriodicGeometry periodic_geometry(uint64_t num, uint64_t den, uint32_t taps, uint32_t channels,
                                   bool allow_matrix, bool allow_split) {
    int knob = mfma_knob();
    if (knob == 3) {   // split-bf16 matrix kernel where its geometry exists
        if (allow_matrix && allow_split) {
            const PeriodicGeometry g = split_geometry(num, den, taps, channels);
            if (g.ok) return g;
        }
        knob = 2;
    }
    if (allow_matrix && channels == 2 && (knob == 1 || knob == 2 || knob == 4)) {
        const PeriodicGeometry g = geometry_for(num, den, taps, channels, true);
        if (g.ok) return g;   // else: two images do not fit the LDS for this rate pair
    }
    return geometry_for(num, den, taps, channels, false);
}

bool periodic_supported(const FirMirror& m, size_t channels, size_t taps, int kernel_mode) {
    if (kernel_mode == RSMP_FIR_KERNEL_GENERIC) return false;
    if (!m.periodic_ok()) return false;
    return periodic_geometry(m.num(), m.den(), static_cast<uint32_t>(taps), static_cast<uint32_t>(channels),
                             kernel_mode != RSMP_FIR_KERNEL_PERIODIC_VECTOR,
                             kernel_mode != RSMP_FIR_KERNEL_PERIODIC_F32).ok;
}

bool periodic_worthwhile(const FirMirror& planned, size_t produced_frames, int kernel_mode) {
    if (kernel_mode == RSMP_FIR_KERNEL_PERIODIC || kernel_mode == RSMP_FIR_KERNEL_PERIODIC_VECTOR ||
        kernel_mode == RSMP_FIR_KERNEL_PERIODIC_F32)
        return produced_frames > 0;
    // AUTO: a launch shorter than a few workgroup spans leaves most lanes idle.
    (void)planned;
    return produced_frames >= 16384;
}

uint32_t periodic_blocks(const PeriodicGeometry& geo, uint64_t abs_out, uint32_t n_out) {
    if (n_out == 0) return 0;
    const uint64_t q_first = abs_out / geo.b;
    const uint64_t q_last = (abs_out + n_out - 1) / geo.b;
    return static_cast<uint32_t>((q_last - q_first) / geo.pw + 1);
}

size_t periodic_wrap_words(uint64_t abs_out, uint32_t n_out, uint64_t den) {
    if (n_out == 0) return 1;
    const uint64_t k0 = abs_out / den, k1 = (abs_out + n_out - 1) / den;
    return static_cast<size_t>((k1 - k0) / 32 + 1);
}

void periodic_fill_wrap_bits(const std::vector<uint32_t>& wraps, uint64_t abs_out, uint64_t den,
                             uint32_t* words, size_t n_words) {
    std::memset(words, 0, n_words * sizeof(uint32_t));
    const uint64_t k0 = abs_out / den;
    for (uint32_t n : wraps) {
        const uint64_t k = (abs_out + n) / den - k0;
        words[k >> 5] |= 1u << (k & 31);
    }
}

// The split kernel's builds: two channels in two or three planes, with or without the diagnostic code, windows of 1 .. 5
// steps; channel pairs, one channel, an odd count: two planes, no diagnostic build; two rounds of lane tasks (periods of
// 161 .. 320 frames): two channels or pairs, windows of 5 or 6 steps, diagnostic builds of the 6-step window and of the
// two-channel 5-step one.
// PCM input (FirStreamDesc::in_bits): the two-channel fp16 builds of the 128-tap windows -- 160 taps in one round
// (44.1 <-> 48 kHz) or two, 192 taps in two rounds (96 -> 44.1 kHz) -- exist for the three widths; kNotSupported
// for any other geometry (the caller converts with rsmp_pcm_to_stereo_f32_device first).
// PCM output (FirStreamDesc::out_bits): the same three windows, from f32 or PCM input, as builds of their own that read the
// width from the descriptor -- and, from f32 input, the channel-pair builds of those windows (an even count of 4 .. 16 channels);
// kNotSupported for any other geometry (the caller converts with rsmp_f32_to_pcm_device afterwards).
// dither != 0 (FirStreamDesc::dither): their twins that add TPDF dither -- white, or with format.dither_shape ==
// RSMP_DITHER_SHAPE_HIGHPASS the high-pass twins of those (SplitBuild::hp).  stats: their twins that count what they store, with or
// without dither (one build for both: a uniform branch).
SplitChoice split_build_for(const PeriodicGeometry& geo, bool diag, const FirFormat& format) {
    const uint32_t pcm_bits = format.in_bits, out_bits = format.out_bits;
    const bool one_channel = geo.cg == 1, odd_count = geo.cg == 3;
    const bool wide = geo.lp > 1 || one_channel;
    const bool two_rounds = geo.rounds == 2;
    const int nk = static_cast<int>(geo.row_len / 32);
    const bool diag_long = two_rounds && diag && (nk == 6 || (nk == 5 && !wide));
    SplitBuild b{nk, 2, false, 0, two_rounds ? 2 : 1, 0, false, false, false};
    if (two_rounds) {
        b.wide = wide ? 1 : 0;
        b.diag = diag_long;
    } else if (one_channel) b.wide = 2;
    else if (odd_count) b.wide = 3;
    else if (wide) b.wide = 1;
    else {
        b.planes = geo.planes == 3 ? 3 : 2;
        b.diag = diag;
    }
    if (nk < 1 || nk > (two_rounds ? 6 : 5) || (two_rounds && nk < 5)) return {b, BuildError::kInvalid};
    if (pcm_bits != 0 || out_bits != 0) {
        const bool window_ok = nk == 5 || (two_rounds && nk == 6);
        const auto width_ok = [](uint32_t w) { return w == 16 || w == 24 || w == 32; };
        // (channel pairs -- an even count of 4 .. 16 channels -- write PCM from f32 input; they do not read it)
        const bool pairs_out = wide && geo.cg == 2 && pcm_bits == 0 && out_bits != 0;
        if ((wide && !pairs_out) || one_channel || odd_count || geo.planes != 2 || diag || !window_ok || (pcm_bits != 0 && !width_ok(pcm_bits)) ||
            (out_bits != 0 && !width_ok(out_bits)))
            return {b, BuildError::kNotSupported};
        const FirOut mode = format.out_mode();
        b = SplitBuild{nk, 2, false, pairs_out ? 1 : 0, two_rounds ? 2 : 1, static_cast<int>(pcm_bits), out_bits != 0, mode == kFirOutPcmTpdf, mode == kFirOutPcmStats,
                       mode == kFirOutPcmTpdf && format.dither_shape == RSMP_DITHER_SHAPE_HIGHPASS};
    }
    return {b, BuildError::kNone};
}

// ---- the format rule: which streams and launches read or write PCM (fir_format.h, fir_periodic_plan.h) ----------------------
FormatFault format_stream_fault(const FirFormat& format, size_t channels) {
    const auto width_ok = [](uint32_t w) { return w == 0 || w == 16 || w == 24 || w == 32; };
    if (!width_ok(format.in_bits) || !width_ok(format.out_bits)) return FormatFault::kWidth;
    if (format.in_bits != 0 && channels != 2) return FormatFault::kInChannels;
    if (format.out_bits != 0 && (channels % 2 != 0 || channels > 16)) return FormatFault::kOutChannels;
    return FormatFault::kNone;
}
FormatFault format_group_fault(const FirFormat& format, const PeriodicGeometry& geo) {
    if (!format.pcm()) return FormatFault::kNone;
    if (geo.mfma == 3 && split_build_for(geo, false, format).error == BuildError::kNone) return FormatFault::kNone;
    return format.in_bits != 0 ? FormatFault::kInGroup : FormatFault::kOutGroup;
}
const char* format_fault_text(FormatFault fault) {
    static const char* const texts[] = {   // (in FormatFault's order)
        "", "PCM widths: in_bits 0 (f32) / 16 / 24 / 32, out_bits 16 / 24 / 32 (any other format: f32 output and rsmp_f32_to_pcm_device)",
        "PCM input: two-channel streams only (rsmp_pcm_to_stereo_f32_device converts a stereo file; pass any other count as f32)",
        "PCM output: two-channel streams only or, from f32 input, an even count up to 16; one channel, odd counts, more than 16: f32 output and rsmp_f32_to_pcm_device",
        "PCM input is read in place by the two-channel split kernel of the 128-tap rate pairs only (44.1 <-> 48, 96 -> 44.1 / 48 kHz ...): convert with rsmp_pcm_to_stereo_f32_device first",
        "PCM output is written in place by the split kernel of the 128-tap rate pairs only, for two channels or an even count up to 16 (44.1 <-> 48, 96 -> 44.1 / 48 kHz ...): take f32 output and convert with rsmp_f32_to_pcm_device"};
    return texts[static_cast<int>(fault)];
}
bool generic_tiled_ok(const FirFormat& format, uint32_t min_channels, uint32_t max_channels) { return format.out_bits == 0 || (min_channels == 2 && max_channels == 2); }
bool split_groups_may_share(const FirFormat& format) { return !format.pcm(); }

// ---- the generic streams' kernel: latency or tiled (fir_generic_plan.h) ---------------------------------------------------------
uint32_t fir_generic_bulk_tile(uint32_t max_channels, uint32_t max_taps, double max_ratio) {
    if (max_channels == 0 || max_ratio <= 0.0) return 0;
    const uint32_t cap = generic_bulk_window_cap(max_channels);
    if (cap < max_taps + 8u) return 0;
    double t = (static_cast<double>(cap) - max_taps - 4.0) / max_ratio;
    if (t > kBulkTileMax) t = kBulkTileMax;
    const uint32_t tile = static_cast<uint32_t>(t) / 64u * 64u;
    return tile >= kBulkTileMin ? tile : 0u;
}

// Long launches of streams without a short period (arbitrary rates, src/resampler_fir.rs:295-301) take the tiled kernel, whose
// workgroups sort a tile's outputs by phase row and stage its window in LDS; streaming calls keep the one-launch latency path.
// PCM output: the tiled kernel's builds are two-channel; a generic stream of more channels -- a launch too short for the periodic
// kernels, a rate pair without a short period -- keeps the batch's generic streams on the latency kernel, which stores by value
// index for any count, at any length.
GenericLaunchChoice generic_launch_choice(const GenericLaunchRequest& rq, bool bulk_on) {
    GenericLaunchChoice c;
    c.grid_x = (rq.max_out + kFirTile - 1) / kFirTile;
    if (!bulk_on) { c.reason = GenericLatencyReason::kSwitchedOff; return c; }
    if (rq.max_out < kFirBulkMinOut) { c.reason = GenericLatencyReason::kShort; return c; }
    const uint32_t tile = fir_generic_bulk_tile(rq.max_channels, rq.max_taps, rq.max_ratio);
    if (tile == 0) { c.reason = GenericLatencyReason::kNoTile; return c; }
    if (!generic_tiled_ok(rq.format, rq.min_channels, rq.max_channels)) { c.reason = GenericLatencyReason::kFormat; return c; }
    const uint32_t uniform_channels = rq.min_channels == rq.max_channels ? rq.max_channels : 0u;
    c.kernel = GenericKernel::kTiled;
    c.reason = GenericLatencyReason::kNone;
    c.ch_build = rq.format.out_bits != 0 ? 2 : uniform_channels == 2 ? 2 : uniform_channels == 1 ? 1 : 0;
    c.full = rq.min_taps == 128 && rq.max_taps == 128;
    c.tile = tile;
    c.window_cap_frames = generic_bulk_window_cap(rq.max_channels);
    c.grid_x = (rq.max_out + tile - 1) / tile;
    c.lds_bytes = static_cast<uint32_t>((2 * kBulkRows + kBulkScanWords) * sizeof(uint32_t) + kBulkSegs * sizeof(rsmp_fir_segment) +
                                        static_cast<size_t>(tile) * (kBulkMetaBytes + kBulkSortedBytes) + kBulkWindowAlign +
                                        static_cast<size_t>(c.window_cap_frames) * rq.max_channels * sizeof(float));
    return c;
}

// Slots of launch_fir_periodic's kernel table.  0..2 = vector kernel: two channels with one lane per period / CG 2,
// any even channel count / CG 1.  (4-tap chunks with 16-wave workgroups at 8 waves per SIMD measured
// 13 % slower than 8-tap chunks: the 64-VGPR cap spills.)  Matrix-core consumers: 3 / 4 = coefficient
// ring (any window length), 2 / 4 period groups per unit; 5..7 = ring timing experiments
// (RSMP_FIR_MFMA_DBG 1..3); 8..13 = coefficient tile in registers, 2 groups per unit, windows of
// 48 / 96 / 144 taps, padded (8..10) or back-to-back (11..13) rows; 14..19 = the same with 1 group.
int periodic_slot_for(const PeriodicGeometry& geo, int mfma_dbg, bool mfma_ring) {
    const uint32_t nb3 = geo.row_len % 48 == 0 && geo.row_len <= 144 ? geo.row_len / 48 : 0;   // 0..3
    const bool flat_rows = geo.row_stride == 2 * geo.a;
    if (!geo.mfma) return geo.cg == 2 ? (geo.lp == 1 ? 0 : 1) : 2;
    if (geo.mfma == 4) return 4;
    if (geo.mfma == 1 && (!nb3 || mfma_ring)) return -1;   // G = 1 exists only register-resident
    if (mfma_dbg) return 4 + mfma_dbg;
    if (nb3 && !mfma_ring) return (geo.mfma == 1 ? 13 : 7) + static_cast<int>(nb3) + (flat_rows ? 3 : 0);
    return 3;
}

}  // namespace rsmp
