// fft_launch.cpp -- see fft_launch.h.  Plain C++: no HIP header, no kernel.
#include "fft_launch.h"

#include <cmath>
#include <cstdlib>

#include "errors.h"

namespace rsmp {

namespace {

#include "fft_wave_plan.h"

// The budgets of a list's pairs -- fft_wave.hip's with three-value and with whole twiddle rows, fft_pair.hip's with three-value
// rows (it is the ordinary build in both libraries) -- and the index of the pair a plan is.
struct WaveBudgets { WaveBudget rows3, whole; };
template <class... Ps>
const WaveBudgets* wave_budgets(PairList<Ps...>) {
    static constexpr WaveBudgets t[] = {{wave_budget<typename Ps::Fwd, typename Ps::Inv>(false), wave_budget<typename Ps::Fwd, typename Ps::Inv>(true)}...};
    return t;
}
template <class... Ps>
const PairBudget* pair_budgets(PairList<Ps...>) {
    static constexpr PairBudget t[] = {pair_budget<typename Ps::Fwd, typename Ps::Inv>(false)...};
    return t;
}
template <class P>
bool is_pair(const FftShape& s) {
    return P::Fwd::matches(s.fft_in, s.n_stages_f, s.radix_f) && P::Inv::matches(s.fft_out, s.n_stages_i, s.radix_i);
}
template <class... Ps>
int find_pair(PairList<Ps...>, const FftShape& s) {
    int i = 0;
    const bool found = ((is_pair<Ps>(s) ? true : (++i, false)) || ...);
    return found ? i : -1;
}

bool full_length(const FftShape& s) { return s.new_length == (s.fft_in < s.fft_out ? s.fft_in + 1 : s.fft_out); }
bool rc_full(const FftShape& s) { return s.n_rc_f == s.fft_in / 2 - 1 && s.n_rc_i == s.fft_out / 2 - 1; }

bool knob_is_zero(const char* name) { return knob(name) != nullptr && atoi(knob(name)) == 0; }

// One wave per two-channel stream and run of blocks (fft_pair.hip); false when the plan is not one of PairPairs.
bool choose_pair(const FftShape& s, const FftRequest& rq, FftLaunch* out) {
    if (rq.pcm_bits != 0 && rq.pcm_bits != 16 && rq.pcm_bits != 24 && rq.pcm_bits != 32) return false;
    if (!s.chirps || !full_length(s)) return false;
    const int idx = find_pair(PairPairs{}, s);
    if (idx < 0) return false;
    const PairBudget& b = pair_budgets(PairPairs{})[idx];
    if (b.waves == 0) return false;
    // Groups of runs per stream.  A SIMD serves its waves oldest first, so a group's blocks are cut into a long run for
    // an old wave and shorter ones for the younger (fft_pair.hip's run arithmetic).
    const uint32_t waves = static_cast<uint32_t>(b.waves), classes = waves / 4;   // waves per SIMD: ages
    const uint32_t both = fft_pick_run(rq.max_blocks, rq.n_streams, static_cast<double>(rq.cus) * waves, 6 * classes, 64 * classes, classes);
    const uint32_t groups_per_stream = (rq.max_blocks + both - 1) / both;
    const uint32_t total_waves = groups_per_stream * rq.n_streams * classes;
    out->family = FftFamily::kPair;
    out->pair = idx;
    out->bits = static_cast<int>(rq.pcm_bits);
    out->grid[0] = (total_waves + waves - 1) / waves;
    out->block = waves * 64;
    out->lds = b.lds_bytes();
    out->grant_lds = true;
    fft_pair_split(both, classes, out->args);
    out->args[4] = groups_per_stream;
    out->args[5] = total_waves;
    out->n_args = 6;
    return true;
}

// A wave per (stream, channel) and run of blocks (fft_wave.hip); false when the plan is not one of WavePairs.
bool choose_wave(const FftShape& s, const FftRequest& rq, FftLaunch* out) {
    if (rq.max_channels != rq.min_channels) return false;   // one wave layout per launch
    if (!rc_full(s) || !full_length(s)) return false;
    const int idx = find_pair(WavePairs{}, s);
    if (idx < 0) return false;
    const WaveBudgets& both = wave_budgets(WavePairs{})[idx];
    const WaveBudget& b = rq.exact ? both.whole : both.rows3;
    if (!b.served) return false;
    const uint32_t C = rq.max_channels;
    static const bool no_c2 = knob("RSMP_FFT_WAVE_NOC2") != nullptr;   // A/B: the any-channel-count build for two channels
    static const uint32_t wide_knob = [] { const char* e = knob("RSMP_FFT_WAVE_WIDE"); return e ? static_cast<uint32_t>(atoi(e)) : 0u; }();
    // (an even number of channels: channel pairs on the two-channel build)
    const bool paired = C % 2 == 0 && !no_c2;
    const bool c2 = paired && C == 2;
    out->family = FftFamily::kWave;
    out->pair = idx;
    out->chm = c2 ? 1 : paired ? 2 : 0;
    out->occ = c2 ? b.occ_c2 : b.occ_any;
    out->whole_rows = rq.exact;
    const uint32_t waves = b.waves(out->occ, wide_knob);
    const uint32_t resident = out->occ == 2 ? 8u : waves;   // waves a CU holds at once
    const uint32_t run = fft_pick_run(rq.max_blocks, rq.n_streams * C, static_cast<double>(rq.cus) * resident, 6, 64);
    const uint32_t runs_per_stream = (rq.max_blocks + run - 1) / run;
    const uint32_t total_waves = runs_per_stream * rq.n_streams * C;
    out->grid[0] = (total_waves + waves - 1) / waves;
    out->block = waves * 64;
    out->lds = b.lds_bytes(waves);
    out->grant_lds = out->lds > 64 * 1024;   // dynamic LDS above 64 KiB must be opted into
    out->args[0] = run;
    out->args[1] = runs_per_stream;
    out->args[2] = total_waves;
    out->args[3] = C / 2;   // (channel pairs: read by the two-channel build only)
    out->n_args = 4;
    return true;
}

// The workgroup kernels (fft_kernels.hip): the build and its LDS; the run follows the occupancy (fft_choose_run).
void choose_workgroup(const FftShape& s, const FftRequest& rq, FftLaunch* out) {
    out->block = 256;
    out->lds = fft_ola_lds_bytes(s, rq.max_channels);
    if (out->lds > 160 * 1024) {   // the two-buffer kernels do not fit: one buffer, in place, a workgroup per channel
        out->lds = fft_big_lds_bytes(s);
        out->family = out->lds > 160 * 1024 ? FftFamily::kInvalid : FftFamily::kBig;
        out->block = 1024;
        out->grid[2] = rq.max_channels;
        out->grant_lds = true;
        return;
    }
    const bool stereo = rq.max_channels == 2 && rq.min_channels == 2;
    static const bool generic_only = knob("RSMP_FFT_GENERIC") != nullptr;   // A/B: skip the specialised builds
    const bool ct = !generic_only && rc_full(s);
    if (ct && (is_pair<PlanPair<W1176, W1280>>(s) || is_pair<PlanPair<W1280, W1176>>(s))) {
        out->family = stereo ? FftFamily::kCt2 : FftFamily::kCt;
        out->pair = s.fft_in == 1176 ? 0 : 1;
        if (stereo) out->lds = 4 * static_cast<size_t>(s.lds_complex) * 8 + 2 * static_cast<size_t>(s.fft_out) * 4;
    } else {
        // the generic pipeline: for blocks up to 512 frames (both sides) a one-wave workgroup per channel (see the
        // kernel; 96 -> 48 kHz 1.56 -> 1.18 ms, 192 -> 48 kHz 1.48 -> 0.76 ms per 64 x 2^20 frames); above that the
        // four-wave workgroups keep more waves on a CU for the same LDS and win (tools/fft_pairs_bench.py)
        out->family = FftFamily::kGeneric;
        const size_t lds_wave = fft_ola_lds_bytes(s, 1);
        if (s.lds_complex <= 513 && lds_wave <= 160 * 1024) {
            out->block = 64;
            out->grid[2] = rq.max_channels;
            out->lds = lds_wave;
        } else if (out->lds > 80 * 1024) {
            out->block = 1024;   // the long plans: one workgroup per CU is all the LDS holds, so it is 16 waves wide, not 4
        } else if (out->lds > 160 * 1024 / 3) {
            out->block = 512;    // two workgroups per CU
        }
    }
    out->grant_lds = out->lds > 64 * 1024;   // dynamic LDS above 64 KiB must be opted into
}

}  // namespace

uint32_t fft_pick_run(uint32_t max_blocks, uint32_t lanes, double slots, uint32_t lo, uint32_t hi, uint32_t classes) {
    uint32_t run = lo;
    double best = -1.0;
    for (uint32_t cand = lo; cand <= hi; ++cand) {
        const double groups = static_cast<double>((max_blocks + cand - 1) / cand);
        const double waves = classes * groups * lanes;
        const double rounds = std::ceil(waves / slots);
        const double useful = static_cast<double>(max_blocks) / (max_blocks + classes * groups - 1.0);   // halo blocks
        const double score = waves / (rounds * slots) * useful;
        if (score > best + 1e-9) { best = score; run = cand; }
    }
    return run;
}

void fft_pair_split(uint32_t both, uint32_t classes, uint32_t runs[4]) {
    static const double share_knob = [] { const char* e = knob("RSMP_FFT_PAIR_SHARE"); return e ? atof(e) : 0.0; }();   // A/B
    // the share of a SIMD each age gets while all of them run (two ages: by a sweep on the 44.1 -> 48 kHz launch; four: the
    // same falling series, RSMP_FFT_PAIR_SHARE = its ratio)
    double share[4] = {1.0, 0.0, 0.0, 0.0};
    if (classes == 2) {
        share[0] = share_knob > 0.0 && share_knob < 1.0 ? share_knob : 0.6;
        share[1] = 1.0 - share[0];
    } else if (classes >= 3) {
        const double r = share_knob > 0.0 && share_knob <= 1.0 ? share_knob : 0.8;
        double sum = 0.0;
        for (uint32_t c = 0; c < classes; ++c) sum += std::pow(r, static_cast<double>(c));
        for (uint32_t c = 0; c < classes; ++c) share[c] = std::pow(r, static_cast<double>(c)) / sum;
    }
    // (the halo block is part of a wave's work: the shares are of both + classes)
    uint32_t given = 0;
    for (uint32_t c = 0; c < 4; ++c) runs[c] = 0;
    for (uint32_t c = 0; c + 1 < classes; ++c) {
        const long v = std::lround(share[c] * (both + static_cast<double>(classes)) - 1.0);
        runs[c] = static_cast<uint32_t>(v < 1 ? 1 : v);
        if (given + runs[c] > both) runs[c] = both - given;
        given += runs[c];
    }
    runs[classes - 1] = both - given;
}

// one buffer (the stages run in place) + the overlap row of the workgroup's channel
size_t fft_big_lds_bytes(const FftShape& s) { return static_cast<size_t>(s.lds_complex) * 8 + static_cast<size_t>(s.fft_out) * 4; }
// two buffers + the overlap rows of the workgroup's channels
size_t fft_ola_lds_bytes(const FftShape& s, uint32_t channels) {
    return 2 * static_cast<size_t>(s.lds_complex) * 8 + static_cast<size_t>(channels) * s.fft_out * 4;
}

FftLaunch fft_choose(const FftShape& s, const FftRequest& rq) {
    FftLaunch out;
    static const bool no_wave = knob_is_zero("RSMP_FFT_WAVE");   // A/B
    static const bool no_pair = knob_is_zero("RSMP_FFT_PAIR");   // A/B
    const bool stereo = rq.max_channels == 2 && rq.min_channels == 2;
    // (PCM input is read by the two-channel kernels only: FftStreamDesc::in_bits)
    if (rq.pcm_bits != 0 && (no_wave || !stereo)) return out;
    if (rq.out_bits != 0 && rq.out_bits != 16 && rq.out_bits != 24 && rq.out_bits != 32) return out;
    if (rq.pcm_stats && rq.out_bits == 0) return out;   // (the statistics are of a PCM store: an f32 launch has none)
    // two-channel streams: a wave per stream, the frame as one complex sample (not in the exact build)
    // (a launch of a block or two per stream is a streaming call: there the wave-per-channel kernel's two waves per stream
    // finish sooner than one wave running both chains -- 32.6 against 36.3 us per one-block call, tools/fft_call_latency.py)
    if (!no_wave && !no_pair && stereo && rq.max_blocks >= 4 && !rq.exact && choose_pair(s, rq, &out)) {
        out.pcm_stats = rq.pcm_stats;   // (which kernel file's build, fft_launch_hip.cpp: nothing of the launch depends on it)
        return out;
    }
    // (PCM output is stored by the pair kernel only: FftStreamDesc::out_bits)
    if (rq.out_bits != 0) return FftLaunch{};
    if (!no_wave && (choose_wave(s, rq, &out) || rq.pcm_bits != 0)) return out;
    choose_workgroup(s, rq, &out);
    return out;
}

void fft_choose_run(FftLaunch* launch, const FftRequest& rq, int per_cu) {
    const double slots = static_cast<double>(rq.cus) * (per_cu < 1 ? 4 : per_cu);
    const uint32_t run = fft_pick_run(rq.max_blocks, rq.n_streams * launch->grid[2], slots, 8, 64);
    launch->grid[0] = (rq.max_blocks + run - 1) / run;
    launch->grid[1] = rq.n_streams;
    launch->args[0] = run;
    launch->n_args = 1;
}

}  // namespace rsmp
