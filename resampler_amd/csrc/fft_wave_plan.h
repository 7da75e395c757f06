// fft_wave_plan.h -- the geometry of the wave-per-transform FFT kernels (fft_wave.hip, fft_pair.hip): a plan's stages, its
// padded LDS layouts and table sizes, the named plans, the (forward, inverse) pairs each kernel file is built for, and what
// of a pair a CU's LDS holds.  Plain C++17 constants, no HIP: the kernel files (through fft_wave_core.h) and the launch
// rules (fft_launch.cpp) read the same ones.  Included inside `namespace rsmp { namespace { ... } }`, after <cstddef> and
// <cstdint>.
// Whether a radix-7 / 8 stage keeps whole twiddle rows in LDS (`whole_rows`: the operation-for-operation build of
// fft_wave.hip, libresampler_amd_fftexact.so) is a parameter of every size that depends on it, not a build setting of this
// file: fft_launch.cpp is compiled once and serves both libraries.
#pragma once

// LDS stores go 16 lanes at a time over 32 banks (MI355X_MICROARCH.md, LDS table; tools/fft_bank_model.py counts the
// array cycles of every pass of a plan pair).  A stage's lane i stores its value q at R (i - k) + k + q stride
// (k = i mod stride): lanes 16 apart in i are in different blocks of `stride` columns unless stride >= 16, and a
// block is (R - 1) stride values further than the lane index says -- two values per 16 lanes of shift keep the
// 16 lanes of a store on distinct banks iff (R - 1) stride + pad is a multiple of 16 values.  (Radix 7, stride 21:
// 147-value blocks, 2 values of padding; radix 8, stride 20: 4.)
constexpr int stage_out_pad(int r, int stride) { return (16 - ((r - 1) * stride) % 16) % 16; }
constexpr int gcd_c(int a, int b) { return b == 0 ? a : gcd_c(b, a % b); }
// Twiddles a stage keeps per column in LDS: all R - 1 of the row, or -- radix 7 and 8 -- only w, w^2 and w^4 (the
// stage multiplies the others out, see twiddle_expand; the tables of the 1176 <-> 1280 pair shrink from 39 to 29 KB).
constexpr int fetch_count(int r, bool whole_rows) { return (r == 7 || r == 8) && !whole_rows ? 3 : r - 1; }

// A transform of N complex points in `Rs...` Stockham stages (2 .. 5 of them), as the reference's planner orders
// them (src/fft/optimizer.rs).  Where the first two radices multiply to at most 21 values per unit (and a third
// stage exists) they run as one register pass (wave_fused_first); every later stage but the inverse's last is a
// wave_stage; the twiddle tables of all stages sit in LDS.
template <int N_, int... Rs>
struct WavePlan {
    static constexpr int N = N_;
    static constexpr int kStages = sizeof...(Rs);
    static constexpr int kR[sizeof...(Rs)] = {Rs...};
    static_assert(kStages >= 2 && kStages <= 5, "stages");
    static constexpr int stride(int s) { int v = 1; for (int i = 0; i < s; ++i) v *= kR[i]; return v; }
    static_assert(stride(kStages) == N_, "radices");
    static constexpr bool kFused = kStages >= 3 && kR[0] * kR[1] <= 21;
    // Stage twiddles, unique per column: stage s (s >= 1) holds stride(s) rows of R_s - 1.  In LDS the rows of a
    // wave_stage are (R - 1) | 1 values apart: lane k reads row k, and an even row length puts lanes 16 apart
    // (radix 7: six values = 12 dwords) on the same banks.  (The fused pass reads its rows by constant index.)
    static constexpr int row(int r, bool whole_rows) { return fetch_count(r, whole_rows) | 1; }
    static constexpr int pitch(int s, bool whole_rows) { return kFused && s == 1 ? kR[1] - 1 : row(kR[s], whole_rows); }
    static constexpr int tab(int s, bool whole_rows) { int off = 0; for (int i = 1; i < s; ++i) off += stride(i) * pitch(i, whole_rows); return off; }   // LDS offset of stage s
    static constexpr int src(int s) { int off = 0; for (int i = 1; i < s; ++i) off += stride(i) * (kR[i] - 1); return off; }   // offset in the plan's array
    static constexpr int tw(bool whole_rows) { return tab(kStages, whole_rows); }   // values of all stage tables in LDS
    static constexpr int kRc = N_ / 2 - 1;   // real <-> complex twiddles
    // Padding between passes (LDS banks).  The first pass (fused or not) writes kUnit values per lane side by side:
    // an even kUnit puts lanes 32 / gcd(2 kUnit, 32) apart on the same banks, so one value of padding follows every
    // kPadJ units (20 values per unit: every 4) where the next stage's input distance is a multiple of that period.
    // After the blocks of a later stage: stage_out_pad, where the stage that follows reads block by block.
    // in_pad(s): what stage s's input distance N / R_s grows by; in_period(s): elements between two padding values
    // inside that distance (0 = none).
    static constexpr int kUnit = kFused ? kR[0] * kR[1] : kR[0];
    static constexpr int kNext = kFused ? 2 : 1;   // the stage that reads the first pass's output
    // (Plans above 2048 points run at the 256-register cap of their wide workgroups: the padded addressing spilled
    // there -- 2352 -> 2560 points 0.80 -> 1.00 ms -- so they keep the plain layout, but for the radix-7 blocks.)
    static constexpr bool kPadded = N_ <= 2048;
    static constexpr int first_padj() {
        if (!kPadded || kUnit % 2 != 0 || kNext >= kStages) return 0;
        const int p = 32 / gcd_c(2 * kUnit, 32);
        return (N_ / kR[kNext < kStages ? kNext : 0]) % (p * kUnit) == 0 ? p : 0;
    }
    static constexpr int kPadJ = first_padj();
    static constexpr int out_pad(int s) {
        if (s < 1 || s + 1 >= kStages || (kFused && s == 1)) return 0;
        if (stride(s) >= N_ / kR[s]) return 0;   // one block
        const int p = kPadded || (kR[s] == 7 && stride(s) == 21) ? stage_out_pad(kR[s], stride(s)) : 0;
        return p != 0 && N_ / kR[s + 1] == stride(s + 1) ? p : 0;
    }
    static constexpr int in_pad(int s) {
        if (s == kNext) return kPadJ ? (N_ / kR[s]) / (kPadJ * kUnit) : 0;
        return s >= 2 ? out_pad(s - 1) : 0;
    }
    static constexpr int in_period(int s) { return s == kNext && kPadJ && N_ / kR[s] > kPadJ * kUnit ? kPadJ * kUnit : 0; }
    static constexpr int buf_values() {   // what the wave's buffer needs: the points + bin N and its neighbour (real <-> complex passes), or the widest padded layout
        int pad = kPadJ ? N_ / (kPadJ * kUnit) : 0;
        for (int s = 1; s + 1 < kStages; ++s) {
            const int p = out_pad(s) * (N_ / stride(s + 1));
            if (p > pad) pad = p;
        }
        return N_ + (pad > 2 ? pad : 2);
    }
    static constexpr int kBuf = buf_values();
    static bool matches(uint32_t n, uint32_t n_stages, const uint32_t* radix) {
        if (n != static_cast<uint32_t>(N_) || n_stages != static_cast<uint32_t>(kStages)) return false;
        for (int s = 0; s < kStages; ++s)
            if (radix[s] != static_cast<uint32_t>(kR[s])) return false;
        return true;
    }
};

// ---- the plans ----------------------------------------------------------------------------------------------------------
typedef WavePlan<1176, 3, 7, 7, 8> W1176;   // 44.1 kHz side of the 44.1 <-> 48 kHz family
typedef WavePlan<1280, 4, 5, 8, 8> W1280;   // 48 kHz side
typedef WavePlan<512, 8, 8, 8> W512;        // the input block of the power-of-two families (x2, /2, x4, /4, x3, x1.5 ...)
typedef WavePlan<1024, 2, 8, 8, 8> W1024;
typedef WavePlan<256, 4, 8, 8> W256;
typedef WavePlan<128, 2, 8, 8> W128;
typedef WavePlan<64, 8, 8> W64;
typedef WavePlan<768, 3, 4, 8, 8> W768;
typedef WavePlan<1536, 3, 8, 8, 8> W1536;
typedef WavePlan<2048, 4, 8, 8, 8> W2048;
typedef WavePlan<3072, 2, 3, 8, 8, 8> W3072;   // (x6: six trips per stage -- one wave per SIMD with the whole register file)
typedef WavePlan<4096, 8, 8, 8, 8> W4096;      // (x8: three waves per CU are all the LDS holds)
typedef WavePlan<3528, 3, 3, 7, 7, 8> W3528;   // 88.2 kHz against the 16 / 32 kHz families
typedef WavePlan<4704, 3, 4, 7, 7, 8> W4704;   // 176.4 kHz (two waves per CU)
typedef WavePlan<5120, 2, 5, 8, 8, 8> W5120;   // 192 kHz
typedef WavePlan<588, 3, 4, 7, 7> W588;     // 22.05 kHz against the 48 kHz family (input side: the inverse's last radix must be even)
typedef WavePlan<882, 2, 3, 3, 7, 7> W882;
typedef WavePlan<1764, 3, 3, 4, 7, 7> W1764;
typedef WavePlan<2352, 2, 3, 7, 7, 8> W2352; // 88.2 kHz
typedef WavePlan<2560, 5, 8, 8, 8> W2560;    // 96 kHz
typedef WavePlan<640, 2, 5, 8, 8> W640;        // 16 kHz against the 44.1 kHz family

// ---- the (forward, inverse) pairs the kernels are built for ---------------------------------------------------------------
// A kernel file's table of builds (wave_kernels, pair_kernels) is a pack expansion over its list, and the launch rules name
// a build by its index in the same list: a pair in a list IS an instantiation.  The first kHeadPairs entries of both lists
// are the 44.1 <-> 48 kHz pair, all that the timing experiments (RSMP_EXP != 0) instantiate.
template <class FWD, class INV> struct PlanPair { typedef FWD Fwd; typedef INV Inv; };
template <class... Ps> struct PairList { static constexpr int kCount = sizeof...(Ps); };
constexpr int kHeadPairs = 2;
typedef PairList<PlanPair<W1176, W1280>, PlanPair<W1280, W1176>> HeadPairs;

// fft_wave.hip: the 44.1 <-> 48 kHz family (both directions), the families whose input block is 512 frames (x2, /2, /4,
// /8, x3, x1.5 ...) and the pairs of the ten sample rates up to 5120 points.
typedef PairList<
    PlanPair<W1176, W1280>, PlanPair<W1280, W1176>,
    PlanPair<W512, W64>, PlanPair<W512, W128>, PlanPair<W512, W256>, PlanPair<W512, W768>, PlanPair<W512, W1024>,
    PlanPair<W512, W1536>, PlanPair<W512, W2048>, PlanPair<W512, W3072>, PlanPair<W512, W4096>,
    PlanPair<W768, W64>, PlanPair<W768, W128>, PlanPair<W768, W256>, PlanPair<W768, W512>,
    PlanPair<W1536, W64>, PlanPair<W1536, W128>,
    PlanPair<W588, W1280>, PlanPair<W588, W2560>, PlanPair<W882, W640>, PlanPair<W882, W1280>,
    PlanPair<W1764, W640>, PlanPair<W1764, W1280>, PlanPair<W2352, W1280>, PlanPair<W2352, W2560>,
    PlanPair<W1176, W2560>, PlanPair<W1280, W2352>,
    PlanPair<W2560, W2352>, PlanPair<W2560, W1176>, PlanPair<W2560, W588>,
    PlanPair<W640, W882>, PlanPair<W640, W1764>, PlanPair<W640, W3528>, PlanPair<W3528, W640>, PlanPair<W3528, W1280>,
    PlanPair<W1280, W588>, PlanPair<W1280, W882>, PlanPair<W1280, W1764>, PlanPair<W1280, W3528>, PlanPair<W1280, W4704>,
    PlanPair<W4704, W1280>, PlanPair<W4704, W2560>, PlanPair<W5120, W1176>, PlanPair<W5120, W2352>,
    PlanPair<W2560, W4704>, PlanPair<W1176, W5120>, PlanPair<W2352, W5120>, PlanPair<W588, W5120>>
    WavePairs;

// fft_pair.hip, by tools/fft_pairs_bench.py, both kernels in one lease (profiles/r05/fft_pairs_pair_vs_wave.txt): the
// down-sampling pairs gain 8 - 21 %, 512 -> 1024 frames 4 %; a 1764-point inverse, 512 -> 1536 / 2048, 768 -> 256 / 512,
// 882 -> 1280 and 1764 -> 1280 frames spill or run four waves and stay with fft_wave.hip.
typedef PairList<
    PlanPair<W1176, W1280>, PlanPair<W1280, W1176>,
    PlanPair<W512, W64>, PlanPair<W512, W128>, PlanPair<W512, W256>, PlanPair<W512, W768>, PlanPair<W512, W1024>,
    PlanPair<W768, W64>, PlanPair<W768, W128>, PlanPair<W768, W256>, PlanPair<W768, W512>,
    PlanPair<W1536, W64>, PlanPair<W1536, W128>, PlanPair<W588, W1280>, PlanPair<W882, W640>, PlanPair<W1764, W640>,
    PlanPair<W640, W882>, PlanPair<W1280, W588>, PlanPair<W1280, W882>>
    PairPairs;

// ---- what a CU's LDS holds of a pair (values of 8 bytes: one complex) -----------------------------------------------------
constexpr size_t kCuLdsValues = 160 * 1024 / 8;
template <class FWD, class INV> constexpr int kPairBuf = FWD::kBuf > INV::kBuf ? FWD::kBuf : INV::kBuf;   // a wave's buffer
// bins the filter multiplies (the plan's new_length: fft_in + 1 or fft_out, resampler_fft.rs:396-399)
constexpr int filter_bins(int fi, int fo) { return fi < fo ? fi + 1 : fo; }
template <class FWD, class INV> constexpr int kPairNL = filter_bins(FWD::N, INV::N);

// fft_wave.hip.  Waves per CU, by what the CU's LDS holds (one copy of the tables per workgroup + a buffer per wave) and what
// the registers allow: two-channel streams run 12 (<= 168 registers) or 2 x 4 waves; streams of 4, 6, 8 .. channels run as
// channel pairs on the same code with 8-byte accesses (2 x 4 waves); the any-channel-count build (odd counts) needs ~250
// registers (strided sample addressing; it spilled 290 bytes per lane under the 168 cap and ran 25-30 % slower,
// tools/fft_channels_bench.py) and runs 2 x 4.  Plans too long for that run one workgroup of up to 8 waves.
// OCC waves per SIMD: 2 = two workgroups of 4 waves per CU (80 KB of LDS each: the tables + 4 buffers),
// 3 = one workgroup of 12 waves per CU (one copy of the tables + 12 buffers = 158 KB; <= 168 registers),
// 1 = one workgroup of as many waves (<= 8) as the CU's LDS holds buffers for (the long plans; the launch
// decides).  (16 waves per CU for the short plans measured within 2 % of 12: the LDS is the bound, not latency.)
// (the pairs build addresses its frames at a run-time stride: under the 168-register cap of twelve waves per CU it
// spills 25 registers and runs 13 % slower than 2 x 4 waves with all of them -- 8 channels 0.84 against 0.73 ms:
// only the two-channel build runs twelve waves, occupancy 3; the others 2 x 4 waves (2) or one workgroup (1))
constexpr size_t kWaveFlagValues = 32;   // behind the buffers: exchange flags (two 32-bit words per wave, up to 16 waves), then the waves' SIMD ids and block counts
struct WaveBudget {
    bool served;            // (fewer than two waves per CU -- the longest plans with whole twiddle rows -- belong to the workgroup kernels)
    int occ_any, occ_c2;    // OCC of the any-channel / channel-pairs builds, and of the two-channel build
    uint32_t wide;          // waves of an OCC = 1 workgroup
    size_t tables, buf;     // values
    constexpr uint32_t waves(int occ, uint32_t wide_knob) const {   // per workgroup (RSMP_FFT_WAVE_WIDE: fewer of an OCC = 1 workgroup)
        return occ == 3 ? 12u : occ == 2 ? 4u : (wide_knob >= 1 && wide_knob <= wide ? wide_knob : wide);
    }
    constexpr size_t lds_bytes(uint32_t n_waves) const { return (tables + n_waves * buf + kWaveFlagValues) * 8; }
};
// Both transforms above 2048 points (88.2 <-> 96 kHz): four or five trips per stage in registers next to the
// carry do not fit 256 registers -- these pairs run one wave per SIMD with the full register file instead of two
// that spill (88.2 -> 96 kHz: 0.94 -> 0.76 ms).
template <class FWD, class INV> constexpr bool kOneWavePerSimd = (FWD::N > 2048 && INV::N > 2048) || FWD::N > 2560 || INV::N > 2560;
template <class FWD, class INV>
constexpr WaveBudget wave_budget(bool whole_rows) {
    const size_t tables = static_cast<size_t>(FWD::tw(whole_rows) + INV::tw(whole_rows) + FWD::kRc + INV::kRc + kPairNL<FWD, INV>);   // (+ the filter bins in use)
    const size_t buf = kPairBuf<FWD, INV>;
    const bool fit12 = tables + 12 * buf + kWaveFlagValues <= kCuLdsValues, fit4 = 2 * (tables + 4 * buf + kWaveFlagValues) <= kCuLdsValues;
    const uint32_t wide_fit = (kCuLdsValues - tables - kWaveFlagValues) / buf < 8 ? static_cast<uint32_t>((kCuLdsValues - tables - kWaveFlagValues) / buf) : 8u;
    const uint32_t wide = kOneWavePerSimd<FWD, INV> && wide_fit > 4 ? 4u : wide_fit;
    const int occ_any = fit4 ? 2 : 1;
    return WaveBudget{fit4 || wide >= 2, occ_any, fit12 ? 3 : occ_any, wide, tables, buf};
}

// fft_pair.hip.  Waves per CU = per workgroup: eight (two per SIMD, an old and a young one) where the LDS holds the tables
// (stage twiddles, the filter bins in use, the two chirps) and eight buffers, else four; 0 = the pair is not served.
struct PairBudget {
    int waves;
    size_t tables, buf;
    constexpr size_t lds_bytes() const { return (tables + waves * buf) * 8; }
};
template <class FWD, class INV>
constexpr PairBudget pair_budget(bool whole_rows) {
    const size_t buf = kPairBuf<FWD, INV>;
    const size_t tables = static_cast<size_t>(FWD::tw(whole_rows) + INV::tw(whole_rows) + kPairNL<FWD, INV> + FWD::N + INV::N);
    // (plans of up to 512 points need ~105 registers: sixteen waves, four per SIMD, hide more of their many short passes)
    // (twelve waves -- 168 registers -- for the plans of up to 1024 points: 26-55 spilled registers, 512 -> 1024 frames 0.72 ->
    // 0.77 ms, 640 -> 882 0.76 -> 0.87: measured, not kept)
    const int waves = FWD::N <= 768 && INV::N <= 512 && tables + 16 * buf <= kCuLdsValues ? 16
                      : tables + 8 * buf <= kCuLdsValues ? 8 : tables + 4 * buf <= kCuLdsValues ? 4 : 0;
    return PairBudget{waves, tables, buf};
}
