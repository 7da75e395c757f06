// fir_format_check.cpp -- holds the FIR launch path's format rule (fir_format.h, fir_periodic_plan.h; fir_geometry.cpp) to the
// predicates it replaced, written out here as the specification: which streams may read or write PCM (the two PCM entries' rule),
// which periodic groups (what launch_jobs asked of a group's geometry, and that split_build_for agrees), which build stores the
// output (FirFormat::out_mode), and the two conditions the launch phases ask.  The walk is fir_geometry_dump.cpp's -- 91 rate
// pairs, the tap count of every Latency, 1 .. 17 channels, the three kernel modes -- times every format of in_bits and out_bits
// 0 / 16 / 24 / 32 / 8, dither 0 / 1, statistics off / on.  Prints how often every outcome occurred ("count <name> <n>"), so
// that tests/test_fir_format_host.py can refuse a walk that never reached one; plain C++ under ASan + UBSan.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <numeric>

#include "fir_periodic_plan.h"

using namespace rsmp;

namespace {

int failures = 0;
void expect(bool ok, const char* what, const FirFormat& f, uint32_t a, uint32_t b) {
    if (ok) return;
    if (++failures <= 20) fprintf(stderr, "FAILED %s: format %u %u %u %d, %u %u\n", what, f.in_bits, f.out_bits, f.dither, f.stats ? 1 : 0, a, b);
}

bool width_ok(uint32_t w) { return w == 16 || w == 24 || w == 32; }

// What launch_jobs asked of a periodic group's geometry when the launch read or wrote PCM.
bool group_ok_spec(const FirFormat& f, const PeriodicGeometry& g) {
    const uint32_t nk = g.row_len / 32;
    return g.mfma == 3 && g.planes == 2 && g.cg == 2 && (g.lp == 1 || (f.in_bits == 0 && g.lp > 1)) &&
           ((g.rounds == 1 && nk == 5) || (g.rounds == 2 && (nk == 5 || nk == 6)));
}

// What the PCM entries asked of the widths and of a stream's channel count, in their order.
FormatFault stream_fault_spec(const FirFormat& f, size_t ch) {
    if ((f.in_bits != 0 && !width_ok(f.in_bits)) || (f.out_bits != 0 && !width_ok(f.out_bits))) return FormatFault::kWidth;
    if (!f.pcm()) return FormatFault::kNone;
    if (f.in_bits != 0 && ch != 2) return FormatFault::kInChannels;
    if (ch % 2 != 0 || ch > 16) return FormatFault::kOutChannels;
    return FormatFault::kNone;
}

}  // namespace

int main() {
    static const uint32_t rates[10] = {22050, 16000, 32000, 44100, 48000, 88200, 96000, 176400, 192000, 384000};
    static const uint32_t taps_of[4] = {16, 32, 64, 128};
    static const uint32_t channels_of[9] = {1, 2, 3, 4, 6, 8, 12, 16, 17};
    static const bool modes[3][2] = {{true, true}, {false, true}, {true, false}};
    static const uint32_t widths[5] = {0, 16, 24, 32, 8};
    FirFormat formats[100];
    int n_formats = 0;
    for (uint32_t in_bits : widths)
        for (uint32_t out_bits : widths)
            for (uint32_t dither = 0; dither < 2; ++dither)
                for (int stats = 0; stats < 2; ++stats) formats[n_formats++] = FirFormat{in_bits, out_bits, dither, stats != 0};
    uint32_t pairs[91][2];
    int n_pairs = 0;
    for (int i = 0; i < 10; ++i)
        for (int o = 0; o < 10; ++o)
            if (i != o) {
                pairs[n_pairs][0] = rates[i];
                pairs[n_pairs++][1] = rates[o];
            }
    pairs[n_pairs][0] = 24000;
    pairs[n_pairs++][1] = 16000;

    // ---- the periodic groups' part, and split_build_for's agreement with it ----
    unsigned long group_none_f32 = 0, group_none_pcm = 0, group_in = 0, group_out = 0, build_none = 0, build_unsupported = 0, geometries = 0,
                  split_geometries = 0;
    for (uint32_t taps : taps_of)
        for (uint32_t ch : channels_of)
            for (const auto& mode : modes)
                for (int p = 0; p < n_pairs; ++p) {
                    const uint32_t g0 = std::gcd(pairs[p][0], pairs[p][1]);
                    const PeriodicGeometry g = periodic_geometry(pairs[p][0] / g0, pairs[p][1] / g0, taps, ch, mode[0], mode[1]);
                    ++geometries;
                    split_geometries += g.mfma == 3 ? 1 : 0;
                    for (const FirFormat& f : formats) {
                        const FormatFault got = format_group_fault(f, g);
                        if (!f.pcm()) {   // (f32 in and out: no launch was ever refused for its format)
                            expect(got == FormatFault::kNone, "group fault of an f32 launch", f, taps, ch);
                            ++group_none_f32;
                            continue;
                        }
                        expect(got == FormatFault::kNone || got == (f.in_bits != 0 ? FormatFault::kInGroup : FormatFault::kOutGroup),
                               "group fault kind", f, taps, ch);
                        if (stream_fault_spec(f, ch) == FormatFault::kWidth) {   // (refused by the width before any group is asked)
                            expect(got != FormatFault::kNone, "group fault at an invalid width", f, taps, ch);
                            continue;
                        }
                        expect((got == FormatFault::kNone) == group_ok_spec(f, g), "group fault against the rule it replaced", f, taps, ch);
                        if (g.mfma == 3) {
                            const BuildError e = split_build_for(g, false, f).error;
                            expect((got == FormatFault::kNone) == (e == BuildError::kNone), "group fault against split_build_for", f, taps, ch);
                            expect(e != BuildError::kInvalid, "split_build_for: invalid", f, taps, ch);
                            (e == BuildError::kNone ? build_none : build_unsupported) += 1;
                        }
                        (got == FormatFault::kNone ? group_none_pcm : got == FormatFault::kInGroup ? group_in : group_out) += 1;
                    }
                }

    // ---- the streams' part ----
    unsigned long stream_count[4] = {0, 0, 0, 0};   // kNone, kWidth, kInChannels, kOutChannels
    for (const FirFormat& f : formats)
        for (uint32_t ch = 1; ch <= 18; ++ch) {
            const FormatFault got = format_stream_fault(f, ch);
            expect(got == stream_fault_spec(f, ch), "stream fault", f, ch, 0);
            if (static_cast<int>(got) < 4) ++stream_count[static_cast<int>(got)];
        }

    // ---- which build stores the output ----
    unsigned long mode_count[4] = {0, 0, 0, 0};
    for (const FirFormat& f : formats) {
        const FirOut want = f.out_bits == 0 ? kFirOutF32 : f.stats ? kFirOutPcmStats : f.dither == 1 ? kFirOutPcmTpdf : kFirOutPcm;
        expect(f.out_mode() == want, "out_mode", f, 0, 0);
        if (f.in_bits == 0) ++mode_count[f.out_mode()];   // (the twenty combinations of out_bits, dither, stats)
    }
    static_assert(FirFormat{0, 16, 1, true}.out_mode() == kFirOutPcmStats && FirFormat{0, 0, 1, true}.out_mode() == kFirOutF32 &&
                      FirFormat{0, 24, 1, false}.out_mode() == kFirOutPcmTpdf && FirFormat{16, 32, 0, false}.out_mode() == kFirOutPcm,
                  "counted wins over dithered, neither without PCM output");
    static_assert(kFirOutF32 == 0 && kFirOutPcm == 1 && kFirOutPcmTpdf == 2 && kFirOutPcmStats == 3, "the kernels' template argument OUT");

    // ---- what the launch phases ask ----
    unsigned long tiled[2] = {0, 0}, share[2] = {0, 0};
    for (const FirFormat& f : formats) {
        for (uint32_t lo = 1; lo <= 4; ++lo)
            for (uint32_t hi = lo; hi <= 4; ++hi) {
                const bool got = generic_tiled_ok(f, lo, hi);
                expect(got == (f.out_bits == 0 || (lo == 2 && hi == 2)), "generic_tiled_ok", f, lo, hi);
                ++tiled[got ? 1 : 0];
            }
        const bool got = split_groups_may_share(f);
        expect(got == (f.in_bits == 0 && f.out_bits == 0), "split_groups_may_share", f, 0, 0);
        ++share[got ? 1 : 0];
    }

    // ---- the texts: one per fault, each naming the conversion the caller is sent to ----
    static const struct { FormatFault fault; const char* names; } texts[5] = {
        {FormatFault::kWidth, "rsmp_f32_to_pcm_device"},          {FormatFault::kInChannels, "rsmp_pcm_to_stereo_f32_device"},
        {FormatFault::kOutChannels, "rsmp_f32_to_pcm_device"},    {FormatFault::kInGroup, "rsmp_pcm_to_stereo_f32_device"},
        {FormatFault::kOutGroup, "rsmp_f32_to_pcm_device"}};
    unsigned long texts_ok = 0;
    for (const auto& t : texts) {
        const char* text = format_fault_text(t.fault);
        bool ok = strstr(text, t.names) != nullptr;
        for (const auto& o : texts) ok = ok && (o.fault == t.fault || strcmp(text, format_fault_text(o.fault)) != 0);
        expect(ok, "fault text", FirFormat{}, static_cast<uint32_t>(t.fault), 0);
        texts_ok += ok ? 1 : 0;
    }
    expect(format_fault_text(FormatFault::kNone)[0] == '\0', "no text without a fault", FirFormat{}, 0, 0);

    printf("count geometries %lu\ncount split_geometries %lu\n", geometries, split_geometries);
    printf("count group_none_f32 %lu\ncount group_none_pcm %lu\ncount group_in %lu\ncount group_out %lu\n", group_none_f32, group_none_pcm, group_in,
           group_out);
    printf("count build_none %lu\ncount build_unsupported %lu\n", build_none, build_unsupported);
    printf("count stream_none %lu\ncount stream_width %lu\ncount stream_in_channels %lu\ncount stream_out_channels %lu\n", stream_count[0],
           stream_count[1], stream_count[2], stream_count[3]);
    printf("count mode_f32 %lu\ncount mode_pcm %lu\ncount mode_pcm_tpdf %lu\ncount mode_pcm_stats %lu\n", mode_count[0], mode_count[1], mode_count[2],
           mode_count[3]);
    printf("count tiled_no %lu\ncount tiled_yes %lu\ncount share_no %lu\ncount share_yes %lu\ncount texts %lu\n", tiled[0], tiled[1], share[0],
           share[1], texts_ok);
    if (failures) {
        fprintf(stderr, "fir_format_check: %d checks failed\n", failures);
        return 1;
    }
    printf("fir_format_check: ok\n");
    return 0;
}
