// fir_format.h -- the sample format of one FIR launch as a value (one for all its streams; the seeds alone are per stream), and the
// rule which streams and launches a format is supported for (fir_geometry.cpp).  Plain C++, no HIP header.
#pragma once

#include <cstddef>
#include <cstdint>

#include "../../include/resampler_amd.h"
#include "rsmp_hd.h"

namespace rsmp {

// How a build stores its sums (the kernels' template argument OUT): f32, PCM, PCM with TPDF dither -- and PCM that is counted as
// it is stored (rsmp_fir_set_pcm_stats): builds of their own, with the dither a uniform branch on FirStreamDesc::dither.
enum FirOut : int { kFirOutF32 = 0, kFirOutPcm = 1, kFirOutPcmTpdf = 2, kFirOutPcmStats = 3 };
// The split kernel alone: its dithered builds' twins for RSMP_DITHER_SHAPE_HIGHPASS (a second mix per frame; as a run-time branch of
// the white builds it cost those 0.005 ms of a 0.35 ms launch at 16 bits: profiles/pcm_dither_shape.txt).  Not an out_mode(): the
// generic kernels and the repair pass read the shape from the descriptor, and so do the counting builds.
constexpr int kFirOutPcmTpdfHp = 4;

struct FirFormat {
    uint32_t in_bits = 0;    // 0: interleaved f32; 16 / 24 / 32: a WAV file's PCM, read in place (FirStreamDesc::in_bits)
    uint32_t out_bits = 0;   // 0: interleaved f32; 16 / 24 / 32: PCM, quantised where it is stored (FirStreamDesc::out_bits)
    uint32_t dither = 0;     // RSMP_DITHER_*, read only with out_bits != 0 (FirStreamDesc::dither)
    bool stats = false;      // the PCM output is counted (rsmp_fir_set_pcm_stats), only with out_bits != 0
    uint32_t dither_shape = 0;   // RSMP_DITHER_SHAPE_*, read only with out_bits != 0 and dither == RSMP_DITHER_TPDF (FirStreamDesc::dither_shape):
                                 // a run-time value of the generic kernels, the repair pass and every counting build; of the split
                                 // kernel's dithered builds it selects the high-pass twins (SplitBuild::hp)
    bool pcm() const { return in_bits != 0 || out_bits != 0; }
    // Counted wins over dithered (the counting builds serve both dither modes); neither exists without PCM output.
    RSMP_HD constexpr FirOut out_mode() const {
        return out_bits == 0 ? kFirOutF32 : stats ? kFirOutPcmStats : dither == RSMP_DITHER_TPDF ? kFirOutPcmTpdf : kFirOutPcm;
    }
};

// The streams' part of the rule (the periodic groups' part: format_group_fault, fir_periodic_plan.h).  kWidth: a width that is none of
// 0 / 16 / 24 / 32; kInChannels: PCM input on other than two channels; kOutChannels: PCM output on one channel, an odd count or more
// than 16 -- in this order; kInGroup / kOutGroup: no build of the split kernel reads / writes PCM for a periodic group.
enum class FormatFault { kNone, kWidth, kInChannels, kOutChannels, kInGroup, kOutGroup };
FormatFault format_stream_fault(const FirFormat& format, size_t channels);
const char* format_fault_text(FormatFault fault);   // what the caller is told (RSMP_ERR_INVALID_ARGUMENT); kNone: ""
// May the generic streams of a launch, of min .. max channels, take the tiled kernel (fir_generic_bulk.hip: its PCM-output builds are
// two-channel)?  May several periodic groups of the split kernel share launches (launch_fir_split_multi: f32 in and out)?
bool generic_tiled_ok(const FirFormat& format, uint32_t min_channels, uint32_t max_channels);
bool split_groups_may_share(const FirFormat& format);

}  // namespace rsmp
