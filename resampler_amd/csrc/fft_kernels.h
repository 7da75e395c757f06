// fft_kernels.h -- device-side descriptors and launch wrappers of the FFT overlap-add path.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/resampler_amd.h"   // rsmp_pcm_stats
#include "fft_launch.h"

namespace rsmp {

constexpr int kMaxFftStages = 8;

// Device image of one FftResamplerPlan (fft_plan.h).  All pointers are HBM pointers.
struct FftPlanDev {
    uint32_t fft_in, fft_out;            // frames per block = complex FFT lengths (N/2 trick)
    uint32_t n_stages_f, n_stages_i;
    uint32_t radix_f[kMaxFftStages], radix_i[kMaxFftStages];
    uint32_t tw_off_f[kMaxFftStages], tw_off_i[kMaxFftStages];
    const float2* tw_f;                  // forward stage twiddles (unique per column)
    const float2* tw_i;                  // inverse stage twiddles
    const float2* rc_f;                  // real-FFT expansion twiddles (x0.5)
    const float2* rc_i;                  // real-FFT reduction twiddles (conjugated)
    uint32_t n_rc_f, n_rc_i;
    const float2* filter;                // fft_in + 1 bins
    uint32_t new_length;                 // bins multiplied by the filter, the rest are zero
    uint32_t lds_complex;                // max(fft_in, fft_out) + 1
    const float2* chirp_f;               // exp(-2 pi i n / (2 fft_in)), n < fft_in   (fft_pair.hip: two channels as one complex signal)
    const float2* chirp_i;               // exp(-2 pi i n / (2 fft_out)), n < fft_out
};

// One stream's share of a launch: n_blocks consecutive blocks of all its channels.
struct FftStreamDesc {
    const float* in;      // interleaved, n_blocks * fft_in * channels values
    float* out;           // interleaved, n_blocks * fft_out * channels values
    const float* overlap; // stream state before the launch: [channels][fft_out] (resampler_fft.rs:51)
    float* overlap_next;  // receives the state after the launch (another buffer: the workgroup that reads
                          // the old state and the one that writes the new one are not ordered)
    uint32_t n_blocks;
    uint32_t channels;
    uint32_t in_bits;     // 0: `in` is f32; 16 / 24 / 32: `in` is little-endian PCM of that width (two-channel streams on the wave kernel only)
    uint32_t out_bits;    // 0: `out` receives f32; 16 / 24 / 32: `out` is a byte buffer that receives little-endian PCM of that width
                          // (24-bit packed), n_blocks * fft_out frames (the PCM-output builds of the pair kernel only: no other kernel reads it)
};
// What the PCM-output builds know about a stream beyond its FftStreamDesc: an array parallel to the descriptors, passed to
// those builds alone.  Value (frame n of the launch, channel c) takes the noise of index (abs_out + n) * 2 + c (fir_pcm_dither).
struct FftPcmOutDesc {
    uint64_t seed;        // the stream's own
    uint64_t abs_out;     // output frames the handle had produced before this launch
    uint32_t dither;      // RSMP_DITHER_NONE / RSMP_DITHER_TPDF: one mode for all the streams of a launch
    float pcm_k;          // the factor every store multiplies by: f32(gain) * 2^(out_bits-1), the stream's own gain (fir_pcm_gain_scale)
    uint32_t shape;       // RSMP_DITHER_SHAPE_*: one shape for all the streams of a launch, read under RSMP_DITHER_TPDF only (fir_dither_value_hp)
    uint32_t reserved;
};
static_assert(sizeof(FftPcmOutDesc) == 32, "read by the PCM-output builds alone: the f32 kernels do not know the type");

// pcm_bits != 0: every stream's `in` is PCM of that width (FftStreamDesc::in_bits); hipErrorNotSupported where no kernel
// that reads PCM serves the plan / channel count.  Which kernel, grid, block and LDS a launch gets: fft_launch.h.
// out_bits != 0 (with d_pcm, the streams' FftPcmOutDesc): every stream's `out` receives PCM of that width
// (FftStreamDesc::out_bits); hipErrorNotSupported where the launch is not the pair kernel's (fft_pcm_out_served).
hipError_t launch_fft_ola(const FftPlanDev& plan, const FftStreamDesc* d_descs, uint32_t n_streams,
                          uint32_t max_blocks, uint32_t max_channels, uint32_t min_channels,
                          hipStream_t stream, uint32_t pcm_bits = 0, uint32_t out_bits = 0, const FftPcmOutDesc* d_pcm = nullptr,
                          rsmp_pcm_stats* const* d_acc = nullptr);
// d_acc != nullptr (with out_bits != 0): the launch also counts what it stores (the counting builds, fft_pair_pcm_stats.hip) and
// merges stream i's counts into *d_acc[i], its handle's totals in device memory -- a table of its own behind the FftPcmOutDesc
// array, whose 24 bytes per stream every PCM build reads and which therefore stays as it is.
// Whether a launch of two-channel streams with PCM output gets a kernel: asked before anything is touched.
bool fft_pcm_out_served(const FftPlanDev& plan, uint32_t n_streams, uint32_t max_blocks, uint32_t pcm_bits, uint32_t out_bits);
// The kernel files' launchers: the build `c` names (fft_choose), launched as it says; hipErrorNotSupported where the file
// was not built with it (the timing experiments' builds).  fft_pair.hip: one wave per two-channel stream, the frame
// (L, R) as the complex sample L + i R; fft_wave.hip: a wave per channel; fft_kernels.hip: the workgroup kernels.
hipError_t launch_fft_ola_pair(const FftLaunch& c, const FftPlanDev& plan, const FftStreamDesc* d_descs, hipStream_t stream);
hipError_t launch_fft_ola_pair_pcm_out(const FftLaunch& c, const FftPlanDev& plan, const FftStreamDesc* d_descs, const FftPcmOutDesc* d_pcm,
                                       hipStream_t stream);   // fft_pair_pcm_out.hip: the pair launch of a request with out_bits != 0
hipError_t launch_fft_ola_pair_pcm_stats(const FftLaunch& c, const FftPlanDev& plan, const FftStreamDesc* d_descs, const FftPcmOutDesc* d_pcm,
                                         rsmp_pcm_stats* const* d_acc, hipStream_t stream);   // fft_pair_pcm_stats.hip: ... and pcm_stats
hipError_t launch_fft_ola_wave(const FftLaunch& c, const FftPlanDev& plan, const FftStreamDesc* d_descs, hipStream_t stream);
hipError_t launch_fft_ola_workgroup(FftLaunch c, const FftRequest& rq, const FftPlanDev& plan, const FftStreamDesc* d_descs,
                                    hipStream_t stream);
// Whether this library's wave kernels are the operation-for-operation build (libresampler_amd_fftexact.so).
bool fft_wave_is_exact();
// filter_spectrum[0 .. fft_in] = forward real FFT of d_filter_time[0 .. 2*fft_in)
// (resampler_fft.rs:375-376); plan.filter is ignored.
hipError_t launch_fft_filter_spectrum(const FftPlanDev& plan, const float* d_filter_time,
                                      float2* d_filter_spectrum, hipStream_t stream);
size_t fft_big_lds_bytes(const FftPlanDev& plan);   // one-buffer kernel of the largest plans
size_t fft_ola_lds_bytes(const FftPlanDev& plan, uint32_t channels);

}  // namespace rsmp
