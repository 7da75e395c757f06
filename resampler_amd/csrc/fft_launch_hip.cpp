// fft_launch_hip.cpp -- launch_fft_ola: the plan's shape and the device's CU count into the launch rules (fft_launch.cpp),
// the decision to the kernel file that holds the build.  HIP runtime API, no kernels.
#include "fft_kernels.h"

namespace rsmp {

namespace {

FftShape shape_of(const FftPlanDev& p) {
    FftShape s{};
    s.fft_in = p.fft_in; s.fft_out = p.fft_out;
    s.n_stages_f = p.n_stages_f; s.n_stages_i = p.n_stages_i;
    for (int i = 0; i < kMaxFftStages; ++i) { s.radix_f[i] = p.radix_f[i]; s.radix_i[i] = p.radix_i[i]; }
    s.n_rc_f = p.n_rc_f; s.n_rc_i = p.n_rc_i;
    s.new_length = p.new_length; s.lds_complex = p.lds_complex;
    s.chirps = p.chirp_f != nullptr && p.chirp_i != nullptr;
    return s;
}

}  // namespace

size_t fft_big_lds_bytes(const FftPlanDev& plan) { return fft_big_lds_bytes(shape_of(plan)); }
size_t fft_ola_lds_bytes(const FftPlanDev& plan, uint32_t channels) { return fft_ola_lds_bytes(shape_of(plan), channels); }

namespace {

FftRequest request_of(uint32_t n_streams, uint32_t max_blocks, uint32_t max_channels, uint32_t min_channels, uint32_t pcm_bits, uint32_t out_bits,
                      bool pcm_stats = false) {
    int dev = 0, cus = 256;
    (void)hipGetDevice(&dev);
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    return FftRequest{n_streams, max_blocks, max_channels, min_channels, pcm_bits, fft_wave_is_exact(), cus, out_bits, pcm_stats};
}

}  // namespace

bool fft_pcm_out_served(const FftPlanDev& plan, uint32_t n_streams, uint32_t max_blocks, uint32_t pcm_bits, uint32_t out_bits) {
    if (n_streams == 0 || max_blocks == 0 || out_bits == 0) return false;
    return fft_choose(shape_of(plan), request_of(n_streams, max_blocks, 2, 2, pcm_bits, out_bits)).family == FftFamily::kPair;
}

hipError_t launch_fft_ola(const FftPlanDev& plan, const FftStreamDesc* d_descs, uint32_t n_streams,
                          uint32_t max_blocks, uint32_t max_channels, uint32_t min_channels,
                          hipStream_t stream, uint32_t pcm_bits, uint32_t out_bits, const FftPcmOutDesc* d_pcm, rsmp_pcm_stats* const* d_acc) {
    if (n_streams == 0 || max_blocks == 0) return hipSuccess;
    const FftRequest rq = request_of(n_streams, max_blocks, max_channels, min_channels, pcm_bits, out_bits, d_acc != nullptr);
    const FftLaunch c = fft_choose(shape_of(plan), rq);
    switch (c.family) {
        case FftFamily::kPair:
            if (c.pcm_stats) return launch_fft_ola_pair_pcm_stats(c, plan, d_descs, d_pcm, d_acc, stream);
            return out_bits != 0 ? launch_fft_ola_pair_pcm_out(c, plan, d_descs, d_pcm, stream) : launch_fft_ola_pair(c, plan, d_descs, stream);
        case FftFamily::kWave: return launch_fft_ola_wave(c, plan, d_descs, stream);
        case FftFamily::kNotSupported: return hipErrorNotSupported;
        case FftFamily::kInvalid: return hipErrorInvalidValue;
        default: return launch_fft_ola_workgroup(c, rq, plan, d_descs, stream);
    }
}

}  // namespace rsmp
