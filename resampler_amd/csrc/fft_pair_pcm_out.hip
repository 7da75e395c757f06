// fft_pair_pcm_out.hip -- the PCM-output builds of the two-channel pair kernel (fft_pair_body.h, RSMP_PAIR_PCM_OUT) and their launcher:
// a translation unit of its own, so that they compile beside fft_pair.o and that object stays what it was.
#define RSMP_PAIR_PCM_OUT 1
#include "fft_pair_body.h"

namespace rsmp {

namespace {

typedef void (*PairPcmKernel)(FftPlanDev, const FftStreamDesc*, const FftPcmOutDesc*, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t);

// The PCM-output builds of a pair by the INPUT's BITS / 8 (the output's width is a run-time value), as fft_pair.hip's table.
struct PairBuilds { PairPcmKernel bits[5]; };
template <class FWD, class INV>
constexpr PairBuilds pair_builds() {
    if constexpr (pair_waves<FWD, INV>() == 0) return PairBuilds{{nullptr, nullptr, nullptr, nullptr, nullptr}};
    else return PairBuilds{{fft_ola_pair_pcm_kernel<FWD, INV, 0>, nullptr, fft_ola_pair_pcm_kernel<FWD, INV, 16>, fft_ola_pair_pcm_kernel<FWD, INV, 24>, fft_ola_pair_pcm_kernel<FWD, INV, 32>}};
}
template <class... Ps>
PairPcmKernel pair_pcm_kernel(PairList<Ps...>, int pair, int bits) {
    static constexpr PairBuilds table[] = {pair_builds<typename Ps::Fwd, typename Ps::Inv>()...};
    return pair < static_cast<int>(sizeof...(Ps)) ? table[pair].bits[bits / 8] : nullptr;
}

}  // namespace

// The build fft_choose (fft_launch.cpp) names for a request with out_bits != 0, launched as it says.
hipError_t launch_fft_ola_pair_pcm_out(const FftLaunch& c, const FftPlanDev& plan, const FftStreamDesc* d_descs, const FftPcmOutDesc* d_pcm,
                                       hipStream_t stream) {
#if RSMP_EXP != 0   // (timing experiments instantiate the 44.1 <-> 48 kHz pair alone)
    const PairPcmKernel fn = pair_pcm_kernel(HeadPairs{}, c.pair, c.bits);
#else
    const PairPcmKernel fn = pair_pcm_kernel(PairPairs{}, c.pair, c.bits);
#endif
    if (fn == nullptr || d_pcm == nullptr) return hipErrorNotSupported;
    if (c.whole_rows != kWholeRows) return hipErrorInvalidValue;   // (the LDS bytes are for another build of this file)
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(fn, dim3(c.grid[0]), dim3(c.block), c.lds, stream, plan, d_descs, d_pcm, c.args[0], c.args[1], c.args[2], c.args[3], c.args[4], c.args[5]);
    return hipGetLastError();
}

}  // namespace rsmp
