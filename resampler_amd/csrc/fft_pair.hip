// fft_pair.hip -- the f32-output builds of the two-channel pair kernel (fft_pair_body.h: one wave per stream, the frame
// (L, R) as the complex sample L + i R) and their launcher.  The PCM-output builds are fft_pair_pcm_out.hip's.
#define RSMP_PAIR_PCM_OUT 0
#include "fft_pair_body.h"

namespace rsmp {

namespace {

typedef void (*PairKernel)(FftPlanDev, const FftStreamDesc*, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t);

// The builds of a pair by BITS / 8 (a pair the LDS does not serve has none: the launch rules never choose it), and the
// table over a list of pairs.
struct PairBuilds { PairKernel bits[5]; };
template <class FWD, class INV>
constexpr PairBuilds pair_builds() {
    if constexpr (pair_waves<FWD, INV>() == 0) return PairBuilds{{nullptr, nullptr, nullptr, nullptr, nullptr}};
    else return PairBuilds{{fft_ola_pair_kernel<FWD, INV, 0>, nullptr, fft_ola_pair_kernel<FWD, INV, 16>, fft_ola_pair_kernel<FWD, INV, 24>, fft_ola_pair_kernel<FWD, INV, 32>}};
}
template <class... Ps>
PairKernel pair_kernel(PairList<Ps...>, int pair, int bits) {
    static constexpr PairBuilds table[] = {pair_builds<typename Ps::Fwd, typename Ps::Inv>()...};
    return pair < static_cast<int>(sizeof...(Ps)) ? table[pair].bits[bits / 8] : nullptr;
}

}  // namespace

// The build fft_choose (fft_launch.cpp) names, launched as it says.
hipError_t launch_fft_ola_pair(const FftLaunch& c, const FftPlanDev& plan, const FftStreamDesc* d_descs, hipStream_t stream) {
#if RSMP_EXP != 0   // (timing experiments instantiate the 44.1 <-> 48 kHz pair alone)
    const PairKernel fn = pair_kernel(HeadPairs{}, c.pair, c.bits);
#else
    const PairKernel fn = pair_kernel(PairPairs{}, c.pair, c.bits);
#endif
    if (fn == nullptr) return hipErrorNotSupported;
    if (c.whole_rows != kWholeRows) return hipErrorInvalidValue;   // (the LDS bytes are for another build of this file)
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(fn, dim3(c.grid[0]), dim3(c.block), c.lds, stream, plan, d_descs, c.args[0], c.args[1], c.args[2], c.args[3], c.args[4], c.args[5]);
    return hipGetLastError();
}

}  // namespace rsmp
