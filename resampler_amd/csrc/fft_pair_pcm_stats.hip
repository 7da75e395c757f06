// fft_pair_pcm_stats.hip -- the COUNTING PCM-output builds of the two-channel pair kernel (fft_pair_body.h, RSMP_PAIR_PCM_OUT 2) and
// their launcher: the stores of fft_pair_pcm_out.hip's builds, and what they did to the values merged into the handles' totals
// (rsmp_fft_set_pcm_stats).  A translation unit of its own, so that fft_pair.o and fft_pair_pcm_out.o stay what they were: whether a
// launch counts is the choice of the build, not a branch in theirs.
#define RSMP_PAIR_PCM_OUT 2
#include "fft_pair_body.h"

namespace rsmp {

namespace {

typedef void (*PairPcmStatsKernel)(FftPlanDev, const FftStreamDesc*, const FftPcmOutDesc*, rsmp_pcm_stats* const*, uint32_t, uint32_t, uint32_t, uint32_t,
                                   uint32_t, uint32_t);

// The counting builds of a pair by the INPUT's BITS / 8 (the output's width is a run-time value), as fft_pair_pcm_out.hip's table.
struct PairBuilds { PairPcmStatsKernel bits[5]; };
template <class FWD, class INV>
constexpr PairBuilds pair_builds() {
    if constexpr (pair_waves<FWD, INV>() == 0) return PairBuilds{{nullptr, nullptr, nullptr, nullptr, nullptr}};
    else return PairBuilds{{fft_ola_pair_pcm_stats_kernel<FWD, INV, 0>, nullptr, fft_ola_pair_pcm_stats_kernel<FWD, INV, 16>,
                            fft_ola_pair_pcm_stats_kernel<FWD, INV, 24>, fft_ola_pair_pcm_stats_kernel<FWD, INV, 32>}};
}
template <class... Ps>
PairPcmStatsKernel pair_pcm_stats_kernel(PairList<Ps...>, int pair, int bits) {
    static constexpr PairBuilds table[] = {pair_builds<typename Ps::Fwd, typename Ps::Inv>()...};
    return pair < static_cast<int>(sizeof...(Ps)) ? table[pair].bits[bits / 8] : nullptr;
}

}  // namespace

// The build fft_choose (fft_launch.cpp) names for a request with out_bits != 0 and pcm_stats, launched as it says: the launch of
// launch_fft_ola_pair_pcm_out with one more table, the streams' totals.
hipError_t launch_fft_ola_pair_pcm_stats(const FftLaunch& c, const FftPlanDev& plan, const FftStreamDesc* d_descs, const FftPcmOutDesc* d_pcm,
                                         rsmp_pcm_stats* const* d_acc, hipStream_t stream) {
#if RSMP_EXP != 0   // (timing experiments instantiate the 44.1 <-> 48 kHz pair alone)
    const PairPcmStatsKernel fn = pair_pcm_stats_kernel(HeadPairs{}, c.pair, c.bits);
#else
    const PairPcmStatsKernel fn = pair_pcm_stats_kernel(PairPairs{}, c.pair, c.bits);
#endif
    if (fn == nullptr || d_pcm == nullptr || d_acc == nullptr) return hipErrorNotSupported;
    if (c.whole_rows != kWholeRows) return hipErrorInvalidValue;   // (the LDS bytes are for another build of this file)
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(fn, dim3(c.grid[0]), dim3(c.block), c.lds, stream, plan, d_descs, d_pcm, d_acc, c.args[0], c.args[1], c.args[2], c.args[3], c.args[4],
                       c.args[5]);
    return hipGetLastError();
}

}  // namespace rsmp
