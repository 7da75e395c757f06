// fft_launch.h -- which FFT overlap-add kernel a launch gets, with what grid, block, LDS and scalar arguments: the rules
// that used to sit in the launchers of fft_kernels.hip, fft_wave.hip and fft_pair.hip, as plain C++ (no HIP header) that
// builds in seconds and runs under the sanitizers as a stand-alone program (tests/host/fft_launch_dump.cpp; pinned by
// tests/golden/fft_launch.json).  The kernel files keep a table from the build chosen here to its function pointer.
#pragma once

#include <cstddef>
#include <cstdint>

namespace rsmp {

// What of a plan (FftPlanDev, fft_kernels.h) the rules look at.
struct FftShape {
    uint32_t fft_in, fft_out;
    uint32_t n_stages_f, n_stages_i;
    uint32_t radix_f[8], radix_i[8];
    uint32_t n_rc_f, n_rc_i;
    uint32_t new_length, lds_complex;
    bool chirps;   // chirp_f and chirp_i exist (fft_pair.hip)
};

struct FftRequest {
    uint32_t n_streams, max_blocks;       // both > 0
    uint32_t max_channels, min_channels;
    uint32_t pcm_bits;                    // 0: f32 input
    bool exact;                           // fft_wave_is_exact(): whole twiddle rows in the wave kernels, no pair kernel
    int cus;
    // 0: f32 output.  16 / 24 / 32: PCM of that width from the kernel's store -- the pair kernel's launch exactly as for
    // out_bits = 0 (the same cut into runs), kNotSupported where that request would get another family.
    uint32_t out_bits = 0;
    // The counting builds of the PCM store (fft_pair_pcm_stats.hip): the launch of the same request without it, field for field
    // -- the flag picks the kernel file, nothing else --; with out_bits = 0 there is nothing to count: kNotSupported.
    bool pcm_stats = false;
};

enum class FftFamily : uint8_t {
    kPair,     // fft_pair.hip: a wave per two-channel stream
    kWave,     // fft_wave.hip: a wave per channel
    kCt,       // fft_kernels.hip: the 44.1 <-> 48 kHz workgroup kernel
    kCt2,      // ... its two-channel build
    kGeneric,  // ... any plan whose two buffers fit the LDS
    kBig,      // ... one buffer, in place
    kNotSupported, kInvalid
};

struct FftLaunch {
    FftFamily family = FftFamily::kNotSupported;
    // the build within the family
    int pair = 0;           // index into PairPairs / WavePairs (fft_wave_plan.h); ct, ct2: 0 = 1176 -> 1280 points, 1 = the reverse
    int chm = 0, occ = 0;   // wave: the kernel's CHM and OCC
    int bits = 0;           // pair: BITS
    bool whole_rows = false;   // pair, wave: the twiddle rows the LDS bytes are for (fft_wave_plan.h); the kernel file checks its own
    // generic: the block size is the build (64: a one-wave workgroup per channel)
    uint32_t grid[3] = {0, 1, 1}, block = 0;
    size_t lds = 0;
    bool grant_lds = false;   // hipFuncSetAttribute(MaxDynamicSharedMemorySize, 160 KiB) before the launch
    // the scalar kernel arguments behind (plan, descs) -- wave: run, runs_per_stream, total_waves, channel pairs;
    // pair: the runs of the four ages, groups per stream, total_waves; workgroup kernels: run
    uint32_t args[6] = {0, 0, 0, 0, 0, 0};
    int n_args = 0;
    bool pcm_stats = false;   // pair, out_bits != 0: the request's flag, carried to the launcher (fft_pair_pcm_stats.hip's builds)
};

// Blocks per run.  Every run after a stream's first recomputes its predecessor block (1 / run extra work), and the launch
// ends with a partly filled round unless the number of waves (or workgroups) is close to a multiple of the `slots` the chip
// holds at once: the first candidate of lo .. hi that maximises useful work per occupied slot.  `lanes` = the runs that
// cover the same blocks (streams x channels); `classes` = runs a candidate is cut into (fft_pair.hip's ages: a candidate
// is then the blocks of a group of runs).
uint32_t fft_pick_run(uint32_t max_blocks, uint32_t lanes, double slots, uint32_t lo, uint32_t hi, uint32_t classes = 1);
// fft_pair.hip: a group's `both` blocks over its `classes` (1, 2 or 4) ages.
void fft_pair_split(uint32_t both, uint32_t classes, uint32_t runs[4]);

// The whole decision.  For the pair and wave families it is complete; for the workgroup kernels (ct, ct2, generic, big) the
// run depends on the occupancy the runtime reports for the chosen build: fft_choose leaves grid[0] and args empty and
// fft_choose_run fills them in (per_cu < 1: the query failed).
FftLaunch fft_choose(const FftShape& shape, const FftRequest& rq);
void fft_choose_run(FftLaunch* launch, const FftRequest& rq, int per_cu);

size_t fft_big_lds_bytes(const FftShape& shape);   // one-buffer kernel of the largest plans
size_t fft_ola_lds_bytes(const FftShape& shape, uint32_t channels);

}  // namespace rsmp
