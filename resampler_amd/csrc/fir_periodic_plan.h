// fir_periodic_plan.h -- everything about the periodic kernels that is decided on the host without a device: the geometry
// of a launch (fir_geometry.cpp), which kernel build runs it, the class-table image (fir_class_table.cpp), the deal of
// workgroups among the jobs of a shared launch (fir_split_deal.cpp), and what the host planner (fir_hostplan.cpp) asks.
// Plain C++: standard headers only, never a HIP header.  fir_periodic.h adds what needs HIP types.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include "fir_format.h"
#include "fir_plan.h"

namespace rsmp {

constexpr uint32_t kClassTile = 8;
constexpr uint32_t kMfmaClassTile = 16;   // classes per tile of the matrix-core kernels (M of 16x16x4 / 16x16x32)

struct PeriodicGeometry {
    bool ok = false;
    uint32_t a = 0, b = 0;       // super period: a input frames -> b output frames
    uint32_t den = 0;            // true period of the phase pattern (b = r * den)
    uint32_t taps = 0;
    uint32_t row_len = 0;        // taps + max in-tile shift, rounded up to whole chunks (8; mfma 48; split kernel 32)
    uint32_t n_tiles = 0;        // ceil(b / class tile); class tile = 8 (vector kernels) or 16 (mfma)
    uint32_t cg = 0;             // channels per lane (1 or 2); split kernel: 1 one channel, 2 pairs, 3 odd count
    uint32_t lp = 0;             // lanes per period = channels / cg; split kernel: channel pairs of a frame
    uint32_t pw = 0;             // periods per workgroup (<= 64 / lp)
    uint32_t row_stride = 0;     // LDS dwords between period rows (odd frame count: conflict-free); split kernel: rows of an image
    uint32_t waves = 0;          // waves per workgroup
    uint32_t producers = 0;      // > 0 (matrix-core kernels only): double-buffered kernel, this many waves only stage
    uint32_t images = 0;         // double-buffered kernels: LDS images in the ring (split kernel: 2 to 4; else 2)
    uint32_t mfma = 0;           // > 0: matrix-core kernel (16-class tiles); period groups of 16 per work unit;
                                 // 3: split kernel (fir_split.hip)
    uint32_t planes = 0;         // split kernel: 16-bit planes per f32 operand (3: bf16, exact; 2: fp16)
    uint32_t groups = 0;         // split kernel: tile groups of ten class tiles (1 or 2)
    uint32_t rounds = 0;         // split kernel: rounds of lane tasks per stager and item (1: periods <= 160 frames; 2: <= 320)
    uint32_t n_units = 0;        // work units per item: n_tiles (vector kernels) or tiles x unit splits (mfma)
    uint32_t lds_bytes = 0;
    bool inline_wraps = false;   // den >= 8: wrap variant computed inside the kernel
    bool operator==(const PeriodicGeometry& o) const {
        return a == o.a && b == o.b && den == o.den && taps == o.taps && row_len == o.row_len &&
               cg == o.cg && lp == o.lp && pw == o.pw && row_stride == o.row_stride &&
               waves == o.waves && producers == o.producers && mfma == o.mfma && images == o.images &&
               planes == o.planes;
    }
};

// First input frame of class j's window, relative to the period start: floor(j a / b).
inline uint32_t class_offset(uint32_t a, uint32_t b, uint32_t j) {
    return static_cast<uint32_t>((static_cast<uint64_t>(j) * a) / b);
}

// ---- geometry (fir_geometry.cpp) -------------------------------------------------------------------------------------
// allow_matrix = false: vector kernels only (RSMP_FIR_KERNEL_PERIODIC_VECTOR); allow_split = false:
// never the split-bf16 kernel (RSMP_FIR_KERNEL_PERIODIC_F32)
PeriodicGeometry periodic_geometry(uint64_t num, uint64_t den, uint32_t taps, uint32_t channels,
                                   bool allow_matrix = true, bool allow_split = true);
// Split-bf16 matrix kernel (fir_split.hip): mfma == 3; row_stride = rows of an LDS image.
PeriodicGeometry split_geometry(uint64_t num, uint64_t den, uint32_t taps, uint32_t channels);
// Number of period blocks (grid.x) a stream's launch needs.
uint32_t periodic_blocks(const PeriodicGeometry& geo, uint64_t abs_out, uint32_t n_out);

// What the host planner asks.
bool periodic_supported(const FirMirror& m, size_t channels, size_t taps, int kernel_mode);
bool periodic_worthwhile(const FirMirror& planned, size_t produced_frames, int kernel_mode);
// Bitmap of wrapped outputs for one launch: bit K <-> the output with absolute index
// (abs_out / den + K) * den.  Returns the number of 32-bit words.
size_t periodic_wrap_words(uint64_t abs_out, uint32_t n_out, uint64_t den);
void periodic_fill_wrap_bits(const std::vector<uint32_t>& wraps, uint64_t abs_out, uint64_t den,
                             uint32_t* words, size_t n_words);

// ---- which build of a kernel runs a geometry (fir_geometry.cpp) ------------------------------------------------------
// RSMP_FIR_MFMA_RING: the f32 matrix-core kernel's coefficient ring for every window (geometry and launch read it).
bool mfma_ring_knob();
// The split kernel's template arguments.
struct SplitBuild {
    int nk, planes;   // window steps of 32 taps; 16-bit planes
    bool diag;        // the build with the debug switches and the phase clock
    int wide;         // 0 two channels, 1 channel pairs, 2 one channel, 3 an odd channel count
    int rounds;
    int bits;         // PCM input of that width (0: f32)
    bool pcm_out;     // PCM output (its width is the descriptor's, read at run time)
    bool dither;      // ... with TPDF dither (the seeds are the descriptors')
    bool stats;       // ... counted as it is stored (SplitArgs::stat); these builds read the dither mode and shape from the descriptor (dither = false)
    bool hp = false;  // with dither: the twin that makes high-pass noise (RSMP_DITHER_SHAPE_HIGHPASS)
    bool operator==(const SplitBuild& o) const {
        return nk == o.nk && planes == o.planes && diag == o.diag && wide == o.wide && rounds == o.rounds && bits == o.bits &&
               pcm_out == o.pcm_out && dither == o.dither && stats == o.stats && hp == o.hp;
    }
};
enum class BuildError { kNone, kInvalid, kNotSupported };   // the launchers' hipErrorInvalidValue / hipErrorNotSupported
struct SplitChoice {
    SplitBuild build;
    BuildError error;
};
// diag: RSMP_FIR_DEBUG or RSMP_FIR_WTRACE is set; format: the launch's (fir_format.h).
SplitChoice split_build_for(const PeriodicGeometry& geo, bool diag, const FirFormat& format);
// The periodic groups' part of the format rule (fir_format.h): a launch that reads or writes PCM needs a build of the split kernel for
// every periodic group -- split_build_for decides.  kInGroup where the format reads PCM, else kOutGroup; kNone for f32 in and out.
FormatFault format_group_fault(const FirFormat& format, const PeriodicGeometry& geo);
// Slot of launch_fir_periodic's kernel table for a geometry of the vector or f32 matrix-core kernels, or -1 (no such
// build).  mfma_dbg: RSMP_FIR_MFMA_DBG (0 .. 3); mfma_ring: mfma_ring_knob().
constexpr int kPeriodicSlots = 20;
int periodic_slot_for(const PeriodicGeometry& geo, int mfma_dbg, bool mfma_ring);

// ---- class-table image (fir_class_table.cpp) -------------------------------------------------------------------------
// Per class tile: where its window starts and what its wrap variant (if any) needs.
struct TileMeta {
    uint32_t base;         // first input frame of the tile's window, relative to the period start
    int32_t wrap_col;      // column (0..7) whose class has an integer exact position, or -1
    uint32_t wrap_jd;      // (class index of that column) / den
    int32_t extra_col;     // frame (relative to the period start, may be -1) of the one sample
                           // the wrap window has in front of the tile window; -2 = none
    float extra_coef;      // its coefficient (row 1023, tap 0)
    uint32_t pad[3];
};
static_assert(sizeof(TileMeta) == 32, "TileMeta is read with one s_load_dwordx8");

struct HostClassTable {
    std::vector<float> coef;       // [tile][row_len][8]; mfma: [tile][row_len / 16][64 lanes][4 steps]; split: split_store_class
    std::vector<float> wrap_coef;  // [tile][row_len]
    std::vector<TileMeta> meta;    // [tile]
};
// `coeffs`: the [1024][taps] polyphase table; `drift`: the f64 drift the rows are mixed for.  Touches no device.
HostClassTable build_class_table(const std::vector<float>& coeffs, const PeriodicGeometry& g, double drift);
size_t split_table_floats(const PeriodicGeometry& g);
void split_store_class(std::vector<float>& coef, const PeriodicGeometry& g, uint32_t tile, uint32_t m,
                       uint32_t shift, const std::vector<float>& mixed);

// ---- the deal of workgroups (fir_split_deal.cpp) ---------------------------------------------------------------------
// One launch of the split kernel for several jobs: its workgroups are dealt to the jobs in proportion to their staging
// work (items x frames of a period: the stagers bound the kernel).  At least one workgroup per job and no more than it has
// items; a job with two tile groups gets a multiple of sixteen where there are sixteen to give (see the .cpp); the rest by
// largest remainder.  n <= kMaxSplitJobs.  False: fewer workgroups than jobs.
struct DealJob {
    uint32_t total_items, a, groups;
};
bool split_deal(const DealJob* jobs, uint32_t n, uint32_t cus, uint32_t* share);

}  // namespace rsmp
