// fir_lockstep_plan.h -- everything about the lock-step batch (fir_lockstep.h) that is decided on the host without a device:
// the geometry of a (rate pair, taps, channels, step size) combination and the byte layout of the step kernel's LDS that
// it sizes, how a class of streams is cut into workgroups and in which order they are dispatched, and the grids, blocks and
// CU reserve of the run planner's three kernels (fir_lockstep_geometry.cpp).  The lock-step counterpart of
// fir_periodic_plan.h.  Plain C++: standard headers only; fir_lockstep.h adds what needs the runtime's types.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include "fir_periodic_plan.h"
#include "rsmp_hd.h"

namespace rsmp {

constexpr uint32_t kLsWaves = 8;              // waves per workgroup (two workgroups per CU: <= 128 VGPRs)
constexpr uint32_t kLsMaxSlots = 16;          // streams per workgroup
constexpr uint32_t kLsSegCap = 40;            // exact position runs kept per stream and step
constexpr uint32_t kLsMaxBlk = 12;            // 16-tap blocks of a tile window held in registers (row_len <= 192)
constexpr uint32_t kLsLdsLimit = 160 * 1024;
constexpr uint32_t kLsLdsPerWorkgroup = 80 * 1024 - 512;   // two workgroups per CU (160 KB, less the allocation granule)
constexpr uint32_t kLsImageRowBytes = 160;   // split image: (2 channels x 2 planes) x 32 B + 32 B of padding (fir_split.hip)
constexpr uint32_t kLsImageRowBytesPacked = 128;   // ... without the padding
constexpr uint32_t kLsSyncBytes = 32;         // n_cols, unit counter, image counter, early flag, ready counter

struct LockstepGroup {         // one workgroup's share: `count` streams of one geometry (HBM)
    uint32_t first, count;     // streams [first, first + count) of the batch's internal order
    uint32_t channels, taps;
    uint32_t periodic;         // 0: every output in the reference's two-row form (any ratio)
    uint32_t num, den;         // in_hz / out_hz reduced
    uint32_t a, b;             // super period: a = r * num input frames -> b = r * den outputs
    uint32_t row_len, n_tiles; // padded window of a 16-class tile; tiles per super period
    uint32_t guard_frames;     // zeroed frames in front of a stream's span in LDS (>= a)
    uint32_t span_frames;      // capacity of the span itself (buffered + new frames)
    uint32_t region_frames;    // guard + span + zeroed tail (>= a + row_len)
    uint32_t max_out;          // output frames one step can produce
    uint32_t wrap_words;       // bitmap words per stream: ceil(max_out / 32)
    uint32_t wrap_cap;         // wrap list entries per stream
    uint32_t max_cols;         // column table entries
    const float* class_coef;   // [tile][row_len / 16][64 lanes][4 steps] (A-operand order)
    const TileMeta* class_meta;
    uint32_t lds_bytes;        // what this group needs
    uint32_t slots;            // streams per workgroup the LDS layout is sized for (>= count)
    uint32_t split;            // 1: two-channel streams on the fp16 matrix cores with split operands (fir_split.hip's
                               //    arithmetic): class_coef is the split table, the LDS holds a transposed fp16 image
    uint32_t rows;             // split: rows (frames) of the image: last tile's window start + row_len
    uint32_t row_bytes;        // split: bytes per image row: 160 (32 B of padding: conflict-free transposed reads), or
                               //        128 where only the unpadded image leaves room for two workgroups per CU
    uint32_t pad0;             // (host side only: which DriftClass the group's tables belong to)
};

// ---- the step kernel's LDS ------------------------------------------------------------------------------------------------
// The fixed regions at its front, in this order; the kernel's structs are held to these sizes where it declares them.
constexpr uint32_t kLsPlanLdsBytes = 64;                                  // sizeof(PlanLds): one stream's step
constexpr uint32_t kLsStashSlotBytes = 96;                                // room per stream in the stash; a state takes 88 of it
constexpr uint32_t kLsFrontPlans = kLsMaxSlots * kLsPlanLdsBytes;         // plan records: PlanLds[16]
constexpr uint32_t kLsFrontSync = kLsSyncBytes;                           // sync words
constexpr uint32_t kLsFrontStash = kLsMaxSlots * kLsStashSlotBytes;       // state stash: FirMirrorState[16] packed at its front, then channel 0's peaks
constexpr uint32_t kLsFrontPeaks1 = 64;                                   // channel 1's peaks: colpeak1[16]
constexpr uint32_t kLsFrontPtrs = kLsMaxSlots * 32;                       // pointers: (hist, in, hist_next) per slot
constexpr uint32_t kLsStashOff = kLsFrontPlans + kLsFrontSync;
// the 128 bytes of the stash behind its sixteen states: colpeak[16] (channel 0), peak counter, the columns' scales: channel 0
// (4 words), channel 1 (4 words)
constexpr uint32_t kLsPeakOff = kLsStashOff + kLsMaxSlots * static_cast<uint32_t>(sizeof(FirMirrorState));
constexpr uint32_t kLsPeak1Off = kLsStashOff + kLsFrontStash;             // (a scale per channel, as fir_split.hip)
constexpr uint32_t kLsPtrsOff = kLsPeak1Off + kLsFrontPeaks1;
static_assert(sizeof(FirMirrorState) == 88 && kLsStashSlotBytes >= sizeof(FirMirrorState), "the stash holds 16 states of 88 bytes in 16 x 96 bytes");
static_assert(kLsPeakOff + 25 * 4 <= kLsPeak1Off, "the last 128 bytes of the stash hold channel 0's 25 words of column peaks");
static_assert(kLsMaxSlots * 4 <= kLsFrontPeaks1 && kLsPeakOff % 4 == 0 && kLsPtrsOff % 16 == 0, "colpeak1[16]; aligned pointers behind it");

struct LsLayout {
    uint32_t ptrs, colsrc, cols, segs, wbits, wlist, spans, total;   // byte offsets
};
// data_bytes: the spans of the streams (slots x region_frames x channels f32) or the split image (rows x 160 B)
RSMP_HD inline LsLayout ls_layout(uint32_t slots, uint32_t max_cols, uint32_t wrap_words, uint32_t wrap_cap, uint32_t data_bytes) {
    LsLayout l;
    l.ptrs = kLsPtrsOff;
    l.colsrc = l.ptrs + kLsFrontPtrs;
    l.cols = l.colsrc + 16 * 32;                                  // split: where each of the 16 columns' frames come from
    l.segs = (l.cols + max_cols * 16 + 7) & ~7u;
    l.wbits = l.segs + slots * kLsSegCap * 24;
    l.wlist = l.wbits + slots * wrap_words * 4;
    l.spans = (l.wlist + slots * wrap_cap * 4 + 15) & ~15u;
    l.total = l.spans + data_bytes;
    return l;
}
RSMP_HD inline uint32_t ls_data_bytes(bool split, uint32_t rows, uint32_t row_bytes, uint32_t slots, uint32_t region_frames,
                                      uint32_t channels) {
    return split ? rows * row_bytes : slots * region_frames * channels * 4u;
}

// A plan record (LsPlanHeader, fir_lockstep.h): the header, kLsSegCap runs of 24 B each, then the wrap list.
constexpr uint32_t kLsRecSegs = 160, kLsRecWraps = kLsRecSegs + kLsSegCap * 24;
inline uint32_t lockstep_rec_stride(uint32_t wrap_cap) { return (kLsRecWraps + 4 * wrap_cap + 15) / 16 * 16; }

// ---- geometry (fir_lockstep_geometry.cpp) ---------------------------------------------------------------------------------
// Geometry of one (rate pair, taps, channels, step size) combination.
struct LockstepGeometry {
    bool periodic = false;
    uint32_t num = 0, den = 0, r = 0, a = 0, b = 0, taps = 0, row_len = 0, n_tiles = 0;
    uint32_t guard_frames = 0, span_frames = 0, region_frames = 0, max_out = 0, cols_per_stream = 0;
    uint32_t slots = 1;        // streams per workgroup
    uint32_t wrap_words = 0, wrap_cap = 0, max_cols = 0, lds_bytes = 0;
    bool split = false;        // fp16x2 split operands (two-channel streams, unless exact f32 products are asked for)
    uint32_t rows = 0;         // split: rows of the LDS image
    uint32_t row_bytes = 0;    // split: bytes per image row (160, or 128 without padding)
};
// allow_split = false: exact-f32 products (RSMP_FIR_KERNEL_PERIODIC_F32 on the streams, or RSMP_LS_EXACT=1).
// lds_bytes == 0: the combination does not fit the LDS.
LockstepGeometry lockstep_geometry(uint64_t num, uint64_t den, double ratio, uint32_t taps,
                                   uint32_t channels, uint32_t step_frames, bool allow_split = true);
// The PeriodicGeometry view of it that build_class_table understands (f32 matrix-core layout, or the split
// kernel's fp16x2 layout).
PeriodicGeometry lockstep_class_geometry(const LockstepGeometry& g);

// ---- workgroups (fir_lockstep_geometry.cpp) -------------------------------------------------------------------------------
// The streams [first, end) of the batch's internal order, all of geometry `geo` and drift class `class_index`, cut into
// workgroups of geo.slots streams and appended to `groups`.
struct LsCutMax { uint32_t lds_bytes, rec_stride; };   // the largest a launch (dynamic LDS) and a plan record must hold
LsCutMax lockstep_cut_groups(std::vector<LockstepGroup>& groups, const LockstepGeometry& geo, uint32_t channels, size_t first, size_t end,
                             const float* class_coef, const TileMeta* class_meta, uint32_t class_index);
// Workgroup order = dispatch order on a device of `cus` CUs: the slow geometries first, the very slowest alone on a CU.
void lockstep_order_groups(std::vector<LockstepGroup>& groups, uint32_t cus);

// ---- the run planner's launches (fir_lockstep_geometry.cpp) ---------------------------------------------------------------
// The planner's serial kernels (chain, replay) pack kLsPlanPack streams into a workgroup -- one CU -- for batches of fewer than
// kLsPlanPackBelow streams: the CUs they take are then few and known (LsPlanShape), whoever reaches the chip first.
constexpr uint32_t kLsPlanPack = 4, kLsPlanPackBelow = 256;   // (pack 1 / 2 / 4 / 8 at 128 streams: 0.89 / 0.71-0.86 / 0.73 / 0.83-0.95 us per step, profiles/r06/ab_c4_shard.txt: eight waves of this much CODE on one CU starve each other of instructions)
// The replay (K3) of a small batch gives every chunk of 64 calls a wave of its own, a round of at most this many at a time.
constexpr uint32_t kLsWrapWaves = 16;   // (at most: a run of 256 calls has four chunks, a bulk launch of 4096 calls sixty-four)
uint32_t lockstep_plan_pack(size_t n_streams);   // (RSMP_LS_PACK, debug: 1 / 2 / 4 -- the chain kernel is bounded to 64 * kLsPlanPack threads)
// What launch_fir_lockstep_plan launches for a run of k calls per stream, and the CUs that takes.
struct LsPlanShape {
    uint32_t k1_blocks_per_stream, k1_grid;   // K1 (predictions): blocks of 256 calls
    uint32_t pack, k2_grid, k2_block;         // K2 (chain): `pack` streams per workgroup, a wave each
    uint32_t k3_waves;                        // K3 (replay): one workgroup per stream; a wave per chunk of 64 calls for packed batches, else one
    uint32_t parallel_chain;                  // K2: chunks of lean calls by the parallel chain (RSMP_LS_PCHAIN=0, debug: never)
    uint32_t chain_cus;                       // CUs the chain takes (unpacked: four one-wave workgroups a CU)
    uint32_t replay_cus;                      // CUs the replay of a packed batch takes: sixteen waves a CU (unpacked: 0, not reserved for)
};
LsPlanShape lockstep_plan_shape(size_t n_streams, uint32_t k);

}  // namespace rsmp
