// fir_generic_plan.h -- which kernel the generic (reference-form) streams of a FIR launch get: the latency kernel
// (fir_generic.hip) or the tiled one (fir_generic_bulk.hip), which build of the tiled one, its tile, grid and LDS -- and the
// numbers that rule shares with the two kernel files.  Plain C++, no HIP header below it; the rule itself is in fir_geometry.cpp
// and is compiled by a host compiler for the stand-alone tests (tests/host/fir_generic_builds_dump.cpp).
#pragma once

#include <cstddef>
#include <cstdint>

#include "fir_format.h"

namespace rsmp {

constexpr uint32_t kFirTile = 32;           // output frames per workgroup tile (latency kernel): one pass of 32 x 8 lanes
constexpr uint32_t kFirBulkMinOut = 8192;   // launches whose longest generic stream produces fewer frames keep fir_generic_kernel

// ---- the tiled kernel's tile and its LDS (fir_generic_bulk.hip lays the regions out in this order)
constexpr uint32_t kBulkTileMax = 4096;              // output frames per workgroup
constexpr uint32_t kBulkTileMin = 512;               // a smaller tile: none (the latency kernel)
constexpr uint32_t kBulkWindowBytes = 64u * 1024u;   // LDS for the input window
constexpr uint32_t kBulkRows = 1024;                 // phases (resampler_fir.rs:17): the counting sort's counts and offsets, a word each
constexpr uint32_t kBulkScanWords = 32;              // the scan's wave totals (16 used)
constexpr uint32_t kBulkSegs = 256;                  // run descriptors of a tile kept in LDS (a 512-frame call is ~10 runs: a tile of 4096 outputs ~80)
constexpr uint32_t kBulkMetaBytes = 8;               // BulkMeta, one per output frame of the tile
constexpr uint32_t kBulkSortedBytes = 2;             // the tile's outputs by phase row, a uint16 each
constexpr uint32_t kBulkWindowAlign = 16;            // the window starts at the next multiple
constexpr uint32_t kBulkLdsOptIn = 160u * 1024u;     // hipFuncAttributeMaxDynamicSharedMemorySize of every tiled build

// Frames of `max_channels` channels the window region holds.
constexpr uint32_t generic_bulk_window_cap(uint32_t max_channels) { return max_channels ? kBulkWindowBytes / (4u * max_channels) : 0u; }

// Tiles of `tile` output frames whose windows fit the LDS for every stream of the launch: the largest multiple of 64 up to
// kBulkTileMax with ceil(tile * max_ratio) + taps + 2 frames of max_channels channels inside kBulkWindowBytes; 0 = none (many
// channels at a high ratio: the caller keeps fir_generic_kernel).
uint32_t fir_generic_bulk_tile(uint32_t max_channels, uint32_t max_taps, double max_ratio);

// What launch_jobs knows of a launch's generic streams.
struct GenericLaunchRequest {
    FirFormat format;
    uint32_t max_out = 0;                        // output frames of the longest generic stream
    uint32_t min_channels = 0, max_channels = 0;
    uint32_t min_taps = 0, max_taps = 0;
    double max_ratio = 0.0;                      // in_hz / out_hz, the largest
};
enum class GenericKernel { kLatency, kTiled };
// Why a launch keeps the latency kernel (kNone: it is tiled), in the order the rule asks.
enum class GenericLatencyReason { kNone, kSwitchedOff, kShort, kNoTile, kFormat };
struct GenericLaunchChoice {
    GenericKernel kernel = GenericKernel::kLatency;
    GenericLatencyReason reason = GenericLatencyReason::kShort;
    // tiled: the build <ch_build, full> -- ch_build 1 / 2 = every stream has that many channels, 0 = any counts; full = every stream
    // has 128 taps (the PCM-output builds: ch_build 2 always) --, the tile, the frames the window region holds and the LDS bytes;
    // latency: all zero.  grid_x: workgroups per stream, of either kernel.
    int ch_build = 0;
    bool full = false;
    uint32_t tile = 0, window_cap_frames = 0, grid_x = 0, lds_bytes = 0;
};
// bulk_on: RSMP_FIR_GENERIC_BULK (debug) is not 0.  max_out == 0: nothing to launch (latency, grid_x 0).
GenericLaunchChoice generic_launch_choice(const GenericLaunchRequest& rq, bool bulk_on = true);

}  // namespace rsmp
