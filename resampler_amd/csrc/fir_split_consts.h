// fir_split_consts.h -- the numbers that tie the split kernel (fir_split.hip) to the host code that plans for it: its
// geometry (fir_geometry.cpp), its class-table image (fir_class_table.cpp), the deal of workgroups (fir_split_deal.cpp).
// Constants and constexpr functions only; standard headers and rsmp_hd.h, never a HIP header.
#pragma once

#include <cstdint>

#include "rsmp_hd.h"

namespace rsmp {

constexpr uint32_t kProducers = 6, kConsumers = 10, kWaves = 16;   // five stagers + one wrap-only producer
constexpr uint32_t kStagers = 5;                       // (row block, period pair) combos in flight per producer
static_assert(kStagers + 1 == kProducers && kProducers + kConsumers == kWaves, "one wrap-only producer; sixteen waves");

// LDS of a workgroup: control words, wrap results, the consumers' touch zone, then the ring of images.
constexpr uint32_t kCtrlBytes = 256;                   // staged[2], done[2]
constexpr uint32_t kWrapBytes = 4 * 16 * 16;           // up to four slots x 16 periods x (ch0, ch1, take, -)
constexpr uint32_t kTouchBytes = 3 * 256;              // landing zone of the consumers' L2 prefetch touches
constexpr uint32_t kImageBase = kCtrlBytes + kWrapBytes + kTouchBytes;
constexpr uint32_t kLdsLimit = 160 * 1024;
// An image row: per channel and plane one 32-byte plane row (16 periods x 16 bits), + 32 bytes of padding.
// In 32-byte units the stride is 7 (three bf16 planes) or 5 (two fp16 planes): odd, so the eight rows a
// transposed read touches per 32 lanes fall on distinct bank groups (64 banks x 4 B = 8 units).
RSMP_HD constexpr uint32_t row_bytes(int planes) { return planes == 3 ? 7u * 32u : 5u * 32u; }
static_assert(row_bytes(2) / 32 % 2 == 1 && row_bytes(3) / 32 % 2 == 1, "odd row stride in 32-byte units");

// Two-plane split: the taps are scaled by 2^13 before they are cut into fp16 planes (taps down to 2^-27 keep their full
// relative precision: fp16 normals start at 2^-14); the kernel's output scale takes the 2^13 out again.
constexpr float kCScale = 8192.0f;
constexpr int kWrapTaps = 8;                           // taps of the wrap variant per lane (16 lanes per period)

// Staging an item is four lane tasks per pair of frames of the period; a round gives the stagers 64 lanes each.  The
// kernel relies on lane tasks <= 64 * kStagers * rounds: split_geometry picks `rounds` by it, and periods stop at
// kSplitMaxAB frames, which two rounds just hold.
constexpr uint32_t kSplitMaxAB = 320;                  // frames / outputs of a (super) period at most
constexpr uint32_t split_lane_tasks(uint32_t a) { return 4 * ((a + 1) / 2); }
constexpr uint32_t split_task_room(uint32_t rounds) { return 64 * kStagers * rounds; }
static_assert(split_lane_tasks(kSplitMaxAB) <= split_task_room(2), "two rounds hold the longest period");

constexpr uint32_t kItemWords = 8;   // stream | flags << 24, pair | group << 8, n_block0, k_block0, f0 (2), off0, -

// Several jobs (rate pairs) in one launch: at most this many; fir_split_all_kernel's bodies by id.
constexpr uint32_t kMaxSplitJobs = 8;
constexpr uint32_t kSplitBuild5x1 = 0, kSplitBuild5x2 = 1, kSplitBuild6x2 = 2;

}  // namespace rsmp
