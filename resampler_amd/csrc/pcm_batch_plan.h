// pcm_batch_plan.h -- the plan of a batched PCM conversion (rsmp_pcm_batch_*): how the values of many streams are cut into tiles,
// how a tile finds its stream, and how the tiles are dealt to the workgroups of a persistent grid.  Plain C++: the kernels
// (pcm_batch.hip) and the stand-alone host check (tests/host/pcm_batch_plan_check.cpp) compile the same functions.
//
// Tiles.  Stream s of n_values[s] values is cut into ceil(n_values[s] / kPcmBatchTile) tiles; tile j of a stream covers its values
// [j * T, min((j + 1) * T, n)).  T is a multiple of 4, so every tile starts at a multiple of 4 values from its stream's base -- a
// lane's four values are one 16-byte load of f32 and 8 / 12 / 16 whole bytes of PCM at a 4-byte aligned address -- and no tile
// holds values of two streams.  Only a stream's last tile can be short; the n % 4 values behind its last whole four are one lane's.
// The launch's tiles are numbered stream after stream: prefix[s] is the number of tiles in front of stream s, prefix[n] their
// total.  An empty stream has no tile (prefix[s] == prefix[s + 1]).  The total must fit 32 bits.
#pragma once

#include <cstddef>
#include <cstdint>

#include "rsmp_hd.h"

namespace rsmp {

constexpr uint32_t kPcmBatchThreads = 256;                                  // lanes of a workgroup
constexpr uint32_t kPcmBatchFours = 4;                                      // fours of values a lane takes from one tile
constexpr uint32_t kPcmBatchTile = kPcmBatchThreads * kPcmBatchFours * 4;   // T: values of one tile
constexpr uint32_t kPcmBatchWgPerCu = 4;                                    // workgroups of the persistent grid per compute unit
static_assert(kPcmBatchTile % 4 == 0, "a tile starts at a multiple of 4 values");

// How the tiles are dealt to the G workgroups of the grid (both deal every tile exactly once: pcm_batch_deal below).
//   contiguous: workgroup w takes a range of consecutive tiles, floor(tiles / G) of them and one more for the first tiles % G
//               workgroups -- few stream changes per workgroup;
//   strided:    workgroup w takes tiles w, w + G, w + 2G, ... -- the whole grid on one contiguous stretch at a time.
enum PcmBatchOrder : uint32_t { kPcmBatchContiguous = 0, kPcmBatchStrided = 1 };

// One stream as the kernels read it (device table, 64 bytes): rsmp_pcm_batch_item with the gain already folded into the factor
// every store multiplies by, k = f32(gain) * 2^(bits-1) (fir_pcm_gain_scale).  The to-f32 kernel reads src, dst and n_values only.
struct PcmBatchStream {
    const void* src;
    void* dst;
    uint64_t n_values;
    uint64_t seed;
    uint64_t first_index;
    void* stats;   // rsmp_pcm_stats*, or null
    float k;
    uint32_t channels;
    uint64_t reserved;
};
static_assert(sizeof(PcmBatchStream) == 64, "one stream of the device table is 64 bytes");

RSMP_HD inline uint64_t pcm_batch_stream_tiles(uint64_t n_values) { return n_values / kPcmBatchTile + (n_values % kPcmBatchTile != 0 ? 1u : 0u); }

// The stream of tile `tile` (< prefix[n_streams]): the s with prefix[s] <= tile < prefix[s + 1] -- never an empty stream, whose two
// entries are equal.  Binary search over the n_streams + 1 entries; THE function: the kernels call it for the first tile of a
// workgroup and walk forward from there (pcm_batch_walk).
RSMP_HD inline uint32_t pcm_batch_find_stream(const uint32_t* prefix, uint32_t n_streams, uint32_t tile) {
    uint32_t lo = 0, hi = n_streams;   // invariant: prefix[lo] <= tile < prefix[hi]
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (prefix[mid] <= tile) lo = mid;
        else hi = mid;
    }
    return lo;
}
// The stream of `tile` given the stream `s` of an earlier tile of the same workgroup (tile numbers only grow).
RSMP_HD inline uint32_t pcm_batch_walk(const uint32_t* prefix, uint32_t s, uint32_t tile) {
    while (prefix[s + 1] <= tile) ++s;
    return s;
}

// Workgroup w's share of `tiles` tiles on a grid of G workgroups (w < G, G >= 1): its tiles are first, first + step, ...,
// `count` of them.
struct PcmBatchDeal {
    uint32_t first, count, step;
};
RSMP_HD inline PcmBatchDeal pcm_batch_deal(uint32_t order, uint32_t w, uint32_t G, uint32_t tiles) {
    if (order == kPcmBatchStrided) return PcmBatchDeal{w, w < tiles ? (tiles - w - 1) / G + 1 : 0u, G};
    const uint32_t q = tiles / G, r = tiles % G;
    const uint64_t first = static_cast<uint64_t>(w) * q + (w < r ? w : r);   // (<= tiles: fits 32 bits)
    return PcmBatchDeal{static_cast<uint32_t>(first), q + (w < r ? 1u : 0u), 1u};
}

// The grid of a launch: a few workgroups per compute unit, never more than there are tiles.
inline uint32_t pcm_batch_grid(uint32_t tiles, uint32_t compute_units) {
    const uint64_t most = static_cast<uint64_t>(compute_units ? compute_units : 1u) * kPcmBatchWgPerCu;
    return static_cast<uint32_t>(tiles < most ? tiles : most);
}

// Fills prefix[0 .. n] from the streams' lengths and returns true; false -- prefix unspecified -- where the tiles of the batch do not
// fit 32 bits.
bool pcm_batch_prefix(const uint64_t* n_values, size_t n, uint32_t* prefix);

}  // namespace rsmp
