// pcm_batch.hip -- batched PCM converters (rsmp_pcm_batch_*): the f32 -> PCM quantiser of rsmp_f32_to_pcm_shaped and the PCM -> f32
// decoder of the fused PCM-input loads over MANY streams in ONE launch, each stream with its own buffers, length, seed, first index,
// gain, channel count and statistics block.  The arithmetic is fir_kernels.h's, value for value: fir_pcm_quantise_gain[_stat] behind
// the noise of fir_pcm_dither_shaped, fir_pcm_value's decoding.  What is new is the plan (pcm_batch_plan.h): tiles of T values that
// never straddle two streams, a prefix of tile counts that a workgroup searches once and then walks, and a persistent grid of a few
// workgroups per compute unit that the tiles are dealt to by rule.
//
// Lanes.  A tile starts at a multiple of 4 values from its stream's base, so a lane takes four values as one 16-byte load of f32
// and writes their 8 / 12 / 16 bytes as whole words at a 4-byte aligned address (the decoder: the other way round), up to
// kPcmBatchFours such fours per tile, all loaded before the first is used.  The n % 4 values behind a stream's last whole four are
// one lane's, each stored with the sample's own bytes (fir_pcm_store_code).  Every byte is written once and none outside
// [dst, dst + n_values * bits / 8).
//
// Noise.  Four consecutive indices share their splitmix64 words: two mixes where the four's first index is even, three where it is
// odd -- the parity is the stream's (first_index; for the high-pass form's earlier values first_index - channels), since a four
// starts at a multiple of 4 from the base.  Each value's pair counter is taken from its own wrapped index, so the bits are the
// definition's (fir_dither_half) across the 2^64 wrap too.
//
// Statistics.  A lane keeps its counts in registers across all of its workgroup's tiles of one stream.  When the workgroup leaves
// the stream -- and at its end -- the waves sum (fir_stat_wave_sum), the workgroup sums the waves through LDS in 64 bits, and one
// lane merges into the stream's block with at most four atomics: about 4 x (workgroups + stream changes seen by workgroups) atomics
// a launch, whatever the number of tiles.  Streams without a block run the tile body that counts nothing: a launch none of whose
// streams is counted takes a build without the counting body at all; in a launch that counts, the choice is one workgroup-uniform
// branch per stream.
#include <hip/hip_runtime.h>

#include <cstring>
#include <new>
#include <vector>

#include "../../include/resampler_amd.h"
#include "common.h"
#include "device_util.h"
#include "fir_kernels.h"
#include "pcm_batch_plan.h"

static_assert(sizeof(rsmp_pcm_batch_item) == 64 && sizeof(rsmp_pcm_batch_item) == sizeof(rsmp::PcmBatchStream), "one stream is 64 bytes on both sides");

namespace {

using rsmp::FirPcmStat;
using rsmp::PcmBatchDeal;
using rsmp::PcmBatchStream;

constexpr uint32_t kThreads = rsmp::kPcmBatchThreads;
constexpr uint32_t kFours = rsmp::kPcmBatchFours;
constexpr uint32_t kTile = rsmp::kPcmBatchTile;
// A lane's counters are 32 bits and so is a wave's sum (fir_stat_wave_sum): a workgroup that stays on one stream merges after this
// many tiles at the latest (2^20 tiles x 16 values a lane x 64 lanes = 2^30).
constexpr uint32_t kFlushTiles = 1u << 20;

enum { kNoiseNone = 0, kNoiseWhite = 1, kNoiseHighpass = 2 };

typedef float v4f __attribute__((ext_vector_type(4)));
// Whole words at a 4-byte aligned address (the streams' PCM buffers promise no more)
typedef uint32_t u32x2_raw __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4_raw __attribute__((ext_vector_type(4)));
// ... in global memory: the streams' pointers come out of a table, so the compiler is told the address space (global loads and
// stores keep their own counter; flat ones would wait for everything outstanding)
typedef const v4f __attribute__((address_space(1)))* g_v4f_cptr;
typedef v4f __attribute__((address_space(1)))* g_v4f_ptr;
typedef u32x2_raw __attribute__((address_space(1), aligned(4)))* g_u32x2_ptr;
typedef const u32x2_raw __attribute__((address_space(1), aligned(4)))* g_u32x2_cptr;
typedef u32x4_raw __attribute__((address_space(1), aligned(4)))* g_u32x4_ptr;
typedef const u32x4_raw __attribute__((address_space(1), aligned(4)))* g_u32x4_cptr;
typedef uint32_t __attribute__((address_space(1)))* g_u32_ptr;
typedef const uint32_t __attribute__((address_space(1)))* g_u32_cptr;

// h(seed, a + j), j = 0 .. 3, indices wrapping in 64 bits (fir_dither_half's bits).  odd: a & 1.
__device__ __forceinline__ void quad_halves(uint64_t seed, uint64_t a, bool odd, uint32_t (&h)[4]) {
    if (!odd) {
        const uint64_t w0 = rsmp::fir_dither_word(seed, a >> 1), w1 = rsmp::fir_dither_word(seed, (a + 2) >> 1);
        h[0] = static_cast<uint32_t>(w0);
        h[1] = static_cast<uint32_t>(w0 >> 32);
        h[2] = static_cast<uint32_t>(w1);
        h[3] = static_cast<uint32_t>(w1 >> 32);
    } else {
        const uint64_t w0 = rsmp::fir_dither_word(seed, a >> 1), w1 = rsmp::fir_dither_word(seed, (a + 1) >> 1),
                       w2 = rsmp::fir_dither_word(seed, (a + 3) >> 1);
        h[0] = static_cast<uint32_t>(w0 >> 32);
        h[1] = static_cast<uint32_t>(w1);
        h[2] = static_cast<uint32_t>(w1 >> 32);
        h[3] = static_cast<uint32_t>(w2);
    }
}

template <int BITS, int NOISE, bool COUNT>
__device__ __forceinline__ uint32_t encode_value(float x, float k, float d, FirPcmStat& mine) {
    if constexpr (COUNT) return static_cast<uint32_t>(rsmp::fir_pcm_quantise_gain_stat(x, k, BITS, d, mine));
    else if constexpr (NOISE != kNoiseNone) return static_cast<uint32_t>(rsmp::fir_pcm_quantise_gain(x, k, BITS, d));
    else return static_cast<uint32_t>(rsmp::fir_pcm_quantise_gain(x, k, BITS));
}

// One tile of one stream: its values [base, base + nv) (base a multiple of 4; nv <= T).
template <int BITS, int NOISE, bool COUNT>
__device__ __forceinline__ void encode_tile(const PcmBatchStream& st, uint64_t base, uint32_t nv, FirPcmStat& mine) {
    const float* __restrict__ in = static_cast<const float*>(st.src) + base;
    uint8_t* __restrict__ out = st.dst ? static_cast<uint8_t*>(st.dst) + base * (BITS / 8) : nullptr;   // (null: measure only)
    const uint32_t fours = nv / 4;
    const uint64_t first = st.first_index + base;   // index of the tile's value 0 (wraps)
    v4f x[kFours];
#pragma unroll
    for (uint32_t u = 0; u < kFours; ++u) {
        const uint32_t g = threadIdx.x + u * kThreads;
        if (g < fours) x[u] = ((g_v4f_cptr)in)[g];
    }
    const bool odd = (st.first_index & 1) != 0, odd_prev = ((st.first_index - st.channels) & 1) != 0;
#pragma unroll
    for (uint32_t u = 0; u < kFours; ++u) {
        const uint32_t g = threadIdx.x + u * kThreads;
        if (g >= fours) continue;
        float d[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if constexpr (NOISE != kNoiseNone) {
            const uint64_t a = first + 4ull * g;
            uint32_t h[4];
            quad_halves(st.seed, a, odd, h);
            if constexpr (NOISE == kNoiseHighpass) {
                uint32_t hp[4];
                quad_halves(st.seed, a - st.channels, odd_prev, hp);
#pragma unroll
                for (int j = 0; j < 4; ++j) d[j] = rsmp::fir_dither_value_hp(h[j], hp[j]);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) d[j] = rsmp::fir_dither_value(h[j]);
            }
        }
        const uint32_t q0 = encode_value<BITS, NOISE, COUNT>(x[u].x, st.k, d[0], mine), q1 = encode_value<BITS, NOISE, COUNT>(x[u].y, st.k, d[1], mine);
        const uint32_t q2 = encode_value<BITS, NOISE, COUNT>(x[u].z, st.k, d[2], mine), q3 = encode_value<BITS, NOISE, COUNT>(x[u].w, st.k, d[3], mine);
        if (!out) continue;
        uint8_t* o = out + static_cast<size_t>(g) * (BITS / 2);
        if constexpr (BITS == 16) {
            *(g_u32x2_ptr)o = u32x2_raw{(q0 & 0xFFFFu) | (q1 << 16), (q2 & 0xFFFFu) | (q3 << 16)};
        } else if constexpr (BITS == 24) {
            *(g_u32x2_ptr)o = u32x2_raw{(q0 & 0xFFFFFFu) | (q1 << 24), ((q1 >> 8) & 0xFFFFu) | (q2 << 16)};
            ((g_u32_ptr)o)[2] = ((q2 >> 16) & 0xFFu) | (q3 << 8);
        } else {
            *(g_u32x4_ptr)o = u32x4_raw{q0, q1, q2, q3};
        }
    }
    // the 0 .. 3 values behind the last whole four (a stream's last tile only): one lane, each value by the definition itself
    if ((nv & 3u) != 0 && threadIdx.x == fours % kThreads) {
        for (uint32_t j = 4 * fours; j < nv; ++j) {
            float d = 0.0f;
            if constexpr (NOISE != kNoiseNone)
                d = rsmp::fir_pcm_dither_shaped(st.seed, first + j, NOISE == kNoiseHighpass ? RSMP_DITHER_SHAPE_HIGHPASS : RSMP_DITHER_SHAPE_WHITE, st.channels);
            const uint32_t q = encode_value<BITS, NOISE, COUNT>(in[j], st.k, d, mine);
            if (out) rsmp::fir_pcm_store_code(out, BITS, j, static_cast<int32_t>(q));
        }
    }
}

// The workgroup's counts of one stream into the stream's block; every lane of the workgroup calls it (uniform control flow).
__device__ __forceinline__ void stats_flush(FirPcmStat& mine, rsmp_pcm_stats* stats, FirPcmStat* waves) {
    const FirPcmStat w = rsmp::fir_stat_wave_sum(mine);
    if ((threadIdx.x & 63u) == 0) waves[threadIdx.x >> 6] = w;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long values = 0, clipped = 0, nans = 0;
        uint32_t peak = 0;
        for (uint32_t j = 0; j < kThreads / 64; ++j) {
            values += waves[j].values;
            clipped += waves[j].clipped;
            nans += waves[j].nans;
            peak = waves[j].peak > peak ? waves[j].peak : peak;
        }
        static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "64-bit atomics on the counts");
        if (values) (void)atomicAdd(reinterpret_cast<unsigned long long*>(&stats->values), values);
        if (clipped) (void)atomicAdd(reinterpret_cast<unsigned long long*>(&stats->clipped), clipped);
        if (nans) (void)atomicAdd(reinterpret_cast<unsigned long long*>(&stats->nans), nans);
        if (peak) (void)atomicMax(reinterpret_cast<uint32_t*>(&stats->peak), peak);   // (the bit pattern of |x| orders non-negative floats and +inf)
    }
    __syncthreads();   // (the next flush writes `waves` again)
    mine = FirPcmStat{0, 0, 0, 0};
}

// The workgroup's tiles of stream `st` (tiles [p0, p1) of the launch): from its i-th tile `tile` on, while they are the stream's.
template <int BITS, int NOISE, bool COUNT>
__device__ __forceinline__ void encode_stream(const PcmBatchStream& st, uint32_t p0, uint32_t p1, const PcmBatchDeal& deal, uint32_t& i, uint64_t& tile,
                                              FirPcmStat* waves) {
    FirPcmStat mine{0, 0, 0, 0};
    uint32_t since = 0;
    for (; i < deal.count && tile < p1; ++i, tile += deal.step) {
        const uint64_t base = (tile - p0) * kTile, left = st.n_values - base;
        encode_tile<BITS, NOISE, COUNT>(st, base, left < kTile ? static_cast<uint32_t>(left) : kTile, mine);
        if constexpr (COUNT) {
            if (++since == kFlushTiles) {
                stats_flush(mine, static_cast<rsmp_pcm_stats*>(st.stats), waves);
                since = 0;
            }
        }
    }
    if constexpr (COUNT) stats_flush(mine, static_cast<rsmp_pcm_stats*>(st.stats), waves);
}

// ANYCOUNT: some stream of the launch has a statistics block.
template <int BITS, int NOISE, bool ANYCOUNT>
__global__ __launch_bounds__(kThreads) void pcm_batch_encode_kernel(const PcmBatchStream* __restrict__ streams, const uint32_t* __restrict__ prefix,
                                                                    uint32_t n_streams, uint32_t tiles, uint32_t order) {
    __shared__ FirPcmStat waves[kThreads / 64];
    const PcmBatchDeal deal = rsmp::pcm_batch_deal(order, blockIdx.x, gridDim.x, tiles);
    if (deal.count == 0) return;
    uint64_t tile = deal.first;
    uint32_t s = rsmp::pcm_batch_find_stream(prefix, n_streams, deal.first);
    for (uint32_t i = 0;;) {
        const PcmBatchStream st = streams[s];   // (workgroup-uniform: scalar loads)
        const uint32_t p0 = prefix[s], p1 = prefix[s + 1];
        if (ANYCOUNT && st.stats != nullptr) encode_stream<BITS, NOISE, ANYCOUNT>(st, p0, p1, deal, i, tile, waves);
        else encode_stream<BITS, NOISE, false>(st, p0, p1, deal, i, tile, waves);
        if (i == deal.count) break;
        s = rsmp::pcm_batch_walk(prefix, s, static_cast<uint32_t>(tile));
    }
}

// ---- PCM -> f32 ---------------------------------------------------------------------------------------------------------------------
// fir_pcm_value's arithmetic on a sample already in a register: s / 2^(bits-1), the reference's -2^31 at 32 bits (main.rs:131).
template <int BITS>
__device__ __forceinline__ float decode_value(int32_t s) {
    if constexpr (BITS == 16) return static_cast<float>(s) * (1.0f / 32768.0f);
    else if constexpr (BITS == 24) return static_cast<float>(s) * (1.0f / 8388608.0f);
    else return static_cast<float>(s) * (-1.0f / 2147483648.0f);
}
__device__ __forceinline__ int32_t sext24(uint32_t u) { return static_cast<int32_t>(u << 8) >> 8; }

template <int BITS>
__device__ __forceinline__ void decode_tile(const PcmBatchStream& st, uint64_t base, uint32_t nv) {
    const uint8_t* __restrict__ in = static_cast<const uint8_t*>(st.src) + base * (BITS / 8);
    float* __restrict__ out = static_cast<float*>(st.dst) + base;
    const uint32_t fours = nv / 4;
    uint32_t w[kFours][4];
#pragma unroll
    for (uint32_t u = 0; u < kFours; ++u) {
        const uint32_t g = threadIdx.x + u * kThreads;
        if (g >= fours) continue;
        const uint8_t* p = in + static_cast<size_t>(g) * (BITS / 2);
        if constexpr (BITS == 16) {
            const u32x2_raw v = *(g_u32x2_cptr)p;
            w[u][0] = v.x; w[u][1] = v.y;
        } else if constexpr (BITS == 24) {
            const u32x2_raw v = *(g_u32x2_cptr)p;
            w[u][0] = v.x; w[u][1] = v.y; w[u][2] = ((g_u32_cptr)p)[2];
        } else {
            const u32x4_raw v = *(g_u32x4_cptr)p;
            w[u][0] = v.x; w[u][1] = v.y; w[u][2] = v.z; w[u][3] = v.w;
        }
    }
#pragma unroll
    for (uint32_t u = 0; u < kFours; ++u) {
        const uint32_t g = threadIdx.x + u * kThreads;
        if (g >= fours) continue;
        int32_t s0, s1, s2, s3;
        if constexpr (BITS == 16) {
            s0 = static_cast<int16_t>(w[u][0] & 0xFFFFu); s1 = static_cast<int16_t>(w[u][0] >> 16);
            s2 = static_cast<int16_t>(w[u][1] & 0xFFFFu); s3 = static_cast<int16_t>(w[u][1] >> 16);
        } else if constexpr (BITS == 24) {
            s0 = sext24(w[u][0] & 0xFFFFFFu);
            s1 = sext24((w[u][0] >> 24) | ((w[u][1] & 0xFFFFu) << 8));
            s2 = sext24((w[u][1] >> 16) | ((w[u][2] & 0xFFu) << 16));
            s3 = sext24(w[u][2] >> 8);
        } else {
            s0 = static_cast<int32_t>(w[u][0]); s1 = static_cast<int32_t>(w[u][1]);
            s2 = static_cast<int32_t>(w[u][2]); s3 = static_cast<int32_t>(w[u][3]);
        }
        ((g_v4f_ptr)out)[g] = v4f{decode_value<BITS>(s0), decode_value<BITS>(s1), decode_value<BITS>(s2), decode_value<BITS>(s3)};
    }
    if ((nv & 3u) != 0 && threadIdx.x == fours % kThreads)
        for (uint32_t j = 4 * fours; j < nv; ++j) out[j] = rsmp::fir_pcm_value(in, BITS, j);
}

template <int BITS>
__global__ __launch_bounds__(kThreads) void pcm_batch_decode_kernel(const PcmBatchStream* __restrict__ streams, const uint32_t* __restrict__ prefix,
                                                                    uint32_t n_streams, uint32_t tiles, uint32_t order) {
    const PcmBatchDeal deal = rsmp::pcm_batch_deal(order, blockIdx.x, gridDim.x, tiles);
    if (deal.count == 0) return;
    uint64_t tile = deal.first;
    uint32_t s = rsmp::pcm_batch_find_stream(prefix, n_streams, deal.first);
    for (uint32_t i = 0;;) {
        const PcmBatchStream st = streams[s];
        const uint32_t p0 = prefix[s], p1 = prefix[s + 1];
        for (; i < deal.count && tile < p1; ++i, tile += deal.step) {
            const uint64_t base = (tile - p0) * kTile, left = st.n_values - base;
            decode_tile<BITS>(st, base, left < kTile ? static_cast<uint32_t>(left) : kTile);
        }
        if (i == deal.count) break;
        s = rsmp::pcm_batch_walk(prefix, s, static_cast<uint32_t>(tile));
    }
}

bool bits_ok(int bits) { return bits == 16 || bits == 24 || bits == 32; }

}  // namespace

// The descriptor tables of a handle: a ring of slots, each a pinned host table and its device twin of max_streams entries (the
// streams, then the prefix of tile counts: one copy).  A call fills the next slot's host table, uploads it on the caller's stream
// in front of its kernel and records the slot's event behind the kernel; the host waits only where all the slots are in flight --
// for the call made kSlots calls ago.  So calls follow each other on any streams without a host wait, and `items` is free when
// a call returns.
struct rsmp_pcm_batch {
    static constexpr int kSlots = 4;
    int device = 0;
    size_t max_streams = 0;
    uint32_t compute_units = 1;
    int order_forced = -1;   // (diagnostic: RSMP_PCM_BATCH_ORDER under RSMP_DEBUG=1; -1: the rule below)
    rsmp::PinnedBuffer h_table[kSlots];
    rsmp::DeviceBuffer d_table[kSlots];
    rsmp::EventHolder done[kSlots];
    bool used[kSlots] = {false, false, false, false};
    int slot = 0;
    std::vector<uint64_t> lens;
    std::vector<uint32_t> prefix;
    uint32_t last_workgroups = 0;
    uint64_t last_tiles = 0;
};

extern "C" rsmp_pcm_batch* rsmp_pcm_batch_new(size_t max_streams, int device) {
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) {
        (void)rsmp::fail(RSMP_ERR_NO_DEVICE, "no HIP device (this engine has no CPU path)");
        return nullptr;
    }
    if (max_streams == 0 || max_streams > (size_t{1} << 24) || device < 0 || device >= n_dev) {
        (void)rsmp::fail(RSMP_ERR_INVALID_ARGUMENT, "rsmp_pcm_batch_new: 1 <= max_streams <= 2^24, an existing device");
        return nullptr;
    }
    rsmp_pcm_batch* b = new (std::nothrow) rsmp_pcm_batch;
    if (!b) {
        (void)rsmp::fail(RSMP_ERR_INVALID_ARGUMENT, "rsmp_pcm_batch_new: out of memory");
        return nullptr;
    }
    b->device = device;
    b->max_streams = max_streams;
    rsmp::DeviceGuard guard(device);
    int cus = 0;
    hipError_t e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device);
    b->compute_units = e == hipSuccess && cus > 0 ? static_cast<uint32_t>(cus) : 1u;
    // (diagnostic: the other tile order, for tools/pcm_batch_bench.py; read under RSMP_DEBUG=1 only)
    if (const char* k = rsmp::knob("RSMP_PCM_BATCH_ORDER")) b->order_forced = (k[0] == 's' || k[0] == '1') ? rsmp::kPcmBatchStrided : rsmp::kPcmBatchContiguous;
    const size_t bytes = max_streams * sizeof(rsmp::PcmBatchStream) + (max_streams + 1) * sizeof(uint32_t);
    for (int s = 0; s < rsmp_pcm_batch::kSlots && e == hipSuccess; ++s) {
        e = b->h_table[s].reserve(bytes);
        if (e == hipSuccess) e = b->d_table[s].reserve(bytes);
        if (e == hipSuccess) e = b->done[s].create(hipEventDisableTiming);
    }
    if (e != hipSuccess) {
        (void)rsmp::fail(RSMP_ERR_HIP, "rsmp_pcm_batch_new: %s", hipGetErrorString(e));
        delete b;
        return nullptr;
    }
    b->lens.resize(max_streams);
    b->prefix.resize(max_streams + 1);
    return b;
}

extern "C" void rsmp_pcm_batch_free(rsmp_pcm_batch* b) {
    if (!b) return;
    rsmp::DeviceGuard guard(b->device);
    for (int s = 0; s < rsmp_pcm_batch::kSlots; ++s)   // the tables go only behind the launches that read them
        if (b->used[s]) (void)hipEventSynchronize(b->done[s]);
    delete b;
}

extern "C" size_t rsmp_pcm_batch_tile_values(void) { return kTile; }

extern "C" int rsmp_pcm_batch_last_grid(const rsmp_pcm_batch* b, uint32_t* workgroups, uint64_t* tiles) {
    if (!b) return rsmp::fail(RSMP_ERR_INVALID_ARGUMENT, "rsmp_pcm_batch_last_grid: null handle");
    if (workgroups) *workgroups = b->last_workgroups;
    if (tiles) *tiles = b->last_tiles;
    return RSMP_OK;
}

namespace {

// Everything that can refuse a call, before anything is enqueued.  to_pcm: the f32 -> PCM call (else PCM -> f32).
int batch_check(const char* who, rsmp_pcm_batch* b, const rsmp_pcm_batch_item* items, size_t n, int bits, int dither, int shape, bool to_pcm) {
    if (!b) return rsmp::fail(RSMP_ERR_INVALID_ARGUMENT, "%s: null handle", who);
    if (n != 0 && !items) return rsmp::fail(RSMP_ERR_INVALID_ARGUMENT, "%s: null items", who);
    if (n > b->max_streams) return rsmp::fail(RSMP_ERR_INVALID_ARGUMENT, "%s: %zu streams, the handle was made for %zu", who, n, b->max_streams);
    if (!bits_ok(bits)) return rsmp::fail(RSMP_ERR_INVALID_ARGUMENT, "%s: 16 / 24 / 32 bits", who);
    if (to_pcm && ((dither != RSMP_DITHER_NONE && dither != RSMP_DITHER_TPDF) || (shape != RSMP_DITHER_SHAPE_WHITE && shape != RSMP_DITHER_SHAPE_HIGHPASS)))
        return rsmp::fail(RSMP_ERR_INVALID_ARGUMENT, "%s: RSMP_DITHER_NONE / RSMP_DITHER_TPDF, RSMP_DITHER_SHAPE_WHITE / RSMP_DITHER_SHAPE_HIGHPASS", who);
    for (size_t i = 0; i < n; ++i) {
        const rsmp_pcm_batch_item& it = items[i];
        if (it.reserved != 0) return rsmp::fail(RSMP_ERR_INVALID_ARGUMENT, "%s: stream %zu: reserved must be 0", who, i);
        const uintptr_t src = reinterpret_cast<uintptr_t>(it.src), dst = reinterpret_cast<uintptr_t>(it.dst), stats = reinterpret_cast<uintptr_t>(it.stats);
        if (to_pcm) {
            if (!rsmp::fir_pcm_gain_ok(it.gain)) return rsmp::fail(RSMP_ERR_INVALID_ARGUMENT, "%s: stream %zu: a finite gain with 2^-32 <= |gain| <= 2^32", who, i);
            if (it.channels == 0) return rsmp::fail(RSMP_ERR_INVALID_ARGUMENT, "%s: stream %zu: channels >= 1", who, i);
            if (it.n_values == 0) continue;
            if (!it.src || (!it.dst && !it.stats)) return rsmp::fail(RSMP_ERR_INVALID_ARGUMENT, "%s: stream %zu: non-null src, and dst or stats", who, i);
            if (src % 16 != 0 || dst % 4 != 0 || stats % 8 != 0)
                return rsmp::fail(RSMP_ERR_INVALID_ARGUMENT, "%s: stream %zu: src 16-byte aligned, dst 4-byte aligned, stats 8-byte aligned", who, i);
        } else {
            if (it.stats) return rsmp::fail(RSMP_ERR_INVALID_ARGUMENT, "%s: stream %zu: stats must be NULL", who, i);
            if (it.n_values == 0) continue;
            if (!it.src || !it.dst) return rsmp::fail(RSMP_ERR_INVALID_ARGUMENT, "%s: stream %zu: non-null src and dst", who, i);
            if (src % 4 != 0 || dst % 16 != 0) return rsmp::fail(RSMP_ERR_INVALID_ARGUMENT, "%s: stream %zu: src 4-byte aligned, dst 16-byte aligned", who, i);
        }
    }
    for (size_t i = 0; i < n; ++i) b->lens[i] = items[i].n_values;
    if (!rsmp::pcm_batch_prefix(b->lens.data(), n, b->prefix.data()))
        return rsmp::fail(RSMP_ERR_INVALID_ARGUMENT, "%s: the batch has more than 2^32 - 1 tiles of %u values", who, kTile);
    return RSMP_OK;
}

// The tile order of a launch (measured at 64 streams x 2.28 M values, profiles/pcm_batch.txt): a launch that counts takes contiguous
// ranges -- a workgroup then changes stream, and merges, about once (strided: at nearly every tile, +20 .. 40 %) --, a launch that
// counts nothing the strided order, the whole grid on one stretch at a time (undithered and PCM -> f32 5 .. 13 % faster, dithered
// level or inside the spread).
uint32_t batch_order(const rsmp_pcm_batch* b, bool counting) {
    if (b->order_forced >= 0) return static_cast<uint32_t>(b->order_forced);
    return counting ? rsmp::kPcmBatchContiguous : rsmp::kPcmBatchStrided;
}

// Fills and uploads the next slot's table (b->prefix holds the call's prefix) and hands back its device addresses.
int batch_stage(rsmp_pcm_batch* b, const rsmp_pcm_batch_item* items, size_t n, int bits, bool to_pcm, hipStream_t stream, int* slot_out,
                const PcmBatchStream** d_streams, const uint32_t** d_prefix) {
    const int slot = b->slot;
    b->slot = (slot + 1) % rsmp_pcm_batch::kSlots;
    if (b->used[slot]) {   // the launch that read this slot, kSlots calls ago, is through
        RSMP_HIP_CHECK(hipEventSynchronize(b->done[slot]));
        b->used[slot] = false;
    }
    PcmBatchStream* h = b->h_table[slot].as<PcmBatchStream>();
    for (size_t i = 0; i < n; ++i) {
        const rsmp_pcm_batch_item& it = items[i];
        h[i] = PcmBatchStream{it.src, it.dst, it.n_values, it.seed, it.first_index, to_pcm ? static_cast<void*>(it.stats) : nullptr,
                              to_pcm ? rsmp::fir_pcm_gain_scale(it.gain, static_cast<uint32_t>(bits)) : 0.0f, it.channels, 0};
    }
    const size_t table = n * sizeof(PcmBatchStream), bytes = table + (n + 1) * sizeof(uint32_t);
    std::memcpy(reinterpret_cast<char*>(h) + table, b->prefix.data(), (n + 1) * sizeof(uint32_t));
    RSMP_HIP_CHECK(hipMemcpyAsync(b->d_table[slot].get(), h, bytes, hipMemcpyHostToDevice, stream));
    b->used[slot] = true;   // (from here on the slot's memory is in use: the event below, or the one recorded by an earlier call, guards it)
    *slot_out = slot;
    *d_streams = b->d_table[slot].as<PcmBatchStream>();
    *d_prefix = reinterpret_cast<const uint32_t*>(b->d_table[slot].as<char>() + table);
    return RSMP_OK;
}

}  // namespace

extern "C" int rsmp_pcm_batch_f32_to_pcm_device(rsmp_pcm_batch* b, const rsmp_pcm_batch_item* items, size_t n, int bits, int dither, int shape,
                                                void* stream) {
    if (int rc = batch_check("rsmp_pcm_batch_f32_to_pcm_device", b, items, n, bits, dither, shape, true)) return rc;
    const uint32_t tiles = b->prefix[n];
    b->last_workgroups = 0;
    b->last_tiles = 0;
    if (tiles == 0) return RSMP_OK;
    bool any_stats = false;
    for (size_t i = 0; i < n; ++i) any_stats = any_stats || (items[i].n_values != 0 && items[i].stats != nullptr);
    rsmp::DeviceGuard guard(b->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    int slot = 0;
    const PcmBatchStream* d_streams = nullptr;
    const uint32_t* d_prefix = nullptr;
    if (int rc = batch_stage(b, items, n, bits, true, s, &slot, &d_streams, &d_prefix)) return rc;
    const dim3 grid(rsmp::pcm_batch_grid(tiles, b->compute_units));
    const int noise = dither != RSMP_DITHER_TPDF ? kNoiseNone : shape == RSMP_DITHER_SHAPE_HIGHPASS ? kNoiseHighpass : kNoiseWhite;
    const uint32_t ns = static_cast<uint32_t>(n), order = batch_order(b, any_stats);
#define RSMP_BATCH_LAUNCH(BITS, NOISE, COUNT) \
    hipLaunchKernelGGL((pcm_batch_encode_kernel<BITS, NOISE, COUNT>), grid, dim3(kThreads), 0, s, d_streams, d_prefix, ns, tiles, order)
#define RSMP_BATCH_NOISE(BITS, COUNT)                                        \
    do {                                                                     \
        if (noise == kNoiseNone) RSMP_BATCH_LAUNCH(BITS, kNoiseNone, COUNT); \
        else if (noise == kNoiseWhite) RSMP_BATCH_LAUNCH(BITS, kNoiseWhite, COUNT); \
        else RSMP_BATCH_LAUNCH(BITS, kNoiseHighpass, COUNT);                 \
    } while (0)
#define RSMP_BATCH_BITS(COUNT)                         \
    do {                                               \
        if (bits == 16) RSMP_BATCH_NOISE(16, COUNT);   \
        else if (bits == 24) RSMP_BATCH_NOISE(24, COUNT); \
        else RSMP_BATCH_NOISE(32, COUNT);              \
    } while (0)
    if (any_stats) RSMP_BATCH_BITS(true);
    else RSMP_BATCH_BITS(false);
#undef RSMP_BATCH_BITS
#undef RSMP_BATCH_NOISE
#undef RSMP_BATCH_LAUNCH
    const hipError_t launched = hipGetLastError();
    RSMP_HIP_CHECK(rsmp::event_record(b->done[slot], s));
    RSMP_HIP_CHECK(launched);
    b->last_workgroups = grid.x;
    b->last_tiles = tiles;
    return RSMP_OK;
}

extern "C" int rsmp_pcm_batch_pcm_to_f32_device(rsmp_pcm_batch* b, const rsmp_pcm_batch_item* items, size_t n, int bits, void* stream) {
    if (int rc = batch_check("rsmp_pcm_batch_pcm_to_f32_device", b, items, n, bits, RSMP_DITHER_NONE, RSMP_DITHER_SHAPE_WHITE, false)) return rc;
    const uint32_t tiles = b->prefix[n];
    b->last_workgroups = 0;
    b->last_tiles = 0;
    if (tiles == 0) return RSMP_OK;
    rsmp::DeviceGuard guard(b->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    int slot = 0;
    const PcmBatchStream* d_streams = nullptr;
    const uint32_t* d_prefix = nullptr;
    if (int rc = batch_stage(b, items, n, bits, false, s, &slot, &d_streams, &d_prefix)) return rc;
    const dim3 grid(rsmp::pcm_batch_grid(tiles, b->compute_units));
    const uint32_t ns = static_cast<uint32_t>(n), order = batch_order(b, false);
    if (bits == 16) hipLaunchKernelGGL(pcm_batch_decode_kernel<16>, grid, dim3(kThreads), 0, s, d_streams, d_prefix, ns, tiles, order);
    else if (bits == 24) hipLaunchKernelGGL(pcm_batch_decode_kernel<24>, grid, dim3(kThreads), 0, s, d_streams, d_prefix, ns, tiles, order);
    else hipLaunchKernelGGL(pcm_batch_decode_kernel<32>, grid, dim3(kThreads), 0, s, d_streams, d_prefix, ns, tiles, order);
    const hipError_t launched = hipGetLastError();
    RSMP_HIP_CHECK(rsmp::event_record(b->done[slot], s));
    RSMP_HIP_CHECK(launched);
    b->last_workgroups = grid.x;
    b->last_tiles = tiles;
    return RSMP_OK;
}

// The decoder's definition, on the host (no device needed): sample j -> s / 2^(bits-1), the reference's -2^31 divisor at 32 bits
// (resample/src/main.rs:131) -- fir_pcm_value's arithmetic.
extern "C" int rsmp_pcm_to_f32(const void* pcm, size_t n_samples, int bits, float* out) {
    if (!bits_ok(bits) || (n_samples != 0 && (!pcm || !out)))
        return rsmp::fail(RSMP_ERR_INVALID_ARGUMENT, "rsmp_pcm_to_f32: 16 / 24 / 32 bits, non-null buffers");
    const uint8_t* p = static_cast<const uint8_t*>(pcm);
    for (size_t j = 0; j < n_samples; ++j) {
        if (bits == 16) {
            const uint32_t u = static_cast<uint32_t>(p[2 * j]) | (static_cast<uint32_t>(p[2 * j + 1]) << 8);
            out[j] = static_cast<float>(static_cast<int16_t>(u)) * (1.0f / 32768.0f);
        } else if (bits == 24) {
            const uint32_t u = static_cast<uint32_t>(p[3 * j]) | (static_cast<uint32_t>(p[3 * j + 1]) << 8) | (static_cast<uint32_t>(p[3 * j + 2]) << 16);
            out[j] = static_cast<float>(static_cast<int32_t>(u << 8) >> 8) * (1.0f / 8388608.0f);
        } else {
            const uint32_t u = static_cast<uint32_t>(p[4 * j]) | (static_cast<uint32_t>(p[4 * j + 1]) << 8) | (static_cast<uint32_t>(p[4 * j + 2]) << 16) |
                               (static_cast<uint32_t>(p[4 * j + 3]) << 24);
            out[j] = static_cast<float>(static_cast<int32_t>(u)) * (-1.0f / 2147483648.0f);
        }
    }
    return RSMP_OK;
}
