// fir_kernels.h -- device-side work descriptors and launch wrappers of the FIR path.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/resampler_amd.h"
#include "fir_format.h"
#include "fir_generic_plan.h"
#include "fir_nonfinite.h"

namespace rsmp {

// One stream's share of a launch.  A launch covers `n_out` output frames of every stream in the
// batch; the input of a stream is the virtual concatenation [hist | in]: `hist_frames` frames
// that were already buffered inside the resampler when the launch started (the reference's
// input_buffers[read_position .. read_position+available_frames], resampler_fir.rs:187-191)
// followed by the frames accepted during the launch.  Everything is interleaved f32.
struct FirStreamDesc {
    const float* in;               // frames accepted in this launch (device)
    const float* hist;             // frames buffered before the launch (device)
    float* out;                    // output frames (device): interleaved f32, or PCM bytes (out_bits)
    const float* coeffs;           // [1024][taps] polyphase table (device)
    const rsmp_fir_segment* segs;  // exact position runs, sorted by out_start (device)
    const uint32_t* tile_seg;      // index of the run containing output frame tile*kFirTile
    float* hist_next;              // receives the frames still buffered after the launch
    const float* class_coef;       // periodic kernel: class table [tile][row_len][8] (device)
    const float* class_wrap_coef;  // periodic kernel: wrap-variant coefficients [tile][row_len]
    const void* class_meta;        // periodic kernel: TileMeta[tile]
    const uint32_t* wrap_bits;     // periodic kernel: bitmap of outputs taking the wrap variant
    const uint32_t* wraps;         // fix-up kernel: outputs needing the row-1023 variant
    uint32_t n_out;                // output frames in this launch
    uint32_t n_segs;
    uint32_t hist_frames;
    uint32_t in_frames;            // frames accepted in this launch
    uint32_t tail_start;           // first frame of [hist|in] that stays buffered afterwards
    uint32_t tail_frames;          // how many stay buffered
    uint32_t n_wraps;
    uint32_t channels;
    uint32_t taps;
    // periodic kernel: in_hz/out_hz = num/den reduced, absolute counters at launch start
    uint32_t num, den;
    // PCM output with TPDF dither only: RSMP_DITHER_SHAPE_*, one shape for all the streams of a launch (fir_pcm_dither_shaped below).
    // It sits in what was padding in front of abs_out: no other field moves.  No f32 build and no undithered build reads it.
    uint32_t dither_shape;
    uint64_t abs_out;              // output frames produced since reset, before this launch
    uint64_t abs_consumed;         // input frames retired since reset, before this launch
    uint64_t wrap_k0;              // wrap_bits bit K <-> absolute output (wrap_k0 + K) * den
    double drift;                  // periodic kernels: the f64 drift the stream's class table was built for
    // 0: `in` is interleaved f32.  16 / 24 / 32: `in` is a WAV file's little-endian PCM of that width, `channels` samples
    // a frame, converted where it is read as resample/src/main.rs:128-137 converts it (fir_pcm_value below); `hist`
    // -- the frames an earlier launch left buffered -- is f32 always.
    uint32_t in_bits;
    // 0: `out` receives interleaved f32.  16 / 24 / 32: `out` receives little-endian PCM of that width (24-bit packed, three
    // bytes a sample), every sum quantised where it is stored (fir_pcm_quantise below); one width for all the streams of a
    // launch.  `hist_next` -- the frames that stay buffered -- is f32 always.
    uint32_t out_bits;
    // PCM output only: RSMP_DITHER_NONE / RSMP_DITHER_TPDF, one mode for all the streams of a launch -- the host picks the kernels'
    // dithered builds by it --, and the stream's own seed.  Value (frame n of the launch, channel c) takes the noise of index
    // (abs_out + n) * channels + c (fir_pcm_dither below).  No build without PCM output reads either field, no undithered one the seed.
    uint32_t dither;
    // PCM output only: the factor every store multiplies by, k = f32(gain) * 2^(out_bits-1) with the stream's own gain (fir_pcm_gain_scale
    // below; gain 1: fir_pcm_scale(out_bits)).  The host writes it for every PCM-output launch; no build without PCM output reads it.
    float pcm_k;
    uint64_t dither_seed;
};
static_assert(offsetof(FirStreamDesc, dither_shape) == 140 && offsetof(FirStreamDesc, abs_out) == 144, "dither_shape fills the padding in front of abs_out");
static_assert(offsetof(FirStreamDesc, pcm_k) == 188 && offsetof(FirStreamDesc, dither_seed) == 192 && sizeof(FirStreamDesc) == 200,
              "pcm_k fills the hole in front of dither_seed: the descriptor keeps its size and every other field its place");

// One sample of a stream's `in`, index `i` in values (frame * channels + channel).
// main.rs:131: `sample as f32 / (1 << (bits - 1)) as f32`; the literal is an i32, so 32-bit files divide by -2^31.
__device__ __forceinline__ float fir_pcm_value(const void* in, uint32_t bits, size_t i) {
    if (bits == 16) return static_cast<float>(static_cast<const int16_t*>(in)[i]) * (1.0f / 32768.0f);
    if (bits == 32) return static_cast<float>(static_cast<const int32_t*>(in)[i]) * (-1.0f / 2147483648.0f);
    const uint8_t* p = static_cast<const uint8_t*>(in) + 3 * i;
    const uint32_t u = static_cast<uint32_t>(p[0]) | (static_cast<uint32_t>(p[1]) << 8) | (static_cast<uint32_t>(p[2]) << 16);
    return static_cast<float>(static_cast<int32_t>(u << 8) >> 8) * (1.0f / 8388608.0f);
}
__device__ __forceinline__ float fir_in_value(const FirStreamDesc& d, size_t i) {
    return d.in_bits == 0 ? d.in[i] : fir_pcm_value(d.in, d.in_bits, i);
}

// f32 -> PCM code of `bits` (16 / 24 / 32): round_half_to_even(x * 2^(bits-1)), saturated to [-2^(bits-1), 2^(bits-1) - 1]; NaN -> 0.
// The product is exact (a power of two; an overflow to +-inf saturates like any other value out of range), +inf is the top code
// and -inf the bottom one, -0.0 and denormals give 0.  No dither (that is fir_pcm_quantise_dither below).  The 32-bit top code 2^31 - 1 is no f32 value: the comparison
// saturates, not a clamp in f32.  Decoding a code with fir_pcm_value and quantising it again at the same width is the identity
// for 16 and 24 bits.  For 32 bits it is NOT: the reference's input divisor is -2^31 (main.rs:131), the scale here is +2^31 -- an
// f32 value means what it says on the way out --, so that round trip gives saturate(-f32(s)): polarity inverted, the bottom
// code saturated to the top one.
__host__ __device__ __forceinline__ float fir_pcm_scale(uint32_t bits) { return bits == 16 ? 32768.0f : bits == 24 ? 8388608.0f : 2147483648.0f; }
// (v: the scaled value, already rounded to an integer, +-inf or NaN)
__host__ __device__ __forceinline__ int32_t fir_pcm_code(float v, uint32_t bits) {
    if (!(v == v)) return 0;
    if (bits == 32) return v >= 2147483648.0f ? INT32_MAX : v <= -2147483648.0f ? INT32_MIN : static_cast<int32_t>(v);
    const float top = bits == 16 ? 32767.0f : 8388607.0f, bottom = bits == 16 ? -32768.0f : -8388608.0f;
    return static_cast<int32_t>(v > top ? top : v < bottom ? bottom : v);
}
__host__ __device__ __forceinline__ int32_t fir_pcm_quantise(float x, uint32_t bits) { return fir_pcm_code(rintf(x * fir_pcm_scale(bits)), bits); }

// TPDF dither (RSMP_DITHER_TPDF): value `i` of a stream -- i = frame * channels + channel, counted from the stream's start or
// reset -- is quantised as
//   q = saturate(round_half_to_even(f32(x * 2^(bits-1)) + d(seed, i))),  NaN -> 0,
// one f32 addition behind the exact product (an fma of the same operands gives the same bits); saturation and NaN as above.  The
// noise has no state, it is a function of the seed and the index: splitmix64 of the counter i / 2 + 1 gives 64 bits, the low 32
// for even i and the high 32 for odd i (one mix serves a two-channel frame); the difference of their two 16-bit halves, times
// 2^-16, is triangular on (-1, 1) LSB with variance 1/6.  A stream's bytes therefore do not depend on how it is cut into calls.
constexpr uint64_t kFirDitherStep = 0x9E3779B97F4A7C15ull;   // splitmix64's counter step: pair p starts from seed + (p + 1) * step
__host__ __device__ __forceinline__ uint64_t fir_dither_mix(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
__host__ __device__ __forceinline__ uint64_t fir_dither_word(uint64_t seed, uint64_t pair) {   // pair = i >> 1
    return fir_dither_mix(seed + (pair + 1) * kFirDitherStep);
}
__host__ __device__ __forceinline__ float fir_dither_value(uint32_t h) {   // h: the value's 32 bits of the word
    return static_cast<float>(static_cast<int32_t>(h & 0xFFFFu) - static_cast<int32_t>(h >> 16)) * (1.0f / 65536.0f);
}
__host__ __device__ __forceinline__ float fir_pcm_dither(uint64_t seed, uint64_t i) {
    const uint64_t w = fir_dither_word(seed, i >> 1);
    return fir_dither_value(static_cast<uint32_t>((i & 1) ? w >> 32 : w));
}
// High-pass TPDF dither (RSMP_DITHER_SHAPE_HIGHPASS; rsmp_f32_to_pcm_shaped): THE definition, every site calls fir_dither_value_hp.
// With h(seed, i) the 32 bits above (fir_dither_half) and r1 = h & 0xFFFF, value i of a stream of `channels` channels takes
//   d = f32(r1(i) - r1(i - channels)) * 2^-16,        i - channels wrapping in 64 bits,
// u[n] - u[n-1] of one uniform sequence per channel: the white form's density and variance, consecutive values of a channel
// correlated by -1/2, the power 1 - cos(w) times the white level.  Still a function of (seed, index): no state, no error feedback.
// The earlier value's word is an earlier counter's mix -- for a two-channel frame or a channel pair the word `pairs` counters
// back, key - pairs * kFirDitherStep -- EXCEPT in the stream's first frame: index 2^64 - channels + c has the counter
// 2^63 - channels / 2 + ..., not -channels / 2 + ... (i >> 1 drops the bit the subtraction borrowed), so that frame's earlier key is
// the stepped-back key with bit 63 flipped (2^63 * kFirDitherStep = 2^63 mod 2^64: the step is odd).  fir_dither_prev_key does that.
__host__ __device__ __forceinline__ uint32_t fir_dither_half(uint64_t seed, uint64_t i) {   // h(seed, i)
    const uint64_t w = fir_dither_word(seed, i >> 1);
    return static_cast<uint32_t>((i & 1) ? w >> 32 : w);
}
__host__ __device__ __forceinline__ float fir_dither_value_hp(uint32_t h, uint32_t h_prev) {   // h, h_prev: the 32 bits of values i and i - channels
    return static_cast<float>(static_cast<int32_t>(h & 0xFFFFu) - static_cast<int32_t>(h_prev & 0xFFFFu)) * (1.0f / 65536.0f);
}
// (key: the mix counter of a frame's even-indexed pair of values, seed + (pair + 1) * kFirDitherStep; back: pairs a frame * kFirDitherStep;
// first: the frame is the stream's frame 0)
__host__ __device__ __forceinline__ uint64_t fir_dither_prev_key(uint64_t key, uint64_t back, bool first) {
    return (key - back) ^ (first ? 0x8000000000000000ull : 0ull);
}
__host__ __device__ __forceinline__ float fir_pcm_dither_shaped(uint64_t seed, uint64_t i, uint32_t shape, uint32_t channels) {
    const uint32_t h = fir_dither_half(seed, i);
    return shape == RSMP_DITHER_SHAPE_HIGHPASS ? fir_dither_value_hp(h, fir_dither_half(seed, i - channels)) : fir_dither_value(h);
}
// The quantiser with the noise `d` of the value's index added: THE definition of dithered output, every site calls it.
__host__ __device__ __forceinline__ int32_t fir_pcm_quantise_dither(float x, uint32_t bits, float d) {
    return fir_pcm_code(rintf(x * fir_pcm_scale(bits) + d), bits);
}
// Output gain (rsmp_fir_set_pcm_gain, rsmp_fft_set_pcm_gain, rsmp_f32_to_pcm_gain): THE definition of PCM output under a gain, every
// store site of the fused paths calls it.  Value `i` of a stream is quantised as
//   k = f32(gain) * 2^(bits-1)              (exact: a power-of-two multiple of an f32; a normal f32 for every accepted gain)
//   p = f32(x * k)                          (one rounding)
//   q = saturate(round_half_to_even(f32(p + d(seed, i)))),  p NaN -> 0
// with d = 0 without dither (p + 0 rounds as p does: the undithered form has no addition); i, saturation and the 32-bit top code
// as above.  The product and the sum are separate operations: an fma would round x * k + d once and give other bytes for a gain
// that is no power of two (the library is compiled with -ffp-contract=off).  With gain == 1, k is fir_pcm_scale(bits) and the
// bytes are fir_pcm_quantise[_dither]'s for every input.  Accepted gains: finite, 2^-32 <= |gain| <= 2^32 (negative: polarity).
// Consequence: for a power-of-two gain the bytes are the plain quantiser's of x * gain; for any gain they are its bytes of
// f32(x * gain) wherever |x * gain| >= 2^-126 (x * gain and x * k then round at the same bit), and below that both give code 0
// without dither.
__host__ __device__ __forceinline__ bool fir_pcm_gain_ok(float gain) {
    const float a = gain < 0.0f ? -gain : gain;
    return a >= 0x1p-32f && a <= 0x1p32f;   // (NaN fails both comparisons, 0 the first, inf the second)
}
__host__ __device__ __forceinline__ float fir_pcm_gain_scale(float gain, uint32_t bits) { return gain * fir_pcm_scale(bits); }
__host__ __device__ __forceinline__ int32_t fir_pcm_quantise_gain(float x, float k, uint32_t bits) { return fir_pcm_code(rintf(x * k), bits); }
__host__ __device__ __forceinline__ int32_t fir_pcm_quantise_gain(float x, float k, uint32_t bits, float d) { return fir_pcm_code(rintf(x * k + d), bits); }
// What the quantiser did to the values it was given (rsmp_pcm_stats, include/resampler_amd.h): THE definition, every site that
// counts calls fir_pcm_stat.  x: the value before scaling; v: the quantiser's own rounded value, rintf(x * 2^(bits-1) + d).
//   values  every value;   nans  x is NaN (stored as 0, not clipped);
//   clipped v is not NaN and outside the code range: v > 2^(bits-1) - 1 or v < -2^(bits-1) -- at 32 bits, whose top code is no
//           f32 value, v >= 2^31 or v < -2^31.  +-inf clip, +1.0 clips, -1.0 does not;
//   peak    the largest |x| among the values that are not NaN, as its bit pattern (which orders non-negative floats and +inf as
//           unsigned integers): before scaling, before dither; 0 when there is none.
// Two sets merge field by field (sums, max), so no field depends on the order of evaluation.  The counters of a launch's table
// are 32 bits (a 1024-frame chunk holds 2048 values), the public totals 64.
struct FirPcmStat {
    uint32_t values, clipped, nans, peak;
};
__host__ __device__ __forceinline__ void fir_pcm_stat(float x, float v, uint32_t bits, FirPcmStat& s) {
    ++s.values;
    if (!(x == x)) {
        ++s.nans;
        return;
    }
    if (v == v) {
        if (bits == 32) s.clipped += (v >= 2147483648.0f || v < -2147483648.0f) ? 1u : 0u;
        else s.clipped += (v > (bits == 16 ? 32767.0f : 8388607.0f) || v < (bits == 16 ? -32768.0f : -8388608.0f)) ? 1u : 0u;
    }
    union { float f; uint32_t u; } a;
    a.f = x;
    const uint32_t m = a.u & 0x7FFFFFFFu;   // |x|
    if (m > s.peak) s.peak = m;
}
__host__ __device__ __forceinline__ void fir_pcm_stat_merge(FirPcmStat& s, const FirPcmStat& o) {
    s.values += o.values;
    s.clipped += o.clipped;
    s.nans += o.nans;
    if (o.peak > s.peak) s.peak = o.peak;
}
// fir_pcm_quantise_dither that also says what it did (d = 0: fir_pcm_quantise's code -- x * scale + 0 rounds as x * scale does).
__host__ __device__ __forceinline__ int32_t fir_pcm_quantise_stat(float x, uint32_t bits, float d, FirPcmStat& s) {
    const float v = rintf(x * fir_pcm_scale(bits) + d);
    fir_pcm_stat(x, v, bits, s);
    return fir_pcm_code(v, bits);
}
// The statistics under a gain describe what was quantised, p = f32(x * k): nans: p is NaN; clipped: by v, as above; peak: the
// largest |p| * 2^-(bits-1), in f32 -- the peak of the gained signal (exact: a power of two; with gain 1 it is |x|, except where
// x * 2^(bits-1) overflows f32 -- |x| >= 2^(129-bits) --, which gives +inf).  THE definition for the fused paths' counting builds and
// for rsmp_f32_to_pcm_gain.
__host__ __device__ __forceinline__ float fir_pcm_unscale(uint32_t bits) { return bits == 16 ? 0x1p-15f : bits == 24 ? 0x1p-23f : 0x1p-31f; }
__host__ __device__ __forceinline__ int32_t fir_pcm_quantise_gain_stat(float x, float k, uint32_t bits, float d, FirPcmStat& s) {
    const float p = x * k;
    const float v = rintf(p + d);
    fir_pcm_stat(p * fir_pcm_unscale(bits), v, bits, s);
    return fir_pcm_code(v, bits);
}
// Where a counting launch keeps its statistics: four words {values, clipped, nans, peak bits} per stream and 1024-output-frame
// chunk (kNfChunkShift: the repair pass's chunks), entry (stream * chunks + chunk); zeroed before the launch's main kernels.  The
// first pass merges every value it stores into its frame's chunk with atomics; the repair pass, which rewrites marked chunks whole,
// OVERWRITES their entries; fir_pcm_stats_fold behind it sums a stream's entries into the handle's totals.
struct FirStatArgs {
    uint32_t* table;
    uint32_t chunks;   // entries per stream
};
// Where fir_pcm_stats_fold puts stream s's sums: the handle's totals in device memory, merged -- or replaced, where the handle was
// cleared (rsmp_fir_pcm_stats_clear, reset) since its last counting launch.
struct FirStatTarget {
    rsmp_pcm_stats* acc;
    uint32_t overwrite, reserved;
};
// One wave's share of an entry: `s` summed over the wave's lanes (all 64 active), then one lane's atomics -- none for a zero.
__device__ __forceinline__ FirPcmStat fir_stat_wave_sum(FirPcmStat s) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        s.values += __shfl_xor(s.values, m, 64);
        const uint32_t p = __shfl_xor(s.peak, m, 64);
        s.peak = p > s.peak ? p : s.peak;
    }
    if (__any(s.clipped | s.nans)) {   // (rare: clean audio has neither)
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            s.clipped += __shfl_xor(s.clipped, m, 64);
            s.nans += __shfl_xor(s.nans, m, 64);
        }
    }
    return s;
}
__device__ __forceinline__ void fir_stat_atomic_merge(uint32_t* entry, const FirPcmStat& s) {
    if (s.values) (void)atomicAdd(entry, s.values);
    if (s.clipped) (void)atomicAdd(entry + 1, s.clipped);
    if (s.nans) (void)atomicAdd(entry + 2, s.nans);
    if (s.peak) (void)atomicMax(entry + 3, s.peak);
}
// One sample of a stream's PCM `out`, index `i` in values: the lane writes the sample's own bytes and no others.
__device__ __forceinline__ void fir_pcm_store_code(void* out, uint32_t bits, size_t i, int32_t q) {
    if (bits == 16) {
        static_cast<int16_t*>(out)[i] = static_cast<int16_t>(q);
    } else if (bits == 32) {
        static_cast<int32_t*>(out)[i] = q;
    } else {
        uint8_t* p = static_cast<uint8_t*>(out) + 3 * i;
        p[0] = static_cast<uint8_t>(q);
        p[1] = static_cast<uint8_t>(q >> 8);
        p[2] = static_cast<uint8_t>(q >> 16);
    }
}
__device__ __forceinline__ void fir_pcm_store(void* out, uint32_t bits, size_t i, float y) { fir_pcm_store_code(out, bits, i, fir_pcm_quantise(y, bits)); }
// ... and by the factor `k` of a stream's descriptor (fir_pcm_quantise_gain)
__device__ __forceinline__ void fir_pcm_store(void* out, uint32_t bits, size_t i, float y, float k) { fir_pcm_store_code(out, bits, i, fir_pcm_quantise_gain(y, k, bits)); }
// A counting build's store of value `i` (as fir_out_store below): the bytes of the plain / dithered builds, and `s` says what was done.
__device__ __forceinline__ void fir_out_store_stat(const FirStreamDesc& d, size_t i, float y, FirPcmStat& s) {
    const float noise = d.dither == RSMP_DITHER_TPDF ? fir_pcm_dither_shaped(d.dither_seed, d.abs_out * d.channels + i, d.dither_shape, d.channels) : 0.0f;
    fir_pcm_store_code(d.out, d.out_bits, i, fir_pcm_quantise_gain_stat(y, d.pcm_k, d.out_bits, noise, s));
}
// Value `i` of a stream's output in this launch.  OUT: the PCM-output builds of the generic kernels and of the repair pass (out_bits
// != 0), with and without dither; the f32 builds do not read the fields.
template <int OUT>
__device__ __forceinline__ void fir_out_store(const FirStreamDesc& d, size_t i, float y) {
    if constexpr (OUT == kFirOutPcmTpdf)
        fir_pcm_store_code(d.out, d.out_bits, i, fir_pcm_quantise_gain(y, d.pcm_k, d.out_bits, fir_pcm_dither_shaped(d.dither_seed, d.abs_out * d.channels + i, d.dither_shape, d.channels)));
    else if constexpr (OUT == kFirOutPcm) fir_pcm_store(d.out, d.out_bits, i, y, d.pcm_k);
    else d.out[i] = y;
}

// Generic kernel: any ratio, reference-form two-row interpolation; grid = (max tiles, streams).
// (format, here and below: the launch's FirFormat (fir_format.h) -- format.out_mode() selects the builds that store f32, PCM, dithered
// PCM or counted PCM; st, for a counting launch: its statistics table, stream s's entries the s-th row; hipErrorInvalidValue without one)
hipError_t launch_fir_generic(const FirStreamDesc* d_descs, uint32_t n_streams, uint32_t max_out,
                              uint32_t max_channels, hipStream_t stream, bool fuse_tail = false, const FirFormat& format = FirFormat{}, const FirStatArgs& st = {});
// The same arithmetic for LONG launches (fir_generic_bulk.hip): tiles of up to 4096 output frames per workgroup, their outputs sorted
// by phase row, the tile's input window in LDS.  Which launches take it, which build, tile, grid and LDS: generic_launch_choice
// (fir_generic_plan.h); `choice` is its answer for the launch, hipErrorInvalidValue for one that is not tiled.  Does not copy the
// tails (launch_fir_tail_copy).
hipError_t launch_fir_generic_bulk(const FirStreamDesc* d_descs, uint32_t n_streams, const GenericLaunchChoice& choice, hipStream_t stream,
                                   const FirFormat& format = FirFormat{}, const FirStatArgs& st = {});
// Re-evaluates, in the reference's two-row form, the output chunks a periodic launch marked as non-finite
// (fir_nonfinite.h); exits at once when the launch marked nothing.
// (done / done_attached, here and in launch_fir_tail_copy: as in launch_fir_repair_multi below -- the launch completes `done`
// itself; *done_attached stays false when there was nothing to launch)
hipError_t launch_fir_repair(const FirStreamDesc* d_descs, uint32_t n_streams, const NfArgs& nf, hipStream_t stream,
                             hipEvent_t done = nullptr, bool* done_attached = nullptr, const FirFormat& format = FirFormat{}, const FirStatArgs& st = {});   // (counting: never completes `done` -- the fold follows)
// The same for up to eight groups of streams (each with its own marks) in one launch.
struct RepairJob {
    const FirStreamDesc* d_descs;
    uint32_t n_streams;
    NfArgs nf;
    uint32_t stat_first = 0;   // counting launches: the row of the launch's statistics table that holds the job's first stream
};
constexpr uint32_t kMaxRepairJobs = 8;
// (tail_descs: the launch also copies the tails of these n_tail streams -- what launch_fir_tail_copy does -- in one more row
// of its grid)
// (done / done_attached: an event the LAST of these launches completes itself -- hipExtLaunchKernel's stop event, no packet of its
// own behind the kernel as hipEventRecord puts there; *done_attached = false: there was no such launch, record it yourself)
hipError_t launch_fir_repair_multi(const RepairJob* jobs, size_t n_jobs, hipStream_t stream, const FirStreamDesc* tail_descs = nullptr,
                                   uint32_t n_tail = 0, uint32_t max_tail_values = 0, hipEvent_t done = nullptr, bool* done_attached = nullptr,
                                   const FirFormat& format = FirFormat{}, const FirStatArgs& st = {});
// Behind a counting launch and its repair pass: a workgroup per stream sums the stream's row of st.table into d_targets[s]
// (device memory).  (done / done_attached: as above)
hipError_t launch_fir_pcm_stats_fold(const FirStatArgs& st, uint32_t n_streams, const FirStatTarget* d_targets, hipStream_t stream,
                                     hipEvent_t done = nullptr, bool* done_attached = nullptr);
// Copies the still-buffered tail of [hist|in] into hist_next; grid = (blocks, streams).
hipError_t launch_fir_tail_copy(const FirStreamDesc* d_descs, uint32_t n_streams,
                                uint32_t max_tail_values, hipStream_t stream, hipEvent_t done = nullptr, bool* done_attached = nullptr);

}  // namespace rsmp
