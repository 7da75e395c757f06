// cli_kernels.hip -- the reference CLI's helpers around the hot path, on the GPU:
//   * the two comparison interpolators, linear and 4-point 3rd-order Hermite
//     (resample/src/interpolation_resampler.rs:41-126): one lane per output value, position in f64 exactly
//     as the reference computes it (output index / ratio), arithmetic in the reference's order;
//   * WAV sample conversion (resample/src/main.rs:128-156): 16 / 24 / 32-bit little-endian PCM -> f32
//     (`s as f32 / (1 << (bits - 1)) as f32`) with mono duplicated to stereo, so a decoded file goes from
//     its PCM bytes in HBM to the interleaved f32 frames the resamplers take in one pass;
//   * the way back, f32 -> 16 / 24 / 32-bit little-endian PCM (fir_pcm_quantise, fir_kernels.h: round half to even, saturate,
//     NaN -> 0), without or with TPDF dither (fir_pcm_quantise_dither), on the host and as a streaming pass on the device,
//     and the same under an output gain (fir_pcm_quantise_gain: the two-pass reference of the fused stores' gain).
// Both are HBM-bound elementwise kernels: coalesced loads / stores, nothing to stage.
#include <hip/hip_runtime.h>

#include <cstring>

#include <cmath>
#include <cstdint>

#include "../../include/resampler_amd.h"
#include "common.h"
#include "device_util.h"
#include "fir_kernels.h"

namespace {

constexpr int kThreads = 256;

template <bool HERMITE>
__global__ __launch_bounds__(kThreads) void interp_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                          uint32_t channels, uint64_t input_frames,
                                                          uint64_t output_frames, double ratio) {
    const uint64_t e = blockIdx.x * static_cast<uint64_t>(kThreads) + threadIdx.x;
    if (e >= output_frames * channels) return;
    const uint64_t o = e / channels;
    const uint32_t ch = static_cast<uint32_t>(e - o * channels);
    const double input_pos = static_cast<double>(o) / ratio;                  // :51, :93
    const uint64_t idx = static_cast<uint64_t>(floor(input_pos));
    const float frac = static_cast<float>(input_pos - static_cast<double>(idx));
    const uint64_t last = input_frames - 1;
    if constexpr (!HERMITE) {
        if (idx >= last) {                                                    // :55-62
            out[e] = in[last * channels + ch];
            return;
        }
        const float s0 = in[idx * channels + ch], s1 = in[(idx + 1) * channels + ch];
        out[e] = s0 * (1.0f - frac) + s1 * frac;                              // :71
    } else {
        const uint64_t i_prev = idx > 0 ? idx - 1 : 0;                        // :99-106
        const uint64_t i_cur = idx < last ? idx : last;
        const uint64_t i_n1 = idx + 1 < last ? idx + 1 : last;
        const uint64_t i_n2 = idx + 2 < last ? idx + 2 : last;
        const float previous = in[i_prev * channels + ch], current = in[i_cur * channels + ch];
        const float next_1 = in[i_n1 * channels + ch], next_2 = in[i_n2 * channels + ch];
        const float c0 = current;                                             // :114-117
        const float c1 = (next_1 - previous) * 0.5f;
        const float c2 = previous - current * 2.5f + next_1 * 2.0f - next_2 * 0.5f;
        const float c3 = (next_2 - previous) * 0.5f + (current - next_1) * 1.5f;
        out[e] = ((c3 * frac + c2) * frac + c1) * frac + c0;                   // :119
    }
}

template <int BITS>
__global__ __launch_bounds__(kThreads) void pcm_kernel(const uint8_t* __restrict__ pcm, float* __restrict__ out,
                                                       uint64_t n_samples, uint32_t mono) {
    const uint64_t i = blockIdx.x * static_cast<uint64_t>(kThreads) + threadIdx.x;
    if (i >= n_samples) return;
    int32_t s;
    if constexpr (BITS == 16) {
        s = reinterpret_cast<const int16_t*>(pcm)[i];
    } else if constexpr (BITS == 24) {
        const uint32_t u = static_cast<uint32_t>(pcm[3 * i]) | (static_cast<uint32_t>(pcm[3 * i + 1]) << 8) |
                           (static_cast<uint32_t>(pcm[3 * i + 2]) << 16);
        s = static_cast<int32_t>(u << 8) >> 8;
    } else {
        s = reinterpret_cast<const int32_t*>(pcm)[i];
    }
    // main.rs:131 `(1 << (bits_per_sample - 1)) as f32`: the literal is an i32, so 32-bit files divide by
    // 1i32 << 31 = i32::MIN = -2^31 -- the reference decodes them with inverted polarity, and so does this.
    const float max_value = BITS == 32 ? -2147483648.0f : static_cast<float>(1 << (BITS - 1));
    const float v = static_cast<float>(s) / max_value;
    if (mono) {                                                               // main.rs:141-146
        reinterpret_cast<float2*>(out)[i] = make_float2(v, v);
    } else {
        out[i] = v;
    }
}

// f32 -> PCM: a lane takes four values (one 16-byte load) and writes their 8 / 12 / 16 bytes -- whole words at a 4-byte aligned
// address, since the lane's first byte is 8 / 12 / 16 x its index from a 4-byte aligned base; the last lane of the buffer takes the
// n % 4 values left over one by one, each with stores of the sample's own bytes.  Every byte is written once, by the lane that
// owns it, and none past n * BITS / 8.
template <int BITS>
__global__ __launch_bounds__(kThreads) void f32_to_pcm_kernel(const float* __restrict__ in, uint8_t* __restrict__ out, uint64_t n) {
    typedef float v4f_in __attribute__((ext_vector_type(4)));
    const uint64_t n4 = n / 4, stride = static_cast<uint64_t>(gridDim.x) * kThreads;
    for (uint64_t i = blockIdx.x * static_cast<uint64_t>(kThreads) + threadIdx.x; i <= n4; i += stride) {
        if (i == n4) {   // the 0 .. 3 values behind the last whole four
            for (uint64_t k = 4 * n4; k < n; ++k) rsmp::fir_pcm_store(out, BITS, k, in[k]);
            break;
        }
        const v4f_in x = reinterpret_cast<const v4f_in*>(in)[i];
        const uint32_t q0 = static_cast<uint32_t>(rsmp::fir_pcm_quantise(x.x, BITS)), q1 = static_cast<uint32_t>(rsmp::fir_pcm_quantise(x.y, BITS));
        const uint32_t q2 = static_cast<uint32_t>(rsmp::fir_pcm_quantise(x.z, BITS)), q3 = static_cast<uint32_t>(rsmp::fir_pcm_quantise(x.w, BITS));
        uint32_t* o = reinterpret_cast<uint32_t*>(out + i * (BITS / 2));
        if constexpr (BITS == 16) {
            o[0] = (q0 & 0xFFFFu) | (q1 << 16);
            o[1] = (q2 & 0xFFFFu) | (q3 << 16);
        } else if constexpr (BITS == 24) {
            o[0] = (q0 & 0xFFFFFFu) | (q1 << 24);
            o[1] = ((q1 >> 8) & 0xFFFFu) | (q2 << 16);
            o[2] = ((q2 >> 16) & 0xFFu) | (q3 << 8);
        } else {
            o[0] = q0; o[1] = q1; o[2] = q2; o[3] = q3;
        }
    }
}

// The same lanes, loads and stores with TPDF dither: value k of the buffer has the index first + k (wrapping) and takes the noise
// fir_pcm_dither(seed, first + k) -- each value by the definition itself, whatever the parity of `first`.
template <int BITS>
__global__ __launch_bounds__(kThreads) void f32_to_pcm_tpdf_kernel(const float* __restrict__ in, uint8_t* __restrict__ out, uint64_t n, uint64_t seed,
                                                                   uint64_t first) {
    typedef float v4f_in __attribute__((ext_vector_type(4)));
    const uint64_t n4 = n / 4, stride = static_cast<uint64_t>(gridDim.x) * kThreads;
    auto code = [&](float x, uint64_t k) { return static_cast<uint32_t>(rsmp::fir_pcm_quantise_dither(x, BITS, rsmp::fir_pcm_dither(seed, first + k))); };
    for (uint64_t i = blockIdx.x * static_cast<uint64_t>(kThreads) + threadIdx.x; i <= n4; i += stride) {
        if (i == n4) {   // the 0 .. 3 values behind the last whole four
            for (uint64_t k = 4 * n4; k < n; ++k) rsmp::fir_pcm_store_code(out, BITS, k, static_cast<int32_t>(code(in[k], k)));
            break;
        }
        const v4f_in x = reinterpret_cast<const v4f_in*>(in)[i];
        const uint32_t q0 = code(x.x, 4 * i), q1 = code(x.y, 4 * i + 1), q2 = code(x.z, 4 * i + 2), q3 = code(x.w, 4 * i + 3);
        uint32_t* o = reinterpret_cast<uint32_t*>(out + i * (BITS / 2));
        if constexpr (BITS == 16) {
            o[0] = (q0 & 0xFFFFu) | (q1 << 16);
            o[1] = (q2 & 0xFFFFu) | (q3 << 16);
        } else if constexpr (BITS == 24) {
            o[0] = (q0 & 0xFFFFFFu) | (q1 << 24);
            o[1] = ((q1 >> 8) & 0xFFFFu) | (q2 << 16);
            o[2] = ((q2 >> 16) & 0xFFu) | (q3 << 8);
        } else {
            o[0] = q0; o[1] = q1; o[2] = q2; o[3] = q3;
        }
    }
}

// The same lanes, loads and stores, counted (fir_pcm_stat: the rule of rsmp_f32_to_pcm_stats), without or with TPDF dither; `out`
// may be null: measure only.  A lane keeps its own sums; they are added up inside the wave, then inside the workgroup, and the
// workgroup's first lane merges them into *stats with at most four atomics.
template <int BITS, bool TPDF>
__global__ __launch_bounds__(kThreads) void f32_to_pcm_stats_kernel(const float* __restrict__ in, uint8_t* __restrict__ out, uint64_t n, uint64_t seed,
                                                                    uint64_t first, rsmp_pcm_stats* __restrict__ stats) {
    typedef float v4f_in __attribute__((ext_vector_type(4)));
    const uint64_t n4 = n / 4, stride = static_cast<uint64_t>(gridDim.x) * kThreads;
    rsmp::FirPcmStat mine{0, 0, 0, 0};
    auto code = [&](float x, uint64_t k) {
        const float d = TPDF ? rsmp::fir_pcm_dither(seed, first + k) : 0.0f;
        return static_cast<uint32_t>(rsmp::fir_pcm_quantise_stat(x, BITS, d, mine));
    };
    for (uint64_t i = blockIdx.x * static_cast<uint64_t>(kThreads) + threadIdx.x; i <= n4; i += stride) {
        if (i == n4) {   // the 0 .. 3 values behind the last whole four
            for (uint64_t k = 4 * n4; k < n; ++k) {
                const int32_t q = static_cast<int32_t>(code(in[k], k));
                if (out) rsmp::fir_pcm_store_code(out, BITS, k, q);
            }
            break;
        }
        const v4f_in x = reinterpret_cast<const v4f_in*>(in)[i];
        const uint32_t q0 = code(x.x, 4 * i), q1 = code(x.y, 4 * i + 1), q2 = code(x.z, 4 * i + 2), q3 = code(x.w, 4 * i + 3);
        if (!out) continue;
        uint32_t* o = reinterpret_cast<uint32_t*>(out + i * (BITS / 2));
        if constexpr (BITS == 16) {
            o[0] = (q0 & 0xFFFFu) | (q1 << 16);
            o[1] = (q2 & 0xFFFFu) | (q3 << 16);
        } else if constexpr (BITS == 24) {
            o[0] = (q0 & 0xFFFFFFu) | (q1 << 24);
            o[1] = ((q1 >> 8) & 0xFFFFu) | (q2 << 16);
            o[2] = ((q2 >> 16) & 0xFFu) | (q3 << 8);
        } else {
            o[0] = q0; o[1] = q1; o[2] = q2; o[3] = q3;
        }
    }
    // (a lane's counts stay far below 2^32: the grid has a lane per four values up to 8 workgroups a CU, and walks on from there)
    __shared__ rsmp::FirPcmStat waves[kThreads / 64];
    const rsmp::FirPcmStat w = rsmp::fir_stat_wave_sum(mine);
    if ((threadIdx.x & 63) == 0) waves[threadIdx.x >> 6] = w;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long values = 0, clipped = 0, nans = 0;
        uint32_t peak = 0;
        for (int k = 0; k < kThreads / 64; ++k) {
            values += waves[k].values;
            clipped += waves[k].clipped;
            nans += waves[k].nans;
            peak = waves[k].peak > peak ? waves[k].peak : peak;
        }
        static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "64-bit atomics on the counts");
        if (values) (void)atomicAdd(reinterpret_cast<unsigned long long*>(&stats->values), values);
        if (clipped) (void)atomicAdd(reinterpret_cast<unsigned long long*>(&stats->clipped), clipped);
        if (nans) (void)atomicAdd(reinterpret_cast<unsigned long long*>(&stats->nans), nans);
        if (peak) (void)atomicMax(reinterpret_cast<uint32_t*>(&stats->peak), peak);   // (the bit pattern of |x| orders non-negative floats and +inf)
    }
}

int check_device() {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
        return rsmp::fail(RSMP_ERR_NO_DEVICE, "no HIP device (this engine has no CPU path)");
    return RSMP_OK;
}

}  // namespace

extern "C" size_t rsmp_interp_output_len(size_t channels, uint32_t in_hz, uint32_t out_hz, size_t in_len) {
    if (channels == 0 || in_hz == 0 || out_hz == 0) return 0;
    const double ratio = static_cast<double>(out_hz) / static_cast<double>(in_hz);
    return static_cast<size_t>(std::ceil(static_cast<double>(in_len / channels) * ratio)) * channels;
}

extern "C" int rsmp_interp_resample_device(int mode, size_t channels, uint32_t in_hz, uint32_t out_hz,
                                           const float* d_in, size_t in_len, float* d_out, size_t out_cap,
                                           size_t* produced, void* stream) {
    if (int rc = check_device()) return rc;
    if ((mode != RSMP_INTERP_LINEAR && mode != RSMP_INTERP_HERMITE) || channels == 0 || in_hz == 0 || out_hz == 0)
        return rsmp::fail(RSMP_ERR_INVALID_ARGUMENT, "rsmp_interp_resample: invalid mode / channels / rate");
    if (in_len % channels != 0) return rsmp::fail(RSMP_ERR_INVALID_INPUT_BUFFER_SIZE, "Input buffer size is invalid");
    const size_t need = rsmp_interp_output_len(channels, in_hz, out_hz, in_len);
    if (need > out_cap)
        return rsmp::fail(RSMP_ERR_CAPACITY, "interpolator output needs %zu values, room for %zu", need, out_cap);
    if (produced) *produced = need;
    if (need == 0) return RSMP_OK;
    const double ratio = static_cast<double>(out_hz) / static_cast<double>(in_hz);
    const uint64_t in_frames = in_len / channels, out_frames = need / channels;
    const dim3 grid(static_cast<uint32_t>((need + kThreads - 1) / kThreads));
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (mode == RSMP_INTERP_LINEAR)
        hipLaunchKernelGGL(interp_kernel<false>, grid, dim3(kThreads), 0, s, d_in, d_out, static_cast<uint32_t>(channels),
                           in_frames, out_frames, ratio);
    else
        hipLaunchKernelGGL(interp_kernel<true>, grid, dim3(kThreads), 0, s, d_in, d_out, static_cast<uint32_t>(channels),
                           in_frames, out_frames, ratio);
    RSMP_HIP_CHECK(hipGetLastError());
    return RSMP_OK;
}

extern "C" int rsmp_interp_resample(int mode, size_t channels, uint32_t in_hz, uint32_t out_hz, const float* in,
                                    size_t in_len, float* out, size_t out_cap, size_t* produced) {
    if (int rc = check_device()) return rc;
    rsmp::DeviceBuffer d_in, d_out;
    RSMP_HIP_CHECK(d_in.reserve((in_len + 4) * sizeof(float)));
    RSMP_HIP_CHECK(d_out.reserve((out_cap + 4) * sizeof(float)));
    if (in_len) RSMP_HIP_CHECK(hipMemcpy(d_in.get(), in, in_len * sizeof(float), hipMemcpyHostToDevice));
    size_t p = 0;
    const int rc = rsmp_interp_resample_device(mode, channels, in_hz, out_hz, d_in.as<float>(), in_len,
                                               d_out.as<float>(), out_cap, &p, nullptr);
    if (rc != RSMP_OK) return rc;
    RSMP_HIP_CHECK(hipDeviceSynchronize());
    if (p) RSMP_HIP_CHECK(hipMemcpy(out, d_out.get(), p * sizeof(float), hipMemcpyDeviceToHost));
    if (produced) *produced = p;
    return RSMP_OK;
}

extern "C" int rsmp_pcm_to_stereo_f32_device(const void* d_pcm, int bits, int channels, size_t n_samples,
                                             float* d_out, void* stream) {
    if (int rc = check_device()) return rc;
    if ((bits != 16 && bits != 24 && bits != 32) || (channels != 1 && channels != 2))
        return rsmp::fail(RSMP_ERR_INVALID_ARGUMENT, "rsmp_pcm_to_stereo_f32: 16 / 24 / 32 bits, 1 or 2 channels");
    if (n_samples == 0) return RSMP_OK;
    const dim3 grid(static_cast<uint32_t>((n_samples + kThreads - 1) / kThreads));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const uint8_t* p = static_cast<const uint8_t*>(d_pcm);
    const uint32_t mono = channels == 1 ? 1u : 0u;
    if (bits == 16) hipLaunchKernelGGL(pcm_kernel<16>, grid, dim3(kThreads), 0, s, p, d_out, static_cast<uint64_t>(n_samples), mono);
    else if (bits == 24) hipLaunchKernelGGL(pcm_kernel<24>, grid, dim3(kThreads), 0, s, p, d_out, static_cast<uint64_t>(n_samples), mono);
    else hipLaunchKernelGGL(pcm_kernel<32>, grid, dim3(kThreads), 0, s, p, d_out, static_cast<uint64_t>(n_samples), mono);
    RSMP_HIP_CHECK(hipGetLastError());
    return RSMP_OK;
}

// f32 -> PCM kernels' grid: a lane per four values and one for the rest
static dim3 f32_to_pcm_grid(size_t n_values) {
    int cus = 256;
    int device = 0;
    (void)hipGetDevice(&device);
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device);
    const uint64_t lanes = n_values / 4 + 1;
    const uint64_t blocks = (lanes + kThreads - 1) / kThreads, most = static_cast<uint64_t>(cus) * 8u;   // (eight workgroups of 256 a CU walk the buffer side by side)
    return dim3(static_cast<uint32_t>(blocks < most ? blocks : most));
}

// The definition itself, on the host (no device needed).
extern "C" int rsmp_f32_to_pcm(const float* in, size_t n_values, int bits, void* out_pcm) {
    if ((bits != 16 && bits != 24 && bits != 32) || (n_values != 0 && (!in || !out_pcm)))
        return rsmp::fail(RSMP_ERR_INVALID_ARGUMENT, "rsmp_f32_to_pcm: 16 / 24 / 32 bits, non-null buffers");
    uint8_t* o = static_cast<uint8_t*>(out_pcm);
    const size_t bytes = static_cast<size_t>(bits) / 8;
    for (size_t i = 0; i < n_values; ++i) {
        const uint32_t q = static_cast<uint32_t>(rsmp::fir_pcm_quantise(in[i], static_cast<uint32_t>(bits)));
        for (size_t b = 0; b < bytes; ++b) o[i * bytes + b] = static_cast<uint8_t>(q >> (8 * b));   // little-endian
    }
    return RSMP_OK;
}

extern "C" int rsmp_f32_to_pcm_device(const float* d_in, size_t n_values, int bits, void* d_pcm, void* stream) {
    if ((bits != 16 && bits != 24 && bits != 32) || (n_values != 0 && (!d_in || !d_pcm)))
        return rsmp::fail(RSMP_ERR_INVALID_ARGUMENT, "rsmp_f32_to_pcm_device: 16 / 24 / 32 bits, non-null buffers");
    if (reinterpret_cast<uintptr_t>(d_in) % 16 != 0 || reinterpret_cast<uintptr_t>(d_pcm) % 4 != 0)
        return rsmp::fail(RSMP_ERR_INVALID_ARGUMENT, "rsmp_f32_to_pcm_device: d_in 16-byte aligned, d_pcm 4-byte aligned");
    if (int rc = check_device()) return rc;
    if (n_values == 0) return RSMP_OK;
    const dim3 grid = f32_to_pcm_grid(n_values);
    hipStream_t s = static_cast<hipStream_t>(stream);
    uint8_t* o = static_cast<uint8_t*>(d_pcm);
    if (bits == 16) hipLaunchKernelGGL(f32_to_pcm_kernel<16>, grid, dim3(kThreads), 0, s, d_in, o, static_cast<uint64_t>(n_values));
    else if (bits == 24) hipLaunchKernelGGL(f32_to_pcm_kernel<24>, grid, dim3(kThreads), 0, s, d_in, o, static_cast<uint64_t>(n_values));
    else hipLaunchKernelGGL(f32_to_pcm_kernel<32>, grid, dim3(kThreads), 0, s, d_in, o, static_cast<uint64_t>(n_values));
    RSMP_HIP_CHECK(hipGetLastError());
    return RSMP_OK;
}

// The definition with dither, on the host (no device needed).
extern "C" int rsmp_f32_to_pcm_dither(const float* in, size_t n_values, int bits, int dither, uint64_t seed, uint64_t first_index, void* out_pcm) {
    if ((bits != 16 && bits != 24 && bits != 32) || (dither != RSMP_DITHER_NONE && dither != RSMP_DITHER_TPDF) || (n_values != 0 && (!in || !out_pcm)))
        return rsmp::fail(RSMP_ERR_INVALID_ARGUMENT, "rsmp_f32_to_pcm_dither: 16 / 24 / 32 bits, RSMP_DITHER_NONE / RSMP_DITHER_TPDF, non-null buffers");
    if (dither == RSMP_DITHER_NONE) return rsmp_f32_to_pcm(in, n_values, bits, out_pcm);
    uint8_t* o = static_cast<uint8_t*>(out_pcm);
    const size_t bytes = static_cast<size_t>(bits) / 8;
    for (size_t i = 0; i < n_values; ++i) {
        const float d = rsmp::fir_pcm_dither(seed, first_index + i);
        const uint32_t q = static_cast<uint32_t>(rsmp::fir_pcm_quantise_dither(in[i], static_cast<uint32_t>(bits), d));
        for (size_t b = 0; b < bytes; ++b) o[i * bytes + b] = static_cast<uint8_t>(q >> (8 * b));   // little-endian
    }
    return RSMP_OK;
}

extern "C" int rsmp_f32_to_pcm_dither_device(const float* d_in, size_t n_values, int bits, int dither, uint64_t seed, uint64_t first_index,
                                             void* d_pcm, void* stream) {
    if ((bits != 16 && bits != 24 && bits != 32) || (dither != RSMP_DITHER_NONE && dither != RSMP_DITHER_TPDF) || (n_values != 0 && (!d_in || !d_pcm)))
        return rsmp::fail(RSMP_ERR_INVALID_ARGUMENT, "rsmp_f32_to_pcm_dither_device: 16 / 24 / 32 bits, RSMP_DITHER_NONE / RSMP_DITHER_TPDF, non-null buffers");
    if (dither == RSMP_DITHER_NONE) return rsmp_f32_to_pcm_device(d_in, n_values, bits, d_pcm, stream);
    if (reinterpret_cast<uintptr_t>(d_in) % 16 != 0 || reinterpret_cast<uintptr_t>(d_pcm) % 4 != 0)
        return rsmp::fail(RSMP_ERR_INVALID_ARGUMENT, "rsmp_f32_to_pcm_dither_device: d_in 16-byte aligned, d_pcm 4-byte aligned");
    if (int rc = check_device()) return rc;
    if (n_values == 0) return RSMP_OK;
    const dim3 grid = f32_to_pcm_grid(n_values);
    hipStream_t s = static_cast<hipStream_t>(stream);
    uint8_t* o = static_cast<uint8_t*>(d_pcm);
    const uint64_t n = n_values;
    if (bits == 16) hipLaunchKernelGGL(f32_to_pcm_tpdf_kernel<16>, grid, dim3(kThreads), 0, s, d_in, o, n, seed, first_index);
    else if (bits == 24) hipLaunchKernelGGL(f32_to_pcm_tpdf_kernel<24>, grid, dim3(kThreads), 0, s, d_in, o, n, seed, first_index);
    else hipLaunchKernelGGL(f32_to_pcm_tpdf_kernel<32>, grid, dim3(kThreads), 0, s, d_in, o, n, seed, first_index);
    RSMP_HIP_CHECK(hipGetLastError());
    return RSMP_OK;
}

// The definition of the statistics, on the host (no device needed): what rsmp_f32_to_pcm_dither writes, and what it did.
extern "C" int rsmp_f32_to_pcm_stats(const float* in, size_t n_values, int bits, int dither, uint64_t seed, uint64_t first_index, void* out_pcm,
                                     rsmp_pcm_stats* stats) {
    if ((bits != 16 && bits != 24 && bits != 32) || (dither != RSMP_DITHER_NONE && dither != RSMP_DITHER_TPDF) || !stats || (n_values != 0 && !in))
        return rsmp::fail(RSMP_ERR_INVALID_ARGUMENT, "rsmp_f32_to_pcm_stats: 16 / 24 / 32 bits, RSMP_DITHER_NONE / RSMP_DITHER_TPDF, non-null input and statistics");
    uint8_t* o = static_cast<uint8_t*>(out_pcm);
    const size_t bytes = static_cast<size_t>(bits) / 8;
    rsmp_pcm_stats t{};
    uint32_t peak = 0;
    for (size_t i = 0; i < n_values; ++i) {
        rsmp::FirPcmStat one{0, 0, 0, peak};
        const float d = dither == RSMP_DITHER_TPDF ? rsmp::fir_pcm_dither(seed, first_index + i) : 0.0f;
        const uint32_t q = static_cast<uint32_t>(rsmp::fir_pcm_quantise_stat(in[i], static_cast<uint32_t>(bits), d, one));
        t.values += one.values;
        t.clipped += one.clipped;
        t.nans += one.nans;
        peak = one.peak;
        if (o)
            for (size_t b = 0; b < bytes; ++b) o[i * bytes + b] = static_cast<uint8_t>(q >> (8 * b));   // little-endian
    }
    std::memcpy(&t.peak, &peak, sizeof peak);
    *stats = t;
    return RSMP_OK;
}

extern "C" int rsmp_f32_to_pcm_stats_device(const float* d_in, size_t n_values, int bits, int dither, uint64_t seed, uint64_t first_index,
                                            void* d_pcm, rsmp_pcm_stats* d_stats, void* stream) {
    if ((bits != 16 && bits != 24 && bits != 32) || (dither != RSMP_DITHER_NONE && dither != RSMP_DITHER_TPDF) || !d_stats || (n_values != 0 && !d_in))
        return rsmp::fail(RSMP_ERR_INVALID_ARGUMENT, "rsmp_f32_to_pcm_stats_device: 16 / 24 / 32 bits, RSMP_DITHER_NONE / RSMP_DITHER_TPDF, non-null input and statistics");
    if (reinterpret_cast<uintptr_t>(d_in) % 16 != 0 || reinterpret_cast<uintptr_t>(d_pcm) % 4 != 0 || reinterpret_cast<uintptr_t>(d_stats) % 8 != 0)
        return rsmp::fail(RSMP_ERR_INVALID_ARGUMENT, "rsmp_f32_to_pcm_stats_device: d_in 16-byte aligned, d_pcm 4-byte aligned, d_stats 8-byte aligned");
    if (int rc = check_device()) return rc;
    if (n_values == 0) return RSMP_OK;
    const dim3 grid = f32_to_pcm_grid(n_values);
    hipStream_t s = static_cast<hipStream_t>(stream);
    uint8_t* o = static_cast<uint8_t*>(d_pcm);
    const uint64_t n = n_values;
#define RSMP_STATS_LAUNCH(BITS, TPDF) hipLaunchKernelGGL((f32_to_pcm_stats_kernel<BITS, TPDF>), grid, dim3(kThreads), 0, s, d_in, o, n, seed, first_index, d_stats)
    if (dither == RSMP_DITHER_TPDF) {
        if (bits == 16) RSMP_STATS_LAUNCH(16, true);
        else if (bits == 24) RSMP_STATS_LAUNCH(24, true);
        else RSMP_STATS_LAUNCH(32, true);
    } else {
        if (bits == 16) RSMP_STATS_LAUNCH(16, false);
        else if (bits == 24) RSMP_STATS_LAUNCH(24, false);
        else RSMP_STATS_LAUNCH(32, false);
    }
#undef RSMP_STATS_LAUNCH
    RSMP_HIP_CHECK(hipGetLastError());
    return RSMP_OK;
}

// ---- the quantiser under a gain (fir_pcm_quantise_gain, fir_kernels.h): what the fused PCM stores do, as a pass of its own -----
// The two-pass reference of the fused paths' output gain.  The entries above keep their kernels and their arithmetic; these are
// builds of their own, by width and dither mode, that take the factor k = gain * 2^(bits-1) as an argument and count when asked.
namespace {

// f32_to_pcm_stats_kernel's lanes, loads and stores; `out` and `stats` may each be null.
// HP: the high-pass form of the TPDF noise (fir_pcm_dither_shaped: value i with the value `channels` indices before it) -- builds of
// their own beside the white ones, which stay what they were.
template <int BITS, bool TPDF, bool HP = false>
__global__ __launch_bounds__(kThreads) void f32_to_pcm_gain_kernel(const float* __restrict__ in, uint8_t* __restrict__ out, uint64_t n, float k, uint64_t seed,
                                                                   uint64_t first, rsmp_pcm_stats* __restrict__ stats, uint32_t channels = 0) {
    typedef float v4f_in __attribute__((ext_vector_type(4)));
    const uint64_t n4 = n / 4, stride = static_cast<uint64_t>(gridDim.x) * kThreads;
    rsmp::FirPcmStat mine{0, 0, 0, 0};
    auto code = [&](float x, uint64_t i) {
        const float d = !TPDF ? 0.0f : HP ? rsmp::fir_pcm_dither_shaped(seed, first + i, RSMP_DITHER_SHAPE_HIGHPASS, channels) : rsmp::fir_pcm_dither(seed, first + i);
        return static_cast<uint32_t>(rsmp::fir_pcm_quantise_gain_stat(x, k, BITS, d, mine));
    };
    for (uint64_t i = blockIdx.x * static_cast<uint64_t>(kThreads) + threadIdx.x; i <= n4; i += stride) {
        if (i == n4) {   // the 0 .. 3 values behind the last whole four
            for (uint64_t j = 4 * n4; j < n; ++j) {
                const int32_t q = static_cast<int32_t>(code(in[j], j));
                if (out) rsmp::fir_pcm_store_code(out, BITS, j, q);
            }
            break;
        }
        const v4f_in x = reinterpret_cast<const v4f_in*>(in)[i];
        const uint32_t q0 = code(x.x, 4 * i), q1 = code(x.y, 4 * i + 1), q2 = code(x.z, 4 * i + 2), q3 = code(x.w, 4 * i + 3);
        if (!out) continue;
        uint32_t* o = reinterpret_cast<uint32_t*>(out + i * (BITS / 2));
        if constexpr (BITS == 16) {
            o[0] = (q0 & 0xFFFFu) | (q1 << 16);
            o[1] = (q2 & 0xFFFFu) | (q3 << 16);
        } else if constexpr (BITS == 24) {
            o[0] = (q0 & 0xFFFFFFu) | (q1 << 24);
            o[1] = ((q1 >> 8) & 0xFFFFu) | (q2 << 16);
            o[2] = ((q2 >> 16) & 0xFFu) | (q3 << 8);
        } else {
            o[0] = q0; o[1] = q1; o[2] = q2; o[3] = q3;
        }
    }
    if (!stats) return;   // (uniform: a kernel argument)
    __shared__ rsmp::FirPcmStat waves[kThreads / 64];
    const rsmp::FirPcmStat w = rsmp::fir_stat_wave_sum(mine);
    if ((threadIdx.x & 63) == 0) waves[threadIdx.x >> 6] = w;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long values = 0, clipped = 0, nans = 0;
        uint32_t peak = 0;
        for (int j = 0; j < kThreads / 64; ++j) {
            values += waves[j].values;
            clipped += waves[j].clipped;
            nans += waves[j].nans;
            peak = waves[j].peak > peak ? waves[j].peak : peak;
        }
        if (values) (void)atomicAdd(reinterpret_cast<unsigned long long*>(&stats->values), values);
        if (clipped) (void)atomicAdd(reinterpret_cast<unsigned long long*>(&stats->clipped), clipped);
        if (nans) (void)atomicAdd(reinterpret_cast<unsigned long long*>(&stats->nans), nans);
        if (peak) (void)atomicMax(reinterpret_cast<uint32_t*>(&stats->peak), peak);
    }
}

bool pcm_gain_args_ok(int bits, float gain, int dither) {
    return (bits == 16 || bits == 24 || bits == 32) && rsmp::fir_pcm_gain_ok(gain) && (dither == RSMP_DITHER_NONE || dither == RSMP_DITHER_TPDF);
}

}  // namespace

// The definition under a gain, on the host (no device needed): bytes and, where asked for, what was done.
extern "C" int rsmp_f32_to_pcm_gain(const float* in, size_t n_values, int bits, float gain, int dither, uint64_t seed, uint64_t first_index, void* out_pcm,
                                    rsmp_pcm_stats* stats) {
    if (!pcm_gain_args_ok(bits, gain, dither) || (n_values != 0 && (!in || (!out_pcm && !stats))))
        return rsmp::fail(RSMP_ERR_INVALID_ARGUMENT, "rsmp_f32_to_pcm_gain: 16 / 24 / 32 bits, a finite gain with 2^-32 <= |gain| <= 2^32, RSMP_DITHER_NONE / RSMP_DITHER_TPDF, non-null input, and output or statistics");
    uint8_t* o = static_cast<uint8_t*>(out_pcm);
    const size_t bytes = static_cast<size_t>(bits) / 8;
    const float k = rsmp::fir_pcm_gain_scale(gain, static_cast<uint32_t>(bits));
    rsmp::FirPcmStat acc{0, 0, 0, 0};
    rsmp_pcm_stats t{};
    for (size_t i = 0; i < n_values; ++i) {
        rsmp::FirPcmStat one{0, 0, 0, acc.peak};
        const uint32_t q = static_cast<uint32_t>(dither == RSMP_DITHER_TPDF
                                                     ? rsmp::fir_pcm_quantise_gain_stat(in[i], k, static_cast<uint32_t>(bits), rsmp::fir_pcm_dither(seed, first_index + i), one)
                                                     : rsmp::fir_pcm_quantise_gain_stat(in[i], k, static_cast<uint32_t>(bits), 0.0f, one));
        t.values += one.values;
        t.clipped += one.clipped;
        t.nans += one.nans;
        acc.peak = one.peak;
        if (o)   // (null: measure only)
            for (size_t b = 0; b < bytes; ++b) o[i * bytes + b] = static_cast<uint8_t>(q >> (8 * b));   // little-endian
    }
    if (stats) {
        std::memcpy(&t.peak, &acc.peak, sizeof acc.peak);
        *stats = t;
    }
    return RSMP_OK;
}

extern "C" int rsmp_f32_to_pcm_gain_device(const float* d_in, size_t n_values, int bits, float gain, int dither, uint64_t seed, uint64_t first_index,
                                           void* d_pcm, rsmp_pcm_stats* d_stats, void* stream) {
    if (!pcm_gain_args_ok(bits, gain, dither) || (n_values != 0 && (!d_in || (!d_pcm && !d_stats))))
        return rsmp::fail(RSMP_ERR_INVALID_ARGUMENT, "rsmp_f32_to_pcm_gain_device: 16 / 24 / 32 bits, a finite gain with 2^-32 <= |gain| <= 2^32, RSMP_DITHER_NONE / RSMP_DITHER_TPDF, non-null buffers");
    if (reinterpret_cast<uintptr_t>(d_in) % 16 != 0 || reinterpret_cast<uintptr_t>(d_pcm) % 4 != 0 || reinterpret_cast<uintptr_t>(d_stats) % 8 != 0)
        return rsmp::fail(RSMP_ERR_INVALID_ARGUMENT, "rsmp_f32_to_pcm_gain_device: d_in 16-byte aligned, d_pcm 4-byte aligned, d_stats 8-byte aligned");
    if (int rc = check_device()) return rc;
    if (n_values == 0) return RSMP_OK;
    const dim3 grid = f32_to_pcm_grid(n_values);
    hipStream_t s = static_cast<hipStream_t>(stream);
    uint8_t* o = static_cast<uint8_t*>(d_pcm);
    const uint64_t n = n_values;
    const float k = rsmp::fir_pcm_gain_scale(gain, static_cast<uint32_t>(bits));
#define RSMP_GAIN_LAUNCH(BITS, TPDF) hipLaunchKernelGGL((f32_to_pcm_gain_kernel<BITS, TPDF>), grid, dim3(kThreads), 0, s, d_in, o, n, k, seed, first_index, d_stats, 0u)
    if (dither == RSMP_DITHER_TPDF) {
        if (bits == 16) RSMP_GAIN_LAUNCH(16, true);
        else if (bits == 24) RSMP_GAIN_LAUNCH(24, true);
        else RSMP_GAIN_LAUNCH(32, true);
    } else {
        if (bits == 16) RSMP_GAIN_LAUNCH(16, false);
        else if (bits == 24) RSMP_GAIN_LAUNCH(24, false);
        else RSMP_GAIN_LAUNCH(32, false);
    }
#undef RSMP_GAIN_LAUNCH
    RSMP_HIP_CHECK(hipGetLastError());
    return RSMP_OK;
}

// The same with a shape of the TPDF noise (fir_pcm_dither_shaped): the two-pass reference of rsmp_fir_set_pcm_dither_shape /
// rsmp_fft_set_pcm_dither_shape.  White, or no dither: rsmp_f32_to_pcm_gain itself.
extern "C" int rsmp_f32_to_pcm_shaped(const float* in, size_t n_values, int bits, float gain, int dither, int shape, uint32_t channels, uint64_t seed,
                                      uint64_t first_index, void* out_pcm, rsmp_pcm_stats* stats) {
    if (!pcm_gain_args_ok(bits, gain, dither) || (shape != RSMP_DITHER_SHAPE_WHITE && shape != RSMP_DITHER_SHAPE_HIGHPASS) || channels == 0 ||
        (n_values != 0 && (!in || (!out_pcm && !stats))))
        return rsmp::fail(RSMP_ERR_INVALID_ARGUMENT, "rsmp_f32_to_pcm_shaped: 16 / 24 / 32 bits, a finite gain with 2^-32 <= |gain| <= 2^32, RSMP_DITHER_NONE / RSMP_DITHER_TPDF, RSMP_DITHER_SHAPE_WHITE / RSMP_DITHER_SHAPE_HIGHPASS, channels >= 1, non-null input, and output or statistics");
    if (dither != RSMP_DITHER_TPDF || shape == RSMP_DITHER_SHAPE_WHITE) return rsmp_f32_to_pcm_gain(in, n_values, bits, gain, dither, seed, first_index, out_pcm, stats);
    uint8_t* o = static_cast<uint8_t*>(out_pcm);
    const size_t bytes = static_cast<size_t>(bits) / 8;
    const float k = rsmp::fir_pcm_gain_scale(gain, static_cast<uint32_t>(bits));
    rsmp::FirPcmStat acc{0, 0, 0, 0};
    rsmp_pcm_stats t{};
    for (size_t i = 0; i < n_values; ++i) {
        rsmp::FirPcmStat one{0, 0, 0, acc.peak};
        const uint32_t q = static_cast<uint32_t>(rsmp::fir_pcm_quantise_gain_stat(
            in[i], k, static_cast<uint32_t>(bits), rsmp::fir_pcm_dither_shaped(seed, first_index + i, static_cast<uint32_t>(shape), channels), one));
        t.values += one.values;
        t.clipped += one.clipped;
        t.nans += one.nans;
        acc.peak = one.peak;
        if (o)   // (null: measure only)
            for (size_t b = 0; b < bytes; ++b) o[i * bytes + b] = static_cast<uint8_t>(q >> (8 * b));   // little-endian
    }
    if (stats) {
        std::memcpy(&t.peak, &acc.peak, sizeof acc.peak);
        *stats = t;
    }
    return RSMP_OK;
}

extern "C" int rsmp_f32_to_pcm_shaped_device(const float* d_in, size_t n_values, int bits, float gain, int dither, int shape, uint32_t channels, uint64_t seed,
                                             uint64_t first_index, void* d_pcm, rsmp_pcm_stats* d_stats, void* stream) {
    if (!pcm_gain_args_ok(bits, gain, dither) || (shape != RSMP_DITHER_SHAPE_WHITE && shape != RSMP_DITHER_SHAPE_HIGHPASS) || channels == 0 ||
        (n_values != 0 && (!d_in || (!d_pcm && !d_stats))))
        return rsmp::fail(RSMP_ERR_INVALID_ARGUMENT, "rsmp_f32_to_pcm_shaped_device: 16 / 24 / 32 bits, a finite gain with 2^-32 <= |gain| <= 2^32, RSMP_DITHER_NONE / RSMP_DITHER_TPDF, RSMP_DITHER_SHAPE_WHITE / RSMP_DITHER_SHAPE_HIGHPASS, channels >= 1, non-null buffers");
    if (dither != RSMP_DITHER_TPDF || shape == RSMP_DITHER_SHAPE_WHITE)
        return rsmp_f32_to_pcm_gain_device(d_in, n_values, bits, gain, dither, seed, first_index, d_pcm, d_stats, stream);
    if (reinterpret_cast<uintptr_t>(d_in) % 16 != 0 || reinterpret_cast<uintptr_t>(d_pcm) % 4 != 0 || reinterpret_cast<uintptr_t>(d_stats) % 8 != 0)
        return rsmp::fail(RSMP_ERR_INVALID_ARGUMENT, "rsmp_f32_to_pcm_shaped_device: d_in 16-byte aligned, d_pcm 4-byte aligned, d_stats 8-byte aligned");
    if (int rc = check_device()) return rc;
    if (n_values == 0) return RSMP_OK;
    const dim3 grid = f32_to_pcm_grid(n_values);
    hipStream_t s = static_cast<hipStream_t>(stream);
    uint8_t* o = static_cast<uint8_t*>(d_pcm);
    const uint64_t n = n_values;
    const float k = rsmp::fir_pcm_gain_scale(gain, static_cast<uint32_t>(bits));
#define RSMP_SHAPED_LAUNCH(BITS) hipLaunchKernelGGL((f32_to_pcm_gain_kernel<BITS, true, true>), grid, dim3(kThreads), 0, s, d_in, o, n, k, seed, first_index, d_stats, channels)
    if (bits == 16) RSMP_SHAPED_LAUNCH(16);
    else if (bits == 24) RSMP_SHAPED_LAUNCH(24);
    else RSMP_SHAPED_LAUNCH(32);
#undef RSMP_SHAPED_LAUNCH
    RSMP_HIP_CHECK(hipGetLastError());
    return RSMP_OK;
}

// The gain a second pass needs to bring the first pass's peak to target_peak: f32(target_peak / peak).
extern "C" int rsmp_pcm_normalise_gain(const rsmp_pcm_stats* stats, float target_peak, float* gain) {
    if (!stats || !gain) return rsmp::fail(RSMP_ERR_INVALID_ARGUMENT, "rsmp_pcm_normalise_gain: null argument");
    const float peak = stats->peak;
    if (!(peak > 0.0f) || std::isinf(peak))
        return rsmp::fail(RSMP_ERR_INVALID_ARGUMENT, "rsmp_pcm_normalise_gain: the peak is zero or not finite: nothing to normalise by");
    const float g = target_peak / peak;
    if (!rsmp::fir_pcm_gain_ok(g))
        return rsmp::fail(RSMP_ERR_INVALID_ARGUMENT, "rsmp_pcm_normalise_gain: target_peak / peak is no gain the PCM entries accept (finite, 2^-32 <= |gain| <= 2^32)");
    *gain = g;
    return RSMP_OK;
}

// ---- measurement aid: the chip's streaming rate --------------------------------------------------------------
// A plain copy, 16 bytes per lane and instruction, four workgroups per compute unit walking the buffer side by side (the
// whole grid touches one contiguous stretch per iteration): what a kernel that reads as much as it writes can reach at
// all.  tools/copy_probe.hip swept the shape on the pool's MI355X (0.56 GB buffers): this one 5.83 TB/s of read +
// written bytes; eight workgroups per CU 4.9, four loads in flight per lane 4.2-4.4, non-temporal accesses 4.3-5.6 --
// the guide's figure is 6.29 TB/s.  bench.py prices every roofline fraction against the 8 TB/s spec AND reports this
// figure beside it (`roofline.device_copy`).
namespace {
typedef float v4f_copy __attribute__((ext_vector_type(4)));
__global__ __launch_bounds__(256) void stream_copy_kernel(const v4f_copy* __restrict__ src, v4f_copy* __restrict__ dst, uint64_t n16) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * 256u;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x; i < n16; i += stride) dst[i] = src[i];
}
}  // namespace

extern "C" int rsmp_device_stream_copy(const float* d_src, float* d_dst, size_t n_values, void* stream) {
    if (int rc = check_device()) return rc;
    if ((reinterpret_cast<uintptr_t>(d_src) | reinterpret_cast<uintptr_t>(d_dst)) % 16 != 0 || n_values % 4 != 0)
        return rsmp::fail(RSMP_ERR_INVALID_ARGUMENT, "rsmp_device_stream_copy: 16-byte aligned buffers of whole 16-byte pieces");
    if (n_values == 0) return RSMP_OK;
    int cus = 256;
    int device = 0;
    (void)hipGetDevice(&device);
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device);
    hipLaunchKernelGGL(stream_copy_kernel, dim3(static_cast<uint32_t>(cus) * 4u), dim3(256), 0, static_cast<hipStream_t>(stream),
                       reinterpret_cast<const v4f_copy*>(d_src), reinterpret_cast<v4f_copy*>(d_dst), static_cast<uint64_t>(n_values / 4));
    RSMP_HIP_CHECK(hipGetLastError());
    return RSMP_OK;
}
