// fir_periodic.hip -- throughput FIR kernels for rational rate pairs on gfx950 (see fir_periodic.h
// for the idea; DESIGN.md section 4.1 for the measurements).  They replace the same reference code
// as fir_generic.hip (src/resampler_fir.rs:542-590 + src/fir/avx.rs:5-61) for launches long enough
// to work in whole periods.  Two kernels share the staging, geometry and class-table code:
//
//   fir_periodic_db_kernel                matrix-core consumers (default for 2 channels): one
//       workgroup per CU owning two LDS images; producer waves stage with LDS-DMA,
//       consumer waves run v_mfma_f32_16x16x4_f32 streams over 16-class tiles (exact f32), the
//       coefficient tile in registers, samples from LDS, stores without any transpose; the wrap
//       variant is computed by a producer from the staged image;
//   fir_periodic_kernel                   vector kernel, two workgroups per CU alternating between
//       staging and computing: lane = period, the 8 coefficients of a tap wave-uniform through the
//       scalar cache into the SGPR operand of v_pk_fma_f32, 4x4 DPP transposes before the stores,
//       a 9th accumulator for the wrap variant.  Any channel count, any period length.
//
// HBM traffic = input span once per work item (+ row_len halo) + output once; the class table
// (<= a few hundred KB) stays in L2 / scalar cache.
#include "fir_periodic.h"

#include <hip/hip_ext.h>

#include <cstdio>
#include <cstdlib>

#include "common.h"
#include "fir_kernel_launch.h"
#include "fir_periodic_consts.h"

namespace rsmp {

namespace {

struct GeoArgs {
    uint32_t a, b, r, row_len, n_tiles, lp, pw, row_stride, waves, channels, xprev_len;
    uint32_t producers;   // double-buffered kernel: waves that only stage
    uint32_t den;         // true period of the phase pattern (b = r * den)
    uint32_t images;      // double-buffered kernel: LDS images in the ring (2 or 4)
    uint32_t unit_shift;  // matrix-core path: log2(work units per class tile)
    uint32_t inline_wraps;
    uint32_t debug;  // RSMP_FIR_DEBUG: bit0 skip staging, bit1 skip the tap loops (timing only)
    uint32_t stagger_ticks;  // one-time start delay of the second workgroup slot (100 MHz ticks)
    unsigned long long* trace;  // RSMP_FIR_TRACE diagnostic build only: 6 u64 per workgroup
    unsigned long long* wtrace; // RSMP_FIR_WTRACE: kWtraceSlots timestamped events per wave
    uint32_t blocks_per_stream, total_items;
    unsigned long long* work_counter;   // launch-wide item queue: zero between launches
    uint32_t n_claimers;                // waves that claim from it; each ends on exactly one failing claim
    NfArgs nf;                          // non-finite sums are marked here (fir_nonfinite.h)
};

constexpr uint32_t kWtraceSlots = 160, kWtraceWaves = 16;

// One ticket of the launch-wide item queue.  Every claimer stops at its first failing claim, so the
// launch's last ticket is total_items + n_claimers - 1: whoever draws it puts the counter back to zero.
// The queue is thereby self-contained per launch: nothing on the host predicts its value, and a launch
// that fails to start leaves it untouched.
__device__ __forceinline__ unsigned long long queue_claim(const GeoArgs& geo) {
    const unsigned long long t = atomicAdd(geo.work_counter, 1ull);
    if (t == static_cast<unsigned long long>(geo.total_items) + geo.n_claimers - 1ull) (void)atomicExch(geo.work_counter, 0ull);
    return t;
}

typedef const float __attribute__((address_space(4)))* const_f32_ptr;   // scalar-cache loads
typedef const float __attribute__((address_space(1)))* gconst_f32_ptr;  // global (not flat) loads
typedef float __attribute__((address_space(1)))* g_f32_ptr;
typedef const uint32_t __attribute__((address_space(1)))* gconst_u32_ptr;
typedef const uint32_t __attribute__((address_space(4)))* const_u32_ptr;
typedef float v2f __attribute__((ext_vector_type(2)));
typedef float v4f __attribute__((ext_vector_type(4)));

// Copies a wave-uniform, read-only POD through the scalar cache (s_load) into registers.
template <class T>
__device__ __forceinline__ T load_uniform(const T* p) {
    static_assert(sizeof(T) % 4 == 0, "dword-sized PODs only");
    T v;
    const_u32_ptr src = (const_u32_ptr)p;
    uint32_t* dst = reinterpret_cast<uint32_t*>(&v);
#pragma unroll
    for (size_t i = 0; i < sizeof(T) / 4; ++i) dst[i] = src[i];
    return v;
}

template <int CG> struct Acc {
    float v[kClassTile][CG];
    float w[CG];  // wrap variant of one column
};

template <int CG>
__device__ __forceinline__ void load_x(float (&xs)[CG], const float* p) {
    if constexpr (CG == 2) {
        const float2 t = *reinterpret_cast<const float2*>(p);
        xs[0] = t.x;
        xs[1] = t.y;
    } else {
        xs[0] = p[0];
    }
}

// `count` taps: sample(s) from LDS (stride `cstride` dwords per frame), 8 coefficients per tap
// (+1 for the wrap variant) from the class table through scalar loads.
template <int CG, bool WRAP>
__device__ __forceinline__ void accumulate(Acc<CG>& acc, const float* __restrict__ x,
                                           uint32_t cstride, const_f32_ptr g, const_f32_ptr gw,
                                           uint32_t count) {
    uint32_t m = 0;
    for (; m + 4 <= count; m += 4) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            float xs[CG];
            load_x<CG>(xs, x + (m + u) * cstride);
#pragma unroll
            for (int i = 0; i < (int)kClassTile; ++i) {
                const float c = g[(m + u) * kClassTile + i];
#pragma unroll
                for (int k = 0; k < CG; ++k) acc.v[i][k] = fmaf(c, xs[k], acc.v[i][k]);
            }
            if constexpr (WRAP) {
                const float c = gw[m + u];
#pragma unroll
                for (int k = 0; k < CG; ++k) acc.w[k] = fmaf(c, xs[k], acc.w[k]);
            }
        }
    }
    for (; m < count; ++m) {
        float xs[CG];
        load_x<CG>(xs, x + m * cstride);
#pragma unroll
        for (int i = 0; i < (int)kClassTile; ++i) {
            const float c = g[m * kClassTile + i];
#pragma unroll
            for (int k = 0; k < CG; ++k) acc.v[i][k] = fmaf(c, xs[k], acc.v[i][k]);
        }
        if constexpr (WRAP) {
            const float c = gw[m];
#pragma unroll
            for (int k = 0; k < CG; ++k) acc.w[k] = fmaf(c, xs[k], acc.w[k]);
        }
    }
}

__device__ __forceinline__ float dpp_quad_xor1(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xF, 0xF, true));
}
__device__ __forceinline__ float dpp_quad_xor2(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x4E, 0xF, 0xF, true));
}

// ---- fast path (2 channels, both per lane): packed-FMA chunks of 8 taps ---------------------------
typedef const v2f __attribute__((address_space(4)))* const_v2f_ptr;

// acc[2p] += c_p.lo * x, acc[2p+1] += c_p.hi * x for the four coefficient pairs of one tap: src0 is
// an SGPR pair whose low / high half is broadcast to both lanes of the packed FMA by op_sel.
__device__ __forceinline__ void pk_fma8(v2f (&acc)[8], v2f c0, v2f c1, v2f c2, v2f c3, v2f x) {
    asm("v_pk_fma_f32 %0, %8, %12, %0 op_sel_hi:[0,1,1]\n\t"
        "v_pk_fma_f32 %1, %8, %12, %1 op_sel:[1,0,0] op_sel_hi:[1,1,1]\n\t"
        "v_pk_fma_f32 %2, %9, %12, %2 op_sel_hi:[0,1,1]\n\t"
        "v_pk_fma_f32 %3, %9, %12, %3 op_sel:[1,0,0] op_sel_hi:[1,1,1]\n\t"
        "v_pk_fma_f32 %4, %10, %12, %4 op_sel_hi:[0,1,1]\n\t"
        "v_pk_fma_f32 %5, %10, %12, %5 op_sel:[1,0,0] op_sel_hi:[1,1,1]\n\t"
        "v_pk_fma_f32 %6, %11, %12, %6 op_sel_hi:[0,1,1]\n\t"
        "v_pk_fma_f32 %7, %11, %12, %7 op_sel:[1,0,0] op_sel_hi:[1,1,1]"
        : "+v"(acc[0]), "+v"(acc[1]), "+v"(acc[2]), "+v"(acc[3]), "+v"(acc[4]), "+v"(acc[5]),
          "+v"(acc[6]), "+v"(acc[7])
        : "s"(c0), "s"(c1), "s"(c2), "s"(c3), "v"(x));
}

// NT taps (8 or 4): 4*NT coefficient pairs (NT/2 x s_load_dwordx16) against NT frames.  One wait
// covers 8*NT packed FMAs; that is what lets a handful of waves per SIMD hide the scalar-cache miss
// latency (each line of the table is touched by one wave only).  NT = 8 needs 64 SGPRs for the
// coefficients (12-wave workgroups, 6 waves per SIMD); NT = 4 halves that and leaves room for
// 16-wave workgroups at 8 waves per SIMD.
template <bool WRAP, int NT>
__device__ __forceinline__ void taps(v2f (&acc)[8], v2f& accw, const v2f (&x)[NT],
                                     const_v2f_ptr gc, const_f32_ptr gwc) {
    v2f c[4 * NT];
#pragma unroll
    for (int i = 0; i < 4 * NT; ++i) c[i] = gc[i];
#pragma unroll
    for (int u = 0; u < NT; ++u) {
        pk_fma8(acc, c[4 * u], c[4 * u + 1], c[4 * u + 2], c[4 * u + 3], x[u]);
        if constexpr (WRAP) {
            const float w = gwc[u];
            accw.x = fmaf(w, x[u].x, accw.x);
            accw.y = fmaf(w, x[u].y, accw.y);
        }
    }
}

template <bool WRAP, int NT>
__device__ __forceinline__ void tile_taps_c2(v2f (&acc)[8], v2f& accw, const float* rowA,
                                             const float* rowB, uint32_t n1, uint32_t row_len,
                                             const_f32_ptr g, const_f32_ptr gw) {
    const uint32_t n_chunks = row_len / NT;
    const uint32_t chunks_a = n1 / NT;          // chunks entirely inside the lane's own row
    const_v2f_ptr gc = (const_v2f_ptr)g;
    uint32_t c = 0;
    for (; c < chunks_a; ++c) {
        v2f x[NT];
#pragma unroll
        for (int u = 0; u < NT; ++u) x[u] = *reinterpret_cast<const v2f*>(rowA + 2 * NT * c + 2 * u);
        taps<WRAP, NT>(acc, accw, x, gc + 4 * NT * c, gw + NT * c);
    }
    if (c < n_chunks && (n1 % NT)) {            // the chunk that straddles the two rows
        v2f x[NT];
#pragma unroll
        for (int u = 0; u < NT; ++u) {
            const uint32_t m = NT * c + u;
            const float* px = m < n1 ? rowA + 2 * m : rowB + 2 * (m - n1);
            x[u] = *reinterpret_cast<const v2f*>(px);
        }
        taps<WRAP, NT>(acc, accw, x, gc + 4 * NT * c, gw + NT * c);
        ++c;
    }
    for (; c < n_chunks; ++c) {
        const float* pb = rowB + 2 * (NT * c - n1);
        v2f x[NT];
#pragma unroll
        for (int u = 0; u < NT; ++u) x[u] = *reinterpret_cast<const v2f*>(pb + 2 * u);
        taps<WRAP, NT>(acc, accw, x, gc + 4 * NT * c, gw + NT * c);
    }
}

// ---- one channel per lane (CG == 1): packed FMAs over class pairs ------------------------------------
// acc[p] = (class 2p, class 2p + 1) += (c[2p], c[2p + 1]) * x for the four class pairs of two consecutive taps:
// src0 is the SGPR pair of the two coefficients, src1 a VGPR pair holding the two taps' samples, of which
// op_sel broadcasts the low (first tap) or the high one (second tap) to both halves.  Half the vector
// instructions of one v_fma_f32 per class and tap; every class still accumulates its taps in order.
__device__ __forceinline__ void pk_fma8_c1(v2f (&acc)[4], v2f c0, v2f c1, v2f c2, v2f c3, v2f d0, v2f d1, v2f d2, v2f d3, v2f x) {
    asm("v_pk_fma_f32 %0, %4, %12, %0 op_sel_hi:[1,0,1]\n\t"
        "v_pk_fma_f32 %1, %5, %12, %1 op_sel_hi:[1,0,1]\n\t"
        "v_pk_fma_f32 %2, %6, %12, %2 op_sel_hi:[1,0,1]\n\t"
        "v_pk_fma_f32 %3, %7, %12, %3 op_sel_hi:[1,0,1]\n\t"
        "v_pk_fma_f32 %0, %8, %12, %0 op_sel:[0,1,0] op_sel_hi:[1,1,1]\n\t"
        "v_pk_fma_f32 %1, %9, %12, %1 op_sel:[0,1,0] op_sel_hi:[1,1,1]\n\t"
        "v_pk_fma_f32 %2, %10, %12, %2 op_sel:[0,1,0] op_sel_hi:[1,1,1]\n\t"
        "v_pk_fma_f32 %3, %11, %12, %3 op_sel:[0,1,0] op_sel_hi:[1,1,1]"
        : "+v"(acc[0]), "+v"(acc[1]), "+v"(acc[2]), "+v"(acc[3])
        : "s"(c0), "s"(c1), "s"(c2), "s"(c3), "s"(d0), "s"(d1), "s"(d2), "s"(d3), "v"(x));
}

template <bool WRAP, int NT>
__device__ __forceinline__ void taps_c1(v2f (&acc)[4], float& accw, const float (&x)[NT], const_v2f_ptr gc, const_f32_ptr gwc) {
    static_assert(NT % 2 == 0, "taps go in pairs");
    v2f c[4 * NT];
#pragma unroll
    for (int i = 0; i < 4 * NT; ++i) c[i] = gc[i];
#pragma unroll
    for (int u = 0; u < NT; u += 2) {
        pk_fma8_c1(acc, c[4 * u], c[4 * u + 1], c[4 * u + 2], c[4 * u + 3], c[4 * u + 4], c[4 * u + 5], c[4 * u + 6], c[4 * u + 7],
                   v2f{x[u], x[u + 1]});
        if constexpr (WRAP) {
            accw = fmaf(gwc[u], x[u], accw);
            accw = fmaf(gwc[u + 1], x[u + 1], accw);
        }
    }
}

// rowA / rowB: the lane's channel in its own period row (from the tile's window start) and in the next row;
// `cs` dwords between frames
template <bool WRAP, int NT>
__device__ __forceinline__ void tile_taps_c1(v2f (&acc)[4], float& accw, const float* rowA, const float* rowB, uint32_t cs,
                                             uint32_t n1, uint32_t row_len, const_f32_ptr g, const_f32_ptr gw) {
    const uint32_t n_chunks = row_len / NT;
    const uint32_t chunks_a = n1 / NT;          // chunks entirely inside the lane's own row
    const_v2f_ptr gc = (const_v2f_ptr)g;
    uint32_t c = 0;
    for (; c < chunks_a; ++c) {
        float x[NT];
#pragma unroll
        for (int u = 0; u < NT; ++u) x[u] = rowA[(NT * c + u) * cs];
        taps_c1<WRAP, NT>(acc, accw, x, gc + 4 * NT * c, gw + NT * c);
    }
    if (c < n_chunks && (n1 % NT)) {            // the chunk that straddles the two rows
        float x[NT];
#pragma unroll
        for (int u = 0; u < NT; ++u) {
            const uint32_t m = NT * c + u;
            x[u] = m < n1 ? rowA[m * cs] : rowB[(m - n1) * cs];
        }
        taps_c1<WRAP, NT>(acc, accw, x, gc + 4 * NT * c, gw + NT * c);
        ++c;
    }
    for (; c < n_chunks; ++c) {
        const float* pb = rowB + (NT * c - n1) * cs;
        float x[NT];
#pragma unroll
        for (int u = 0; u < NT; ++u) x[u] = pb[u * cs];
        taps_c1<WRAP, NT>(acc, accw, x, gc + 4 * NT * c, gw + NT * c);
    }
}

// Up to 768 threads = 12 waves (3 per SIMD); two workgroups per CU -> 6 waves per SIMD -> at
// most 80 VGPRs.
// C2 = true: exactly two channels, both handled by one lane (CG == 2) -- the headline config.
// Per-item state of a wave: what a class tile needs beyond its own index.
struct ItemCtx {
    const_f32_ptr table, wtable;      // class table, wrap rows
    const TileMeta* metas;
    gconst_u32_ptr wrap_bits;
    g_f32_ptr out;
    int32_t n_block0;                 // launch-relative output index of (period q0, class 0)
    int32_t k_block0;                 // wrap-bitmap index of (period q0, class 0)
    int32_t n_limit;                  // outputs in this launch
    const float* lane_row;            // LDS: first sample of the lane's period row (+ channel group)
    const float* xprev;               // LDS: frame in front of each period
    uint32_t wrap_tag;                // matrix-core path: image index | (item sequence + 1) << 2
    uint32_t stream;                  // the stream's index in the launch (non-finite marks)
    uint32_t pl_c, gi, lane;
    bool lane_on;
};

struct ItemGeom {                     // wave-uniform placement of a work item
    uint64_t q0;
    int32_t n_block0, k_block0;
    bool valid;
};

__device__ __forceinline__ ItemGeom item_geom(const GeoArgs& geo, const FirStreamDesc& d,
                                              uint32_t block_idx) {
    ItemGeom ig;
    const uint64_t q_first = d.abs_out / geo.b;
    ig.q0 = q_first + static_cast<uint64_t>(block_idx) * geo.pw;
    ig.valid = d.n_out != 0 && ig.q0 * geo.b < d.abs_out + d.n_out;
    // launch-relative index of output (period q0, class 0); fits int32 (n_out < 2^31)
    ig.n_block0 = static_cast<int32_t>(static_cast<int64_t>(ig.q0 * geo.b) -
                                       static_cast<int64_t>(d.abs_out));
    // bit index of (period q0, class 0) in the wrap bitmap
    ig.k_block0 = static_cast<int32_t>(static_cast<int64_t>(ig.q0 * geo.r) -
                                       static_cast<int64_t>(d.wrap_k0));
    return ig;
}

template <int CG, bool C2>
__device__ __forceinline__ ItemCtx item_ctx(const GeoArgs& geo, const FirStreamDesc& d,
                                            const ItemGeom& ig, const float* rows, const float* xprev,
                                            uint32_t lane, uint32_t stream_idx) {
    ItemCtx cx;
    cx.stream = stream_idx;
    const uint32_t pl = C2 ? lane : lane / geo.lp;     // period of this lane inside the block
    cx.gi = C2 ? 0u : lane - pl * geo.lp;              // channel group of this lane
    cx.lane_on = pl < geo.pw;
    cx.pl_c = cx.lane_on ? pl : 0;                     // idle lanes shadow lane 0 (no stores)
    cx.lane = lane;
    cx.lane_row = rows + cx.pl_c * geo.row_stride + cx.gi * CG;
    cx.xprev = xprev;
    cx.wrap_tag = 0;
    cx.table = (const_f32_ptr)(d.class_coef);
    cx.wtable = (const_f32_ptr)(d.class_wrap_coef);
    cx.metas = static_cast<const TileMeta*>(d.class_meta);
    cx.wrap_bits = (gconst_u32_ptr)d.wrap_bits;
    cx.out = (g_f32_ptr)d.out;
    cx.n_block0 = ig.n_block0;
    cx.k_block0 = ig.k_block0;
    cx.n_limit = static_cast<int32_t>(d.n_out);
    return cx;
}

// ---- stage -----------------------------------------------------------------------------------------
// LDS-DMA (global_load_lds, 4 B per lane): the rows region is filled 256 B per wave instruction
// straight from [hist|in] with no VGPR round trip.  Wave `part` of `parts` takes every parts-th
// 64-dword piece.  Source addresses are clamped into the stream; the wave then zeroes the
// out-of-stream dwords of its own pieces (after they have landed), so stagers never wait for one
// another.  Returns with the wave's DMA possibly still in flight unless the span touches a stream
// edge; the caller waits (vmcnt) before publishing the image.
__device__ __forceinline__ void stage_image(const GeoArgs& geo, const FirStreamDesc& d, uint64_t q0,
                                            uint32_t C, float* rows, float* xprev, uint32_t part,
                                            uint32_t parts, uint32_t lane) {
    const int64_t hist_values = static_cast<int64_t>(d.hist_frames) * C;
    const int64_t total_values = hist_values + static_cast<int64_t>(d.in_frames) * C;  // > 0
    gconst_f32_ptr hist = (gconst_f32_ptr)d.hist;
    gconst_f32_ptr in = (gconst_f32_ptr)d.in;
    // virtual value index of the span's first sample: absolute frame q0*a minus the frames
    // retired before this launch, times C
    const int64_t w_span = (static_cast<int64_t>(q0 * geo.a) - static_cast<int64_t>(d.abs_consumed)) * C;
    const uint32_t row_values = geo.a * C;
    const bool flat = geo.row_stride == row_values;   // odd a: rows are back to back
    const uint32_t region = (geo.pw + 1) * geo.row_stride;
    // virtual value index feeding LDS dword L of the rows region (pad dwords of even-a rows
    // re-read the next row's first frame; they are never used)
    auto w_of = [&](uint32_t L) -> int64_t {
        if (flat) return w_span + L;
        const uint32_t p = L / geo.row_stride;
        return w_span + static_cast<int64_t>(p) * row_values + (L - p * geo.row_stride);
    };
    auto src_of = [&](int64_t w) -> gconst_f32_ptr {
        const int64_t wc = w < 0 ? 0 : (w >= total_values ? total_values - 1 : w);
        return wc < hist_values ? hist + wc : in + (wc - hist_values);
    };
    typedef __attribute__((address_space(3))) void* lds_void_ptr;
    const int64_t span_values = static_cast<int64_t>(geo.pw + 1) * row_values;
    const bool edge = w_span < 0 || w_span + span_values > total_values;
    if (flat && w_span >= hist_values && !edge) {
        // interior item: the span is one contiguous piece of `in`.  16 bytes per lane: 1 KB per wave
        // instruction, a quarter of the instructions (the vector memory pipe is shared with the
        // consumers' loads and stores).  The last, partial piece goes dword-wise.
        const uint32_t whole = region & ~255u;
        gconst_f32_ptr src = in + (w_span - hist_values);
        for (uint32_t base = part * 256; base < whole; base += parts * 256)
            __builtin_amdgcn_global_load_lds(src + base + lane * 4, (lds_void_ptr)(rows + base), 16, 0, 0);
        for (uint32_t base = whole + part * 64; base < region; base += parts * 64)
            if (base + lane < region)
                __builtin_amdgcn_global_load_lds(src + base + lane, (lds_void_ptr)(rows + base), 4, 0, 0);
    } else {
        for (uint32_t base = part * 64; base < region; base += parts * 64) {
            const uint32_t L = base + lane;
            if (L < region)
                __builtin_amdgcn_global_load_lds(src_of(w_of(L)), (lds_void_ptr)(rows + base), 4, 0, 0);
        }
    }
    for (uint32_t e = part * 64 + lane; e < geo.pw * C; e += parts * 64) {
        const uint32_t p = C == 1 ? e : e / C;
        const int64_t w = w_span + static_cast<int64_t>(p) * row_values - C + (e - p * C);
        float val = *src_of(w);
        if (w < 0 || w >= total_values) val = 0.f;
        xprev[e] = val;
    }
    if (edge) {   // wave-uniform
        __builtin_amdgcn_s_waitcnt(0);   // own DMA pieces have landed
        for (uint32_t base = part * 64; base < region; base += parts * 64) {
            const uint32_t L = base + lane;
            if (L < region) {
                const int64_t w = w_of(L);
                if (w < 0 || w >= total_values) rows[L] = 0.f;
            }
        }
    }
}

// ---- one class tile: taps, wrap pick, transposed stores -----------------------------------------
template <int CG, bool C2, int NT>
__device__ __forceinline__ void process_tile(const GeoArgs& geo, const ItemCtx& cx, uint32_t t,
                                             const TileMeta& tm) {
    const uint32_t C = C2 ? 2u : geo.channels;
    const uint32_t j0 = t * kClassTile;
    const uint32_t ob = tm.base;
    const_f32_ptr g = cx.table + static_cast<size_t>((geo.debug & 32) ? 0 : t) * geo.row_len * kClassTile;
    const_f32_ptr gw = cx.wtable + static_cast<size_t>(t) * geo.row_len;
    const bool has_wrap = geo.inline_wraps && tm.wrap_col >= 0;
    // window [ob, ob+row_len) of the lane's period row, spilling into the next row
    const uint32_t n1 = geo.a - ob < geo.row_len ? geo.a - ob : geo.row_len;
    const int32_t n_lane0 = cx.n_block0 + static_cast<int32_t>(cx.pl_c * geo.b + j0);  // class j0
    const int32_t n_limit = cx.n_limit;
    const float* lane_row = cx.lane_row;

    float av[kClassTile][CG];
    float aw[CG];
    if constexpr (C2) {
        v2f acc[8], accw = {0.f, 0.f};
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] = v2f{0.f, 0.f};
        if (!(geo.debug & 2)) {
            if (has_wrap)
                tile_taps_c2<true, NT>(acc, accw, lane_row + ob * 2, lane_row + geo.row_stride, n1,
                                       geo.row_len, g, gw);
            else
                tile_taps_c2<false, NT>(acc, accw, lane_row + ob * 2, lane_row + geo.row_stride, n1,
                                        geo.row_len, g, gw);
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) { av[i][0] = acc[i].x; av[i][1] = acc[i].y; }
        aw[0] = accw.x;
        aw[1] = accw.y;
    } else if constexpr (CG == 1) {
        v2f acc[4];
        float accw = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i] = v2f{0.f, 0.f};
        if (!(geo.debug & 2)) {
            if (has_wrap)
                tile_taps_c1<true, NT>(acc, accw, lane_row + ob * C, lane_row + geo.row_stride, C, n1, geo.row_len, g, gw);
            else
                tile_taps_c1<false, NT>(acc, accw, lane_row + ob * C, lane_row + geo.row_stride, C, n1, geo.row_len, g, gw);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) { av[2 * i][0] = acc[i].x; av[2 * i + 1][0] = acc[i].y; }
        aw[0] = accw;
    } else {
        Acc<CG> acc;
#pragma unroll
        for (int i = 0; i < (int)kClassTile; ++i)
#pragma unroll
            for (int k = 0; k < CG; ++k) acc.v[i][k] = 0.f;
#pragma unroll
        for (int k = 0; k < CG; ++k) acc.w[k] = 0.f;
        if (!(geo.debug & 2)) {
            if (has_wrap) {
                accumulate<CG, true>(acc, lane_row + ob * C, C, g, gw, n1);
                if (n1 < geo.row_len)
                    accumulate<CG, true>(acc, lane_row + geo.row_stride, C, g + n1 * kClassTile,
                                         gw + n1, geo.row_len - n1);
            } else {
                accumulate<CG, false>(acc, lane_row + ob * C, C, g, gw, n1);
                if (n1 < geo.row_len)
                    accumulate<CG, false>(acc, lane_row + geo.row_stride, C, g + n1 * kClassTile,
                                          gw + n1, geo.row_len - n1);
            }
        }
#pragma unroll
        for (int i = 0; i < (int)kClassTile; ++i)
#pragma unroll
            for (int k = 0; k < CG; ++k) av[i][k] = acc.v[i][k];
#pragma unroll
        for (int k = 0; k < CG; ++k) aw[k] = acc.w[k];
    }

    if (has_wrap) {
        if (tm.extra_col != -2) {
            float xs[CG];
            load_x<CG>(xs, tm.extra_col >= 0 ? lane_row + tm.extra_col * C
                                             : cx.xprev + cx.pl_c * C + cx.gi * CG);
#pragma unroll
            for (int k = 0; k < CG; ++k) aw[k] = fmaf(tm.extra_coef, xs[k], aw[k]);
        }
        const int32_t nw = n_lane0 + tm.wrap_col;
        bool take = false;
        if (nw >= 0 && nw < n_limit) {
            const uint32_t K = static_cast<uint32_t>(cx.k_block0 + static_cast<int32_t>(cx.pl_c * geo.r + tm.wrap_jd));
            take = (cx.wrap_bits[K >> 5] >> (K & 31)) & 1u;
        }
#pragma unroll
        for (int i = 0; i < (int)kClassTile; ++i)
            if (i == tm.wrap_col && take) {
#pragma unroll
                for (int k = 0; k < CG; ++k) av[i][k] = aw[k];
            }
    }

    // ---- non-finite sums: the chunk is redone in the reference's form by the repair launch ---------
    {
        float chk = 0.f;   // every frame and channel the lane stores (inf - inf = NaN: still not finite)
#pragma unroll
        for (int i = 0; i < (int)kClassTile; ++i)
#pragma unroll
            for (int k = 0; k < CG; ++k) chk += av[i][k];
        nf_mark(geo.nf, cx.lane_on && nf_is_bad(chk), cx.stream, n_lane0, static_cast<int32_t>(kClassTile), n_limit);
    }
    // ---- store -------------------------------------------------------------------------------
    g_f32_ptr out = cx.out;
    const uint32_t lane = cx.lane;
    bool done = false;
    if (geo.debug & 16) {   // timing only: keep the sums alive with one conditional store
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < (int)kClassTile; ++i)
#pragma unroll
            for (int k = 0; k < CG; ++k) s += av[i][k];
        if (s == 12345.678f) out[0] = s;
        done = true;
    }
    if constexpr (C2) {
        // Quad transpose: lane r of a quad ends up with quarter r (2 frames = 16 B) of the four
        // periods of the quad; store s then covers period quad_base + s contiguously.
        const bool full_tile = j0 + kClassTile <= geo.b;
        const bool mine_full = n_lane0 >= 0 && n_lane0 + (int32_t)kClassTile <= n_limit;
        const bool mine_none = n_lane0 >= n_limit || n_lane0 + (int32_t)kClassTile <= 0 || !cx.lane_on;
        const bool partial = !(mine_full || mine_none);
        if (!done && full_tile && !__any(partial)) {
            v4f B[4];
#pragma unroll
            for (int k = 0; k < 4; ++k)
                B[k] = v4f{av[2 * k][0], av[2 * k][1], av[2 * k + 1][0], av[2 * k + 1][1]};
            const bool odd = lane & 1, hi = lane & 2;
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                const v4f s = odd ? B[2 * p] : B[2 * p + 1];
                const v4f r4 = v4f{dpp_quad_xor1(s.x), dpp_quad_xor1(s.y), dpp_quad_xor1(s.z),
                                   dpp_quad_xor1(s.w)};
                if (odd) B[2 * p] = r4; else B[2 * p + 1] = r4;
            }
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const v4f s = hi ? B[k] : B[k + 2];
                const v4f r4 = v4f{dpp_quad_xor2(s.x), dpp_quad_xor2(s.y), dpp_quad_xor2(s.z),
                                   dpp_quad_xor2(s.w)};
                if (hi) B[k] = r4; else B[k + 2] = r4;
            }
            const uint32_t quad_base = lane & ~3u, r = lane & 3u;
            const int32_t n_quad0 = cx.n_block0 + static_cast<int32_t>(quad_base * geo.b + j0);
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const int32_t ns = n_quad0 + s * static_cast<int32_t>(geo.b);
                if (quad_base + s < geo.pw && ns >= 0 && ns + (int32_t)kClassTile <= n_limit) {
                    typedef v4f __attribute__((address_space(1), aligned(8)))* g_f4a8_ptr;
                    *((g_f4a8_ptr)(out + static_cast<size_t>(ns) * 2 + r * 4)) = B[s];
                }
            }
            done = true;
        }
    }
    if (!done && cx.lane_on) {
#pragma unroll
        for (int i = 0; i < (int)kClassTile; ++i) {
            const int32_t n = n_lane0 + i;
            if (j0 + i < geo.b && n >= 0 && n < n_limit) {
                g_f32_ptr o = out + static_cast<size_t>(n) * C + cx.gi * CG;
                if constexpr (CG == 2) {
                    typedef v2f __attribute__((address_space(1)))* g_f2_ptr;
                    *((g_f2_ptr)o) = v2f{av[i][0], av[i][1]};
                } else {
                    o[0] = av[i][0];
                }
            }
        }
    }
}

// Diagnostic per-wave event log (RSMP_FIR_WTRACE): (100 MHz timestamp << 8) | tag.
struct WaveTrace {
    unsigned long long* base;
    uint32_t cursor;
    __device__ __forceinline__ void init(const GeoArgs& geo, uint32_t wave) {
        base = (geo.wtrace && wave < kWtraceWaves)
                   ? geo.wtrace + (static_cast<size_t>(blockIdx.x) * kWtraceWaves + wave) * kWtraceSlots
                   : nullptr;
        cursor = 0;
    }
    __device__ __forceinline__ void event(uint32_t tag) {
        if (base && cursor < kWtraceSlots) {
            const unsigned long long v = (__builtin_amdgcn_s_memrealtime() << 8) | tag;
            if ((threadIdx.x & 63) == 0) base[cursor] = v;
            ++cursor;
        }
    }
};

// ---- single-image kernel ---------------------------------------------------------------------------
// One staged image per workgroup, barriers between stage and compute; two workgroups per CU overlap
// each other's phases.  Used when two images do not fit the 160 KB of LDS (long periods) -- the
// double-buffered kernel below is the fast path.
// DIAG (here and in fir_periodic_db_kernel): the diagnostic instantiation honours RSMP_FIR_DEBUG (timing
// experiments that switch parts of the kernel off) and the RSMP_FIR_TRACE / RSMP_FIR_WTRACE clocks; the
// shipping instantiation sees them as constant zero / null and carries none of that code.
template <int CG, bool C2, int NT, bool DIAG>
__global__ __launch_bounds__(768, 6) void fir_periodic_kernel(const FirStreamDesc* __restrict__ descs,
                                                              GeoArgs geo_arg) {
    GeoArgs geo = geo_arg;
    if constexpr (!DIAG) {
        geo.debug = 0;
        geo.trace = nullptr;
        geo.wtrace = nullptr;
    }
    extern __shared__ __attribute__((aligned(16))) float lds[];
    // Persistent workgroups: the grid is two workgroups per CU and each walks the launch's work
    // items (stream, period block).  A fresh dispatch per block cost ~10 us of empty LDS slot
    // between workgroups (measured with RSMP_FIR_TRACE) -- a third of each slot's time.
    unsigned long long t_trace[4] = {0, 0, 0, 0};
    if (geo.trace) t_trace[0] = __builtin_amdgcn_s_memrealtime();
    if (geo.stagger_ticks && blockIdx.x >= gridDim.x / 2) {
        const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
        while (__builtin_amdgcn_s_memrealtime() - t0 < geo.stagger_ticks) __builtin_amdgcn_s_sleep(16);
    }

    const uint32_t C = C2 ? 2u : geo.channels;
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    WaveTrace wt;
    wt.init(geo, wave);
    uint32_t* tile_counter = reinterpret_cast<uint32_t*>(lds);   // next unclaimed class tile
    float* __restrict__ xprev = lds + 4;               // [pw][C]: the frame in front of each period
    float* __restrict__ rows = lds + geo.xprev_len;    // [pw + 1][row_stride]

    // Work items are claimed from a launch-wide queue (one 64-bit counter that only ever grows; the
    // host passes the value it had before this launch).  Static striding left the younger of the
    // two workgroups of a CU -- which loses VALU arbitration to the older one -- with a third of
    // its items still to do after its neighbour had finished.  The claim for the next item is made
    // while the current one is being staged, so it is never on the critical path.
    uint32_t* next_item = reinterpret_cast<uint32_t*>(lds) + 1;
    auto claim = [&]() -> uint32_t {
        const unsigned long long t = queue_claim(geo);
        return t < geo.total_items ? static_cast<uint32_t>(t) : 0xFFFFFFFFu;
    };
    if (threadIdx.x == 0) *next_item = claim();
    __syncthreads();
    uint32_t item = *next_item;
    while (item != 0xFFFFFFFFu) {
        const uint32_t stream_idx = item / geo.blocks_per_stream;
        const uint32_t block_idx = item - stream_idx * geo.blocks_per_stream;
        // The descriptor is wave-uniform and read-only: fetch it through the scalar cache.
        const FirStreamDesc d = load_uniform(descs + stream_idx);
        const ItemGeom ig = item_geom(geo, d, block_idx);
        wt.event(1);          // item begins (waiting for the other waves)
        __syncthreads();      // every wave has read `item` and is done with the previous LDS image
        wt.event(2);
        if (threadIdx.x == 0) *next_item = claim();
        if (!ig.valid) {      // padding item of a ragged batch
            __syncthreads();
            item = *next_item;
            continue;
        }
        if (!(geo.debug & 1)) stage_image(geo, d, ig.q0, C, rows, xprev, wave, geo.waves, lane);
        if (threadIdx.x == 0) *tile_counter = 0;
        wt.event(3);          // staging issued
        __builtin_amdgcn_s_waitcnt(0);   // vmcnt(0): LDS-DMA is tracked by vmcnt
        wt.event(4);          // own pieces landed
        __syncthreads();
        wt.event(5);          // everyone's pieces landed
        if (geo.trace) t_trace[1] = __builtin_amdgcn_s_memrealtime();

        const ItemCtx cx = item_ctx<CG, C2>(geo, d, ig, rows, xprev, lane, stream_idx);
        // Class tiles are claimed dynamically: a workgroup's waves are spread unevenly over the
        // four SIMDs (and share them with the other resident workgroup), so a static split leaves
        // the least loaded SIMD idle while the most loaded one finishes.  The claim of the next
        // tile (an LDS atomic) and the fetch of its descriptor are issued while the current tile
        // computes, so a tile switch exposes neither latency.
        uint32_t t_claim = 0;
        if (lane == 0) t_claim = atomicAdd(tile_counter, 1u);
        uint32_t t = __builtin_amdgcn_readfirstlane(t_claim);
        TileMeta tm_cur = load_uniform(cx.metas + (t < geo.n_tiles ? t : 0));
        while (t < geo.n_tiles) {
            wt.event(6);      // tile begins
            if (lane == 0) t_claim = atomicAdd(tile_counter, 1u);   // next tile, consumed below
            process_tile<CG, C2, NT>(geo, cx, t, tm_cur);
            wt.event(7);      // tile done (stores issued)
            t = __builtin_amdgcn_readfirstlane(t_claim);
            tm_cur = load_uniform(cx.metas + (t < geo.n_tiles ? t : 0));
        }
        item = *next_item;   // written before the barrier that preceded the tile loop
    }   // items
    if (geo.trace) {
        t_trace[2] = __builtin_amdgcn_s_memrealtime();
        __builtin_amdgcn_s_waitcnt(0);   // stores acknowledged
        t_trace[3] = __builtin_amdgcn_s_memrealtime();
        if (threadIdx.x == 0) {
            unsigned long long* rec = geo.trace + 6ull * blockIdx.x;
            unsigned hw_id, xcc;
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw_id));
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
            rec[0] = t_trace[0]; rec[1] = t_trace[1]; rec[2] = t_trace[2]; rec[3] = t_trace[3];
            rec[4] = hw_id; rec[5] = xcc;
        }
    }
}

// ---- matrix-core work unit -----------------------------------------------------------------------
// The polyphase sum of one 16-class tile over 16 periods of one channel is a 16 x K x 16 product
// (classes x window taps x periods): D = A * B with A[class][tap] the tile's shifted, zero-padded,
// phase-mixed coefficients and B[tap][period] the period rows in LDS.  v_mfma_f32_16x16x4_f32 does
// 1024 exact f32 FMAs (bitwise an fmaf chain over the 4 taps) in 32 SIMD cycles -- the packed-FMA
// peak, but issued by ONE instruction instead of eight, with operands from VGPRs instead of the
// scalar cache, so two waves per SIMD keep the pipe full where the vector kernel needs six and still
// stalls.  Operand layout of the instruction (lane l): A = coef[class l % 16][tap 4c + l / 16],
// B = x[tap 4c + l / 16][period l % 16], D = 4 registers = classes 4 * (l / 16) + 0..3 of period
// l % 16 -- four consecutive output frames, i.e. with both channels 32 contiguous bytes per lane and
// 128 per period: the stores need no transpose.
//   A: the class table is stored in operand order [tile][step][lane] -> one coalesced 256-byte
//      global load per step, L2 resident (92 KB), prefetched 4-8 steps ahead;
//   B: one ds_read_b64 (both channels of a frame) per 16-period group and step feeds two MFMAs.
// A work unit = one tile x G groups of 16 periods (G = 2: 20 units per 160-class item).
// Wrapped outputs (exact position an integer, f64 position just below) are left to
// fir_wrap_fixup_kernel, as for every geometry without the inline wrap variant.
typedef __attribute__((address_space(1))) const float* gptr_f32;

// ---- store of a matrix-core unit: lane = (period, 4 consecutive classes), both channels -> 32
// contiguous bytes per lane, 128 per period: no transpose ------------------------------------------
template <int G>
__device__ __forceinline__ void mfma_store_unit(const GeoArgs& geo, const ItemCtx& cx,
                                                const v4f (&acc)[G][2], const bool (&p_on)[G],
                                                const uint32_t (&p_idx)[G], uint32_t j0) {
    g_f32_ptr out = cx.out;
    if (geo.debug & 16) {
        float s = 0.f;
#pragma unroll
        for (int g = 0; g < G; ++g) s += acc[g][0].x + acc[g][1].y + acc[g][0].z + acc[g][1].w;
        if (s == 12345.678f) out[0] = s;
        return;
    }
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const v4f s0 = acc[g][0], s1 = acc[g][1];
        nf_mark(geo.nf, p_on[g] && nf_is_bad(nf_sum8(s0, s1)), cx.stream,
                cx.n_block0 + static_cast<int32_t>(p_idx[g] * geo.b + j0), 4, cx.n_limit);
    }
#pragma unroll
    for (int g = 0; g < G; ++g) {
        if (!p_on[g]) continue;
        const int32_t n0 = cx.n_block0 + static_cast<int32_t>(p_idx[g] * geo.b + j0);
        const v4f lo = v4f{acc[g][0].x, acc[g][1].x, acc[g][0].y, acc[g][1].y};
        const v4f hi = v4f{acc[g][0].z, acc[g][1].z, acc[g][0].w, acc[g][1].w};
        if (j0 + 4 <= geo.b && n0 >= 0 && n0 + 4 <= cx.n_limit) {
            typedef v4f __attribute__((address_space(1), aligned(8)))* g_f4a8_ptr;
            g_f4a8_ptr o = (g_f4a8_ptr)(out + static_cast<size_t>(n0) * 2);
            o[0] = lo;
            o[1] = hi;
        } else {
            const float v[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int32_t n = n0 + r;
                if (j0 + r < geo.b && n >= 0 && n < cx.n_limit) {
                    typedef v2f __attribute__((address_space(1)))* g_f2_ptr;
                    *((g_f2_ptr)(out + static_cast<size_t>(n) * 2)) = v2f{v[2 * r], v[2 * r + 1]};
                }
            }
        }
    }
}

// A-operand registers of a consumer wave: three sets of four steps.  The coefficient stream runs
// 8-12 steps ahead of the MFMAs and straight across unit boundaries (the next unit is claimed
// while the current one runs), so a unit never starts by waiting for its first coefficients.  A set
// is refilled right after its last use and needed again two blocks later.  The window length is
// padded to a multiple of three blocks (48 taps, zero coefficients), so every unit starts on set 0
// and the loop body is one branch-free basic block: no register copies (which would have to wait
// for the youngest load) and exact s_waitcnt counts from the compiler.
struct MfmaPipe {
    float a[3][4];
    bool primed;      // sets 0, 1, 2 hold blocks 0, 1, 2 of the unit about to run
};

// FLAT: period rows are back to back in LDS (odd a), so a window that runs past its row simply
// continues in the next one and a step's LDS offset is a compile-time immediate.
template <int G, bool FLAT, int DBG>
__device__ __forceinline__ void process_unit_mfma(const GeoArgs& geo, const ItemCtx& cx,
                                                  const float* rows, uint32_t unit, uint32_t ob,
                                                  MfmaPipe& pipe, uint32_t unit_next, bool has_next,
                                                  WaveTrace& wt) {
    const uint32_t hs = geo.unit_shift;                // log2(units per tile)
    const uint32_t T = unit >> hs, h = unit & ((1u << hs) - 1);
    const uint32_t lane = cx.lane;
    const uint32_t k = lane >> 4, pi = lane & 15;
    const uint32_t n_steps = geo.row_len >> 2, n_blocks = n_steps >> 2;   // a multiple of 3
    // taps of the window that lie in the lane's own period row; the rest continue in the next row
    const uint32_t n1 = geo.a - ob < geo.row_len ? geo.a - ob : geo.row_len;
    const uint32_t jump = geo.row_stride - geo.a * 2;  // dwords skipped between two period rows
    // first step at which this lane's tap (4c + k) has crossed into the next row
    const uint32_t c_jump = n1 > k ? (n1 - k + 3) >> 2 : 0;

    const float* xbase[G];
    bool p_on[G];
    uint32_t p_idx[G];
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const uint32_t pl = 16 * (G * h + g) + pi;
        p_on[g] = pl < geo.pw;
        p_idx[g] = pl;
        xbase[g] = rows + (p_on[g] ? pl : 0) * geo.row_stride + 2 * (ob + k);
    }
    // Coefficients: wave-uniform base pointer (SGPR pair) + lane offset; the stream moves on to the
    // next unit's table when this one's blocks are exhausted.
    gptr_f32 tab = (gptr_f32)(cx.table);
    const uint32_t tile_floats = n_steps * 64;
    gptr_f32 a_ptr = tab + static_cast<size_t>(T) * tile_floats;
    gptr_f32 a_next = has_next ? tab + static_cast<size_t>(unit_next >> hs) * tile_floats : a_ptr;
    uint32_t a_blk = 0;   // block the stream pointer stands at
    auto load_a = [&](float (&dst)[4]) {
        if constexpr (DBG & 1) {   // timing experiment: one hot 256-byte line
#pragma unroll
            for (uint32_t s = 0; s < 4; ++s) dst[s] = tab[lane];
            return;
        }
        typedef const v4f __attribute__((address_space(1)))* gptr_v4f;
        const v4f v = ((gptr_v4f)a_ptr)[lane];   // four steps of this lane: one 1 KB wave load
        dst[0] = v.x; dst[1] = v.y; dst[2] = v.z; dst[3] = v.w;
        ++a_blk;
        a_ptr = a_blk == n_blocks ? a_next : a_ptr + 256;
    };

    v4f acc[G][2];
#pragma unroll
    for (int g = 0; g < G; ++g) {
        acc[g][0] = v4f{0.f, 0.f, 0.f, 0.f};
        acc[g][1] = v4f{0.f, 0.f, 0.f, 0.f};
    }
    // samples of step c (c may run up to three steps past the window: those values are never used;
    // the image is padded so that the reads stay inside it)
    auto load_b = [&](v2f (&x)[G], uint32_t c_var, uint32_t c_imm) {
        if constexpr (DBG & 2) {   // timing experiment: no LDS reads
#pragma unroll
            for (int g = 0; g < G; ++g) x[g] = v2f{1.f + c_imm, 2.f};
            return;
        }
        if constexpr (FLAT) {
#pragma unroll
            for (int g = 0; g < G; ++g) x[g] = *reinterpret_cast<const v2f*>(xbase[g] + 8 * c_imm);
        } else {
            const uint32_t c = c_var + c_imm;
            const uint32_t off = 8 * c + (c >= c_jump ? jump : 0);
#pragma unroll
            for (int g = 0; g < G; ++g) x[g] = *reinterpret_cast<const v2f*>(xbase[g] + off);
        }
    };
    if (pipe.primed) {
        a_blk = 3;
        a_ptr += 3 * 256;
        if (n_blocks == 3) a_ptr = a_next;
    } else {
        load_a(pipe.a[0]);
        load_a(pipe.a[1]);
        load_a(pipe.a[2]);
    }
    // samples: a ring of four steps, loaded three steps ahead of their MFMAs; four steps per block,
    // so the ring position of a step is static as well
    v2f x[4][G];
    load_b(x[0], 0, 0);
    load_b(x[1], 0, 1);
    load_b(x[2], 0, 2);
    wt.event(20);   // operands requested
    for (uint32_t blk = 0; blk < n_blocks; blk += 3) {
#pragma unroll
        for (uint32_t u = 0; u < 3; ++u) {
#pragma unroll
            for (uint32_t s = 0; s < 4; ++s) {
                load_b(x[(s + 3) & 3], 4 * blk, 4 * u + s + 3);
#pragma unroll
                for (int g = 0; g < G; ++g) {
                    acc[g][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(pipe.a[u][s], x[s][g].x, acc[g][0], 0, 0, 0);
                    acc[g][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(pipe.a[u][s], x[s][g].y, acc[g][1], 0, 0, 0);
                }
            }
            // keep the refill here: the scheduler otherwise sinks all twelve loads to the loop end,
            // where the next iteration immediately waits for them
            __builtin_amdgcn_sched_barrier(0);
            load_a(pipe.a[u]);
            __builtin_amdgcn_sched_barrier(0);
        }
        if constexpr (FLAT) {
#pragma unroll
            for (int g = 0; g < G; ++g) xbase[g] += 96;   // 12 steps x 4 frames x 2 channels
        }
    }
    pipe.primed = has_next;
    wt.event(21);   // MFMAs issued

    mfma_store_unit<G>(geo, cx, acc, p_on, p_idx, T * kMfmaClassTile + 4 * k);
}

constexpr uint32_t kNoItem = 0xFFFFFFFFu;
constexpr uint32_t kDbMaxImages = 4;
static_assert(kDbMaxImages * 7 <= 32, "control arrays end where the item posts begin");
// control words: seven arrays of kDbMaxImages (see fir_periodic_db_kernel) + one item post per image
constexpr uint32_t kDbPostBase = 32;   // kDbMaxImages posts of kPostWords words follow
constexpr uint32_t kDbMailBase = 64;   // producer 0 -> other producers: the claimed item, one slot per s & 3
static_assert(kDbMailBase + 4 <= kDbCtrlWords, "the control words (fir_periodic_consts.h: the host sizes the LDS by them) hold the mail slots");

__device__ __forceinline__ uint32_t lds_load_acquire(uint32_t* p) {
    return __hip_atomic_load(p, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ void lds_store_release(uint32_t* p, uint32_t v) {
    __hip_atomic_store(p, v, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// Sample ring of the pipelined matrix-core units: kRing steps, loaded kRing - 1 steps ahead of their
// MFMAs.  Must divide 12 (the window is a multiple of 12 steps) so that a step's ring slot is the
// same in every unit.
constexpr uint32_t kRing = 4;

// Everything about a unit that can be computed ahead of its MFMAs.
template <int G>
struct MfmaUnit {
    const float* xbase[G];   // LDS: the lane's sample of step 0 (tap k of period pi of group g)
    g_f32_ptr out[G];        // where the lane's 4 frames x 2 channels go
    uint32_t mode[G];        // 0 nothing to store, 1 all four frames in range, 2 some of them
    int32_t n0[G];           // launch-relative index of the lane's first output frame
    uint32_t j0;             // first of the lane's four classes
    uint32_t c_jump;         // (padded rows only) first step at which the lane's tap is in the next row
    uint32_t tile, unit;
    // 0, or for a tile holding a wrap class: 1 | image << 1 | wrap index << 3 | class-in-tile << 4 |
    // (item sequence + 1) << 8 -- where a producer leaves the wrap results and how to tell they are there
    uint32_t wrap;
    bool fast;               // wave-uniform: every lane stores all four frames of every group
    gptr_f32 table;          // the item's class table (streams of one launch may differ in drift)
    int32_t n_limit;         // outputs of the item's stream in this launch
    uint32_t stream;         // the stream's index in the launch (non-finite marks)
};

// The addressing of a unit, in three pieces so that it can be spread over several MFMA gaps.
template <int G>
__device__ __forceinline__ void mfma_unit_setup_common(MfmaUnit<G>& u, const GeoArgs& geo,
                                                       const ItemCtx& cx, uint32_t unit,
                                                       uint32_t& ob, uint32_t& h) {
    const uint32_t T = unit >> geo.unit_shift;         // 1 or 2 units per tile
    h = unit & ((1u << geo.unit_shift) - 1);
    const uint32_t k = cx.lane >> 4;
    // first frame of the tile's window: floor(16 T a / b), < 2^16 * 2^12 (32-bit math)
    ob = (T * kMfmaClassTile * geo.a) / geo.b;
    // taps of the window that lie in the lane's own period row; the rest continue in the next row
    const uint32_t n1 = geo.a - ob < geo.row_len ? geo.a - ob : geo.row_len;
    u.c_jump = n1 > k ? (n1 - k + 3) >> 2 : 0;
    u.tile = T;
    u.unit = unit;
    u.fast = true;
    // classes i * den (i < r <= kMfmaWrapMax) have an integer exact position: their outputs may take
    // the wrap variant, which a producer wave has left in LDS (den >= 16: at most one per tile)
    u.wrap = 0;
    if (geo.inline_wraps && !(geo.debug & 2048)) {
#pragma unroll
        for (uint32_t i = 0; i < kMfmaWrapMax; ++i) {
            const uint32_t jw = i * geo.den;
            if (i < geo.r && jw / kMfmaClassTile == T)
                u.wrap = 1u | (cx.wrap_tag & 3u) << 1 | i << 3 | (jw % kMfmaClassTile) << 4 | (cx.wrap_tag >> 2) << 8;
        }
    }
    u.table = (gptr_f32)(cx.table);
    u.n_limit = cx.n_limit;
    u.stream = cx.stream;
    u.j0 = T * kMfmaClassTile + 4 * k;
}

template <int G>
__device__ __forceinline__ void mfma_unit_setup_group(MfmaUnit<G>& u, int g, const GeoArgs& geo,
                                                      const ItemCtx& cx, const float* rows, uint32_t ob,
                                                      uint32_t h) {
    const uint32_t k = cx.lane >> 4, pi = cx.lane & 15;
    const uint32_t pl = 16 * (G * h + g) + pi;
    const bool on = pl < geo.pw;
    u.xbase[g] = rows + (on ? pl : 0) * geo.row_stride + 2 * (ob + k);
    const int32_t n0 = cx.n_block0 + static_cast<int32_t>(pl * geo.b + u.j0);
    u.n0[g] = n0;
    u.out[g] = cx.out + static_cast<int64_t>(n0) * 2;
    const bool all = u.j0 + 4 <= geo.b && n0 >= 0 && n0 + 4 <= cx.n_limit;
    const bool none = u.j0 >= geo.b || n0 + 4 <= 0 || n0 >= cx.n_limit;
    u.mode[g] = !on || none ? 0u : (all ? 1u : 2u);
    u.fast = u.fast && __all(u.mode[g] == 1);
}

template <int G>
__device__ __forceinline__ MfmaUnit<G> mfma_unit_setup(const GeoArgs& geo, const ItemCtx& cx,
                                                      const float* rows, uint32_t unit) {
    MfmaUnit<G> u;
    uint32_t ob, h;
    mfma_unit_setup_common<G>(u, geo, cx, unit, ob, h);
#pragma unroll
    for (int g = 0; g < G; ++g) mfma_unit_setup_group<G>(u, g, geo, cx, rows, ob, h);
    return u;
}

// Sums of a finished unit waiting to be stored: the stores (a 4 x 2 register shuffle and two
// dwordx4 per group) are issued inside the NEXT unit's MFMA stream.
template <int G>
struct MfmaPending {
    v4f acc[G][2];
    MfmaUnit<G> unit;
    bool valid;
};

// lane = (period, 4 consecutive classes), both channels -> 32 contiguous bytes per lane, 128 per
// period: no transpose
// Inside an MFMA stream every taken branch costs an instruction refetch during which the wave issues
// nothing (about 50 cycles; fifteen of them per unit cost 20 % of the pipe).  The common case -- every
// lane of the wave stores all its frames -- is therefore one predictable, not-taken test and
// straight-line stores; stream edges take the slow path.
template <int G>
__device__ __forceinline__ void mfma_store_pending_group(const GeoArgs& geo, const MfmaPending<G>& pend, int g) {
    const MfmaUnit<G>& u = pend.unit;
    if (pend.valid) {
        const v4f s0 = pend.acc[g][0], s1 = pend.acc[g][1];
        nf_mark(geo.nf, u.mode[g] != 0 && nf_is_bad(nf_sum8(s0, s1)), u.stream, u.n0[g], 4, u.n_limit);
    }
    if (__builtin_expect(pend.valid && u.fast && !u.wrap && !(geo.debug & 16), 1)) {
        const v4f a0 = pend.acc[g][0], a1 = pend.acc[g][1];
        typedef v4f __attribute__((address_space(1), aligned(8)))* g_f4a8_ptr;
        g_f4a8_ptr o = (g_f4a8_ptr)(u.out[g]);
        o[0] = v4f{a0.x, a1.x, a0.y, a1.y};
        o[1] = v4f{a0.z, a1.z, a0.w, a1.w};
        return;
    }
    if (!pend.valid) return;
    if (geo.debug & 16) {
        const float s = pend.acc[g][0].x + pend.acc[g][1].y + pend.acc[g][0].z + pend.acc[g][1].w;
        if (s == 12345.678f) u.out[0][0] = s;
        return;
    }
    v4f a0 = pend.acc[g][0], a1 = pend.acc[g][1];
    if (u.wrap) {   // wave-uniform: this tile holds a class whose outputs may take the wrap variant
        // (computed by a producer after it published the image; long done by now as a rule)
        extern __shared__ __attribute__((aligned(16))) float lds_base[];
        const uint32_t wb = (u.wrap >> 1) & 3, wi = (u.wrap >> 3) & 1, wc = (u.wrap >> 4) & 15, wseq = u.wrap >> 8;
        uint32_t* flag = reinterpret_cast<uint32_t*>(lds_base) + 24 + wb;
        while ((lds_load_acquire(flag) & 0xFFFFFFu) != wseq) __builtin_amdgcn_s_sleep(1);
        const float* wv = lds_base + kDbCtrlWords + geo.images * db_image_len(geo.xprev_len, geo.pw, geo.row_stride) +
                          wb * mfma_wrap_words(geo.pw) + wi * (mfma_wrap_words(geo.pw) / kMfmaWrapMax);
        const uint32_t lane = threadIdx.x & 63;
        const uint32_t pl = 16 * (G * (u.unit & ((1u << geo.unit_shift) - 1)) + g) + (lane & 15);   // the lane's period in the image
        if ((lane >> 4) == (wc >> 2) && u.mode[g] != 0) {
            const v4f w = *reinterpret_cast<const v4f*>(wv + pl * 4);
            if (__float_as_uint(w.z) != 0u) {
                const uint32_t wr = wc & 3;
                if (wr == 0) { a0.x = w.x; a1.x = w.y; }
                else if (wr == 1) { a0.y = w.x; a1.y = w.y; }
                else if (wr == 2) { a0.z = w.x; a1.z = w.y; }
                else { a0.w = w.x; a1.w = w.y; }
            }
        }
    }
    const v4f lo = v4f{a0.x, a1.x, a0.y, a1.y};
    const v4f hi = v4f{a0.z, a1.z, a0.w, a1.w};
    if (u.mode[g] == 1) {
        typedef v4f __attribute__((address_space(1), aligned(8)))* g_f4a8_ptr;
        g_f4a8_ptr o = (g_f4a8_ptr)(u.out[g]);
        o[0] = lo;
        o[1] = hi;
    } else if (u.mode[g] == 2) {
        const float v[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int32_t n = u.n0[g] + r;
            if (u.j0 + r < geo.b && n >= 0 && n < u.n_limit) {
                typedef v2f __attribute__((address_space(1)))* g_f2_ptr;
                *((g_f2_ptr)(u.out[g] + 2 * r)) = v2f{v[2 * r], v[2 * r + 1]};
            }
        }
    }
}

template <int G>
__device__ __forceinline__ void mfma_store_pending(const GeoArgs& geo, MfmaPending<G>& pend) {
#pragma unroll
    for (int g = 0; g < G; ++g) mfma_store_pending_group<G>(geo, pend, g);
    pend.valid = false;
}

// Register-resident, software-pipelined variant for windows of 12 * NB3 steps (NB3 = 1..3: <= 144 taps;
// with a 192-tap tile in registers the build spilled).
//  * The whole coefficient tile of a unit (3 * NB3 dwordx4 per lane) sits in registers.  As soon as
//    a block has been used, its register is refilled with the same block of the NEXT unit's tile --
//    requested a full unit time (2-5 us) before its first use.  The vector memory pipe is shared
//    with the producers' LDS-DMA (HBM misses) and with the output stores (vmcnt is in order: a load
//    issued after a store also waits for that store), so a ring that runs only ~1000 cycles ahead
//    stalls on both; here every coefficient load is older than the stores that precede its use.
//  * The next unit's addressing (an integer division, LDS and output addresses, range checks) and
//    its first three sample loads are issued INSIDE this unit's MFMA stream.  While one wave of a
//    SIMD streams MFMAs, the other wave's vector instructions hardly get issued (measured: its
//    "setup" lasted exactly as long as the partner's MFMA burst), so work left between two
//    bursts is not hidden by the partner; inside the burst it rides in the MFMAs' own shadow.
template <int NB3>
struct MfmaTileRegs {
    v4f a[3 * NB3];
    bool primed;      // a[] holds (or is about to receive) the tile of the unit about to run
};

template <int G, bool FLAT, int NB3>
__device__ __forceinline__ void mfma_unit_run(const GeoArgs& geo, const ItemCtx& cx, const float* rows,
                                              const MfmaUnit<G>& cur, MfmaUnit<G>& nxt,
                                              v2f (&x)[kRing][G], MfmaTileRegs<NB3>& regs,
                                              MfmaPending<G>& pend, uint32_t unit_next, bool has_next,
                                              WaveTrace& wt) {
    static_assert(NB3 >= 1 && NB3 <= 3, "windows of 48, 96 or 144 taps");
    constexpr uint32_t kBlocks = 3 * NB3, kSteps = 4 * kBlocks;
    typedef const v4f __attribute__((address_space(1)))* gptr_v4f;
    const uint32_t jump = geo.row_stride - geo.a * 2;  // dwords skipped between two period rows
    // `cx` and `rows` are those of the NEXT unit's item (the same as this one's except across an
    // item boundary); everything about the current unit is in `cur`.
    if (!regs.primed) {
        gptr_v4f src = (gptr_v4f)(cur.table + static_cast<size_t>(cur.tile) * (kSteps * 64)) + cx.lane;
#pragma unroll
        for (uint32_t j = 0; j < kBlocks; ++j) regs.a[j] = src[j * 64];
    }
    // refill source: the next unit's tile (this one's again if there is none: harmless)
    gptr_v4f nsrc = has_next ? (gptr_v4f)((gptr_f32)(cx.table) + static_cast<size_t>(unit_next >> geo.unit_shift) * (kSteps * 64)) + cx.lane
                             : (gptr_v4f)(cur.table + static_cast<size_t>(cur.tile) * (kSteps * 64)) + cx.lane;
    regs.primed = has_next;

    // samples of step c of unit `u` (c may run up to three steps past the window of the last unit of
    // an image: those values are never used; the image is padded so that the reads stay inside it)
    auto load_b = [&](v2f (&dst)[G], const MfmaUnit<G>& u, uint32_t c) {
        if constexpr (FLAT) {
#pragma unroll
            for (int g = 0; g < G; ++g) dst[g] = *reinterpret_cast<const v2f*>(u.xbase[g] + 8 * c);
        } else {
            const uint32_t off = 8 * c + (c >= u.c_jump ? jump : 0);
#pragma unroll
            for (int g = 0; g < G; ++g) dst[g] = *reinterpret_cast<const v2f*>(u.xbase[g] + off);
        }
    };
    v4f acc[G][2];
    uint32_t nxt_ob = 0, nxt_h = 0;
    wt.event(20);
#pragma unroll
    for (uint32_t c = 0; c < kSteps; ++c) {
        // samples run kRing - 1 steps ahead, straight into the next unit
        constexpr uint32_t kAhead = kRing - 1;
        if (c + kAhead < kSteps) load_b(x[(c + kAhead) % kRing], cur, c + kAhead);
        else load_b(x[(c + kAhead) % kRing], nxt, c + kAhead - kSteps);
        const v4f av = regs.a[c >> 2];
        const float a = (c & 3) == 0 ? av.x : (c & 3) == 1 ? av.y : (c & 3) == 2 ? av.z : av.w;
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const v4f z = v4f{0.f, 0.f, 0.f, 0.f};
            acc[g][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, x[c % kRing][g].x, c == 0 ? z : acc[g][0], 0, 0, 0);
            acc[g][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, x[c % kRing][g].y, c == 0 ? z : acc[g][1], 0, 0, 0);
        }
        // the loop is straight-line code: without a fence per step the scheduler hoists dozens of
        // LDS reads to the top (and sinks the refills to the bottom)
        __builtin_amdgcn_sched_barrier(0);
        // The next unit's addressing and the previous unit's stores ride in the shadow of this
        // unit's MFMAs, a piece per step (a gap between two MFMAs hides about five instructions).
        if (c == 1) {   // without a next unit: this unit's own index again (results unused)
            mfma_unit_setup_common<G>(nxt, geo, cx, has_next ? unit_next : cur.unit, nxt_ob, nxt_h);
            __builtin_amdgcn_sched_barrier(0);
        }
        if (c >= 2 && c < 2 + G) {
            mfma_unit_setup_group<G>(nxt, c - 2, geo, cx, rows, nxt_ob, nxt_h);
            __builtin_amdgcn_sched_barrier(0);
        }
        if (c >= 2 + G && c < 2 + 2 * G) {
            mfma_store_pending_group<G>(geo, pend, c - 2 - G);
            if (c == 1 + 2 * G) pend.valid = false;
            __builtin_amdgcn_sched_barrier(0);
        }
        if ((c & 3) == 3) {
            regs.a[c >> 2] = nsrc[(c >> 2) * 64];
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    wt.event(21);   // MFMAs issued
    // hand the sums to the next unit's stream (or to the caller's flush at the end of the item)
#pragma unroll
    for (int g = 0; g < G; ++g) {
        pend.acc[g][0] = acc[g][0];
        pend.acc[g][1] = acc[g][1];
    }
    pend.unit = cur;
    pend.valid = true;
}

// ---- double-buffered kernel ------------------------------------------------------------------------
// One 12-wave workgroup per CU owning two LDS images.  The first `producers` waves only stage:
// wait until every consumer has left an image, claim the next work item, DMA it in, publish it.
// The other waves only compute: matrix-core work units of the published image are claimed one at a
// time, and a wave that finds none left moves straight on to the other image -- no workgroup barrier
// anywhere, so staging, the uneven progress of the waves (the SIMD arbiter favours the oldest) and the
// unit count not dividing the wave count cost nothing as long as an image is staged (~4-7 us) faster
// than its units are consumed (~14 us).
// MF = period groups per unit (bits 0-3) | RSMP_FIR_MFMA_DBG << 4 | NB3 << 6 | FLAT << 9; NB3 = 0: the
// coefficients go through a ring (process_unit_mfma), else the tile of 48 * NB3 taps sits in registers
// (mfma_consumer_stream).  CG, C2 and NT are those of fir_periodic_kernel; only <2, true, 8> is built.
//
// LDS control words (u32): [0..1] tile_counter per image, [2..3] consumers that have left the
// image (cumulative over its uses), [4..5] sequence number + 1 of the item the image holds,
// [6..7] its work item (or kNoItem), [8..9] producers finished staging (cumulative),
// [10..11] sequence + 1 of the item whose id has been posted (for the other producers).


// Per-image item post (written by producer 0 before it publishes the image): what a matrix-core
// consumer needs to know about the item, so that moving on to the next item costs a few LDS reads
// instead of a descriptor fetch and 64-bit divisions.
constexpr uint32_t kPostWords = 8;   // out (2), class table (2), n_block0, n_limit, 2 spare
struct ItemPost {
    unsigned long long out, table;
    int32_t n_block0, n_limit;
    uint32_t stream;      // the stream's index in the launch
    uint32_t spare;
};
static_assert(sizeof(ItemPost) == kPostWords * 4, "ItemPost layout");

__device__ __forceinline__ ItemCtx ctx_from_post(const uint32_t* post, uint32_t wrap_tag, uint32_t lane) {
    ItemCtx cx;
    uint32_t w[7];
#pragma unroll
    for (int i = 0; i < 7; ++i) w[i] = __builtin_amdgcn_readfirstlane(post[i]);
    cx.out = (g_f32_ptr)(static_cast<unsigned long long>(w[0]) | (static_cast<unsigned long long>(w[1]) << 32));
    cx.table = (const_f32_ptr)(static_cast<unsigned long long>(w[2]) | (static_cast<unsigned long long>(w[3]) << 32));
    cx.wtable = cx.table;
    cx.metas = nullptr;
    cx.wrap_bits = nullptr;
    cx.n_block0 = static_cast<int32_t>(w[4]);
    cx.k_block0 = 0;
    cx.n_limit = static_cast<int32_t>(w[5]);
    cx.lane_row = nullptr;
    cx.xprev = nullptr;
    cx.wrap_tag = wrap_tag;
    cx.stream = w[6];
    cx.pl_c = 0;
    cx.gi = 0;
    cx.lane = lane;
    cx.lane_on = true;
    return cx;
}

// Consumer wave of the register-resident matrix-core path: ONE MFMA stream over (item, unit) pairs.
// Units are claimed two ahead; when the claims on the current image run out and the next image is
// already published (the normal case: producers are an item ahead), the claim stream simply moves
// on to it, so the last unit of an item prefetches the first unit of the next and the pipe never
// drains between items.  Only when the next image is not ready does the wave flush and wait.
template <int G, bool FLAT, int NB3>
__device__ __forceinline__ void mfma_consumer_stream(const GeoArgs& geo, float* lds, uint32_t image_len,
                                                     uint32_t lane, WaveTrace& wt) {
    uint32_t* ctrl = reinterpret_cast<uint32_t*>(lds);
    uint32_t* tile_counter = ctrl, *left = ctrl + 4, *ready = ctrl + 8, *item_id = ctrl + 12;
    const uint32_t* posts = ctrl + kDbPostBase;
    const uint32_t imask = geo.images - 1;   // images: 2 or 4
    const uint32_t n_units = geo.n_tiles;
    auto rows_of = [&](uint32_t b) -> const float* {
        return lds + kDbCtrlWords + b * image_len + geo.xprev_len;
    };
    auto claim2 = [&](uint32_t b, uint32_t& first, uint32_t& in_flight) {
        uint32_t c1 = 0;
        if (lane == 0) {
            c1 = atomicAdd(tile_counter + b, 1u);
            in_flight = atomicAdd(tile_counter + b, 1u);
        }
        first = __builtin_amdgcn_readfirstlane(c1);
    };
    auto leave = [&](uint32_t b) {
        if (lane == 0) __hip_atomic_fetch_add(left + b, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
    };
    MfmaTileRegs<NB3> regs;
    MfmaPending<G> pend;
    pend.valid = false;
    uint32_t s = 0;
    for (;;) {
        // ---- (re)start the stream on item s: blocking -------------------------------------------
        uint32_t b = s & imask;
        wt.event(1);
        while (lds_load_acquire(ready + b) != s + 1) __builtin_amdgcn_s_sleep(2);
        wt.event(2);
        if (static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(item_id[b])) == kNoItem) return;
        ItemCtx cx = ctx_from_post(posts + kPostWords * b, b | ((s + 1) & 0xFFFFFFu) << 2, lane);
        uint32_t c2 = 0, t, t_next;
        claim2(b, t, c2);
        t_next = __builtin_amdgcn_readfirstlane(c2);
        if (t >= n_units) {   // every unit of this item is taken already
            leave(b);
            ++s;
            continue;
        }
        MfmaUnit<G> cur = mfma_unit_setup<G>(geo, cx, rows_of(b), t), nxt = cur;
        regs.primed = false;
        v2f x[kRing][G];
#pragma unroll
        for (uint32_t c = 0; c + 1 < kRing; ++c) {
            const uint32_t off = 8 * c + (!FLAT && c >= cur.c_jump ? geo.row_stride - 2 * geo.a : 0);
#pragma unroll
            for (int g = 0; g < G; ++g) x[c][g] = *reinterpret_cast<const v2f*>(cur.xbase[g] + off);
        }
        // claim side of the stream: item sn, image bn (ahead of the running side by at most one item)
        uint32_t sn = s, bn = b;
        ItemCtx cxn = cx;
        for (;;) {
            wt.event(6);
            bool more = t_next < n_units;
            const uint32_t b1 = (b + 1) & imask;
            if (!more && sn == s && lds_load_acquire(ready + b1) == s + 2 &&
                static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(item_id[b1])) != kNoItem) {
                // image b is exhausted and the next item is already there: move the claims over
                sn = s + 1;
                bn = b1;
                cxn = ctx_from_post(posts + kPostWords * bn, bn | ((sn + 1) & 0xFFFFFFu) << 2, lane);
                claim2(bn, t_next, c2);
                more = t_next < n_units;
            } else if (more) {
                if (lane == 0) c2 = atomicAdd(tile_counter + bn, 1u);   // the unit after the next
            }
            mfma_unit_run<G, FLAT, NB3>(geo, cxn, rows_of(bn), cur, nxt, x, regs, pend, t_next, more, wt);
            wt.event(7);
            if (!more) break;
            if (sn != s) {   // the unit just run was this wave's last on image b
                // Its stores are still pending (they ride in the next unit's stream).  If they pick up
                // wrap results, those live in image b's LDS area and are announced by image b's flag:
                // once this wave has left, a producer may restage b and overwrite both (the wave would
                // then wait for a flag value that is gone).  Store now in that case.
                if (pend.valid && pend.unit.wrap) mfma_store_pending<G>(geo, pend);
                leave(b);
                s = sn;
                b = bn;
            }
            cur = nxt;
            t_next = __builtin_amdgcn_readfirstlane(c2);
        }
        // no next unit in reach: drain, leave, and start over on the following item
        mfma_store_pending<G>(geo, pend);
        leave(b);
        if (sn != s) {   // the claim stream had moved on but found the next item fully claimed
            leave(bn);
            s = sn;
        }
        ++s;
    }
}

template <int CG, bool C2, int NT, int MF, bool DIAG>
__global__ __launch_bounds__(768) void fir_periodic_db_kernel(const FirStreamDesc* __restrict__ descs,
                                                              GeoArgs geo_arg) {
    static_assert((MF & 15) != 0, "matrix-core consumers only");
    GeoArgs geo = geo_arg;
    if constexpr (!DIAG) {
        geo.debug = 0;
        geo.trace = nullptr;
        geo.wtrace = nullptr;
    }
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const uint32_t C = C2 ? 2u : geo.channels;
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    WaveTrace wt;
    wt.init(geo, wave);
    uint32_t* ctrl = reinterpret_cast<uint32_t*>(lds);
    uint32_t* tile_counter = ctrl, *left = ctrl + 4, *ready = ctrl + 8, *item_id = ctrl + 12;
    uint32_t* staged = ctrl + 16, *posted = ctrl + 20, *wflag = ctrl + 24;
    const uint32_t imask = geo.images - 1, ishift = geo.images == 4 ? 2 : 1;
    const uint32_t image_len = db_image_len(geo.xprev_len, geo.pw, geo.row_stride);
    if (threadIdx.x < kDbCtrlWords) ctrl[threadIdx.x] = 0;
    __syncthreads();   // the only workgroup barrier

    const uint32_t producers = geo.producers, consumers = geo.waves - geo.producers;
    if (wave < producers) {
        // ---- producer ----------------------------------------------------------------------------
        __builtin_amdgcn_s_setprio(3);   // mostly asleep; when it has work, that work gates everyone
        // With as many producers as images each producer owns an image (sequence numbers wave,
        // wave + images, ...) and stages it alone: several images are in flight at once, and nothing
        // is waited for between producers except the turn to claim (claims stay in sequence order
        // so that the first failed claim is also the last item).  Otherwise the producers stage
        // every image together.
        const bool own_image = producers == geo.images;
        uint32_t* claim_turn = ctrl + 28;
        for (uint32_t s = own_image ? wave : 0;; s += own_image ? geo.images : 1) {
            const uint32_t b = s & imask;
            float* xprev = lds + kDbCtrlWords + b * image_len;
            float* rows = xprev + geo.xprev_len;
            // The next item is claimed, and its descriptor fetched and placed, BEFORE waiting for the
            // image: the global atomic, the descriptor load and the 64-bit divisions (~1-2 us) then
            // overlap the wait instead of extending the time between "image free" and "image ready",
            // which the consumers are waiting for.
            // mailbox from producer 0 to the others, indexed by s & 3 like `posted`: producer 0 cannot be
            // four items ahead of a producer that has not yet arrived for item s + 1
            uint32_t* next_item = ctrl + kDbMailBase + (s & 3u);
            uint32_t* posted_s = posted + (s & 3u);
            uint32_t item = kNoItem;
            FirStreamDesc d;
            ItemGeom ig;
            if (wave == 0 || own_image) {
                if (own_image)
                    while (lds_load_acquire(claim_turn) != s) __builtin_amdgcn_s_sleep(2);
                // claim work items until one is real (ragged batches pad with empty ones)
                for (;;) {
                    unsigned long long tkt = 0;
                    if (lane == 0) tkt = queue_claim(geo);
                    const uint32_t lo = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(tkt));
                    const uint32_t hi = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(tkt >> 32));
                    if (hi != 0 || lo >= geo.total_items) { item = kNoItem; break; }
                    item = lo;
                    const uint32_t stream_idx = item / geo.blocks_per_stream;
                    d = load_uniform(descs + stream_idx);
                    ig = item_geom(geo, d, item - stream_idx * geo.blocks_per_stream);
                    if (ig.valid) break;
                }
                if (own_image) {
                    lds_store_release(claim_turn, s + 1);
                } else {
                    if (lane == 0) next_item[0] = item;
                    lds_store_release(posted_s, s + 1);
                }
            } else {
                while (lds_load_acquire(posted_s) != s + 1) __builtin_amdgcn_s_sleep(2);
                item = __builtin_amdgcn_readfirstlane(next_item[0]);
                if (item != kNoItem) {
                    const uint32_t stream_idx = item / geo.blocks_per_stream;
                    d = load_uniform(descs + stream_idx);
                    ig = item_geom(geo, d, item - stream_idx * geo.blocks_per_stream);
                }
            }
            wt.event(11);
            // every consumer has left the image's previous use (s - images)
            while (lds_load_acquire(left + b) != consumers * (s >> ishift)) __builtin_amdgcn_s_sleep(2);
            wt.event(12);
            if ((wave == 0 || own_image) && lane == 0) {
                item_id[b] = item;
                tile_counter[b] = 0;
                if (item != kNoItem) {
                    ItemPost* post = reinterpret_cast<ItemPost*>(ctrl + kDbPostBase + kPostWords * b);
                    post->out = reinterpret_cast<unsigned long long>(d.out);
                    post->table = reinterpret_cast<unsigned long long>(d.class_coef);
                    post->n_block0 = ig.n_block0;
                    post->n_limit = static_cast<int32_t>(d.n_out);
                    post->stream = item / geo.blocks_per_stream;
                }
            }
            if (item != kNoItem && !(geo.debug & 1))
                stage_image(geo, d, ig.q0, C, rows, xprev, own_image ? 0 : wave, own_image ? 1 : producers, lane);
            wt.event(13);
            __builtin_amdgcn_s_waitcnt(0);   // DMA (vmcnt) and LDS stores (lgkmcnt) of this wave are done
            wt.event(14);
            uint32_t n = 0;
            if (!own_image) {
                if (lane == 0) n = __hip_atomic_fetch_add(staged + b, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_WORKGROUP);
                n = __builtin_amdgcn_readfirstlane(n);
            }
            if (own_image || n + 1 == producers * ((s >> ishift) + 1)) {   // the last one to arrive publishes the image
                lds_store_release(ready + b, s + 1);
                // ... and then computes the wrap variant of the item's wrap classes from the staged
                // image (row 1023 on the window one frame earlier, resampler_fir.rs:544, :562-565):
                // lane = period, 2 channels.  It is 0.5 % of the item's arithmetic; the consumers
                // only pick the result up in their store path.
                if (geo.inline_wraps && item != kNoItem) {
                    float* wv = lds + kDbCtrlWords + geo.images * image_len + b * mfma_wrap_words(geo.pw);
                    const uint32_t wstride = mfma_wrap_words(geo.pw) / kMfmaWrapMax;   // floats per wrap class
                    const_f32_ptr wrow = (const_f32_ptr)(d.coeffs) + static_cast<size_t>(1023) * d.taps;
                    gconst_u32_ptr wrap_bits = (gconst_u32_ptr)d.wrap_bits;
                    const uint32_t num = geo.a / geo.r, jump = geo.row_stride - 2 * geo.a;
                    const uint32_t p = lane < geo.pw ? lane : 0;
                    const float* row = rows + p * geo.row_stride;
                    for (uint32_t i = 0; i < geo.r && i < kMfmaWrapMax && !(geo.debug & 1024); ++i) {
                        const int32_t ws = static_cast<int32_t>(i * num) - 1;   // first frame of the window
                        v2f acc = v2f{0.f, 0.f};
                        uint32_t m = 0;
                        if (ws < 0) {   // i == 0: the first tap falls on the frame in front of the period
                            const v2f xv = *reinterpret_cast<const v2f*>(xprev + p * 2);
                            const float w = wrow[0];
                            acc.x = w * xv.x;
                            acc.y = w * xv.y;
                            m = 1;
                        }
                        // the remaining taps are consecutive frames: up to the end of the period row,
                        // then on in the next row
                        const uint32_t f0 = static_cast<uint32_t>(ws + static_cast<int32_t>(m));
                        const uint32_t in_row = f0 < geo.a ? (geo.a - f0 < d.taps - m ? geo.a - f0 : d.taps - m) : 0;
                        const float* px = row + 2 * f0;
                        const_f32_ptr pw_ = wrow + m;
                        auto run = [&](uint32_t count) {
                            uint32_t q = 0;
                            for (; q + 8 <= count; q += 8) {
                                v2f xv[8];
#pragma unroll
                                for (int e = 0; e < 8; ++e) xv[e] = *reinterpret_cast<const v2f*>(px + 2 * (q + e));
#pragma unroll
                                for (int e = 0; e < 8; ++e) {
                                    const float w = pw_[q + e];
                                    acc.x = fmaf(w, xv[e].x, acc.x);
                                    acc.y = fmaf(w, xv[e].y, acc.y);
                                }
                            }
                            for (; q < count; ++q) {
                                const v2f x1 = *reinterpret_cast<const v2f*>(px + 2 * q);
                                const float w = pw_[q];
                                acc.x = fmaf(w, x1.x, acc.x);
                                acc.y = fmaf(w, x1.y, acc.y);
                            }
                            px += 2 * count;
                            pw_ += count;
                        };
                        run(in_row);
                        px += jump;
                        run(d.taps - m - in_row);
                        const int32_t nw = ig.n_block0 + static_cast<int32_t>(p * geo.b + i * geo.den);
                        uint32_t take = 0;
                        if (lane < geo.pw && nw >= 0 && nw < static_cast<int32_t>(d.n_out)) {
                            const uint32_t K = static_cast<uint32_t>(ig.k_block0 + static_cast<int32_t>(p * geo.r + i));
                            take = (wrap_bits[K >> 5] >> (K & 31)) & 1u;
                        }
                        if (lane * 4 < wstride)
                            *reinterpret_cast<v4f*>(wv + i * wstride + lane * 4) =
                                v4f{acc.x, acc.y, __uint_as_float(take), 0.f};
                    }
                    __builtin_amdgcn_s_waitcnt(0);
                    lds_store_release(wflag + b, s + 1);
                }
            }
            if (item == kNoItem) break;
        }
        return;
    }

    // ---- consumer --------------------------------------------------------------------------------
    constexpr int G = MF & 15, DBG = (MF >> 4) & 3, NB3 = (MF >> 6) & 7;
    if constexpr (NB3 != 0) {
        mfma_consumer_stream<G, ((MF >> 9) & 1) != 0, NB3>(geo, lds, image_len, lane, wt);
    } else {
        for (uint32_t s = 0;; ++s) {
            const uint32_t b = s & imask;
            const float* xprev = lds + kDbCtrlWords + b * image_len;
            const float* rows = xprev + geo.xprev_len;
            wt.event(1);
            while (lds_load_acquire(ready + b) != s + 1) __builtin_amdgcn_s_sleep(2);
            wt.event(2);
            const uint32_t item = __builtin_amdgcn_readfirstlane(item_id[b]);
            if (item == kNoItem) break;
            const uint32_t stream_idx = item / geo.blocks_per_stream;
            const FirStreamDesc d = load_uniform(descs + stream_idx);
            const ItemGeom ig = item_geom(geo, d, item - stream_idx * geo.blocks_per_stream);
            const ItemCtx cx = item_ctx<CG, C2>(geo, d, ig, rows, xprev, lane, stream_idx);
            // Two claims are kept in flight: the unit after the current one must be known when the
            // current one starts (its coefficients and addressing are requested then), and the claim's
            // LDS round trip should never be waited for.
            uint32_t c1 = 0, c2 = 0;
            if (lane == 0) {
                c1 = atomicAdd(tile_counter + b, 1u);
                c2 = atomicAdd(tile_counter + b, 1u);
            }
            uint32_t t = __builtin_amdgcn_readfirstlane(c1);
            uint32_t t_next = __builtin_amdgcn_readfirstlane(c2);
            // The image is free again only when its last unit is done, and the SIMD arbiter serves the
            // oldest wave first: a young wave that picks up one of the last units would hold the image
            // for several unit times while everyone else has moved on.  Late units therefore outrank
            // the rest.
            auto set_priority = [&](uint32_t unit) {
                if (geo.n_tiles - 1 - unit < 4) __builtin_amdgcn_s_setprio(2);
                else __builtin_amdgcn_s_setprio(0);
            };
            // first frame of a tile's window: floor(16 T a / b), < 2^16 * 2^12 (32-bit math)
            auto base_of = [&](uint32_t unit) { return ((unit >> geo.unit_shift) * kMfmaClassTile * geo.a) / geo.b; };
            const bool flat = geo.row_stride == 2 * geo.a;
            MfmaPipe pipe;
            pipe.primed = false;
            while (t < geo.n_tiles) {
                wt.event(6);
                set_priority(t);
                if (lane == 0) c2 = atomicAdd(tile_counter + b, 1u);   // the unit after the next
                const bool more = t_next < geo.n_tiles;
                const uint32_t ob = base_of(t);
                if (flat) process_unit_mfma<G, true, DBG>(geo, cx, rows, t, ob, pipe, t_next, more, wt);
                else process_unit_mfma<G, false, DBG>(geo, cx, rows, t, ob, pipe, t_next, more, wt);
                wt.event(7);
                t = t_next;
                t_next = __builtin_amdgcn_readfirstlane(c2);
            }
            __builtin_amdgcn_s_setprio(0);
            // this wave's reads of image b have all returned (their values were consumed above)
            if (lane == 0) __hip_atomic_fetch_add(left + b, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
    }
}

// Outputs whose f64 position fell just below an integer: previous frame, row 1023, frac 0
// (resampler_fir.rs:544, :562-565).  8 lanes per output, as fir_generic.  Used only when the
// geometry cannot take the wrap variant inline (den < 8).
__global__ __launch_bounds__(256) void fir_wrap_fixup_kernel(const FirStreamDesc* __restrict__ descs) {
    const FirStreamDesc& d = descs[blockIdx.y];
    const uint32_t g = threadIdx.x & 7;
    const uint32_t entry = blockIdx.x * 32 + (threadIdx.x >> 3);
    const bool live = entry < d.n_wraps;
    const uint32_t n = live ? d.wraps[entry] : 0;
    const uint64_t m = d.abs_out + n;
    const int64_t exact = static_cast<int64_t>((m / d.den) * d.num);  // m % den == 0
    const int64_t v0 = exact - 1 - static_cast<int64_t>(d.abs_consumed);
    const uint32_t taps = d.taps, C = d.channels;
    const float4* __restrict__ row =
        reinterpret_cast<const float4*>(d.coeffs + static_cast<size_t>(1023) * taps);
    const int64_t hist_frames = d.hist_frames;
    for (uint32_t c = 0; c < C; ++c) {
        float a = 0.f;
        if (live) {
            for (uint32_t qd = g; qd < taps / 4; qd += 8) {
                const float4 k = row[qd];
                const float kk[4] = {k.x, k.y, k.z, k.w};
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int64_t v = v0 + 4 * qd + u;
                    const float x = v < hist_frames
                                        ? d.hist[static_cast<size_t>(v) * C + c]
                                        : d.in[static_cast<size_t>(v - hist_frames) * C + c];
                    a = fmaf(kk[u], x, a);
                }
            }
        }
        a += __shfl_xor(a, 4, 64);
        a += __shfl_xor(a, 2, 64);
        a += __shfl_xor(a, 1, 64);
        if (live && g == 0) d.out[static_cast<size_t>(n) * C + c] = a;
    }
}

GeoArgs to_args(const PeriodicGeometry& g) {
    const uint32_t debug = fir_debug_knob();
    constexpr uint32_t stagger = 1200;   // 12 us, in 10 ns units
    const uint32_t channels = g.lp * g.cg;
    return GeoArgs{g.a, g.b, g.b / g.den, g.row_len, g.mfma ? g.n_units : g.n_tiles, g.lp, g.pw, g.row_stride, g.waves,
                   channels, xprev_len_of(g.pw, channels), g.producers, g.den, g.images ? g.images : 2u,
                   g.mfma ? (g.n_units == 4 * g.n_tiles ? 2u : (g.n_units == 2 * g.n_tiles ? 1u : 0u)) : 0u,
                   g.inline_wraps ? 1u : 0u, debug, stagger, nullptr, nullptr, 0u, 0u, nullptr, 0u, NfArgs{nullptr, 0u, 0u}};
}

}  // namespace

hipError_t launch_fir_periodic(const FirStreamDesc* d_descs, uint32_t n_streams,
                               const PeriodicGeometry& geo, uint32_t max_blocks,
                               unsigned long long* d_work_counter, const NfArgs& nf, hipStream_t stream,
                               bool fuse_tail, uint64_t items_key, const FirFormat& format, const FirStatArgs& st) {
    if (n_streams == 0 || max_blocks == 0) return hipSuccess;
    int device = 0;
    hipError_t e = hipGetDevice(&device);
    if (e != hipSuccess) return e;
    const uint32_t cus = device_cus(device);
    if (geo.mfma == 3) return launch_fir_split(d_descs, n_streams, geo, max_blocks, cus, fuse_tail, nf, stream, items_key, format, st);
    if (format_group_fault(format, geo) != FormatFault::kNone) return hipErrorNotSupported;   // (PCM: the split kernel alone)
    // the build: a slot of the table (periodic_slot_for, fir_geometry.cpp), in its plain or its diagnostic row
    static const int mfma_dbg = [] {   // RSMP_FIR_MFMA_DBG: 1 hot coefficient line, 2 no LDS reads, 3 both
        const char* e = rsmp::knob("RSMP_FIR_MFMA_DBG");
        const int v = e ? atoi(e) : 0;
        return v >= 0 && v <= 3 ? v : 0;
    }();
    static const char* trace_path = rsmp::knob("RSMP_FIR_TRACE");
    static const char* wtrace_path = rsmp::knob("RSMP_FIR_WTRACE");
    GeoArgs args = to_args(geo);
    const bool diag = args.debug != 0 || trace_path != nullptr || wtrace_path != nullptr;
    const int slot = periodic_slot_for(geo, mfma_dbg, mfma_ring_knob());
    if (slot < 0) return hipErrorInvalidValue;
#define RSMP_SK(cg, c2, D) reinterpret_cast<const void*>(fir_periodic_kernel<cg, c2, 8, D>)
#define RSMP_DB(cg, c2, mf, D) reinterpret_cast<const void*>(fir_periodic_db_kernel<cg, c2, 8, mf, D>)
#define RSMP_MF(nb3v, flatv, D) RSMP_DB(2, true, 2 + 64 * (nb3v) + 512 * (flatv), D)
#define RSMP_MF1(nb3v, flatv, D) RSMP_DB(2, true, 1 + 64 * (nb3v) + 512 * (flatv), D)
#define RSMP_FNS(D)                                                                                                  \
    {RSMP_SK(2, true, D), RSMP_SK(2, false, D), RSMP_SK(1, false, D), RSMP_DB(2, true, 2, D), RSMP_DB(2, true, 4, D),  \
     RSMP_DB(2, true, 2 + 16, D), RSMP_DB(2, true, 2 + 32, D), RSMP_DB(2, true, 2 + 48, D), RSMP_MF(1, 0, D),          \
     RSMP_MF(2, 0, D), RSMP_MF(3, 0, D), RSMP_MF(1, 1, D), RSMP_MF(2, 1, D), RSMP_MF(3, 1, D), RSMP_MF1(1, 0, D),      \
     RSMP_MF1(2, 0, D), RSMP_MF1(3, 0, D), RSMP_MF1(1, 1, D), RSMP_MF1(2, 1, D), RSMP_MF1(3, 1, D)}
    static const void* const fns_all[2][kPeriodicSlots] = {RSMP_FNS(false), RSMP_FNS(true)};
#undef RSMP_FNS
#undef RSMP_SK
#undef RSMP_DB
#undef RSMP_MF
#undef RSMP_MF1
    const void* const fn = fns_all[diag ? 1 : 0][slot];
    if ((e = grant_dynamic_lds(device, fn, kLdsMax)) != hipSuccess) return e;

    const dim3 block(geo.waves * 64);
    args.blocks_per_stream = max_blocks;
    args.total_items = max_blocks * n_streams;
    args.nf = nf;
    const uint32_t slots = cus * (geo.lds_bytes > kLdsTwoPerCu ? 1u : 2u);   // workgroups that fit
    const dim3 grid(args.total_items < slots ? args.total_items : slots);
    args.work_counter = d_work_counter;
    // every claiming wave makes exactly one failing claim: one wave per workgroup claims (the kernel's
    // mode in which every producer owns an image and claims for itself needs producers == images, and
    // geometry_for() gives 4 producers for 2 images)
    args.n_claimers = grid.x;
    static TraceBuffer trace, wtrace;
    if (trace_path) {
        if ((e = trace.renew(6ull * grid.x)) != hipSuccess) return e;
        (void)hipMemset(trace.d, 0, trace.words * 8);
        args.trace = trace.d;
    }
    if (wtrace_path) {
        if ((e = wtrace.renew(static_cast<size_t>(grid.x) * kWtraceWaves * kWtraceSlots)) != hipSuccess) return e;
        (void)hipMemset(wtrace.d, 0, wtrace.words * 8);
        args.wtrace = wtrace.d;
    }
    static const bool verbose = rsmp::knob("RSMP_FIR_VERBOSE") != nullptr;
    if (verbose) {
        int blocks = -1;
        (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, fn, geo.waves * 64, geo.lds_bytes);
        fprintf(stderr,
                "[rsmp] periodic launch: a=%u b=%u row_len=%u tiles=%u cg=%u lp=%u pw=%u stride=%u "
                "waves=%u lds=%u items=%u grid=%u occupancy=%d blocks/CU\n",
                geo.a, geo.b, geo.row_len, geo.n_tiles, geo.cg, geo.lp, geo.pw, geo.row_stride,
                geo.waves, geo.lds_bytes, args.total_items, grid.x, blocks);
    }
    void* kargs[2] = {&d_descs, &args};
    e = hipLaunchKernel(fn, grid, block, kargs, geo.lds_bytes, stream);
    if (e != hipSuccess) return e;
    if (trace_path)
        trace.dump(trace_path, stream, [](FILE* f, const std::vector<unsigned long long>& h) {
            for (size_t i = 0; i < h.size() / 6; ++i)
                fprintf(f, "%zu %llu %llu %llu %llu %llu %llu\n", i, h[6 * i], h[6 * i + 1], h[6 * i + 2],
                        h[6 * i + 3], h[6 * i + 4], h[6 * i + 5]);
        });
    if (wtrace_path)   // one line per wave: block wave event...
        wtrace.dump(wtrace_path, stream, [](FILE* f, const std::vector<unsigned long long>& h) {
            for (size_t w = 0; w < h.size() / kWtraceSlots; ++w) {
                fprintf(f, "%zu %zu", w / kWtraceWaves, w % kWtraceWaves);
                for (uint32_t i = 0; i < kWtraceSlots && h[w * kWtraceSlots + i]; ++i)
                    fprintf(f, " %llu:%llu", h[w * kWtraceSlots + i] >> 8, h[w * kWtraceSlots + i] & 255);
                fprintf(f, "\n");
            }
        });
    return hipGetLastError();
}

hipError_t launch_fir_wrap_fixup(const FirStreamDesc* d_descs, uint32_t n_streams,
                                 uint32_t max_wraps, hipStream_t stream, hipEvent_t done, bool* done_attached) {
    if (n_streams == 0 || max_wraps == 0) return hipSuccess;
    if (done && done_attached) {
        hipExtLaunchKernelGGL(fir_wrap_fixup_kernel, dim3((max_wraps + 31) / 32, n_streams), dim3(256), 0, stream, nullptr, done, 0,
                              d_descs);
        *done_attached = true;
    } else {
        hipLaunchKernelGGL(fir_wrap_fixup_kernel, dim3((max_wraps + 31) / 32, n_streams), dim3(256), 0,
                           stream, d_descs);
    }
    return hipGetLastError();
}

}  // namespace rsmp
