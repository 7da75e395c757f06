// fir_class_table.cpp -- the host image of a class table: per output class the two phase rows of the polyphase table
// pre-mixed with the class's frac, shifted into the tile's window, in the order the kernel that reads it wants.
// Plain C++ with _Float16 (the two-plane cut of the split kernel): includes no HIP header; the stand-alone test builds it
// with clang as host code.  Build with -ffp-contract=off: the mix is the reference's two roundings.
#include <cstring>

#include "filter_design.h"
#include "fir_periodic_plan.h"
#include "fir_split_consts.h"

namespace rsmp {

// Class-table image for the split kernel: [tile][k step][plane][lane][8 x 16 bit]; lane (class m =
// lane & 15, k group = lane >> 4) element j holds window position 32 s + 16 (j >> 2) + 4 (lane >> 4) +
// (j & 3) -- the order in which the transposed LDS reads deliver the frames.  Three planes: bf16 by
// truncation (c == p1 + p2 + p3 exactly); two planes: fp16, round to nearest, of 2^13 c.
void split_store_class(std::vector<float>& coef, const PeriodicGeometry& g, uint32_t tile, uint32_t m,
                       uint32_t shift, const std::vector<float>& mixed) {
    const uint32_t nk = g.row_len / 32;
    const uint32_t planes = g.planes;
    uint32_t* words = reinterpret_cast<uint32_t*>(coef.data());
    for (uint32_t s = 0; s < nk; ++s)
        for (uint32_t grp = 0; grp < 4; ++grp)
            for (uint32_t j = 0; j < 8; ++j) {
                const uint32_t pos = 32 * s + 16 * (j >> 2) + 4 * grp + (j & 3);
                float c = 0.f;
                if (pos >= shift && pos - shift < g.taps) c = mixed[pos - shift];
                uint32_t p[3] = {0, 0, 0};
                if (planes == 3) {
                    uint32_t u;
                    std::memcpy(&u, &c, 4);
                    p[0] = u >> 16;
                    float h;
                    uint32_t hu = u & 0xFFFF0000u;
                    std::memcpy(&h, &hu, 4);
                    const float r1 = c - h;
                    std::memcpy(&u, &r1, 4);
                    p[1] = u >> 16;
                    hu = u & 0xFFFF0000u;
                    std::memcpy(&h, &hu, 4);
                    const float r2 = r1 - h;
                    std::memcpy(&u, &r2, 4);
                    p[2] = u >> 16;
                } else {
                    const float sc = c * kCScale;
                    const _Float16 h1 = static_cast<_Float16>(sc);
                    const _Float16 h2 = static_cast<_Float16>(sc - static_cast<float>(h1));
                    uint16_t b1, b2;
                    std::memcpy(&b1, &h1, 2);
                    std::memcpy(&b2, &h2, 2);
                    p[0] = b1;
                    p[1] = b2;
                }
                const uint32_t lane = 16 * grp + m;
                for (uint32_t pl = 0; pl < planes; ++pl) {
                    const size_t dword = ((((static_cast<size_t>(tile) * nk + s) * planes + pl) * 64 + lane) * 4) + (j >> 1);
                    const uint32_t sh = (j & 1) * 16;
                    words[dword] = (words[dword] & ~(0xFFFFu << sh)) | (p[pl] << sh);
                }
            }
}

size_t split_table_floats(const PeriodicGeometry& g) {
    return static_cast<size_t>(g.n_tiles) * (g.row_len / 32) * g.planes * 64 * 4;
}

HostClassTable build_class_table(const std::vector<float>& coeffs, const PeriodicGeometry& g,
                                 double drift) {
    const uint32_t taps = g.taps;
    const uint32_t ct = g.mfma ? kMfmaClassTile : kClassTile;
    HostClassTable out;
    out.coef.assign(g.mfma == 3 ? split_table_floats(g) : static_cast<size_t>(g.n_tiles) * g.row_len * ct, 0.0f);
    out.wrap_coef.assign(static_cast<size_t>(g.n_tiles) * g.row_len, 0.0f);
    out.meta.resize(g.n_tiles);
    std::vector<float> mixed(taps);
    const float* row1023 = coeffs.data() + (kPhases - 1) * taps;
    for (uint32_t t = 0; t < g.n_tiles; ++t) {
        TileMeta& tm = out.meta[t];
        std::memset(&tm, 0, sizeof tm);
        const uint32_t j0 = t * ct;
        tm.base = class_offset(g.a, g.b, j0);
        tm.wrap_col = -1;
        tm.extra_col = -2;
        float* base = out.coef.data() + static_cast<size_t>(t) * g.row_len * ct;
        for (uint32_t i = 0; i < ct && j0 + i < g.b; ++i) {
            const uint32_t j = j0 + i;
            // exact fractional position of class j, plus the stream's current f64 drift
            const uint64_t rem = (static_cast<uint64_t>(j) * g.a) % g.b;
            double fract = static_cast<double>(rem) / static_cast<double>(g.b) + drift;
            if (j % g.den == 0) fract = drift > 0.0 ? drift : 0.0;  // below-integer: wrap variant
            if (fract < 0.0) fract = 0.0;
            // resampler_fir.rs:562-565
            double phase_f = fract * static_cast<double>(kPhases);
            if (phase_f > static_cast<double>(kPhases - 1)) phase_f = static_cast<double>(kPhases - 1);
            const size_t phase1 = static_cast<size_t>(phase_f);
            const size_t phase2 = phase1 + 1 < kPhases - 1 ? phase1 + 1 : kPhases - 1;
            const float frac = static_cast<float>(phase_f - static_cast<double>(phase1));
            const float* c1 = coeffs.data() + phase1 * taps;
            const float* c2 = coeffs.data() + phase2 * taps;
            const float omf = 1.0f - frac;
            for (uint32_t k = 0; k < taps; ++k) mixed[k] = c1[k] * omf + c2[k] * frac;  // avx.rs:41-45
            const uint32_t shift = class_offset(g.a, g.b, j) - tm.base;
            if (g.mfma == 3) {
                split_store_class(out.coef, g, t, i, shift, mixed);
                continue;
            }
            if (g.mfma) {
                // A-operand order of v_mfma_f32_16x16x4_f32 (lane = 16 * (tap % 4) + class), four
                // steps of a lane adjacent: [block = tap / 16][lane][step = (tap / 4) % 4]
                for (uint32_t k = 0; k < taps; ++k) {
                    const uint32_t m = k + shift;
                    base[(m >> 4) * 256 + ((m & 3) * 16 + i) * 4 + ((m >> 2) & 3)] = mixed[k];
                }
                continue;
            }
            for (uint32_t k = 0; k < taps; ++k) base[(k + shift) * kClassTile + i] = mixed[k];

            if (g.inline_wraps && j % g.den == 0) {
                // wrap variant of class j: row 1023 on the window one frame earlier (:544, :562-564)
                tm.wrap_col = static_cast<int32_t>(i);
                tm.wrap_jd = j / g.den;
                float* wc = out.wrap_coef.data() + static_cast<size_t>(t) * g.row_len;
                const int64_t w = static_cast<int64_t>(class_offset(g.a, g.b, j)) - 1;
                if (w >= static_cast<int64_t>(tm.base)) {
                    const uint32_t ws = static_cast<uint32_t>(w - tm.base);
                    for (uint32_t k = 0; k < taps; ++k) wc[k + ws] = row1023[k];
                } else {  // one sample in front of the tile window
                    for (uint32_t k = 1; k < taps; ++k) wc[k - 1] = row1023[k];
                    tm.extra_col = static_cast<int32_t>(tm.base) - 1;
                    tm.extra_coef = row1023[0];
                }
            }
        }
    }
    return out;
}

}  // namespace rsmp
