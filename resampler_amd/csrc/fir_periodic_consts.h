// fir_periodic_consts.h -- the LDS layout numbers the exact-f32 periodic kernels (fir_periodic.hip) share with the host
// code that sizes their geometry (fir_geometry.cpp).  Constants and small functions only; standard headers and
// rsmp_hd.h, never a HIP header.
#pragma once

#include <cstdint>

#include "rsmp_hd.h"

namespace rsmp {

constexpr uint32_t kLdsTwoPerCu = 80 * 1024;   // two workgroups per CU
constexpr uint32_t kLdsMax = 160 * 1024;

// LDS prefix of an image: [4 dwords: dynamic tile counter] [pw][C] previous-frame samples, 16-byte multiple.
RSMP_HD inline uint32_t xprev_len_of(uint32_t pw, uint32_t channels) { return 4 + (pw * channels + 3) / 4 * 4; }

// Double-buffered (matrix-core) kernel: control words in front of the images (see fir_periodic_db_kernel).
constexpr uint32_t kDbCtrlWords = 80;
// floats per image (frame-before-period block + rows), a 16-byte multiple
RSMP_HD inline uint32_t db_image_len(uint32_t xprev_len, uint32_t pw, uint32_t row_stride) {
    // + 96: the matrix-core units prefetch up to 11 steps (88 dwords) past a window's end
    return (xprev_len + (pw + 1) * row_stride + 96 + 3) / 4 * 4;
}
// Wrap classes per super period the matrix-core path handles inside the kernel (b = r * den, r <= this).
constexpr uint32_t kMfmaWrapMax = 2;
// per image: {ch0, ch1, take, -} per period and wrap class
RSMP_HD inline uint32_t mfma_wrap_words(uint32_t pw) { return kMfmaWrapMax * ((pw + 15) / 16 * 16) * 4; }

}  // namespace rsmp
