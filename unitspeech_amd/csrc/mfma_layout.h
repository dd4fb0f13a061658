// Row layout of the 32x32 MFMA accumulator.  Plain C++ (kernels.h includes it; so does a host compiler: tools/f16x3_layout_check.cpp).
#pragma once
#if defined(__HIPCC__)
#define US_HD __host__ __device__
#else
#define US_HD
#endif
namespace us {
// C/D of the 32x32 MFMAs: register r (0..15) of a lane holds column lane & 31 and row mfma32_row(r, lane >> 5); ascending in r, linear, every row once.
constexpr US_HD int mfma32_row(int r, int kl) { return 8 * (r >> 2) + 4 * kl + (r & 3); }
}  // namespace us
