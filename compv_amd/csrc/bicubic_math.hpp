// bicubic_math.hpp -- the per-pixel arithmetic of the bicubic interpolation (include/compv_hip.h, "remap and inverse warp", paragraph F), written once
// for remap_bicubic_kernel of remap_kernels.hip and the host checker (tests/host/bicubic_math_check.cpp).  It takes clamped taps and fractions, so a
// table-driven caller (a bicubic scale) can use it as it stands.
// Every operation is a single IEEE binary32 operation in the order of the definition: the translation units are built with -ffp-contract=off, and
// nothing here may be fused.  Standard library only.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define BICUBIC_HD __host__ __device__ __forceinline__
#else
#define BICUBIC_HD inline
#endif

namespace compvhip {
namespace bicubic {

// COMPV_MATH_CLIP3(0, hi, v) on a tap index: compv_image_scale_bicubic.cxx:73-80
BICUBIC_HD int clamp_tap(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// Where the kernel reads a tap row as ONE 4-byte word: at quad_base(x_0, W).  Tap k is byte x_k - base of it, 0 .. 3 at both clamps (x_k <= x_0 + 3, and
// W - 1 - (W - 4) = 3); base + 3 <= max(W - 1, 3), inside a row of stride >= 4.
BICUBIC_HD int quad_base(int x0, int W) { const int m = W > 4 ? W - 4 : 0; return x0 < m ? x0 : m; }

// integer part by truncation, fraction against floorf (compv_image_remap.cxx:293-297); t2 = t * t, t3 = t2 * t (compv_image_scale_bicubic.cxx:89-92)
BICUBIC_HD void split(float v, int& i, float& t, float& t2, float& t3)
{
	i = static_cast<int>(v);
	t = v - floorf(v);
	t2 = t * t;
	t3 = t2 * t;
}

// HERMITE4_32F_C (compv_image_scale_bicubic.cxx:34-43): the four taps of one source row
BICUBIC_HD float hermite_row(float A, float B, float C, float D, float t, float t2, float t3)
{
	const float a = ((D - A) * 0.5f) + ((B - C) * 1.5f);
	const float b = ((A + (B * -2.5f)) + (C * 2.0f)) + (D * -0.5f);
	const float c = (C - A) * 0.5f;
	return ((a * t3) + (c * t)) + ((b * t2) + B);
}

// HERMITE1_32F_C (:44-53): the four row values.  The same polynomial in another association: the two differ in the last place.
BICUBIC_HD float hermite_col(float A, float B, float C, float D, float t, float t2, float t3)
{
	const float a = ((A * -0.5f) + (B * 1.5f)) + ((C * -1.5f) + (D * 0.5f));
	const float b = (A + (B * -2.5f)) + ((C * 2.0f) + (D * -0.5f));
	const float c = (A * -0.5f) + (C * 0.5f);
	return ((a * t3) + (c * t)) + ((b * t2) + B);
}

// COMPV_MATH_CLIP3(0, 255, v) with compares, not fminf / fmaxf: a zero keeps its sign, a NaN passes
BICUBIC_HD float clip255(float v) { return v < 0.f ? 0.f : (v > 255.f ? 255.f : v); }

// the uint8 output: truncation of the clipped value (compv_math_cast.cxx:215)
BICUBIC_HD uint8_t to_u8(float clipped) { return static_cast<uint8_t>(static_cast<int>(clipped)); }

} // namespace bicubic
} // namespace compvhip
