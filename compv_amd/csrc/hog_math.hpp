// hog_math.hpp -- the scalar arithmetic of the HOG descriptor (include/compv_hip.h, "HOG descriptors", items 1 - 4, 6 and 7), written once for the kernels
// of hog_kernels.hip and for the host checker (tests/host/hog_math_check.cpp); nothing else uses it.  Every operation is one IEEE binary32 operation in
// the order the definition gives (the translation units are built with -ffp-contract=off); the division and the square root are the correctly rounded
// ones on either side, nothing is flushed to zero, nothing is transcendental.  Standard library only.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define HOG_HD __host__ __device__ __forceinline__
#else
#include <cmath>
#define HOG_HD inline
#endif

namespace compvhip {
namespace hog {

// = COMPVHIP_HOG_NORM_* / COMPVHIP_HOG_INTERP_* of include/compv_hip.h after the defaults are resolved
enum { kNormNone = 1, kNormL1 = 2, kNormL1Sqrt = 3, kNormL2 = 4, kNormL2Hys = 5 };
enum { kInterpNearest = 1, kInterpBilinear = 2 };

constexpr float kAtanEps = static_cast<float>(2.2204460492503131e-16);   // compv_math.cxx:39
constexpr float kAtanP1 = 57.2836266f, kAtanP3 = -18.6674461f, kAtanP5 = 8.91400051f, kAtanP7 = -2.53972459f;   // :40-43
constexpr float kNormEps = 1e-6f;                                          // hog_std.cxx:96
constexpr float kHysMax = 0.2f;

// Division and square root are the language's own on both sides: hipcc compiles float32 `/` and sqrtf correctly rounded by default
// (-fhip-fp32-correctly-rounded-divide-sqrt: v_div_scale / v_div_fmas / v_div_fixup, and v_sqrt_f32 followed by its one-ulp correction), with denormals
// kept (float_denorm_mode_32 = 3).  NOT __fsqrt_rn: in this ROCm's headers it is the native, approximate square root (docs/kernels/hog.md).
HOG_HD float fdiv(float a, float b) { return a / b; }
HOG_HD float fsqrt(float a) { return __builtin_sqrtf(a); }
HOG_HD float fabs32(float a) { return __builtin_fabsf(a); }

// ---- 1. gradient: the four neighbours of a pixel; onColumnBorder: x == 0 or x == W - 1, onRowBorder likewise ------------------------------------------
HOG_HD void gradient(int left, int right, int up, int down, bool onColumnBorder, bool onRowBorder, float& gx, float& gy)
{
	gx = onColumnBorder ? 0.f : static_cast<float>(right - left);
	gy = onRowBorder ? 0.f : static_cast<float>(down - up);
}

// ---- 2. magnitude -------------------------------------------------------------------------------------------------------------------------------------
HOG_HD float magnitude(float gx, float gy) { return fsqrt(gx * gx + gy * gy); }

// ---- 3. direction in degrees, [0, 360] ----------------------------------------------------------------------------------------------------------------
HOG_HD float direction(float gx, float gy)
{
	const float ax = fabs32(gx), ay = fabs32(gy);
	const bool flat = ax >= ay;
	const float c = fdiv(flat ? ay : ax, (flat ? ax : ay) + kAtanEps);
	const float c2 = c * c;
	const float p = (((kAtanP7 * c2 + kAtanP5) * c2 + kAtanP3) * c2 + kAtanP1) * c;
	float a = flat ? p : 90.f - p;
	if (gx < 0.f) a = 180.f - a;
	if (gy < 0.f) a = 360.f - a;
	return a;
}

// ---- 4. binning -----------------------------------------------------------------------------------------------------------------------------------------
struct Binning {
	float thetaMax, w, s;   // 360 or 180; the bin width in degrees (an integer: nbins divides thetaMax); 1.f / w
	int nbins;
};
HOG_HD Binning binning(int nbins, bool gradientSigned)
{
	Binning q;
	const int thetaMax = gradientSigned ? 360 : 180;
	q.thetaMax = static_cast<float>(thetaMax);
	q.w = static_cast<float>(thetaMax / nbins);
	q.s = fdiv(1.f, q.w);
	q.nbins = nbins;
	return q;
}
// One pixel's vote into its cell's histogram.  Hist: float& operator[](int bin).  The ORDER of the two BILINEAR additions is part of the result.
template <int INTERP, typename Hist>
HOG_HD void vote(Hist& h, const Binning& q, float m, float a)
{
	const float theta = a > q.thetaMax ? a - q.thetaMax : a;
	if (INTERP == kInterpNearest) {
		const int b = static_cast<int>(theta * q.s);
		if (b >= 0 && b < q.nbins) h[b] = h[b] + m;          // b == nbins (theta == thetaMax): dropped
	}
	else {
		int b = static_cast<int>(theta * q.s - 0.5f);          // truncation; 0 <= b <= nbins - 1 for every theta in [0, thetaMax] ...
		b = b < 0 ? 0 : (b > q.nbins - 1 ? q.nbins - 1 : b);    // ... so this changes no value; it keeps an index inside the histogram whatever comes in
		const float d = (theta - static_cast<float>(b) * q.w) * q.s - 0.5f;
		const float v = fabs32(m * d);
		int other = d >= 0.f ? b + 1 : b - 1;
		other = other < 0 ? q.nbins - 1 : (other > q.nbins - 1 ? 0 : other);
		h[other] = h[other] + v;          // first the neighbour ...
		h[b] = h[b] + (m - v);            // ... then the pixel's own bin
	}
}

// ---- 6. the elements of one block: element i lies in cell row i / rowLen of the block, at float i % rowLen of that row's cpbX adjacent cells -------------------
struct BlockLoad {
	const float* first;     // the block's first cell in the map
	int rowLen, rowStride;  // cpbX * nbins; cellsX * nbins
	HOG_HD float operator()(int i) const
	{
		const int r = i / rowLen;
		return first[static_cast<long long>(r) * rowStride + (i - r * rowLen)];
	}
};

// ---- 7. norms -------------------------------------------------------------------------------------------------------------------------------------------
// The summation order of the reference's SSE2 leaf for `count` terms t(0) .. t(count - 1): accumulator lane l (0 .. 3) of acc0 takes the terms 8k + l, of acc1
// the terms 8k + 4 + l; one more group of 4 goes to acc0 if it fits; the lanes are added acc0 + acc1, then (l0 + l2) + (l1 + l3); the remaining terms follow
// one by one.  lane_partial is what lane l holds after acc0 + acc1, ordered_sum the rest: the blocks kernel gives one GPU lane to each accumulator lane.
template <typename Term>
HOG_HD float lane_partial(const Term& t, int count, int l)
{
	const int c8 = count & ~7, c4 = count & ~3;
	float acc0 = 0.f, acc1 = 0.f;
	for (int i = 0; i < c8; i += 8) { acc0 = acc0 + t(i + l); acc1 = acc1 + t(i + 4 + l); }
	if (c4 > c8) acc0 = acc0 + t(c8 + l);
	return acc0 + acc1;
}
template <typename Term>
HOG_HD float ordered_sum(float l0, float l1, float l2, float l3, const Term& t, int count)
{
	float s = (l0 + l2) + (l1 + l3);
	for (int i = count & ~3; i < count; ++i) s = s + t(i);
	return s;
}
// the terms of the three sums: the value (L1, L1SQRT), its square (L2, the first pass of L2HYS), the square of the clipped first-pass result (L2HYS)
template <typename Load> struct TermValue { const Load& v; HOG_HD float operator()(int i) const { return v(i); } };
template <typename Load> struct TermSquare { const Load& v; HOG_HD float operator()(int i) const { const float x = v(i); return x * x; } };
HOG_HD float clip(float x) { return x < kHysMax ? x : kHysMax; }
template <typename Load> struct TermClippedSquare { const Load& v; float r; HOG_HD float operator()(int i) const { const float x = clip(v(i) * r); return x * x; } };

HOG_HD bool norm_is_l2(int norm) { return norm == kNormL2 || norm == kNormL2Hys; }
// the factor of a sum: 1 / (sum + eps), or 1 / sqrt(sum + eps * eps)
HOG_HD float norm_factor(float sum, int norm)
{
	return norm_is_l2(norm) ? fdiv(1.f, fsqrt(sum + kNormEps * kNormEps)) : fdiv(1.f, sum + kNormEps);
}
// the descriptor's value of block element x; r: the factor of the (first) sum, r2: of L2HYS's second
HOG_HD float norm_value(float x, int norm, float r, float r2)
{
	if (norm == kNormNone) return x;
	if (norm == kNormL1Sqrt) return fsqrt(x * r);
	if (norm == kNormL2Hys) return clip(x * r) * r2;
	return x * r;
}

// The whole of item 7 for one block in sequence (the host checker; the blocks kernel does the same with four lanes): out[i] for i < count.
template <typename Load>
HOG_HD void normalize_block(const Load& v, int count, int norm, float* out)
{
	float r = 0.f, r2 = 0.f;
	if (norm != kNormNone) {
		if (norm_is_l2(norm)) {
			const TermSquare<Load> t{v};
			r = norm_factor(ordered_sum(lane_partial(t, count, 0), lane_partial(t, count, 1), lane_partial(t, count, 2), lane_partial(t, count, 3), t, count), norm);
		}
		else {
			const TermValue<Load> t{v};
			r = norm_factor(ordered_sum(lane_partial(t, count, 0), lane_partial(t, count, 1), lane_partial(t, count, 2), lane_partial(t, count, 3), t, count), norm);
		}
		if (norm == kNormL2Hys) {
			const TermClippedSquare<Load> t{v, r};
			r2 = norm_factor(ordered_sum(lane_partial(t, count, 0), lane_partial(t, count, 1), lane_partial(t, count, 2), lane_partial(t, count, 3), t, count), norm);
		}
	}
	for (int i = 0; i < count; ++i) out[i] = norm_value(v(i), norm, r, r2);
}

} // namespace hog
} // namespace compvhip
