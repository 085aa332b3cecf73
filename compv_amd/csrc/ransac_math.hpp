// ransac_math.hpp -- what the RANSAC families (homography_math.hpp, curvefit_math.hpp) share on the host and on the device, standard library only: the
// correctly rounded scalar operations, the sample generator, the rule that selects the best try and the fold of the 64 partials of a sum64.
#pragma once
#include <float.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define HG_HD __host__ __device__ __forceinline__
#define HG_UNROLL _Pragma("unroll")
#else
#include <cmath>
#define HG_HD inline
#define HG_UNROLL
#endif

namespace compvhip {
namespace ransac {

constexpr int kQuadDraws = 64;

HG_HD double ddiv(double a, double b)
{
#if defined(__HIP_DEVICE_COMPILE__)
	return __ddiv_rn(a, b);
#else
	return a / b;
#endif
}
HG_HD double dsqrt(double a)
{
#if defined(__HIP_DEVICE_COMPILE__)
	return __dsqrt_rn(a);
#else
	return sqrt(a);
#endif
}
HG_HD double dabs(double a) { return __builtin_fabs(a); }

// ---- samples ---------------------------------------------------------------------------------------------------------------------------
HG_HD uint32_t lowbias32(uint32_t x)
{
	x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
	return x;
}
// the M distinct indices of set (pair) p, try t among k >= M points: the generator of the homography's quads (M = 4) and of the curve fits' samples
// (M = 2 or 3).  The slots are addressed by compile-time indices only, so q stays in registers.
template <int M>
HG_HD void drawDistinct(uint32_t seed, uint32_t p, uint32_t t, uint32_t k, int32_t q[M])
{
	const uint32_t base = lowbias32(lowbias32(seed ^ p) + t);
	int filled = 0;
HG_UNROLL
	for (int j = 0; j < M; ++j) q[j] = -1;
	for (int c = 0; c < kQuadDraws && filled < M; ++c) {
		const int32_t idx = (int32_t)(((uint64_t)lowbias32(base + (uint32_t)c) * k) >> 32);
		bool seen = false;
HG_UNROLL
		for (int j = 0; j < M; ++j) seen = seen || (j < filled && q[j] == idx);
		if (!seen) {
HG_UNROLL
			for (int j = 0; j < M; ++j) if (j == filled) q[j] = idx;
			++filled;
		}
	}
	for (int32_t idx = 0; filled < M; ++idx) {          // 64 draws did not fill the slots: the smallest unused indices
		bool seen = false;
HG_UNROLL
		for (int j = 0; j < M; ++j) seen = seen || (j < filled && q[j] == idx);
		if (!seen) {
HG_UNROLL
			for (int j = 0; j < M; ++j) if (j == filled) q[j] = idx;
			++filled;
		}
	}
}

// ---- selection ---------------------------------------------------------------------------------------------------------------------------
// A try is ranked by its inlier count, its variance V (double: the homography; NoVariance: the curve fits, whose rule has no such term and whose
// selection then carries no double) and its index.
struct NoVariance {};
HG_HD bool varianceLess(double a, double b) { return a < b; }
HG_HD bool varianceLess(NoVariance, NoVariance) { return false; }

// (count, variance, try) b beats a among tries of a model of m points: a count below m never wins; then the larger count, the smaller variance
// (either way round by <: a NaN decides nothing), the smaller try index
template <typename V>
HG_HD bool better(int m, int cb, V vb, int tb, int ca, V va, int ta)
{
	if (cb < m) return false;
	if (ca < m) return true;
	if (cb != ca) return cb > ca;
	if (varianceLess(vb, va)) return true;
	if (varianceLess(va, vb)) return false;
	return tb < ta;
}

// ---- sum64 -------------------------------------------------------------------------------------------------------------------------------
// the fold of the 64 partials as an array (partial l is the sum of the terms l, l + 64, ...), in the order of the device's wave_fold64; p is destroyed
HG_HD double fold64(double* p)
{
	for (int stride = 32; stride > 0; stride >>= 1)
		for (int l = 0; l < stride; ++l) p[l] += p[l + stride];
	return p[0];
}

} // namespace ransac
} // namespace compvhip
