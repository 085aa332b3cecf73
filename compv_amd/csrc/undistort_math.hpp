// undistort_math.hpp -- the arithmetic of the lens distortion model (include/compv_hip.h, "lens undistortion"): CompVCalibUtils::initUndistMap,
// dist2DPoints and proj2D of the reference (core/calib/compv_core_calib_utils.cxx), written once for remap_coords<kRemapUndist> of remap_kernels.hip,
// the kernels of undistort_kernels.hip, the host entry points (api_undistort.cpp) and the host checker (tests/host/undistort_math_check.cpp).
// T is float or double.  Every operation is a single IEEE operation in T in the order of the definition: the translation units are built with
// -ffp-contract=off, and nothing here may be fused.  Standard library only.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define UNDIST_HD __host__ __device__ __forceinline__
#else
#define UNDIST_HD inline
#endif

namespace compvhip {
namespace undist {

// the coefficient record of one camera: 14 values of T
enum { kFx = 0, kFy, kCx, kCy, kSkew, kK1, kK2, kP1, kP2, kInv11, kInv21, kInv31, kInv22, kInv32, kCoeffs };
constexpr int kPose = 12;          // a pose of proj2D: R row-major (9), then t (3)

// K: 3 x 3 row-major (fx, skew, cx, fy, cy are read); d: nd in 2 .. 4 values k1, k2[, p1[, p2]].  false: nd outside 2 .. 4 or fx * fy == 0 (c untouched).
template <typename T>
UNDIST_HD bool coeffs(const T* K, const T* d, int nd, T* c)
{
	if (nd < 2 || nd > 4) return false;
	const T fx = K[0], skew = K[1], cx = K[2], fy = K[4], cy = K[5];
	const T prod = fx * fy;
	if (prod == static_cast<T>(0)) return false;
	const T det = static_cast<T>(1) / prod;
	c[kFx] = fx; c[kFy] = fy; c[kCx] = cx; c[kCy] = cy; c[kSkew] = skew;
	c[kK1] = d[0]; c[kK2] = d[1]; c[kP1] = nd > 2 ? d[2] : static_cast<T>(0); c[kP2] = nd > 3 ? d[3] : static_cast<T>(0);
	c[kInv11] = fy * det;
	c[kInv21] = -(skew * det);
	c[kInv31] = ((skew * cy) - (fy * cx)) * det;
	c[kInv22] = fx * det;
	c[kInv32] = -((cy * fx) * det);
	return true;
}

// Distort: normalised (x, y) -> pixel (u, v)
template <typename T>
UNDIST_HD void distort(const T* c, T x, T y, T& u, T& v)
{
	const T one = static_cast<T>(1), two = static_cast<T>(2);
	const T x2 = x * x, y2 = y * y, r2 = x2 + y2, r4 = r2 * r2;
	const T rdist = (one + (c[kK1] * r2)) + (c[kK2] * r4);
	x = x * rdist; y = y * rdist;
	const T a1 = two * (x * y);          // the scaled x, y
	const T a2 = r2 + (two * x2), a3 = r2 + (two * y2);          // the unscaled squares
	x = x + ((c[kP1] * a1) + (c[kP2] * a2));
	y = y + ((c[kP1] * a3) + (c[kP2] * a1));
	u = ((x * c[kFx]) + (c[kSkew] * y)) + c[kCx];
	v = (y * c[kFy]) + c[kCy];
}

// the map entry of pixel (X, Y) and dist2DPoints of the point (X, Y): Kinv, then Distort
template <typename T>
UNDIST_HD void map_entry(const T* c, T X, T Y, T& u, T& v)
{
	const T x = ((c[kInv11] * X) + (c[kInv21] * Y)) + c[kInv31];
	const T y = (c[kInv22] * Y) + c[kInv32];
	distort(c, x, y, u, v);
}

// proj2D of (xp, yp, zp) under the pose Rt: no Kinv step; z == 0 keeps x and y (s = 1)
UNDIST_HD void project(const double* c, const double* Rt, double xp, double yp, double zp, double& u, double& v)
{
	double x = (((Rt[0] * xp) + (Rt[1] * yp)) + (Rt[2] * zp)) + Rt[9];
	double y = (((Rt[3] * xp) + (Rt[4] * yp)) + (Rt[5] * zp)) + Rt[10];
	const double z = (((Rt[6] * xp) + (Rt[7] * yp)) + (Rt[8] * zp)) + Rt[11];
	const double s = z != 0.0 ? 1.0 / z : 1.0;          // a NaN z is "not zero", as in the reference's `z ? ...`
	x = x * s; y = y * s;
	distort(c, x, y, u, v);
}

} // namespace undist
} // namespace compvhip
