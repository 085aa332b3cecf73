// homography_math.hpp -- the scalar arithmetic of the RANSAC homography (include/compv_hip.h, "RANSAC homography", items A - H), written once for the
// kernels of homography_kernels.hip and for the host (compvhip_homography_quads).  Every operation is one IEEE binary64 operation in the order the
// definition gives; divisions and square roots are the correctly rounded ones on either side, nothing is transcendental.  The 9 x 9 matrices are
// addressed as M[e * ST]: ST = 64 interleaves the matrices of a wave's lanes in LDS (lane-consecutive words, no bank conflict whatever the pivot),
// ST = 1 is a plain array.  The scalar operations, the sample generator (drawDistinct) and the selection rule are ransac_math.hpp's; the half-angle
// formulas (halfAngle) also serve the curve fits (curvefit_math.hpp).
#pragma once
#include "ransac_math.hpp"

namespace compvhip {
namespace hg {

// (named one by one: the selection rule and the array fold stay ransac::better and ransac::fold64, so a program that defines its own is not disturbed)
using ransac::dabs;
using ransac::ddiv;
using ransac::drawDistinct;
using ransac::dsqrt;
using ransac::kQuadDraws;
using ransac::lowbias32;

constexpr double kEps = 2.220446049250313e-16;          // 2^-52
constexpr double kSqrt2 = 1.4142135623730950488016887242097;
constexpr double kCosPi4 = 0.70710678118654757;
constexpr int kMaxRotations = 9 * 9 * 30;

// ---- A. quads ---------------------------------------------------------------------------------------------------------------------------
// the four indices of pair p, try t among k >= 4 points
HG_HD void quad(uint32_t seed, uint32_t p, uint32_t t, uint32_t k, int32_t q[4]) { drawDistinct<4>(seed, p, t, k, q); }

// ---- B. collinearity of the quad's source points ---------------------------------------------------------------------------------------
HG_HD bool collinear4(const double x[4], const double y[4])
{
	if (x[0] == x[1]) return x[0] == x[2] && x[0] == x[3];
	const double slope = ddiv(y[1] - y[0], x[1] - x[0]);
	const double intercept = y[0] - slope * x[0];
	return y[2] == slope * x[2] + intercept && y[3] == slope * x[3] + intercept;
}

// ---- C. Hartley normalisation and the rows of M -------------------------------------------------------------------------------------------
struct Norm { double tx, ty, s; };
HG_HD double scaleOf(double mean) { return mean != 0.0 ? ddiv(kSqrt2, mean) : kSqrt2; }
HG_HD double hypotNaive(double a, double b) { return dsqrt(a * a + b * b); }
HG_HD Norm norm4(const double x[4], const double y[4])
{
	Norm n;
	const double inv = ddiv(1.0, 4.0);
	n.tx = (((x[0] + x[1]) + x[2]) + x[3]) * inv;
	n.ty = (((y[0] + y[1]) + y[2]) + y[3]) * inv;
	double mag = hypotNaive(x[0] - n.tx, y[0] - n.ty);
	mag += hypotNaive(x[1] - n.tx, y[1] - n.ty);
	mag += hypotNaive(x[2] - n.tx, y[2] - n.ty);
	mag += hypotNaive(x[3] - n.tx, y[3] - n.ty);
	n.s = scaleOf(mag * inv);
	return n;
}
HG_HD double normalised(double v, double t, double s) { return s * v + (-(t * s)); }
// the two rows a correspondence (x, y) -> (X, Y) of normalised points contributes to M
HG_HD void rowsOf(double x, double y, double X, double Y, double m0[9], double m1[9])
{
	m0[0] = -x; m0[1] = -y; m0[2] = -1.0; m0[3] = 0.0; m0[4] = 0.0; m0[5] = 0.0; m0[6] = X * x; m0[7] = X * y; m0[8] = X;
	m1[0] = 0.0; m1[1] = 0.0; m1[2] = 0.0; m1[3] = -x; m1[4] = -y; m1[5] = -1.0; m1[6] = Y * x; m1[7] = Y * y; m1[8] = Y;
}
// acc[a * 9 + b] (b <= a) += the correspondence's two products, row 0 first; S is symmetric bit for bit (the products commute)
HG_HD void accumulateS(const double m0[9], const double m1[9], double acc[45])
{
	int e = 0;
HG_UNROLL
	for (int a = 0; a < 9; ++a) {
HG_UNROLL
		for (int b = 0; b <= a; ++b) {
			acc[e] += m0[a] * m0[b];
			acc[e] += m1[a] * m1[b];
			++e;
		}
	}
}
// D = S (both triangles) from the 45 accumulators, Q = I
template <int ST>
HG_HD void storeS(const double acc[45], double* D, double* Q)
{
	int e = 0;
HG_UNROLL
	for (int a = 0; a < 9; ++a) {
HG_UNROLL
		for (int b = 0; b <= a; ++b) {
			D[(a * 9 + b) * ST] = acc[e];
			D[(b * 9 + a) * ST] = acc[e];
			++e;
		}
	}
	for (int i = 0; i < 81; ++i) Q[i * ST] = (i % 10 == 0) ? 1.0 : 0.0;
}

// ---- D. Jacobi ---------------------------------------------------------------------------------------------------------------------------
// (cos, sin) of atan2(y, x) / 2 by the half-angle formulas, (x, y) != (0, 0); also the angle of the curve fits' total least squares line
HG_HD void halfAngle(double y, double x, double* cs, double* sn)
{
	const double rho = dsqrt(x * x + y * y);
	const double c2 = ddiv(x, rho), s2 = ddiv(y, rho);
	if (c2 >= 0.0) {
		*cs = dsqrt((1.0 + c2) * 0.5);
		*sn = ddiv(s2, 2.0 * *cs);
	}
	else {
		const double mag = dsqrt((1.0 - c2) * 0.5);
		*sn = (s2 == 0.0 || s2 > 0.0) ? mag : -mag;          // copysign(mag, s2), a zero s2 counting as positive
		*cs = ddiv(s2, 2.0 * *sn);
	}
}
template <int ST>
HG_HD void rotateRows(double* A, int r, int c, double cs, double sn)
{
	for (int j = 0; j < 9; ++j) {
		const double ri = A[(r * 9 + j) * ST], rj = A[(c * 9 + j) * ST];
		A[(r * 9 + j) * ST] = ri * cs + (-sn) * rj;
		A[(c * 9 + j) * ST] = ri * sn + cs * rj;
	}
}
template <int ST>
HG_HD void rotateCols(double* A, int r, int c, double cs, double sn)
{
	for (int i = 0; i < 9; ++i) {
		const double ri = A[(i * 9 + r) * ST], rj = A[(i * 9 + c) * ST];
		A[(i * 9 + r) * ST] = ri * cs + (-sn) * rj;
		A[(i * 9 + c) * ST] = ri * sn + cs * rj;
	}
}
// diagonalises D in place, accumulates the rotations in the rows of Q; returns the number of rotations
template <int ST>
HG_HD int jacobi(double* D, double* Q)
{
	int rotations = 0;
	for (;;) {
		int pr = 1, pc = 0;
		double best = dabs(D[(1 * 9 + 0) * ST]);
		for (int r = 1; r < 9; ++r) {
			for (int c = 0; c < r; ++c) {
				const double v = dabs(D[(r * 9 + c) * ST]);
				if (v > best) { best = v; pr = r; pc = c; }
			}
		}
		if (!(best > kEps) || rotations >= kMaxRotations) break;
		const double drr = D[(pr * 9 + pr) * ST], dcc = D[(pc * 9 + pc) * ST];
		double cs, sn;
		if (drr == dcc) { cs = kCosPi4; sn = kCosPi4; }
		else {
			halfAngle(2.0 * D[(pr * 9 + pc) * ST], dcc - drr, &cs, &sn);
		}
		rotateRows<ST>(Q, pr, pc, cs, sn);
		rotateRows<ST>(D, pr, pc, cs, sn);
		rotateCols<ST>(D, pr, pc, cs, sn);
		++rotations;
	}
	return rotations;
}

HG_HD double dot3(double a0, double a1, double a2, double b0, double b1, double b2) { return (a0 * b0 + a1 * b1) + a2 * b2; }

// h = the row of Q at the smallest diagonal entry of D; de-normalised with the two sides' normalisations; optional promotion; scaled by 1 / h22
template <int ST>
HG_HD void finishH(const double* D, const double* Q, Norm a, Norm b, bool promote, double H[9])
{
	int idx = 8;
	double least = D[(8 * 9 + 8) * ST];
	for (int j = 7; j >= 0; --j) {
		const double v = D[(j * 9 + j) * ST];
		if (v < least) { least = v; idx = j; }
	}
	double hn[9];
HG_UNROLL
	for (int j = 0; j < 9; ++j) hn[j] = Q[(idx * 9 + j) * ST];
	// T1 = {s, 0, 0; 0, s, 0; -tx * s, -ty * s, 1}; M = T1 * Hn^t
	const double t1[9] = { a.s, 0.0, 0.0, 0.0, a.s, 0.0, -a.tx * a.s, -a.ty * a.s, 1.0 };
	double m[9];
HG_UNROLL
	for (int i = 0; i < 3; ++i) {
HG_UNROLL
		for (int j = 0; j < 3; ++j) m[i * 3 + j] = dot3(t1[i * 3], t1[i * 3 + 1], t1[i * 3 + 2], hn[j * 3], hn[j * 3 + 1], hn[j * 3 + 2]);
	}
	// T2 = {1 / s, 0, tx; 0, 1 / s, ty; 0, 0, 1}; H = T2 * M^t
	const double is = ddiv(1.0, b.s);
	const double t2[9] = { is, 0.0, b.tx, 0.0, is, b.ty, 0.0, 0.0, 1.0 };
HG_UNROLL
	for (int i = 0; i < 3; ++i) {
HG_UNROLL
		for (int j = 0; j < 3; ++j) H[i * 3 + j] = dot3(t2[i * 3], t2[i * 3 + 1], t2[i * 3 + 2], m[j * 3], m[j * 3 + 1], m[j * 3 + 2]);
	}
	if (promote) {
HG_UNROLL
		for (int j = 0; j < 8; ++j) if (dabs(H[j]) <= kEps) H[j] = 0.0;
	}
	if (H[8] != 0.0) {
		const double s = ddiv(1.0, H[8]);
HG_UNROLL
		for (int j = 0; j < 9; ++j) H[j] *= s;
	}
}

// computeH of four correspondences (sums in index order); D, Q: 81 words each at stride ST.  Returns the rotation count.
template <int ST>
HG_HD int computeH4(const double sx[4], const double sy[4], const double dx[4], const double dy[4], double* D, double* Q, bool promote, double H[9])
{
	const Norm a = norm4(sx, sy), b = norm4(dx, dy);
	double acc[45];
HG_UNROLL
	for (int e = 0; e < 45; ++e) acc[e] = 0.0;
HG_UNROLL
	for (int i = 0; i < 4; ++i) {
		double m0[9], m1[9];
		rowsOf(normalised(sx[i], a.tx, a.s), normalised(sy[i], a.ty, a.s), normalised(dx[i], b.tx, b.s), normalised(dy[i], b.ty, b.s), m0, m1);
		accumulateS(m0, m1, acc);
	}
	storeS<ST>(acc, D, Q);
	const int rotations = jacobi<ST>(D, Q);
	finishH<ST>(D, Q, a, b, promote, H);
	return rotations;
}

// ---- E. inverse and distance -----------------------------------------------------------------------------------------------------------
HG_HD bool inverse3(const double a[9], double r[9])
{
	const double det = (a[0] * (a[4] * a[8] - a[7] * a[5]) - a[3] * (a[1] * a[8] - a[7] * a[2])) + a[6] * (a[1] * a[5] - a[4] * a[2]);
	if (det == 0.0) return false;
	const double d = ddiv(1.0, det);
	r[0] = ((a[4] * a[8]) - (a[7] * a[5])) * d;
	r[1] = ((a[2] * a[7]) - (a[8] * a[1])) * d;
	r[2] = ((a[1] * a[5]) - (a[4] * a[2])) * d;
	r[3] = ((a[5] * a[6]) - (a[8] * a[3])) * d;
	r[4] = ((a[0] * a[8]) - (a[6] * a[2])) * d;
	r[5] = ((a[2] * a[3]) - (a[5] * a[0])) * d;
	r[6] = ((a[3] * a[7]) - (a[6] * a[4])) * d;
	r[7] = ((a[1] * a[6]) - (a[7] * a[0])) * d;
	r[8] = ((a[0] * a[4]) - (a[3] * a[1])) * d;
	return true;
}
// mse(A * (ax, ay, 1), (bx, by))
HG_HD double mseThrough(const double A[9], double ax, double ay, double bx, double by)
{
	const double X = dot3(A[0], A[1], A[2], ax, ay, 1.0), Y = dot3(A[3], A[4], A[5], ax, ay, 1.0), Z = dot3(A[6], A[7], A[8], ax, ay, 1.0);
	const double scale = ddiv(1.0, Z);
	const double ex = X * scale - bx, ey = Y * scale - by;
	return ex * ex + ey * ey;
}
HG_HD double distance(const double H[9], const double Hinv[9], double sx, double sy, double dx, double dy)
{
	return mseThrough(H, sx, sy, dx, dy) + mseThrough(Hinv, dx, dy, sx, sy);
}

// ---- H. projection ------------------------------------------------------------------------------------------------------------------------
HG_HD void project(const double H[9], double x, double y, double* ox, double* oy)
{
	const double X = dot3(H[0], H[1], H[2], x, y, 1.0), Y = dot3(H[3], H[4], H[5], x, y, 1.0), Z = dot3(H[6], H[7], H[8], x, y, 1.0);
	const double s = ddiv(1.0, Z);
	*ox = X * s; *oy = Y * s;
}

} // namespace hg
} // namespace compvhip
