// curvefit_math.hpp -- the scalar arithmetic of the RANSAC line and parabola fits (include/compv_hip.h, "RANSAC curve fitting", items A - G), written once
// for the kernels of curvefit_kernels.hip, for the host (compvhip_curvefit_samples) and for the host checker tests/host/curvefit_math_check.cpp.  Standard
// library only.  Every operation is one IEEE binary64 operation in the order the definition gives (build with -ffp-contract=off); divisions and square
// roots are the correctly rounded ones on either side, nothing is transcendental.  The sample generator and the selection rule are ransac_math.hpp's,
// the half-angle formulas the homography's (homography_math.hpp): one copy serves both families.
//
// A. Samples.  m = 2 (line) or 3 (parabolas) distinct indices of set s, try t among k > m points: ransac::drawDistinct<m>(seed, s, t, k).
// B. Model of a sample, every expression as the reference writes it (compv_math_stats_fit.cxx:156-168, :252-266):
//      line      rejected when x0 == x1 && y0 == y1;  A = y1 - y0, B = x0 - x1, C = (x1 * y0) - (x0 * y1)                          (Ax + By + C = 0)
//      parabola  rejected when two of x1, x2, x3 are equal;  scale = 1 / (((x1 - x2) * (x1 - x3)) * (x2 - x3));                 (y = Ax^2 + Bx + C)
//                A = (((x3 * (y2 - y1)) + (x2 * (y1 - y3))) + (x1 * (y3 - y2))) * scale
//                B = (((x3 * x3) * (y1 - y2) + (x2 * x2) * (y3 - y1)) + (x1 * x1) * (y2 - y3)) * scale
//                C = (((((x2 * x3) * (x2 - x3)) * y1) + (((x3 * x1) * (x3 - x1)) * y2)) + (((x1 * x2) * (x1 - x2)) * y3)) * scale
//      sideways  the parabola with x and y of every point exchanged.
// C. Residual (compv_math_distance.cxx:263-268, :242, :343):
//      line      s = 1 / sqrt(A * A + B * B);  d = |((A * s) * x + (C * s)) + (B * s) * y|
//      parabola  d = |(((A * (x * x)) + C) + (B * x)) - y|
//    inlier iff d < threshold (strict; a NaN never is).
// E. Refit of n > m points, every sum a sum64 (homography item C), mean = sum * (1 / n):
//      line      a = x - mean_x, b = y - mean_y;  num = (sum a * b) * -2;  den = sum (b * b - a * a);  num == 0 && den == 0: (cos, sin) = (1, 0), else
//                hg::halfAngle(num, den);  A = cos, B = sin, C = -((mean_x * cos) + (mean_y * sin))
//      parabola  u = x - mean;  S1..S4 = sum u, u * u, (u * u) * u, (u * u) * (u * u);  T0..T2 = sum y, u * y, (u * u) * y;  the symmetric system
//                {S4, S3, S2; S3, S2, S1; S2, S1, n} (a, b, c) = (T2, T1, T0) by cofactors (parabolaFromSums below is the definition), one division by
//                the determinant per unknown; a determinant that is 0 or not finite: the refit fails.  A = a, B = b - (2 * a) * mean,
//                C = (c - b * mean) + a * (mean * mean).
#pragma once
#include "homography_math.hpp"

#define CF_HD HG_HD

namespace compvhip {
namespace cf {

using ransac::dabs;
using ransac::ddiv;
using ransac::drawDistinct;
using ransac::dsqrt;

constexpr int kLine = 0, kParabola = 1, kParabolaSideways = 2;          // COMPVHIP_CURVEFIT_LINE, _PARABOLA, _PARABOLA_SIDEWAYS
constexpr int kModels = 3;

struct Curve { double A, B, C; };

CF_HD int modelPoints(int model) { return model == kLine ? 2 : 3; }
// the coordinate a model takes for its x / its y of the point (px, py)
CF_HD double xOf(int model, double px, double py) { return model == kParabolaSideways ? py : px; }
CF_HD double yOf(int model, double px, double py) { return model == kParabolaSideways ? px : py; }

// ---- A. samples ------------------------------------------------------------------------------------------------------------------------------
// the m indices of set s, try t among k > m points; q[2] of a line is 0
CF_HD void sample(int model, uint32_t seed, uint32_t s, uint32_t t, uint32_t k, int32_t q[3])
{
	if (model == kLine) { drawDistinct<2>(seed, s, t, k, q); q[2] = 0; }
	else drawDistinct<3>(seed, s, t, k, q);
}

// ---- B. model of a sample ---------------------------------------------------------------------------------------------------------------------
CF_HD bool lineOf(double x0, double y0, double x1, double y1, Curve* c)
{
	if (x0 == x1 && y0 == y1) return false;
	c->A = y1 - y0;
	c->B = x0 - x1;
	c->C = (x1 * y0) - (x0 * y1);
	return true;
}
CF_HD bool parabolaOf(double x1, double y1, double x2, double y2, double x3, double y3, Curve* c)
{
	if (x1 == x2 || x1 == x3 || x2 == x3) return false;
	const double scale = ddiv(1.0, ((x1 - x2) * (x1 - x3)) * (x2 - x3));
	c->A = (((x3 * (y2 - y1)) + (x2 * (y1 - y3))) + (x1 * (y3 - y2))) * scale;
	c->B = ((((x3 * x3) * (y1 - y2)) + ((x2 * x2) * (y3 - y1))) + ((x1 * x1) * (y2 - y3))) * scale;
	c->C = (((((x2 * x3) * (x2 - x3)) * y1) + (((x3 * x1) * (x3 - x1)) * y2)) + (((x1 * x2) * (x1 - x2)) * y3)) * scale;
	return true;
}
// the model through the first m of the points (px[i], py[i]); false: rejected
CF_HD bool curveOf(int model, const double px[3], const double py[3], Curve* c)
{
	if (model == kLine) return lineOf(px[0], py[0], px[1], py[1], c);
	return parabolaOf(xOf(model, px[0], py[0]), yOf(model, px[0], py[0]), xOf(model, px[1], py[1]), yOf(model, px[1], py[1]), xOf(model, px[2], py[2]),
	                  yOf(model, px[2], py[2]), c);
}

// ---- C. residual ------------------------------------------------------------------------------------------------------------------------------
// what the residual loop reads: a line's coefficients scaled by 1 / sqrt(A * A + B * B), a parabola's as they are
CF_HD Curve prepared(int model, Curve c)
{
	if (model != kLine) return c;
	const double s = ddiv(1.0, dsqrt((c.A * c.A) + (c.B * c.B)));
	Curve r;
	r.A = c.A * s; r.B = c.B * s; r.C = c.C * s;
	return r;
}
CF_HD double residual(int model, const Curve& p, double px, double py)
{
	if (model == kLine) return dabs(((p.A * px) + p.C) + (p.B * py));
	const double x = xOf(model, px, py), y = yOf(model, px, py);
	return dabs((((p.A * (x * x)) + p.C) + (p.B * x)) - y);
}

// ---- E. refit ---------------------------------------------------------------------------------------------------------------------------------
CF_HD double meanOf(double sum, int n) { return sum * ddiv(1.0, (double)n); }
// what point (x, y) adds to the line's two sums about the means
CF_HD void lineTerms(double x, double y, double meanX, double meanY, double* ab, double* den)
{
	const double a = x - meanX, b = y - meanY;
	*ab = a * b;
	*den = (b * b) - (a * a);
}
CF_HD Curve lineFromSums(double meanX, double meanY, double sumAb, double den)
{
	const double num = sumAb * -2.0;
	double cs = 1.0, sn = 0.0;
	if (!(num == 0.0 && den == 0.0)) hg::halfAngle(num, den, &cs, &sn);
	Curve c;
	c.A = cs; c.B = sn; c.C = -((meanX * cs) + (meanY * sn));
	return c;
}
// what point (x, y) (the model's x and y) adds to the parabola's seven sums: S1..S4, T0..T2
CF_HD void parabolaTerms(double x, double y, double mean, double t[7])
{
	const double u = x - mean, uu = u * u;
	t[0] = u; t[1] = uu; t[2] = uu * u; t[3] = uu * uu;
	t[4] = y; t[5] = u * y; t[6] = uu * y;
}
CF_HD bool parabolaFromSums(int n, double mean, const double s[7], Curve* out)
{
	const double m00 = s[3], m01 = s[2], m02 = s[1], m11 = s[1], m12 = s[0], m22 = (double)n;
	const double r0 = s[6], r1 = s[5], r2 = s[4];
	const double c00 = (m11 * m22) - (m12 * m12), c01 = (m02 * m12) - (m01 * m22), c02 = (m01 * m12) - (m02 * m11);
	const double c11 = (m00 * m22) - (m02 * m02), c12 = (m01 * m02) - (m00 * m12), c22 = (m00 * m11) - (m01 * m01);
	const double det = ((m00 * c00) + (m01 * c01)) + (m02 * c02);
	if (det == 0.0 || !(dabs(det) <= DBL_MAX)) return false;
	const double a = ddiv(((c00 * r0) + (c01 * r1)) + (c02 * r2), det);
	const double b = ddiv(((c01 * r0) + (c11 * r1)) + (c12 * r2), det);
	const double c = ddiv(((c02 * r0) + (c12 * r1)) + (c22 * r2), det);
	out->A = a;
	out->B = b - ((2.0 * a) * mean);
	out->C = (c - (b * mean)) + (a * (mean * mean));
	return true;
}

} // namespace cf
} // namespace compvhip
