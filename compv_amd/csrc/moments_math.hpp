// moments_math.hpp -- what the image moments (include/compv_hip.h, "image moments") share on the host and on the device, standard library only: the
// range rule (item B) and the shape record of a raw record (item D).  Every operation of item D is one IEEE binary64 operation in the order the
// definition gives (the translation units are built with -ffp-contract=off); the division and the square roots are the correctly rounded ones on
// either side, and the one angle goes through hg::halfAngle (homography_math.hpp), so nothing is transcendental.
#pragma once
#include "../../include/compv_hip.h"
#include "homography_math.hpp"

namespace compvhip {
namespace moments {

constexpr uint32_t kMaxSide = 32767;

// ---- B. range ----------------------------------------------------------------------------------------------------------------------------
// wmax * W * H * max(W - 1, H - 1)^2 < 2^64, for sizes that passed the other refusals (W * H < 2^31, so the first factor stays below 2^39 and the
// square below 2^30: the product itself may not fit, the quotient does)
HG_HD bool sumsFit(uint64_t wmax, uint64_t W, uint64_t H)
{
	const uint64_t m = (W > H ? W : H) - 1, sq = m * m;
	return sq == 0 || wmax * W * H <= ~static_cast<uint64_t>(0) / sq;
}
// a frame of W x H bytes may be given with these weights (wmax: 255 for VALUE, 1 for UNIT)
HG_HD bool fits(uint64_t W, uint64_t H, int weights)
{
	if (weights != COMPVHIP_MOMENTS_VALUE && weights != COMPVHIP_MOMENTS_UNIT) return false;
	if (!W || !H || W > kMaxSide || H > kMaxSide || W * H >= (static_cast<uint64_t>(1) << 31)) return false;
	return sumsFit(weights == COMPVHIP_MOMENTS_VALUE ? 255 : 1, W, H);
}

// ---- D. shape ----------------------------------------------------------------------------------------------------------------------------
HG_HD void shape(const compvhip_moments& r, compvhip_moments_shape* s)
{
	s->xbar = 0.0; s->ybar = 0.0; s->u20 = 0.0; s->u02 = 0.0; s->u11 = 0.0; s->skew = 0.0; s->cs = 1.0; s->sn = 0.0; s->status = 1; s->pad = 0;
	if (r.m00 == 0) return;
	const double M00 = static_cast<double>(r.m00), M01 = static_cast<double>(r.m01), M10 = static_cast<double>(r.m10);
	const double M11 = static_cast<double>(r.m11), M02 = static_cast<double>(r.m02), M20 = static_cast<double>(r.m20);
	const double scale = hg::ddiv(1.0, M00);
	const double ybar = M01 * scale, xbar = M10 * scale;
	const double u20 = (M20 * scale) - (xbar * xbar);
	const double u02 = (M02 * scale) - (ybar * ybar);
	const double u11 = (M11 * scale) - (xbar * ybar);
	const double den = u20 - u02;
	if (hg::dabs(den) > hg::kEps) hg::halfAngle(2.0 * u11, den, &s->cs, &s->sn);
	const double a = M02 - (ybar * M01);
	const double b = M11 - (xbar * M01);
	s->skew = hg::dabs(a) > hg::kEps ? hg::ddiv(b, a) : 0.0;
	s->xbar = xbar; s->ybar = ybar; s->u20 = u20; s->u02 = u02; s->u11 = u11; s->status = 0;
}

} // namespace moments
} // namespace compvhip
