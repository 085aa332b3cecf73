// curvefit_math_check.cpp -- compv_amd/csrc/curvefit_math.hpp run on the host (standard library only, no GPU): the whole RANSAC fit of ONE set, in the
// order the kernels of curvefit_kernels.hip take (one try after another, ranked by the kernels' own rule, ransac::better; the 64 partials of sum64 as an
// array, ransac::fold64), so that tests/test_curvefit_host.py
// can hold the header's arithmetic against tests/curvefit_model.py bit for bit.
//   in:  int32 k, tries, hasSamples, set, model; uint32 seed; float64 threshold; float64 pts[k][2]; int32 samples[tries][m] (if hasSamples)
//   out: the result record (40 bytes); uint8 mask[k]; int32 counts[tries]; int32 samples[tries][m]
// Build with -ffp-contract=off (one rounding per operation).
#include "../../compv_amd/csrc/curvefit_math.hpp"

#include <cstdio>
#include <cstring>
#include <vector>

using namespace compvhip::cf;
namespace ransac = compvhip::ransac;

struct Result { double A, B, C; int32_t inliers, bestTry, status, k; };

// the model of a sample of set points; false: out of range or rejected
static bool tryCurve(int model, const std::vector<double>& pts, int k, const int32_t* q, Curve* c)
{
	const int m = modelPoints(model);
	double px[3] = { 0.0, 0.0, 0.0 }, py[3] = { 0.0, 0.0, 0.0 };
	for (int i = 0; i < m; ++i) {
		if ((uint32_t)q[i] >= (uint32_t)k) return false;
		px[i] = pts[2 * q[i]]; py[i] = pts[2 * q[i] + 1];
	}
	return curveOf(model, px, py, c);
}

static bool refit(int model, const std::vector<double>& sel, Curve* out)
{
	const int n = (int)(sel.size() / 2), m = modelPoints(model);
	if (n == m) {
		double px[3] = { 0.0, 0.0, 0.0 }, py[3] = { 0.0, 0.0, 0.0 };
		for (int i = 0; i < m; ++i) { px[i] = sel[2 * i]; py[i] = sel[2 * i + 1]; }
		return curveOf(model, px, py, out);
	}
	if (model == kLine) {
		double px[64] = {}, py[64] = {}, pab[64] = {}, pden[64] = {};
		for (int i = 0; i < n; ++i) { px[i & 63] += sel[2 * i]; py[i & 63] += sel[2 * i + 1]; }
		const double meanX = meanOf(ransac::fold64(px), n), meanY = meanOf(ransac::fold64(py), n);
		for (int i = 0; i < n; ++i) {
			double ab, den;
			lineTerms(sel[2 * i], sel[2 * i + 1], meanX, meanY, &ab, &den);
			pab[i & 63] += ab; pden[i & 63] += den;
		}
		const double sab = ransac::fold64(pab), sden = ransac::fold64(pden);
		*out = lineFromSums(meanX, meanY, sab, sden);
		return true;
	}
	double pu[64] = {};
	for (int i = 0; i < n; ++i) pu[i & 63] += xOf(model, sel[2 * i], sel[2 * i + 1]);
	const double mean = meanOf(ransac::fold64(pu), n);
	std::vector<double> part(64 * 7, 0.0);
	for (int i = 0; i < n; ++i) {
		double t[7];
		parabolaTerms(xOf(model, sel[2 * i], sel[2 * i + 1]), yOf(model, sel[2 * i], sel[2 * i + 1]), mean, t);
		for (int e = 0; e < 7; ++e) part[(i & 63) * 7 + e] += t[e];
	}
	double s[7];
	for (int e = 0; e < 7; ++e) {
		double p[64];
		for (int l = 0; l < 64; ++l) p[l] = part[l * 7 + e];
		s[e] = ransac::fold64(p);
	}
	return parabolaFromSums(n, mean, s, out);
}

int main(int argc, char** argv)
{
	if (argc != 3) return 2;
	FILE* f = fopen(argv[1], "rb");
	if (!f) return 2;
	int32_t head[6]; double threshold;
	if (fread(head, 4, 6, f) != 6 || fread(&threshold, 8, 1, f) != 1) return 2;
	const int k = head[0], tries = head[1], hasSamples = head[2], set = head[3], model = head[4];
	uint32_t seed; memcpy(&seed, &head[5], 4);
	if (model < 0 || model >= kModels || k < 0 || tries < 1) return 2;
	const int m = modelPoints(model);
	std::vector<double> pts(2 * (size_t)(k > 0 ? k : 1));
	std::vector<int32_t> samples((size_t)m * tries, 0);
	if (k > 0 && fread(pts.data(), 16, k, f) != (size_t)k) return 2;
	if (hasSamples && fread(samples.data(), 4 * m, tries, f) != (size_t)tries) return 2;
	fclose(f);

	Result res = {};
	res.bestTry = -1; res.k = k;
	std::vector<uint8_t> mask(k, 0);
	std::vector<int32_t> counts(tries, 0);
	if (k < m) res.status = 2;
	else if (k == m) {
		const int32_t q[3] = { 0, 1, 2 };
		Curve c;
		if (tryCurve(model, pts, k, q, &c)) {
			res.A = c.A; res.B = c.B; res.C = c.C; res.inliers = m; res.bestTry = 0;
			for (int i = 0; i < k; ++i) mask[i] = 1;
		}
		else res.status = 1;
	}
	else {
		int bc = 0, bt = -1;
		for (int t = 0; t < tries; ++t) {
			int32_t* q = &samples[(size_t)m * t];
			if (!hasSamples) {
				int32_t q3[3];
				sample(model, seed, (uint32_t)set, (uint32_t)t, (uint32_t)k, q3);
				for (int j = 0; j < m; ++j) q[j] = q3[j];
			}
			Curve c;
			if (tryCurve(model, pts, k, q, &c)) {
				const Curve p = prepared(model, c);
				int count = 0;
				for (int i = 0; i < k; ++i) count += residual(model, p, pts[2 * i], pts[2 * i + 1]) < threshold ? 1 : 0;
				counts[t] = count;
			}
			if (ransac::better(m, counts[t], ransac::NoVariance(), t, bc, ransac::NoVariance(), bt)) { bc = counts[t]; bt = t; }
		}
		if (bc < m) res.status = 1;
		else {
			Curve own = { 0.0, 0.0, 0.0 };
			(void)tryCurve(model, pts, k, &samples[(size_t)m * bt], &own);
			const Curve p = prepared(model, own);
			std::vector<double> sel;
			for (int i = 0; i < k; ++i) {
				if (residual(model, p, pts[2 * i], pts[2 * i + 1]) < threshold) { mask[i] = 1; sel.push_back(pts[2 * i]); sel.push_back(pts[2 * i + 1]); }
			}
			Curve fit = { 0.0, 0.0, 0.0 };
			const bool ok = refit(model, sel, &fit);
			const Curve w = ok ? fit : own;
			res.A = w.A; res.B = w.B; res.C = w.C;
			res.inliers = bc; res.bestTry = bt; res.status = ok ? 0 : 3;
		}
	}
	FILE* o = fopen(argv[2], "wb");
	if (!o) return 2;
	fwrite(&res, sizeof(res), 1, o);
	if (k > 0) fwrite(mask.data(), 1, k, o);
	fwrite(counts.data(), 4, tries, o);
	fwrite(samples.data(), 4 * m, tries, o);
	fclose(o);
	return 0;
}
