// homography_math_check.cpp -- compv_amd/csrc/homography_math.hpp run on the host (standard library only, no GPU): the whole RANSAC homography of ONE
// pair, in the order the kernels of homography_kernels.hip take (one try after another, ranked by the kernels' own rule, ransac::better; the 64
// partials of sum64 as an array, ransac::fold64), so that
// tests/test_homography_host.py can hold the header's arithmetic against tests/homography_model.py bit for bit.
//   in:  int32 k, tries, hasQuads, pair; uint32 seed; int32 pad; float64 threshold; float64 src[k][2], dst[k][2]; int32 quads[tries][4] (if hasQuads)
//   out: the result record (96 bytes); uint8 mask[k]; int32 counts[tries]; float64 variances[tries]; int32 rotations[tries]; int32 quads[tries][4]
// Build with -ffp-contract=off (one rounding per operation).
#include "../../compv_amd/csrc/homography_math.hpp"

#include <cstdio>
#include <cstring>
#include <vector>

using namespace compvhip::hg;
namespace ransac = compvhip::ransac;

struct Result { double H[9]; double variance; int32_t inliers, bestTry, status, rotations; };

static Norm normN(const double* pts, int n)
{
	double px[64] = {}, py[64] = {}, pm[64] = {};
	for (int i = 0; i < n; ++i) { px[i & 63] += pts[2 * i]; py[i & 63] += pts[2 * i + 1]; }
	const double inv = 1.0 / (double)n;
	Norm r;
	r.tx = ransac::fold64(px) * inv; r.ty = ransac::fold64(py) * inv;
	for (int i = 0; i < n; ++i) pm[i & 63] += hypotNaive(pts[2 * i] - r.tx, pts[2 * i + 1] - r.ty);
	r.s = scaleOf(ransac::fold64(pm) * inv);
	return r;
}

static int computeHN(const double* src, const double* dst, int n, double H[9])
{
	double D[81], Q[81];
	if (n == 4) {
		double sx[4], sy[4], dx[4], dy[4];
		for (int i = 0; i < 4; ++i) { sx[i] = src[2 * i]; sy[i] = src[2 * i + 1]; dx[i] = dst[2 * i]; dy[i] = dst[2 * i + 1]; }
		return computeH4<1>(sx, sy, dx, dy, D, Q, true, H);
	}
	const Norm a = normN(src, n), b = normN(dst, n);
	std::vector<double> part(64 * 45, 0.0);
	for (int i = 0; i < n; ++i) {
		double m0[9], m1[9];
		rowsOf(normalised(src[2 * i], a.tx, a.s), normalised(src[2 * i + 1], a.ty, a.s), normalised(dst[2 * i], b.tx, b.s), normalised(dst[2 * i + 1], b.ty, b.s), m0, m1);
		accumulateS(m0, m1, &part[(i & 63) * 45]);
	}
	double acc[45];
	for (int e = 0; e < 45; ++e) {
		double p[64];
		for (int l = 0; l < 64; ++l) p[l] = part[l * 45 + e];
		acc[e] = ransac::fold64(p);
	}
	storeS<1>(acc, D, Q);
	const int rotations = jacobi<1>(D, Q);
	finishH<1>(D, Q, a, b, true, H);
	return rotations;
}

int main(int argc, char** argv)
{
	if (argc != 3) return 2;
	FILE* f = fopen(argv[1], "rb");
	if (!f) return 2;
	int32_t head[6]; double threshold;
	if (fread(head, 4, 6, f) != 6 || fread(&threshold, 8, 1, f) != 1) return 2;
	const int k = head[0], tries = head[1], hasQuads = head[2], pair = head[3];
	uint32_t seed; memcpy(&seed, &head[4], 4);
	std::vector<double> src(2 * (k > 0 ? k : 1)), dst(src.size());
	std::vector<int32_t> quads(4 * tries);
	if (k > 0 && (fread(src.data(), 16, k, f) != (size_t)k || fread(dst.data(), 16, k, f) != (size_t)k)) return 2;
	if (hasQuads && fread(quads.data(), 16, tries, f) != (size_t)tries) return 2;
	fclose(f);

	Result res = {};
	res.variance = DBL_MAX; res.bestTry = -1;
	std::vector<uint8_t> mask(k > 0 ? k : 0, 0);
	std::vector<int32_t> counts(tries, 0), rotations(tries, 0);
	std::vector<double> variances(tries, DBL_MAX), hyp(18 * (size_t)tries, 0.0);
	if (k < 4) res.status = 2;
	else {
		int bc = 0, bt = -1; double bv = DBL_MAX;
		for (int t = 0; t < tries; ++t) {
			int32_t* q = &quads[4 * t];
			if (!hasQuads) quad(seed, (uint32_t)pair, (uint32_t)t, (uint32_t)k, q);
			bool live = false;
			double* H = &hyp[18 * (size_t)t]; double* Hinv = H + 9;
			if ((uint32_t)q[0] < (uint32_t)k && (uint32_t)q[1] < (uint32_t)k && (uint32_t)q[2] < (uint32_t)k && (uint32_t)q[3] < (uint32_t)k) {
				double sx[4], sy[4], dx[4], dy[4], D[81], Q[81];
				for (int i = 0; i < 4; ++i) { sx[i] = src[2 * q[i]]; sy[i] = src[2 * q[i] + 1]; dx[i] = dst[2 * q[i]]; dy[i] = dst[2 * q[i] + 1]; }
				if (!collinear4(sx, sy)) {
					rotations[t] = computeH4<1>(sx, sy, dx, dy, D, Q, false, H);
					live = inverse3(H, Hinv);
				}
			}
			if (live) {
				int count = 0; double sum = 0.0, var = 0.0;
				for (int i = 0; i < k; ++i) {
					const double d = distance(H, Hinv, src[2 * i], src[2 * i + 1], dst[2 * i], dst[2 * i + 1]);
					if (d < threshold) { ++count; sum += d; }
				}
				const double mean = count > 0 ? sum / (double)count : 0.0;
				for (int i = 0; i < k; ++i) {
					const double d = distance(H, Hinv, src[2 * i], src[2 * i + 1], dst[2 * i], dst[2 * i + 1]);
					if (d < threshold) { const double dev = d - mean; var += dev * dev; }
				}
				counts[t] = count;
				variances[t] = count >= 2 ? var / (double)(count - 1) : DBL_MAX;
			}
			if (ransac::better(4, counts[t], variances[t], t, bc, bv, bt)) { bc = counts[t]; bv = variances[t]; bt = t; }
		}
		if (bc >= 4) {
			const double* H = &hyp[18 * (size_t)bt];
			std::vector<double> ss, sd;
			for (int i = 0; i < k; ++i) {
				if (distance(H, H + 9, src[2 * i], src[2 * i + 1], dst[2 * i], dst[2 * i + 1]) < threshold) {
					mask[i] = 1;
					ss.push_back(src[2 * i]); ss.push_back(src[2 * i + 1]); sd.push_back(dst[2 * i]); sd.push_back(dst[2 * i + 1]);
				}
			}
			res.rotations = computeHN(ss.data(), sd.data(), (int)(ss.size() / 2), res.H);
			res.variance = bv; res.inliers = bc; res.bestTry = bt; res.status = 0;
		}
		else {
			res.rotations = computeHN(src.data(), dst.data(), k, res.H);
			res.status = 1;
		}
	}
	FILE* o = fopen(argv[2], "wb");
	if (!o) return 2;
	fwrite(&res, sizeof(res), 1, o);
	if (k > 0) fwrite(mask.data(), 1, k, o);
	fwrite(counts.data(), 4, tries, o);
	fwrite(variances.data(), 8, tries, o);
	fwrite(rotations.data(), 4, tries, o);
	fwrite(quads.data(), 16, tries, o);
	fclose(o);
	return 0;
}
