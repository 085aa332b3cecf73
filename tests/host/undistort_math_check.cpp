// undistort_math_check.cpp -- compv_amd/csrc/undistort_math.hpp on the host: a stand-alone program (standard library only, no GPU) that
// tests/test_undistort_host.py builds with AddressSanitizer and UBSan and feeds the cases of tests/undistort_cases.py.
//
//   undistort_math_check IN OUT
// IN:  int32 f64, nd, x0, y0, Wout, Hout, npts, nproj; K[9], d[nd] of T; npts x {x, y} of T; when nproj: Rt[12] and nproj x {x, y, z}, float64.
// OUT: int32 ok (0: the camera is singular, nothing follows); coeffs[14], mapX[Wout * Hout], mapY[Wout * Hout], npts x {u, v} of T; nproj x {u, v} float64.
// T is float32 (f64 == 0) or float64.  The map is walked the way the kernels walk it -- groups of 4 entries of a row, a partial group at the end --
// and the program aborts when an entry differs from the plain row-major walk.
#include "../../compv_amd/csrc/undistort_math.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace compvhip;

static void die(const char* what)
{
	fprintf(stderr, "undistort_math_check: %s\n", what);
	exit(2);
}

template <typename T>
static std::vector<T> take(FILE* f, size_t n)
{
	std::vector<T> v(n);
	if (n && fread(v.data(), sizeof(T), n, f) != n) die("short input");
	return v;
}

template <typename T>
static void put(FILE* f, const std::vector<T>& v)
{
	if (!v.empty() && fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) die("short output");
}

template <typename T>
static int run(FILE* in, FILE* out, const int32_t* h)
{
	const int nd = h[1], x0 = h[2], y0 = h[3], W = h[4], H = h[5], npts = h[6], nproj = h[7];
	const std::vector<T> K = take<T>(in, 9), d = take<T>(in, static_cast<size_t>(nd > 0 ? nd : 0)), pts = take<T>(in, 2 * static_cast<size_t>(npts));
	std::vector<double> Rt, pts3;
	if (nproj) { Rt = take<double>(in, undist::kPose); pts3 = take<double>(in, 3 * static_cast<size_t>(nproj)); }
	std::vector<T> c(undist::kCoeffs, static_cast<T>(-1));
	const int32_t ok = undist::coeffs(K.data(), d.data(), nd, c.data()) ? 1 : 0;
	fwrite(&ok, 4, 1, out);
	if (!ok) {
		for (T v : c) if (v != static_cast<T>(-1)) die("a refused camera wrote coefficients");
		return 0;
	}
	const size_t n = static_cast<size_t>(W) * H;
	std::vector<T> mx(n), my(n);
	for (int j = 0; j < H; ++j)          // the kernels' walk: a lane's 4 adjacent entries, the last group partial
		for (int i0 = 0; i0 < W; i0 += 4)
			for (int b = 0; b < 4 && i0 + b < W; ++b)
				undist::map_entry(c.data(), static_cast<T>(x0 + i0 + b), static_cast<T>(y0 + j), mx[static_cast<size_t>(j) * W + i0 + b], my[static_cast<size_t>(j) * W + i0 + b]);
	for (size_t k = 0; k < n; ++k) {          // the plain walk
		T u, v;
		undist::map_entry(c.data(), static_cast<T>(x0 + static_cast<int>(k % W)), static_cast<T>(y0 + static_cast<int>(k / W)), u, v);
		if (memcmp(&u, &mx[k], sizeof(T)) || memcmp(&v, &my[k], sizeof(T))) die("the grouped walk differs from the plain one");
	}
	std::vector<T> po(2 * static_cast<size_t>(npts));
	for (int k = 0; k < npts; ++k) undist::map_entry(c.data(), pts[2 * k], pts[2 * k + 1], po[2 * k], po[2 * k + 1]);
	put(out, c); put(out, mx); put(out, my); put(out, po);
	if (nproj) {
		if (sizeof(T) != 8) die("proj2D is float64 only");
		std::vector<double> cd(c.begin(), c.end()), pr(2 * static_cast<size_t>(nproj));
		for (int k = 0; k < nproj; ++k) undist::project(cd.data(), Rt.data(), pts3[3 * k], pts3[3 * k + 1], pts3[3 * k + 2], pr[2 * k], pr[2 * k + 1]);
		put(out, pr);
	}
	return 0;
}

int main(int argc, char** argv)
{
	if (argc != 3) die("usage: undistort_math_check IN OUT");
	FILE* in = fopen(argv[1], "rb");
	FILE* out = fopen(argv[2], "wb");
	if (!in || !out) die("cannot open a file");
	int32_t h[8];
	if (fread(h, 4, 8, in) != 8) die("short header");
	if (h[4] < 0 || h[5] < 0 || h[6] < 0 || h[7] < 0 || h[1] > 16) die("bad header");
	const int rc = h[0] ? run<double>(in, out, h) : run<float>(in, out, h);
	fclose(in);
	if (fclose(out)) die("close");
	return rc;
}
