// pca_math_check.cpp -- compv_amd/csrc/pca_math.hpp on the host: a stand-alone program (standard library only, no GPU) that tests/test_pca_host.py
// builds with AddressSanitizer and UBSan and feeds the cases of tests/golden/golden_pca.npz.
//
//   pca_math_check project IN OUT      IN:  int32 n, D, M, hasMean, chunk (a multiple of 16); hasMean x float mean[D]; float vectors[M][D]; float rows[n][D].
//                                      OUT: float out[n][M] in one call of dot16 per output on the centred row; then float out[n][M] the way the
//                                           kernel feeds the header: columns staged `chunk` at a time, centred as they are staged, the accumulators
//                                           kept across chunks, the 4-groups, the fold and the last columns once behind the last whole group.
//   pca_math_check covariance IN OUT   IN:  int32 n, D, chunk; float obs[n][D].
//                                      OUT: float mean[D]; float covar[D][D] in one call per element; float covar[D][D] fed in chunks.
//   pca_math_check parse FILE OUT      OUT: int32 ok, D, M; then (ok != 0) float mean[D], vectors[M][D], values[M].  A refused file: ok = 0, exit 0.
#include "../../compv_amd/csrc/pca_math.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace compvhip;

static void die(const char* what)
{
	fprintf(stderr, "pca_math_check: %s\n", what);
	exit(2);
}

static void readAll(FILE* in, void* dst, size_t size, size_t count)
{
	if (count && fread(dst, size, count, in) != count) die("short input");
}
static void writeAll(FILE* out, const void* src, size_t size, size_t count)
{
	if (count && fwrite(src, size, count, out) != count) die("short output");
}

// dot16 of two rows fed the way pca_project_kernel feeds it: `chunk` columns staged at a time into buffers of their own
static float chunked(const float* a, const float* b, size_t cols, size_t chunk, const float* mean)
{
	std::vector<float> sa(chunk), sb(chunk);
	pca::Dot16 s;
	s.clear();
	const size_t c16 = cols & ~static_cast<size_t>(15);
	for (size_t k0 = 0; k0 < c16; k0 += chunk) {
		const size_t kc = c16 - k0 < chunk ? c16 - k0 : chunk;
		for (size_t c = 0; c < kc; ++c) { sa[c] = mean ? pca::centre(a[k0 + c], mean[k0 + c]) : a[k0 + c]; sb[c] = b[k0 + c]; }
		for (size_t g = 0; g < kc; g += 16) {
			// a quarter at a time, in the kernel's order
			s.quarter<0>(&sa[g], &sb[g]); s.quarter<1>(&sa[g + 4], &sb[g + 4]); s.quarter<2>(&sa[g + 8], &sb[g + 8]); s.quarter<3>(&sa[g + 12], &sb[g + 12]);
		}
	}
	const size_t nt = cols - c16;
	std::vector<float> ta(nt), tb(nt);          // exactly nt elements: a read behind them is the sanitizer's
	for (size_t c = 0; c < nt; ++c) { ta[c] = mean ? pca::centre(a[c16 + c], mean[c16 + c]) : a[c16 + c]; tb[c] = b[c16 + c]; }
	return s.finish(ta.data(), tb.data(), nt);
}

static int project(FILE* in, FILE* out)
{
	int32_t h[5];
	readAll(in, h, 4, 5);
	if (h[0] < 0 || h[1] < 1 || h[2] < 1 || h[4] < 16 || h[4] % 16) die("bad header");
	const size_t n = h[0], D = h[1], M = h[2], chunk = h[4];
	std::vector<float> mean(h[3] ? D : 0), vectors(M * D), rows(n * D), one(n * M), fed(n * M), c(D);
	readAll(in, mean.data(), 4, mean.size()); readAll(in, vectors.data(), 4, vectors.size()); readAll(in, rows.data(), 4, rows.size());
	for (size_t r = 0; r < n; ++r) {
		for (size_t k = 0; k < D; ++k) c[k] = h[3] ? pca::centre(rows[r * D + k], mean[k]) : rows[r * D + k];
		for (size_t m = 0; m < M; ++m) {
			one[r * M + m] = pca::dot16(c.data(), &vectors[m * D], D);
			fed[r * M + m] = chunked(&rows[r * D], &vectors[m * D], D, chunk, h[3] ? mean.data() : nullptr);
		}
	}
	writeAll(out, one.data(), 4, one.size()); writeAll(out, fed.data(), 4, fed.size());
	return 0;
}

static int covariance(FILE* in, FILE* out)
{
	int32_t h[3];
	readAll(in, h, 4, 3);
	if (h[0] < 1 || h[1] < 1 || h[2] < 16 || h[2] % 16) die("bad header");
	const size_t n = h[0], D = h[1], chunk = h[2], nPad = (n + 15) / 16 * 16;
	std::vector<float> obs(n * D), mean(D), c(D * nPad, -7.f), one(D * D), fed(D * D);          // (the padding of c holds a value no result may show)
	readAll(in, obs.data(), 4, obs.size());
	for (size_t j = 0; j < D; ++j) mean[j] = pca::mean(&obs[j], n, D);
	for (size_t j = 0; j < D; ++j)
		for (size_t i = 0; i < n; ++i) c[j * nPad + i] = pca::centre(obs[i * D + j], mean[j]);
	for (size_t a = 0; a < D; ++a)
		for (size_t b = 0; b < D; ++b) {
			float v = pca::dot16(&c[a * nPad], &c[b * nPad], n), w = chunked(&c[a * nPad], &c[b * nPad], n, chunk, nullptr);
			if (n > 1) { v = v * pca::covarScale(n); w = w * pca::covarScale(n); }
			one[a * D + b] = v; fed[a * D + b] = w;
		}
	writeAll(out, mean.data(), 4, D); writeAll(out, one.data(), 4, one.size()); writeAll(out, fed.data(), 4, fed.size());
	return 0;
}

static int parse(const char* path, FILE* out)
{
	pca::Model m;
	std::string why;
	const bool ok = pca::parse_model(path, m, &why);
	if (!ok && why.empty()) die("a refusal without a reason");
	const int32_t h[3] = { ok ? 1 : 0, m.dim, m.components };
	writeAll(out, h, 4, 3);
	if (ok) {
		if (m.mean.size() != static_cast<size_t>(m.dim) || m.values.size() != static_cast<size_t>(m.components) || m.vectors.size() != m.mean.size() * m.values.size()) die("sizes");
		writeAll(out, m.mean.data(), 4, m.mean.size()); writeAll(out, m.vectors.data(), 4, m.vectors.size()); writeAll(out, m.values.data(), 4, m.values.size());
	}
	else if (m.dim || m.components || !m.mean.empty() || !m.vectors.empty() || !m.values.empty()) die("a refused file wrote something");
	return 0;
}

int main(int argc, char** argv)
{
	if (argc != 4) die("usage: pca_math_check project|covariance|parse IN OUT");
	FILE* out = fopen(argv[3], "wb");
	if (!out) die("cannot open the output");
	int rc;
	if (!strcmp(argv[1], "parse")) rc = parse(argv[2], out);
	else {
		FILE* in = fopen(argv[2], "rb");
		if (!in) die("cannot open the input");
		if (!strcmp(argv[1], "project")) rc = project(in, out);
		else if (!strcmp(argv[1], "covariance")) rc = covariance(in, out);
		else { die("unknown mode"); rc = 2; }
		fclose(in);
	}
	if (fclose(out)) die("close");
	return rc;
}
