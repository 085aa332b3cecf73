// pca_math.hpp -- what the PCA projection (include/compv_hip.h, "PCA projection") shares on the host and on the device, standard library only: the
// sixteen-accumulator dot product of CompVMath::mulABt (item C) as a state that is fed in groups, so a kernel that walks a row in chunks of 16 * k
// columns and a host loop that walks it in one go run the same statements; the centring (item B), the mean (item F) and the parser of the model file
// (item G).  Every operation is one IEEE binary32 operation (the mean: binary64) in the order the definition gives; the translation units are built
// with -ffp-contract=off, so no product is fused into its sum.
#pragma once
#include <locale.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define PCA_HD __host__ __device__ __forceinline__
#define PCA_UNROLL _Pragma("unroll")
#else
#define PCA_HD inline
#define PCA_UNROLL
#endif

namespace compvhip {
namespace pca {

constexpr size_t kMaxDim = size_t(1) << 20;          // D, and aRows / bRows / cols of mulABt
constexpr size_t kMaxComponents = 65535;             // M
constexpr size_t kMaxRows = 0x7fffffff;              // n
constexpr size_t kMaxElems = size_t(1) << 40;        // n * stride stays below

// ---- B. centre ---------------------------------------------------------------------------------------------------------------------------
PCA_HD float centre(float x, float mean) { return x - mean; }

// ---- C. dot16 ----------------------------------------------------------------------------------------------------------------------------
// The state of one output.  Feed it: group16 for every whole group of 16 columns, group4 for every whole group of 4 of what remains, fold() once,
// tail for each of the last 0 .. 3 columns; the value is v[0].
struct Dot16 {
	float v[16];
	PCA_HD void clear()
	{
		PCA_UNROLL
		for (int i = 0; i < 16; ++i) v[i] = 0.f;
	}
	// the columns 4 * Q .. 4 * Q + 3 of a group of 16, into their own four accumulators (the accumulators are independent: any order of the quarters
	// is the same arithmetic)
	template <int Q>
	PCA_HD void quarter(const float* a, const float* b)
	{
		PCA_UNROLL
		for (int i = 0; i < 4; ++i) { const float p = a[i] * b[i]; v[4 * Q + i] = v[4 * Q + i] + p; }
	}
	PCA_HD void group16(const float* a, const float* b) { quarter<0>(a, b); quarter<1>(a + 4, b + 4); quarter<2>(a + 8, b + 8); quarter<3>(a + 12, b + 12); }
	PCA_HD void group4(const float* a, const float* b) { quarter<0>(a, b); }
	PCA_HD void fold()
	{
		v[0] += v[4]; v[1] += v[5]; v[2] += v[6]; v[3] += v[7]; v[8] += v[12]; v[9] += v[13]; v[10] += v[14]; v[11] += v[15];
		v[0] += v[8]; v[1] += v[9]; v[2] += v[10]; v[3] += v[11];
		v[0] += v[2]; v[1] += v[3];
		v[0] += v[1];
	}
	PCA_HD void tail(float a, float b) { const float p = a * b; v[0] = v[0] + p; }
	// the columns [0, cols) of a and b that follow the whole groups of 16 already fed: the groups of 4, the fold, the last columns
	PCA_HD float finish(const float* a, const float* b, size_t cols)
	{
		size_t k = 0;
		for (; k + 4 <= cols; k += 4) group4(a + k, b + k);
		fold();
		for (; k < cols; ++k) tail(a[k], b[k]);
		return v[0];
	}
};

// in one call
PCA_HD float dot16(const float* a, const float* b, size_t cols)
{
	Dot16 s;
	s.clear();
	size_t k = 0;
	for (; k + 16 <= cols; k += 16) s.group16(a + k, b + k);
	return s.finish(a + k, b + k, cols - k);
}

// ---- F. mean and scale -------------------------------------------------------------------------------------------------------------------
// mean_j of the column j of n row-based observations: a binary64 sum in row order, times 1.0 / n, rounded to binary32
PCA_HD float mean(const float* obs, size_t n, size_t stride)
{
	const double scale = 1.0 / static_cast<double>(n);
	double s = 0.0;
	for (size_t i = 0; i < n; ++i) s = s + static_cast<double>(obs[i * stride]);
	return static_cast<float>(s * scale);
}
PCA_HD float covarScale(size_t n) { return 1.f / static_cast<float>(n - 1); }          // n > 1

// ---- limits ------------------------------------------------------------------------------------------------------------------------------
// a stride is at least its row length, and rows * stride stays below 2^40
inline bool strideFits(size_t rows, size_t stride, size_t rowLength) { return stride >= rowLength && stride > 0 && stride < kMaxElems && rows <= (kMaxElems - 1) / stride; }

// ---- G. the model file -------------------------------------------------------------------------------------------------------------------
struct Model {
	int dim = 0, components = 0;
	std::vector<float> mean, vectors, values;          // [dim], [components][dim], [components]
};

namespace json {
struct Mat { bool seen = false, f32 = false, sized = false; long long rows = -1, cols = -1; std::vector<float> data; bool hasData = false; };

struct Reader {
	const char* p; const char* end; int depth = 0; locale_t loc;
	void ws() { while (p < end && (*p == ' ' || *p == '\t' || *p == '\n' || *p == '\r')) ++p; }
	bool lit(char c) { ws(); if (p < end && *p == c) { ++p; return true; } return false; }
	bool peek(char c) { ws(); return p < end && *p == c; }
	bool string(std::string& s)
	{
		s.clear();
		if (!lit('"')) return false;
		while (p < end && *p != '"') {
			if (static_cast<unsigned char>(*p) < 0x20) return false;
			if (*p == '\\') {
				if (++p >= end) return false;
				switch (*p) {
				case '"': case '\\': case '/': s += *p; break;
				case 'b': case 'f': case 'n': case 'r': case 't': s += ' '; break;
				case 'u': if (end - p < 5) return false; p += 4; s += '?'; break;          // (no member name of the grammar needs one)
				default: return false;
				}
				++p;
			}
			else s += *p++;
		}
		if (p >= end) return false;
		++p;
		return true;
	}
	// -?digits[.digits][(e|E)[+-]digits] -> (float)strtod
	bool number(double& d)
	{
		ws();
		const char* b = p;
		if (p < end && *p == '-') ++p;
		const char* digits = p;
		while (p < end && *p >= '0' && *p <= '9') ++p;
		if (p == digits) return false;
		if (p < end && *p == '.') { ++p; const char* f = p; while (p < end && *p >= '0' && *p <= '9') ++p; if (p == f) return false; }
		if (p < end && (*p == 'e' || *p == 'E')) {
			++p;
			if (p < end && (*p == '+' || *p == '-')) ++p;
			const char* x = p;
			while (p < end && *p >= '0' && *p <= '9') ++p;
			if (p == x) return false;
		}
		const std::string word(b, p);
		char* e = nullptr;
		d = strtod_l(word.c_str(), &e, loc);
		return e && !*e;
	}
	bool word(const char* w) { ws(); const size_t n = strlen(w); if (static_cast<size_t>(end - p) >= n && !memcmp(p, w, n)) { p += n; return true; } return false; }
	bool skip()          // any value
	{
		if (++depth > 64) return false;
		bool ok = false;
		std::string s; double d;
		if (peek('{')) {
			++p; ok = true;
			if (!lit('}')) {
				do { ok = string(s) && lit(':') && skip(); } while (ok && lit(','));
				ok = ok && lit('}');
			}
		}
		else if (peek('[')) {
			++p; ok = true;
			if (!lit(']')) {
				do { ok = skip(); } while (ok && lit(','));
				ok = ok && lit(']');
			}
		}
		else if (peek('"')) ok = string(s);
		else ok = word("true") || word("false") || word("null") || number(d);
		--depth;
		return ok;
	}
	bool mat(Mat& m)
	{
		if (m.seen || !lit('{')) return false;
		m.seen = true;
		if (lit('}')) return true;
		std::string key, s; double d;
		do {
			if (!string(key) || !lit(':')) return false;
			if (key == "type") { if (!string(s)) return false; m.f32 = s == "32f"; }
			else if (key == "size") {
				if (m.sized || !lit('[') || !number(d)) return false;
				m.rows = d >= 0 && d <= 4e9 && d == floor(d) ? static_cast<long long>(d) : -1;
				if (!lit(',') || !number(d) || !lit(']')) return false;
				m.cols = d >= 0 && d <= 4e9 && d == floor(d) ? static_cast<long long>(d) : -1;
				m.sized = true;
			}
			else if (key == "data") {
				if (m.hasData || !lit('[')) return false;
				m.hasData = true;
				if (!lit(']')) {
					do {
						if (!number(d)) return false;
						const float f = static_cast<float>(d);
						if (!isfinite(f)) return false;
						if (m.data.size() >= (kMaxDim * 64)) return false;          // far beyond any model the limits admit, before memory runs out
						m.data.push_back(f);
					} while (lit(','));
					if (!lit(']')) return false;
				}
			}
			else if (!skip()) return false;
		} while (lit(','));
		return lit('}');
	}
};
} // namespace json

inline bool parse_text(const char* text, size_t bytes, Model& m, std::string* why)
{
	auto bad = [&](const char* w) { if (why) *why = w; return false; };
	static locale_t loc = newlocale(LC_ALL_MASK, "C", static_cast<locale_t>(0));
	json::Reader r{ text, text + bytes, 0, loc };
	json::Mat mean, vectors, values;
	if (!r.lit('{')) return bad("not a JSON object");
	if (!r.lit('}')) {
		std::string key;
		do {
			if (!r.string(key) || !r.lit(':')) return bad("malformed member");
			json::Mat* which = key == "mean" ? &mean : key == "vectors" ? &vectors : key == "values" ? &values : nullptr;
			if (which ? !r.mat(*which) : !r.skip()) return bad("malformed value");
		} while (r.lit(','));
		if (!r.lit('}')) return bad("unterminated object");
	}
	r.ws();
	if (r.p != r.end) return bad("text behind the object");
	for (const json::Mat* a : { &mean, &vectors, &values }) {
		if (!a->seen || !a->sized || !a->hasData) return bad("mean, vectors or values is missing, or has no size or data");
		if (!a->f32) return bad("a type other than 32f");
		if (a->rows < 0 || a->cols < 0 || static_cast<unsigned long long>(a->rows) * static_cast<unsigned long long>(a->cols) != a->data.size()) return bad("size does not match the data count");
	}
	const long long D = mean.cols, M = values.cols;
	if (mean.rows != 1 || values.rows != 1 || vectors.rows != M || vectors.cols != D) return bad("mean is not 1 x D, values not 1 x M or vectors not M x D");
	if (D < 1 || static_cast<size_t>(D) > kMaxDim || M < 1 || static_cast<size_t>(M) > kMaxComponents) return bad("D outside 1 .. 2^20 or M outside 1 .. 65535");
	m.dim = static_cast<int>(D); m.components = static_cast<int>(M);
	m.mean.swap(mean.data); m.vectors.swap(vectors.data); m.values.swap(values.data);
	return true;
}

inline bool parse_model(const char* path, Model& m, std::string* why)
{
	FILE* fp = path ? fopen(path, "rb") : nullptr;
	if (!fp) { if (why) *why = "cannot open the file"; return false; }
	std::string text;
	char buf[65536];
	size_t got;
	while ((got = fread(buf, 1, sizeof(buf), fp)) > 0) text.append(buf, got);
	const bool failed = ferror(fp) != 0;
	fclose(fp);
	if (failed) { if (why) *why = "read error"; return false; }
	return parse_text(text.data(), text.size(), m, why);
}

} // namespace pca
} // namespace compvhip
