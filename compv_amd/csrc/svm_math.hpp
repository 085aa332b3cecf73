// svm_math.hpp -- the arithmetic of SVM prediction (include/compv_hip.h, "SVM prediction", items A - F), written once for svm_kernels.hip, for the host
// helpers of api_svm.cpp and for the host checker (tests/host/svm_math_check.cpp): the three dot products in the reference's summation order, the table
// exponential, the vote, and the model-file parser.
// Every operation is a single IEEE binary64 operation in the order of the definition: the translation units are built with -ffp-contract=off, and nothing
// here may be fused -- m = d * d; s += m rounds twice, fma(d, d, s) once, and the last bit of a kernel value would differ from the reference's.
// Standard library only (strtod_l of POSIX 2008 for the C locale).
#pragma once
#include <locale.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SVM_HD __host__ __device__ __forceinline__
#else
#define SVM_HD inline
#endif

namespace compvhip {
namespace svm {

constexpr int kLinear = 0, kRbf = 2;          // libsvm's kernel_type numbers
constexpr int kMaxClasses = 32;
constexpr int kMaxPairs = kMaxClasses * (kMaxClasses - 1) / 2;
constexpr int kExpTable = 2048;

// ---- item B: dotSub (CompVMathDotDotSub_C) ----------------------------------------------------------------------------------------------------
// Lane j of one whole group of 16 columns takes the columns j, j + 4, j + 8, j + 12, in this order: s_j += (m_j + m_{j+4}) + (m_{j+8} + m_{j+12}).
SVM_HD void dotsub_lane(double& s, double a0, double a1, double a2, double a3, double b0, double b1, double b2, double b3)
{
	const double d0 = a0 - b0, d1 = a1 - b1, d2 = a2 - b2, d3 = a3 - b3;
	const double m0 = d0 * d0, m1 = d1 * d1, m2 = d2 * d2, m3 = d3 * d3;
	s += ((m0 + m1) + (m2 + m3));
}
// one column of the tail (pairs into s0, s1; a last column into s0)
SVM_HD void dotsub_one(double& s, double a, double b)
{
	const double d = a - b;
	s += d * d;
}
// `n` columns (a multiple of 16) of whole groups: a caller may feed a row chunk by chunk, every chunk a multiple of 16 long
template <typename A>
SVM_HD void dotsub_groups(double s[4], const A* a, const double* b, size_t n)
{
	for (size_t g = 0; g < n; g += 16)
		for (int j = 0; j < 4; ++j)
			dotsub_lane(s[j], a[g + j], a[g + j + 4], a[g + j + 8], a[g + j + 12], b[g + j], b[g + j + 4], b[g + j + 8], b[g + j + 12]);
}
// the n < 16 columns behind the last whole group, once, at the end
template <typename A>
SVM_HD void dotsub_tail(double s[4], const A* a, const double* b, size_t n)
{
	size_t c = 0;
	for (; c + 1 < n; c += 2) { dotsub_one(s[0], a[c], b[c]); dotsub_one(s[1], a[c + 1], b[c + 1]); }
	if (c < n) dotsub_one(s[0], a[c], b[c]);
}
SVM_HD double lanes_sum(double s0, double s1, double s2, double s3)
{
	s0 += s2; s1 += s3; s0 += s1;
	return s0;
}
template <typename A>
SVM_HD double dotsub(const A* a, const double* b, size_t n)
{
	double s[4] = { 0.0, 0.0, 0.0, 0.0 };
	const size_t n16 = n & ~static_cast<size_t>(15);
	dotsub_groups(s, a, b, n16);
	dotsub_tail(s, a + n16, b + n16, n - n16);
	return lanes_sum(s[0], s[1], s[2], s[3]);
}

// ---- item D: the linear kernel value (Kernel::dot on dense nodes): one accumulator, the columns in order; `sum` runs on from chunk to chunk ----
template <typename A>
SVM_HD void linear_dot_chunk(double& sum, const A* a, const double* b, size_t n)
{
	for (size_t c = 0; c < n; ++c) sum += a[c] * b[c];
}

// ---- item E: the coefficient dot (CompVMathDotDot_C): the structure of dotSub on products, the groups counted from the segment's start ---------
SVM_HD void dot_lane(double& s, double a0, double a1, double a2, double a3, double b0, double b1, double b2, double b3)
{
	const double m0 = a0 * b0, m1 = a1 * b1, m2 = a2 * b2, m3 = a3 * b3;
	s += ((m0 + m1) + (m2 + m3));
}
// accumulator j of the dot over n elements: the four are independent, the order inside each is fixed
SVM_HD double dot_lane_total(const double* a, const double* b, int n, int j)
{
	double s = 0.0;
	const int n16 = n & ~15;
	for (int g = 0; g < n16; g += 16) dot_lane(s, a[g + j], a[g + j + 4], a[g + j + 8], a[g + j + 12], b[g + j], b[g + j + 4], b[g + j + 8], b[g + j + 12]);
	if (j < 2)
		for (int c = n16; c + 1 < n; c += 2) s += a[c + j] * b[c + j];
	if (j == 0 && (n & 1)) s += a[n - 1] * b[n - 1];
	return s;
}
SVM_HD double dot(const double* a, const double* b, int n)
{
	return lanes_sum(dot_lane_total(a, b, n, 0), dot_lane_total(a, b, n, 1), dot_lane_total(a, b, n, 2), dot_lane_total(a, b, n, 3));
}

// ---- item C: exp_ref (CompVMathExpExp_minpack1_64f64f_C, after herumi/fmath) -------------------------------------------------------------------
SVM_HD uint64_t bits_of(double d)
{
#if defined(__HIP_DEVICE_COMPILE__)
	return static_cast<uint64_t>(__double_as_longlong(d));
#else
	uint64_t u; memcpy(&u, &d, 8); return u;
#endif
}
SVM_HD double double_of(uint64_t u)
{
#if defined(__HIP_DEVICE_COMPILE__)
	return __longlong_as_double(static_cast<long long>(u));
#else
	double d; memcpy(&d, &u, 8); return d;
#endif
}
// T[i]: the 52 mantissa bits of pow(2, i / 2048) by the host's libm (exp2 of some libraries differs in the last bit of a hundred entries)
inline void exp_table(uint64_t T[kExpTable])
{
	for (int i = 0; i < kExpTable; ++i) T[i] = bits_of(pow(2.0, i / 2048.0)) & ((static_cast<uint64_t>(1) << 52) - 1);
}
// Tab: anything with operator[](int) -> the table entry (a pointer on the host, an LDS view in the kernel)
template <typename Tab>
SVM_HD double exp_ref(double x, const Tab& T)
{
	const double b = 6755399441055744.0;                  // 3 * 2^51
	const double ca = 2954.6394437405970;                  // 2048 / ln 2
	const double cra = 0.00033845077175778578;             // ln 2 / 2048
	const double C1 = 1.0, C2 = 0.16666666685227835, C3 = 3.0000000027955394;
	const double expMin = -708.39641853226408, expMax = 709.78271289338397;
	x = x < expMin ? expMin : (x > expMax ? expMax : x);
	const double d = x * ca + b;
	const double t = (d - b) * cra - x;
	const uint64_t di = bits_of(d);
	const uint64_t u = ((di + 2095104ull) >> 11) << 52;
	const double y = (C3 - t) * (t * t) * C2 - t + C1;
	return y * double_of(u | static_cast<uint64_t>(T[static_cast<int>(di & 2047ull)]));
}
SVM_HD double rbf_value(double dist, double gamma, const uint64_t* T) { return exp_ref(dist * (-gamma), T); }

// ---- item E: decision values, votes, label ---------------------------------------------------------------------------------------------------
// pair p (row-major over i < j) -> its classes
SVM_HD void pair_classes(int p, int nrClass, int& ci, int& cj)
{
	ci = 0;
	while (p >= nrClass - 1 - ci) { p -= nrClass - 1 - ci; ++ci; }
	cj = ci + 1 + p;
}
// the first class with the most votes
SVM_HD int vote_winner(const int* votes, int nrClass)
{
	int best = 0;
	for (int c = 1; c < nrClass; ++c)
		if (votes[c] > votes[best]) best = c;
	return best;
}
// K: the l kernel values of one query; dec: nrClass * (nrClass - 1) / 2 values or nullptr; -> the label
inline int32_t decide(const double* K, int nrClass, int l, const int32_t* nSV, const double* svCoef, const double* rho, const int32_t* label, double* dec)
{
	int start[kMaxClasses], votes[kMaxClasses];
	start[0] = 0;
	for (int c = 1; c < nrClass; ++c) start[c] = start[c - 1] + nSV[c - 1];
	for (int c = 0; c < nrClass; ++c) votes[c] = 0;
	int p = 0;
	for (int i = 0; i < nrClass; ++i)
		for (int j = i + 1; j < nrClass; ++j, ++p) {
			const double sumi = dot(svCoef + static_cast<size_t>(j - 1) * l + start[i], K + start[i], nSV[i]);
			const double sumj = dot(svCoef + static_cast<size_t>(i) * l + start[j], K + start[j], nSV[j]);
			const double d = (sumi + sumj) - rho[p];
			if (dec) dec[p] = d;
			++votes[d > 0 ? i : j];
		}
	return label[vote_winner(votes, nrClass)];
}

// ---- items A, F: the model and its file ------------------------------------------------------------------------------------------------------
struct Model {
	int kernel = kRbf, nrClass = 0, l = 0, dim = 0;
	double gamma = 0.0;
	std::vector<double> sv;          // [l][dim]
	std::vector<double> svCoef;      // [nrClass - 1][l]
	std::vector<double> rho;         // [nrClass * (nrClass - 1) / 2]
	std::vector<int32_t> nSV, label; // [nrClass]
};

// what every model must satisfy, from a file or from the caller's arrays; nullptr: accepted, else the reason
inline const char* refuse_shape(int kernel, int nrClass, int l, int dim, const int32_t* nSV)
{
	if (kernel != kLinear && kernel != kRbf) return "kernel type is neither LINEAR nor RBF";
	if (nrClass < 2 || nrClass > kMaxClasses) return "nr_class outside 2 .. 32";
	if (l < 1 || dim < 1) return "no support vector, or no dimension";
	if (static_cast<int64_t>(l) * dim >= (static_cast<int64_t>(1) << 31) || static_cast<int64_t>(l) * (nrClass - 1) >= (static_cast<int64_t>(1) << 31))
		return "total_sv * dim or total_sv * (nr_class - 1) reaches 2^31";
	int64_t sum = 0;
	for (int c = 0; c < nrClass; ++c) {
		if (nSV[c] < 0) return "negative nr_sv";
		sum += nSV[c];
	}
	if (sum != l) return "nr_sv does not add up to total_sv";
	return nullptr;
}

namespace detail {
inline bool is_space(char c) { return c == ' ' || c == '\t' || c == '\n' || c == '\r' || c == '\v' || c == '\f'; }
// the next whitespace-delimited word of [p, end), as fscanf("%s") reads it
inline bool word(const char*& p, const char* end, std::string& out)
{
	while (p < end && is_space(*p)) ++p;
	const char* b = p;
	while (p < end && !is_space(*p)) ++p;
	out.assign(b, p);
	return !out.empty();
}
inline locale_t c_locale()
{
	static locale_t loc = newlocale(LC_ALL_MASK, "C", static_cast<locale_t>(0));
	return loc;
}
// the whole word as a number in the C locale
inline bool number(const std::string& w, double& v)
{
	char* e = nullptr;
	v = strtod_l(w.c_str(), &e, c_locale());
	return e != w.c_str() && *e == '\0';
}
inline bool integer(const std::string& w, int& v)
{
	char* e = nullptr;
	const long x = strtol(w.c_str(), &e, 10);
	if (e == w.c_str() || *e != '\0' || x < -2147483647L - 1 || x > 2147483647L) return false;
	v = static_cast<int>(x);
	return true;
}
} // namespace detail

// libsvm's text format (svm_save_model / svm_load_model).  false: the file is refused, *why says it (item F): it does not open or parse, is no C-SVC, has a
// kernel other than LINEAR or RBF, or an SV line that is not index:value for the indices 1 .. dim in order.
inline bool parse_model(const char* path, Model& m, std::string* why)
{
	auto no = [&](const char* what) { if (why) *why = what; return false; };
	FILE* fp = path ? fopen(path, "rb") : nullptr;
	if (!fp) return no("the model file does not open");
	std::string text;
	char buf[65536];
	for (size_t n; (n = fread(buf, 1, sizeof(buf), fp)) > 0;) text.append(buf, n);
	fclose(fp);
	const char* p = text.data();
	const char* const end = p + text.size();
	m = Model();
	bool haveType = false, haveKernel = false, haveGamma = false, inSV = false;
	std::string w, v;
	while (!inSV) {
		if (!detail::word(p, end, w)) return no("the header ends before the SV section");
		if (w == "SV") {
			while (p < end && *p != '\n') ++p;
			if (p < end) ++p;
			inSV = true;
		}
		else if (w == "svm_type") {
			if (!detail::word(p, end, v)) return no("svm_type without a value");
			if (v != "c_svc") return no("svm_type is not c_svc");
			haveType = true;
		}
		else if (w == "kernel_type") {
			if (!detail::word(p, end, v)) return no("kernel_type without a value");
			if (v == "linear") m.kernel = kLinear;
			else if (v == "rbf") m.kernel = kRbf;
			else return no("kernel_type is neither linear nor rbf");
			haveKernel = true;
		}
		else if (w == "degree" || w == "nr_class" || w == "total_sv") {
			int x = 0;
			if (!detail::word(p, end, v) || !detail::integer(v, x)) return no("an integer of the header does not parse");
			if (w == "nr_class") { if (x < 2 || x > kMaxClasses) return no("nr_class outside 2 .. 32"); m.nrClass = x; }
			if (w == "total_sv") m.l = x;
		}
		else if (w == "gamma" || w == "coef0") {
			double x = 0.0;
			if (!detail::word(p, end, v) || !detail::number(v, x)) return no("gamma or coef0 does not parse");
			if (w == "gamma") { m.gamma = x; haveGamma = true; }
		}
		else if (w == "rho" || w == "probA" || w == "probB") {
			if (!m.nrClass) return no("rho in front of nr_class");
			std::vector<double> x(static_cast<size_t>(m.nrClass) * (m.nrClass - 1) / 2);
			for (double& e : x)
				if (!detail::word(p, end, v) || !detail::number(v, e)) return no("a pairwise value of the header does not parse");
			if (w == "rho") m.rho = x;          // probA / probB are read over: probabilities are out of scope
		}
		else if (w == "label" || w == "nr_sv") {
			if (!m.nrClass) return no("label or nr_sv in front of nr_class");
			std::vector<int32_t> x(static_cast<size_t>(m.nrClass));
			for (int32_t& e : x) {
				int i = 0;
				if (!detail::word(p, end, v) || !detail::integer(v, i)) return no("a per-class value of the header does not parse");
				e = i;
			}
			(w == "label" ? m.label : m.nSV) = x;
		}
		else return no("unknown text in the header");
	}
	if (!haveType || !haveKernel || !m.nrClass || m.rho.empty() || m.label.empty() || m.nSV.empty()) return no("svm_type, kernel_type, nr_class, rho, label or nr_sv is missing");
	if (m.kernel == kRbf && !haveGamma) return no("an rbf model without gamma");
	if (m.l < 1) return no("total_sv is missing or below 1");
	const int nc1 = m.nrClass - 1;
	m.svCoef.assign(static_cast<size_t>(nc1) * m.l, 0.0);
	std::vector<double> row;
	for (int i = 0; i < m.l; ++i) {
		if (p >= end) return no("fewer SV lines than total_sv");
		const char* e = p;
		while (e < end && *e != '\n') ++e;
		std::string line(p, e);
		p = e < end ? e + 1 : end;
		const char* q = line.data();
		const char* const qe = q + line.size();
		for (int k = 0; k < nc1; ++k) {
			double x = 0.0;
			if (!detail::word(q, qe, v) || v.find(':') != std::string::npos || !detail::number(v, x)) return no("a coefficient of an SV line does not parse");
			m.svCoef[static_cast<size_t>(k) * m.l + i] = x;
		}
		row.clear();
		while (detail::word(q, qe, v)) {
			const size_t colon = v.find(':');
			int idx = 0;
			double x = 0.0;
			if (colon == std::string::npos || !detail::integer(v.substr(0, colon), idx) || !detail::number(v.substr(colon + 1), x)) return no("an index:value of an SV line does not parse");
			if (idx != static_cast<int>(row.size()) + 1) return no("a sparse SV line: the indices are not 1 .. dim in order");
			row.push_back(x);
		}
		if (i == 0) {
			if (row.empty()) return no("an SV line without values");
			if (static_cast<int64_t>(row.size()) * m.l >= (static_cast<int64_t>(1) << 31)) return no("total_sv * dim reaches 2^31");
			m.dim = static_cast<int>(row.size());
			m.sv.reserve(static_cast<size_t>(m.l) * m.dim);
		}
		else if (static_cast<int>(row.size()) != m.dim) return no("a sparse SV line: fewer or more values than the first line");
		m.sv.insert(m.sv.end(), row.begin(), row.end());
	}
	if (const char* bad = refuse_shape(m.kernel, m.nrClass, m.l, m.dim, m.nSV.data())) return no(bad);
	return true;
}

// the whole prediction of one query on the host: K (l values, written), dec (or nullptr) -> label
template <typename A>
inline int32_t predict_one(const Model& m, const uint64_t* T, const A* x, double* K, double* dec)
{
	for (int i = 0; i < m.l; ++i) {
		const double* sv = m.sv.data() + static_cast<size_t>(i) * m.dim;
		if (m.kernel == kRbf) K[i] = rbf_value(dotsub(x, sv, static_cast<size_t>(m.dim)), m.gamma, T);
		else { double s = 0.0; linear_dot_chunk(s, x, sv, static_cast<size_t>(m.dim)); K[i] = s; }
	}
	return decide(K, m.nrClass, m.l, m.nSV.data(), m.svCoef.data(), m.rho.data(), m.label.data(), dec);
}

} // namespace svm
} // namespace compvhip
