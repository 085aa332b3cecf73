// svm_math_check.cpp -- compv_amd/csrc/svm_math.hpp on the host: a stand-alone program, standard library only, no GPU, built by tests/test_svm_host.py
// with AddressSanitizer and UBSan.
//   svm_math_check MODEL IN OUT
// MODEL: a libsvm model file.  Exit status 3 (the reason on stdout) when the parser refuses it; nothing else is read then.
// IN:  int32 type (0 float32, 1 float64), n, stride; n * stride query elements; int32 count; count float64 inputs of exp_ref.
// OUT: int32 kernel, nrClass, l, dim; float64 gamma; sv[l][dim], svCoef[nrClass - 1][l], rho[pairs] float64; nSV, label[nrClass] int32; labels[n] int32;
//      dec[n][pairs], K[n][l] float64; the count exp_ref values.
// K is computed the way svm_kvalues_kernel feeds the header -- whole 16-groups in chunks of 32 columns, the tail once at the end -- and the decision the
// way svm_decide_kernel does, one accumulator of a dot at a time; both are held against the header's one-call forms before anything is written.
#include "../../compv_amd/csrc/svm_math.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace compvhip::svm;

namespace {
[[noreturn]] void die(const char* what)
{
	std::fprintf(stderr, "svm_math_check: %s\n", what);
	std::exit(2);
}

template <typename T>
void readAll(std::FILE* f, T* p, size_t n)
{
	if (n && std::fread(p, sizeof(T), n, f) != n) die("short input");
}
template <typename T>
void writeAll(std::FILE* f, const T* p, size_t n)
{
	if (n && std::fwrite(p, sizeof(T), n, f) != n) die("short output");
}

bool same(double a, double b) { return bits_of(a) == bits_of(b); }

template <typename A>
void predictChunked(const Model& m, const uint64_t* T, const A* x, double* K, double* dec, int32_t* label)
{
	const size_t D = static_cast<size_t>(m.dim), d16 = D & ~static_cast<size_t>(15);
	for (int i = 0; i < m.l; ++i) {
		const double* sv = m.sv.data() + static_cast<size_t>(i) * D;
		if (m.kernel == kRbf) {
			double s[4] = { 0.0, 0.0, 0.0, 0.0 };
			for (size_t k0 = 0; k0 < d16; k0 += 32) dotsub_groups(s, x + k0, sv + k0, d16 - k0 < 32 ? d16 - k0 : 32);
			dotsub_tail(s, x + d16, sv + d16, D - d16);
			K[i] = rbf_value(lanes_sum(s[0], s[1], s[2], s[3]), m.gamma, T);
		}
		else {
			double s = 0.0;
			for (size_t k0 = 0; k0 < D; k0 += 32) linear_dot_chunk(s, x + k0, sv + k0, D - k0 < 32 ? D - k0 : 32);
			K[i] = s;
		}
	}
	std::vector<double> whole(static_cast<size_t>(m.l)), decWhole(m.rho.size());
	const int32_t labelWhole = predict_one(m, T, x, whole.data(), decWhole.data());
	for (int i = 0; i < m.l; ++i)
		if (!same(whole[static_cast<size_t>(i)], K[i])) die("the chunked kernel value differs from the one-call form");
	// the decision, accumulator by accumulator
	int start[kMaxClasses], votes[kMaxClasses];
	for (int c = 0, s = 0; c < m.nrClass; ++c) { start[c] = s; s += m.nSV[static_cast<size_t>(c)]; votes[c] = 0; }
	const int P = m.nrClass * (m.nrClass - 1) / 2;
	for (int p = 0; p < P; ++p) {
		int ci, cj;
		pair_classes(p, m.nrClass, ci, cj);
		double part[8];
		for (int w = 0; w < 8; ++w) {
			const int cls = w >= 4 ? cj : ci, row = w >= 4 ? ci : cj - 1;
			part[w] = dot_lane_total(m.svCoef.data() + static_cast<size_t>(row) * m.l + start[cls], K + start[cls], m.nSV[static_cast<size_t>(cls)], w & 3);
		}
		dec[p] = (lanes_sum(part[0], part[1], part[2], part[3]) + lanes_sum(part[4], part[5], part[6], part[7])) - m.rho[static_cast<size_t>(p)];
		if (!same(dec[p], decWhole[static_cast<size_t>(p)])) die("the per-accumulator decision value differs from the one-call form");
		++votes[dec[p] > 0 ? ci : cj];
	}
	*label = m.label[static_cast<size_t>(vote_winner(votes, m.nrClass))];
	if (*label != labelWhole) die("the label differs from the one-call form");
}
}

int main(int argc, char** argv)
{
	if (argc != 4) die("usage: svm_math_check MODEL IN OUT");
	Model m;
	std::string why;
	if (!parse_model(argv[1], m, &why)) {
		std::printf("refused: %s\n", why.c_str());
		return 3;
	}
	std::FILE* f = std::fopen(argv[2], "rb");
	if (!f) die("cannot open IN");
	int32_t h[3];
	readAll(f, h, 3);
	const int type = h[0];
	if ((type != 0 && type != 1) || h[1] < 0 || h[1] > (1 << 20) || h[2] < m.dim || h[2] > (1 << 20)) die("bad query geometry");
	const size_t n = static_cast<size_t>(h[1]), stride = static_cast<size_t>(h[2]);
	std::vector<float> x32(type == 0 ? n * stride : 0);
	std::vector<double> x64(type == 1 ? n * stride : 0);
	readAll(f, x32.data(), x32.size());
	readAll(f, x64.data(), x64.size());
	int32_t count = 0;
	readAll(f, &count, 1);
	if (count < 0 || count > (1 << 24)) die("bad exp count");
	std::vector<double> ein(static_cast<size_t>(count)), eout(static_cast<size_t>(count));
	readAll(f, ein.data(), ein.size());
	std::fclose(f);

	std::vector<uint64_t> T(kExpTable);
	exp_table(T.data());
	const size_t L = static_cast<size_t>(m.l), P = m.rho.size();
	std::vector<int32_t> labels(n);
	std::vector<double> dec(n * P), K(n * L);
	for (size_t i = 0; i < n; ++i) {
		if (type == 0) predictChunked(m, T.data(), x32.data() + i * stride, K.data() + i * L, dec.data() + i * P, &labels[i]);
		else predictChunked(m, T.data(), x64.data() + i * stride, K.data() + i * L, dec.data() + i * P, &labels[i]);
	}
	for (size_t i = 0; i < eout.size(); ++i) eout[i] = exp_ref(ein[i], T.data());

	std::FILE* o = std::fopen(argv[3], "wb");
	if (!o) die("cannot open OUT");
	const int32_t shape[4] = { m.kernel, m.nrClass, m.l, m.dim };
	writeAll(o, shape, 4);
	writeAll(o, &m.gamma, 1);
	writeAll(o, m.sv.data(), m.sv.size());
	writeAll(o, m.svCoef.data(), m.svCoef.size());
	writeAll(o, m.rho.data(), m.rho.size());
	writeAll(o, m.nSV.data(), m.nSV.size());
	writeAll(o, m.label.data(), m.label.size());
	writeAll(o, labels.data(), labels.size());
	writeAll(o, dec.data(), dec.size());
	writeAll(o, K.data(), K.size());
	writeAll(o, eout.data(), eout.size());
	if (std::fclose(o)) die("cannot close OUT");
	return 0;
}
