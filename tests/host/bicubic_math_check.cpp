// bicubic_math_check.cpp -- compv_amd/csrc/bicubic_math.hpp on the host: a stand-alone program, standard library only, no GPU, built by
// tests/test_bicubic_host.py with AddressSanitizer and UBSan.
//   bicubic_math_check IN OUT
// IN:  int32 W, H, S, Wout, Hout, defaultValue; float32 left, right, top, bottom (the clipped ROI); the frame, H * S bytes; mapX, mapY of Wout * Hout float32.
// OUT: the uint8 plane (Wout * Hout bytes), then the float32 plane (Wout * Hout values): paragraph F of include/compv_hip.h for every pixel.
// With S >= 4 a tap row is read the way the kernel reads it: one 4-byte word at quad_base, tap k = byte x_k - base.  Below, byte by byte.
#include "../../compv_amd/csrc/bicubic_math.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace compvhip::bicubic;

namespace {
[[noreturn]] void die(const char* what)
{
	std::fprintf(stderr, "bicubic_math_check: %s\n", what);
	std::exit(2);
}

template <typename T>
void readAll(std::FILE* f, T* p, size_t n)
{
	if (n && std::fread(p, sizeof(T), n, f) != n) die("short input");
}
}

int main(int argc, char** argv)
{
	if (argc != 3) die("usage: bicubic_math_check IN OUT");
	std::FILE* f = std::fopen(argv[1], "rb");
	if (!f) die("cannot open IN");
	int32_t h[6];
	float roi[4];
	readAll(f, h, 6);
	readAll(f, roi, 4);
	const int W = h[0], H = h[1], S = h[2], Wout = h[3], Hout = h[4], def = h[5];
	if (W < 1 || H < 1 || S < W || Wout < 1 || Hout < 1 || def < 0 || def > 255 || W > 32767 || H > 32767 || S > 65536 || Wout > 32767 || Hout > 32767) die("bad geometry");
	const size_t n = static_cast<size_t>(Wout) * Hout;
	// heap blocks of the exact size: AddressSanitizer sees a read one byte past the frame
	std::vector<uint8_t> frame(static_cast<size_t>(S) * H);
	std::vector<float> mx(n), my(n), outF(n);
	std::vector<uint8_t> outB(n);
	readAll(f, frame.data(), frame.size());
	readAll(f, mx.data(), n);
	readAll(f, my.data(), n);
	std::fclose(f);
	const float left = roi[0], right = roi[1], top = roi[2], bottom = roi[3];
	const bool quad = S >= 4;

	for (size_t i = 0; i < n; ++i) {
		const float x = mx[i], y = my[i];
		if (!(x >= left && x <= right && y >= top && y <= bottom)) {          // ordered compares: a NaN is outside
			outB[i] = static_cast<uint8_t>(def); outF[i] = static_cast<float>(def);
			continue;
		}
		int xi, yi, xk[4], yk[4];
		float xf, xf2, xf3, yf, yf2, yf3;
		split(x, xi, xf, xf2, xf3);
		split(y, yi, yf, yf2, yf3);
		for (int k = 0; k < 4; ++k) { xk[k] = clamp_tap(xi - 1 + k, W - 1); yk[k] = clamp_tap(yi - 1 + k, H - 1); }
		const int base = quad_base(xk[0], W);
		float I[4][4];
		for (int r = 0; r < 4; ++r) {
			const uint8_t* row = frame.data() + static_cast<size_t>(yk[r]) * S;
			if (quad) {
				if (base < 0 || base + 3 >= S) die("the 4-byte word leaves the row");
				uint32_t w;
				std::memcpy(&w, row + base, sizeof(w));          // little endian, like the device
				for (int k = 0; k < 4; ++k) {
					const int sel = xk[k] - base;
					if (sel < 0 || sel > 3) die("a tap selector outside 0 .. 3");
					I[r][k] = static_cast<float>(w >> (8 * sel) & 0xffu);
				}
			}
			else for (int k = 0; k < 4; ++k) I[r][k] = static_cast<float>(row[xk[k]]);
		}
		float c[4];
		for (int r = 0; r < 4; ++r) c[r] = hermite_row(I[r][0], I[r][1], I[r][2], I[r][3], xf, xf2, xf3);
		const float w = clip255(hermite_col(c[0], c[1], c[2], c[3], yf, yf2, yf3));
		outF[i] = w;
		outB[i] = to_u8(w);
	}

	std::FILE* o = std::fopen(argv[2], "wb");
	if (!o) die("cannot open OUT");
	if (std::fwrite(outB.data(), 1, n, o) != n || std::fwrite(outF.data(), sizeof(float), n, o) != n) die("short output");
	std::fclose(o);
	return 0;
}
