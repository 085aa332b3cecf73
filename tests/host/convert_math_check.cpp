// convert_math_check.cpp -- compv_amd/csrc/convert_math.hpp on the host: a stand-alone program, standard library only, no GPU, built by
// tests/test_convert_host.py with AddressSanitizer and UBSan.
//   convert_math_check IN OUT
// IN:  int32 inFmt, outFmt, W, H, generate; then (generate == 0) the source's dense planes one behind the other (conv::layout).  generate == 1: the
//      program builds the exhaustive 4096 x 4096 frame itself -- channel 0 = i & 255, channel 1 = (i >> 8) & 255, channel 2 = i >> 16 at pixel i -- as YUV444P
//      planes or packed RGB24.
// OUT: the destination's dense planes one behind the other.
#include "../../compv_amd/csrc/convert_math.hpp"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace compvhip::conv;

namespace {
struct Planes { std::vector<uint8_t> bytes; size_t off[3], rowBytes[3], rows[3]; int n; };

bool shape(int fmt, size_t W, size_t H, Planes& p)
{
	if (!layout(fmt, W, H, &p.n, p.rowBytes, p.rows)) return false;
	size_t total = 0;
	for (int i = 0; i < 3; ++i) { p.off[i] = total; total += p.rowBytes[i] * p.rows[i]; }
	p.bytes.assign(total, 0);
	return true;
}

// pixel (x, y) of the source -> the channels conv::pixel() expects
void readPixel(int fmt, const Planes& s, size_t x, size_t y, int& c0, int& c1, int& c2)
{
	auto at = [&](int pl, size_t row, size_t byte) { return static_cast<int>(s.bytes.at(s.off[pl] + row * s.rowBytes[pl] + byte)); };
	c0 = c1 = c2 = 0;
	switch (fmt) {
	case kRGBA32: c0 = at(0, y, 4 * x); c1 = at(0, y, 4 * x + 1); c2 = at(0, y, 4 * x + 2); break;
	case kARGB32: c0 = at(0, y, 4 * x + 1); c1 = at(0, y, 4 * x + 2); c2 = at(0, y, 4 * x + 3); break;
	case kBGRA32: c0 = at(0, y, 4 * x + 2); c1 = at(0, y, 4 * x + 1); c2 = at(0, y, 4 * x); break;
	case kRGB24: c0 = at(0, y, 3 * x); c1 = at(0, y, 3 * x + 1); c2 = at(0, y, 3 * x + 2); break;
	case kBGR24: c0 = at(0, y, 3 * x + 2); c1 = at(0, y, 3 * x + 1); c2 = at(0, y, 3 * x); break;
	case kRGB565LE: case kRGB565BE: case kBGR565LE: case kBGR565BE: {
		const uint32_t b0 = static_cast<uint32_t>(at(0, y, 2 * x)), b1 = static_cast<uint32_t>(at(0, y, 2 * x + 1));
		const uint32_t k = (fmt == kRGB565BE || fmt == kBGR565BE) ? ((b0 << 8) | b1) : ((b1 << 8) | b0);
		int hi, mid, lo;
		expand565(k, hi, mid, lo);
		c1 = mid;
		if (fmt == kRGB565LE || fmt == kRGB565BE) { c0 = hi; c2 = lo; } else { c0 = lo; c2 = hi; }
		break;
	}
	case kYUYV422: c0 = at(0, y, 2 * x); c1 = at(0, y, 4 * (x >> 1) + 1); c2 = at(0, y, 4 * (x >> 1) + 3); break;
	case kUYVY422: c0 = at(0, y, 2 * x + 1); c1 = at(0, y, 4 * (x >> 1)); c2 = at(0, y, 4 * (x >> 1) + 2); break;
	case kY: c0 = at(0, y, x); break;
	case kNV12: c0 = at(0, y, x); c1 = at(1, y >> 1, x & ~static_cast<size_t>(1)); c2 = at(1, y >> 1, (x & ~static_cast<size_t>(1)) + 1); break;
	case kNV21: c0 = at(0, y, x); c2 = at(1, y >> 1, x & ~static_cast<size_t>(1)); c1 = at(1, y >> 1, (x & ~static_cast<size_t>(1)) + 1); break;
	case kYUV420P: c0 = at(0, y, x); c1 = at(1, y >> 1, x >> 1); c2 = at(2, y >> 1, x >> 1); break;
	case kYUV422P: c0 = at(0, y, x); c1 = at(1, y, x >> 1); c2 = at(2, y, x >> 1); break;
	case kYUV444P: c0 = at(0, y, x); c1 = at(1, y, x); c2 = at(2, y, x); break;
	default: break;
	}
}

// conv::pixel<IN, OUT> with the formats at run time
void convertPixel(int in, int out, int c0, int c1, int c2, const float* t43, const float* t255, int o[3])
{
	int r = c0, g = c1, b = c2;
	if (in == kY) { g = c0; b = c0; }
	else if (is_yuv_source(in)) yuv_to_rgb(c0, c1, c2, r, g, b);
	if (out == kHSV) rgb_to_hsv(r, g, b, t43, t255, o[0], o[1], o[2]);
	else if (out == kYUV444P) rgb_to_yuv(r, g, b, o[0], o[1], o[2]);
	else if (out == kBGR24) { o[0] = b; o[1] = g; o[2] = r; }
	else { o[0] = r; o[1] = g; o[2] = b; }
}
} // namespace

int main(int argc, char** argv)
{
	if (argc != 3) return 2;
	FILE* f = std::fopen(argv[1], "rb");
	if (!f) return 3;
	int32_t hdr[5];
	if (std::fread(hdr, sizeof(int32_t), 5, f) != 5) return 4;
	const int in = hdr[0], out = hdr[1];
	const size_t W = static_cast<size_t>(hdr[2]), H = static_cast<size_t>(hdr[3]);
	Planes s, d;
	if (!served(in, out) || !shape(in, W, H, s) || !shape(out, W, H, d)) return 5;
	if (hdr[4]) {
		if (W != 4096 || H != 4096 || (in != kYUV444P && in != kRGB24)) return 6;
		for (size_t i = 0; i < W * H; ++i) {
			const uint8_t c[3] = { static_cast<uint8_t>(i & 255), static_cast<uint8_t>((i >> 8) & 255), static_cast<uint8_t>(i >> 16) };
			for (int k = 0; k < 3; ++k) {
				if (in == kYUV444P) s.bytes[s.off[k] + i] = c[k];
				else s.bytes[3 * i + static_cast<size_t>(k)] = c[k];
			}
		}
	}
	else if (std::fread(s.bytes.data(), 1, s.bytes.size(), f) != s.bytes.size()) return 7;
	std::fclose(f);

	float t43[256], t255[256];
	for (int i = 0; i < 256; ++i) { t43[i] = hsv_table_entry(43.f, i); t255[i] = hsv_table_entry(255.f, i); }
	for (size_t y = 0; y < H; ++y)
		for (size_t x = 0; x < W; ++x) {
			int c0, c1, c2, o[3];
			readPixel(in, s, x, y, c0, c1, c2);
			convertPixel(in, out, c0, c1, c2, t43, t255, o);
			if (out == kYUV444P) { for (int k = 0; k < 3; ++k) d.bytes.at(d.off[k] + y * W + x) = static_cast<uint8_t>(o[k]); }
			else {
				const size_t bpp = out == kRGBA32 ? 4 : 3, at = y * d.rowBytes[0] + bpp * x;
				for (size_t k = 0; k < 3; ++k) d.bytes.at(at + k) = static_cast<uint8_t>(o[k]);
				if (bpp == 4) d.bytes.at(at + 3) = 0xff;
			}
		}
	f = std::fopen(argv[2], "wb");
	if (!f) return 8;
	const bool ok = std::fwrite(d.bytes.data(), 1, d.bytes.size(), f) == d.bytes.size();
	return std::fclose(f) == 0 && ok ? 0 : 9;
}
