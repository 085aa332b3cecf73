// convert_math.hpp -- the per-pixel arithmetic and the plane geometry of the colour conversions (include/compv_hip.h, "colour conversion"), written once
// for the kernels of convert_kernels.hip, the host validation (api_features.cpp) and the host checker (tests/host/convert_math_check.cpp).
// Integer arithmetic is plain int with arithmetic right shifts; the HSV floats are single IEEE binary32 operations in the order of the definition
// (the translation units are built with -ffp-contract=off) with correctly rounded division, the rounding to an integer goes through double.
// Standard library only.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define CONV_HD __host__ __device__ __forceinline__
#else
#define CONV_HD inline
#endif

namespace compvhip {
namespace conv {

// = compvhip_pixfmt of include/compv_hip.h
enum {
	kRGBA32 = 0, kARGB32 = 1, kBGRA32 = 2, kRGB24 = 3, kBGR24 = 4, kRGB565LE = 5, kRGB565BE = 6, kBGR565LE = 7, kBGR565BE = 8, kYUYV422 = 9, kUYVY422 = 10, kY = 11,
	kNV12 = 12, kNV21 = 13, kYUV420P = 14, kYUV422P = 15, kYUV444P = 16, kHSV = 17, kFormats = 18
};

CONV_HD int clamp8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// ---- YUV -> RGB: Y' = Y - 16, U' = U - 127, V' = V - 127 (127, not 128: the definition's constant) ---------------------------------------------------
// clamp8(v >> 5), with the clamp in front of the shift: 0 below 0, 8191 >> 5 = 255 above 8191, v >> 5 between.  Written this way round on purpose: for
// "shift, then clamp, then pack two channels" the gfx950 code generator selects v_ashr_pk_u8_i32 and merges its result as if bits 31:16 were zero; on the
// MI355X the word arm then stored 255 in the blue byte of pixels whose blue is 0 (docs/kernels/convert.md).  Same value, no such instruction.
CONV_HD int clamp8_shift5(int v) { return (v < 0 ? 0 : (v > 8191 ? 8191 : v)) >> 5; }

CONV_HD void yuv_to_rgb(int y, int u, int v, int& r, int& g, int& b)
{
	const int yp = 37 * (y - 16), up = u - 127, vp = v - 127;
	r = clamp8_shift5(yp + 51 * vp);
	g = clamp8_shift5(yp - 13 * up - 26 * vp);
	b = clamp8_shift5(yp + 65 * up);
}

// ---- RGB -> YUV: Y as in the grayscale call; U, V from the *_to_uv_planar_11 leaves (no value reaches a clamp: 16..239 and 16..240) -------------------
CONV_HD void rgb_to_yuv(int r, int g, int b, int& y, int& u, int& v)
{
	y = ((33 * r + 65 * g + 13 * b) >> 7) + 16;
	u = clamp8(((-38 * r - 74 * g + 112 * b) >> 8) + 128);
	v = clamp8(((112 * r - 94 * g - 18 * b) >> 8) + 128);
}

// 16-bit 5:6:5 sample (already in host order, red in the top bits) -> 8-bit channels by bit replication
CONV_HD void expand565(uint32_t k, int& c5hi, int& c6, int& c5lo)
{
	uint32_t r = (k & 0xF800u) >> 8; r |= r >> 5;
	uint32_t g = (k & 0x07E0u) >> 3; g |= g >> 6;
	uint32_t b = (k & 0x001Fu) << 3; b |= b >> 5;
	c5hi = static_cast<int>(r); c6 = static_cast<int>(g); c5lo = static_cast<int>(b);
}

// ---- RGB -> HSV ---------------------------------------------------------------------------------------------------------------------------------------
// The two reciprocal tables of the definition: entry i = num * (1 / i), the reciprocal one correctly rounded binary32 division and the product a second
// rounding -- NOT num / i, which differs from it in the last place at many i and moves 6 168 hues and 10 776 saturations of the 2^24 triples.  Entry 0 = 0
// (minus == 0 has diff == 0, max == 0 has minus == 0: the product is 0 either way).  num = 43 for the hue, 255 for the saturation.
CONV_HD float hsv_table_entry(float num, int i) { return i ? num * (1.f / static_cast<float>(i)) : 0.f; }

// "add or subtract 0.5 in double, truncate", then through int to uint8
CONV_HD int round_half_away(float f)
{
	const double d = static_cast<double>(f);
	return static_cast<int>(d >= 0.0 ? d + 0.5 : d - 0.5);
}

// scale43 = table43[max - min], scale255 = table255[max]
CONV_HD void rgb_to_hsv(int r, int g, int b, const float* table43, const float* table255, int& h, int& s, int& v)
{
	int mn = g < b ? g : b; mn = r < mn ? r : mn;
	int mx = g > b ? g : b; mx = r > mx ? r : mx;
	const int diff = (mx == r) ? (g - b) : ((mx == g) ? (b - r) : (r - g));
	const int minus = mx - mn;
	const float s43 = static_cast<float>(diff) * table43[minus];
	const float s255 = static_cast<float>(minus) * table255[mx];
	h = (static_cast<int>(static_cast<uint8_t>(round_half_away(s43))) + ((mx == r) ? 0 : ((mx == g) ? 85 : 171))) & 255;
	s = static_cast<int>(static_cast<uint8_t>(round_half_away(s255)));
	v = mx;
}

// ---- geometry -----------------------------------------------------------------------------------------------------------------------------------------
// plane count, least row bytes and row count of each plane of a W x H image; false for an unknown format or a zero size
inline bool layout(int fmt, size_t W, size_t H, int* planes, size_t minRowBytes[3], size_t rows[3])
{
	if (fmt < 0 || fmt >= kFormats || !W || !H) return false;
	const size_t cw = (W + 1) / 2, ch = (H + 1) / 2;
	int n = 1;
	size_t rb[3] = { 0, 0, 0 }, rr[3] = { 0, 0, 0 };
	rr[0] = H;
	if (fmt <= kBGRA32) rb[0] = 4 * W;
	else if (fmt <= kBGR24 || fmt == kHSV) rb[0] = 3 * W;
	else if (fmt <= kBGR565BE) rb[0] = 2 * W;
	else if (fmt <= kUYVY422) rb[0] = 4 * cw;
	else if (fmt == kY) rb[0] = W;
	else if (fmt <= kNV21) { n = 2; rb[0] = W; rb[1] = 2 * cw; rr[1] = ch; }
	else {
		n = 3; rb[0] = W;
		rb[1] = rb[2] = (fmt == kYUV444P) ? W : cw;
		rr[1] = rr[2] = (fmt == kYUV420P) ? ch : H;
	}
	if (planes) *planes = n;
	for (int p = 0; p < 3; ++p) { if (minRowBytes) minRowBytes[p] = rb[p]; if (rows) rows[p] = rr[p]; }
	return true;
}

CONV_HD bool is_yuv_source(int f) { return f == kYUYV422 || f == kUYVY422 || (f >= kNV12 && f <= kYUV444P); }
CONV_HD bool is_rgb_family(int f) { return f >= kRGBA32 && f <= kBGR565BE; }

// the served (source, destination) pairs
inline bool served(int in, int out)
{
	switch (out) {
	case kRGBA32: return is_yuv_source(in) || in == kY;
	case kRGB24: return is_yuv_source(in) || in == kY || in == kRGBA32 || in == kBGRA32 || in == kBGR24;
	case kBGR24: return in == kRGBA32 || in == kRGB24;
	case kHSV: return in == kRGB24 || in == kRGBA32 || is_yuv_source(in);
	case kYUV444P: return is_rgb_family(in);
	default: return false;
	}
}

// One pixel from source channels to destination channels.  Source: is_yuv_source -> (c0, c1, c2) = (Y, U, V); kY -> c0 = Y; RGB family -> (R, G, B).
// Destination: RGBA32 / RGB24 -> (R, G, B), BGR24 -> (B, G, R), HSV -> (H, S, V), YUV444P -> (Y, U, V).
template <int IN, int OUT>
CONV_HD void pixel(int c0, int c1, int c2, const float* table43, const float* table255, int& o0, int& o1, int& o2)
{
	int r = c0, g = c1, b = c2;
	if (IN == kY) { g = c0; b = c0; }
	else if (IN == kYUYV422 || IN == kUYVY422 || (IN >= kNV12 && IN <= kYUV444P)) yuv_to_rgb(c0, c1, c2, r, g, b);
	if (OUT == kHSV) rgb_to_hsv(r, g, b, table43, table255, o0, o1, o2);
	else if (OUT == kYUV444P) rgb_to_yuv(r, g, b, o0, o1, o2);
	else if (OUT == kBGR24) { o0 = b; o1 = g; o2 = r; }
	else { o0 = r; o1 = g; o2 = b; }
}

} // namespace conv
} // namespace compvhip
