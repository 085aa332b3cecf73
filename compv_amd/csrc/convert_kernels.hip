// convert_kernels.hip -- colour conversion (include/compv_hip.h, "colour conversion"), hand-written HIP for gfx950.
//
// Replaces, behind compvhip_convert_frames / compvhip_convert_u8, the RGBx, HSV and YUV444P arms of CompVImage::convert
// (base/image/compv_image.cxx:662-685) with the plain leaves
//   base/image/compv_image_conv_to_rgbx.cxx:511-776      Y / planar / semi-planar / packed YUV -> RGBA32 | RGB24, RGB family -> RGB24 | BGR24
//   base/image/compv_image_conv_hsv.cxx:285-310          RGB24 | RGBA32 -> HSV
//   base/image/compv_image_conv_to_yuv444p.cxx           RGB family -> YUV444P (leaves in compv_image_conv_rgbfamily.cxx)
// The arithmetic is convert_math.hpp's, shared with the host checker.
//
// One templated streaming kernel: a thread owns 8 adjacent pixels of one row (8 x 3 bytes end on a dword boundary), loads them, converts them in
// registers and stores them.  Two instances per pair:
//   VEC     every plane pointer, rowBytes and frameBytes of both images is a multiple of 16: whole groups move as 4- to 16-byte words per lane (two or three
//           per lane where a group is 24 or 32 bytes); the last, partial group of a row takes the byte loop
//   scalar  anything else: every group takes the byte loop
// HSV instances build the two 256-entry reciprocal tables in LDS first (one division per thread and table).
#include "kernels.hpp"
#include "frame_slices.hpp"
#include "convert_math.hpp"

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace compvhip {
using namespace conv;

constexpr int kConvThreads = 256, kConvGroup = 8;

// bytes of a group of 8 pixels in plane p of format F (0: the format has no such plane)
template <int F> __host__ __device__ constexpr int groupBytes(int p)
{
	return p == 0 ? ((F <= kBGRA32) ? 32 : ((F <= kBGR24 || F == kHSV) ? 24 : (F <= kUYVY422 ? 16 : 8)))
	              : ((F == kNV12 || F == kNV21) ? (p == 1 ? 8 : 0) : ((F == kYUV420P || F == kYUV422P) ? 4 : (F == kYUV444P ? 8 : 0)));
}
// the row of plane p that holds image row y
template <int F> __device__ __forceinline__ int planeRow(int p, int y) { return (p && (F == kNV12 || F == kNV21 || F == kYUV420P)) ? (y >> 1) : y; }

struct MemBytes {   // a group's bytes where they lie
	const uint8_t* p[3];
	__device__ __forceinline__ int get(int pl, int off) const { return p[pl][off]; }
};
struct RegBytes {   // a group's bytes in registers (indices are compile-time constants after unrolling)
	uint32_t w[3][8];
	__device__ __forceinline__ int get(int pl, int off) const { return static_cast<int>((w[pl][off >> 2] >> (8 * (off & 3))) & 0xffu); }
};

// pixel i of the group -> the source channels conv::pixel() expects
template <int F, typename Bytes>
__device__ __forceinline__ void readPixel(const Bytes& s, int i, int& c0, int& c1, int& c2)
{
	if constexpr (F <= kBGRA32) {
		const int o = 4 * i;
		if (F == kRGBA32) { c0 = s.get(0, o); c1 = s.get(0, o + 1); c2 = s.get(0, o + 2); }
		else if (F == kARGB32) { c0 = s.get(0, o + 1); c1 = s.get(0, o + 2); c2 = s.get(0, o + 3); }
		else { c0 = s.get(0, o + 2); c1 = s.get(0, o + 1); c2 = s.get(0, o); }
	}
	else if constexpr (F <= kBGR24) {
		const int o = 3 * i;
		if (F == kRGB24) { c0 = s.get(0, o); c1 = s.get(0, o + 1); c2 = s.get(0, o + 2); }
		else { c0 = s.get(0, o + 2); c1 = s.get(0, o + 1); c2 = s.get(0, o); }
	}
	else if constexpr (F <= kBGR565BE) {
		const uint32_t b0 = static_cast<uint32_t>(s.get(0, 2 * i)), b1 = static_cast<uint32_t>(s.get(0, 2 * i + 1));
		const uint32_t k = (F == kRGB565BE || F == kBGR565BE) ? ((b0 << 8) | b1) : ((b1 << 8) | b0);
		int hi, mid, lo;
		expand565(k, hi, mid, lo);
		c1 = mid;
		if (F == kRGB565LE || F == kRGB565BE) { c0 = hi; c2 = lo; } else { c0 = lo; c2 = hi; }
	}
	else if constexpr (F == kYUYV422) { c0 = s.get(0, 2 * i); c1 = s.get(0, 4 * (i >> 1) + 1); c2 = s.get(0, 4 * (i >> 1) + 3); }
	else if constexpr (F == kUYVY422) { c0 = s.get(0, 2 * i + 1); c1 = s.get(0, 4 * (i >> 1)); c2 = s.get(0, 4 * (i >> 1) + 2); }
	else if constexpr (F == kY) { c0 = s.get(0, i); c1 = c2 = 0; }
	else if constexpr (F == kNV12) { c0 = s.get(0, i); c1 = s.get(1, i & ~1); c2 = s.get(1, (i & ~1) + 1); }
	else if constexpr (F == kNV21) { c0 = s.get(0, i); c2 = s.get(1, i & ~1); c1 = s.get(1, (i & ~1) + 1); }
	else if constexpr (F == kYUV444P) { c0 = s.get(0, i); c1 = s.get(1, i); c2 = s.get(2, i); }
	else { c0 = s.get(0, i); c1 = s.get(1, i >> 1); c2 = s.get(2, i >> 1); }   // 4:2:0 and 4:2:2 planar
}

template <int BYTES> __device__ __forceinline__ void loadWords(const uint8_t* p, uint32_t* w)
{
	if constexpr (BYTES == 32) {
		const uint4 a = reinterpret_cast<const uint4*>(p)[0], b = reinterpret_cast<const uint4*>(p)[1];
		w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w; w[4] = b.x; w[5] = b.y; w[6] = b.z; w[7] = b.w;
	}
	else if constexpr (BYTES == 24) {
		const uint2 a = reinterpret_cast<const uint2*>(p)[0], b = reinterpret_cast<const uint2*>(p)[1], c = reinterpret_cast<const uint2*>(p)[2];
		w[0] = a.x; w[1] = a.y; w[2] = b.x; w[3] = b.y; w[4] = c.x; w[5] = c.y;
	}
	else if constexpr (BYTES == 16) { const uint4 a = reinterpret_cast<const uint4*>(p)[0]; w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w; }
	else if constexpr (BYTES == 8) { const uint2 a = reinterpret_cast<const uint2*>(p)[0]; w[0] = a.x; w[1] = a.y; }
	else if constexpr (BYTES == 4) w[0] = reinterpret_cast<const uint32_t*>(p)[0];
}
template <int BYTES> __device__ __forceinline__ void storeWords(uint8_t* p, const uint32_t* w)
{
	if constexpr (BYTES == 32) {
		reinterpret_cast<uint4*>(p)[0] = make_uint4(w[0], w[1], w[2], w[3]);
		reinterpret_cast<uint4*>(p)[1] = make_uint4(w[4], w[5], w[6], w[7]);
	}
	else if constexpr (BYTES == 24) {
		reinterpret_cast<uint2*>(p)[0] = make_uint2(w[0], w[1]);
		reinterpret_cast<uint2*>(p)[1] = make_uint2(w[2], w[3]);
		reinterpret_cast<uint2*>(p)[2] = make_uint2(w[4], w[5]);
	}
	else if constexpr (BYTES == 8) reinterpret_cast<uint2*>(p)[0] = make_uint2(w[0], w[1]);
}

template <int IN, int OUT, bool VEC>
__global__ __launch_bounds__(kConvThreads) void convert_kernel(ConvertArgs a)
{
	__shared__ float s_t43[256], s_t255[256];
	if constexpr (OUT == kHSV) {
		s_t43[threadIdx.x] = hsv_table_entry(43.f, static_cast<int>(threadIdx.x));
		s_t255[threadIdx.x] = hsv_table_entry(255.f, static_cast<int>(threadIdx.x));
		__syncthreads();
	}
	const int x0 = (blockIdx.x * kConvThreads + threadIdx.x) * kConvGroup;
	const int y = blockIdx.y;
	const size_t frame = blockIdx.z;
	if (x0 >= a.W) return;
	const int n = a.W - x0 < kConvGroup ? a.W - x0 : kConvGroup;
	const size_t g = static_cast<size_t>(x0 / kConvGroup);
	// the group's first byte in every plane it has
	MemBytes src;
	uint8_t* dst[3];
#pragma unroll
	for (int p = 0; p < 3; ++p) {
		src.p[p] = groupBytes<IN>(p) ? a.in[p] + frame * a.inFrame[p] + static_cast<size_t>(planeRow<IN>(p, y)) * a.inRow[p] + g * groupBytes<IN>(p) : nullptr;
		dst[p] = groupBytes<OUT>(p) ? a.out[p] + frame * a.outFrame[p] + static_cast<size_t>(planeRow<OUT>(p, y)) * a.outRow[p] + g * groupBytes<OUT>(p) : nullptr;
	}
	constexpr int obpp = (OUT == kRGBA32) ? 4 : (OUT == kYUV444P ? 1 : 3);
	if (VEC && n == kConvGroup) {
		RegBytes rb;
		loadWords<groupBytes<IN>(0)>(src.p[0], rb.w[0]);
		loadWords<groupBytes<IN>(1)>(src.p[1], rb.w[1]);
		loadWords<groupBytes<IN>(2)>(src.p[2], rb.w[2]);
		uint32_t ow[3][8] = {};
#pragma unroll
		for (int i = 0; i < kConvGroup; ++i) {
			int c0, c1, c2, o[3];
			readPixel<IN>(rb, i, c0, c1, c2);
			pixel<IN, OUT>(c0, c1, c2, s_t43, s_t255, o[0], o[1], o[2]);
			if constexpr (OUT == kYUV444P) {
#pragma unroll
				for (int p = 0; p < 3; ++p) ow[p][i >> 2] |= static_cast<uint32_t>(o[p]) << (8 * (i & 3));
			}
			else {
#pragma unroll
				for (int k = 0; k < obpp; ++k) {
					const int byte = obpp * i + k;
					ow[0][byte >> 2] |= (k < 3 ? static_cast<uint32_t>(o[k]) : 0xffu) << (8 * (byte & 3));
				}
			}
		}
		storeWords<groupBytes<OUT>(0)>(dst[0], ow[0]);
		storeWords<groupBytes<OUT>(1)>(dst[1], ow[1]);
		storeWords<groupBytes<OUT>(2)>(dst[2], ow[2]);
		return;
	}
	for (int i = 0; i < n; ++i) {   // the byte loop: unaligned images, and the last partial group of a row
		int c0, c1, c2, o[3];
		readPixel<IN>(src, i, c0, c1, c2);
		pixel<IN, OUT>(c0, c1, c2, s_t43, s_t255, o[0], o[1], o[2]);
		if constexpr (OUT == kYUV444P) {
			dst[0][i] = static_cast<uint8_t>(o[0]); dst[1][i] = static_cast<uint8_t>(o[1]); dst[2][i] = static_cast<uint8_t>(o[2]);
		}
		else {
			uint8_t* q = dst[0] + obpp * i;
			q[0] = static_cast<uint8_t>(o[0]); q[1] = static_cast<uint8_t>(o[1]); q[2] = static_cast<uint8_t>(o[2]);
			if (obpp == 4) q[3] = 0xff;
		}
	}
}

template <int IN, int OUT>
static hipError_t launchPair(const ConvertArgs& a, bool vec, int frames, hipStream_t stream)
{
	const int groups = (a.W + kConvGroup - 1) / kConvGroup;
	const dim3 grid((groups + kConvThreads - 1) / kConvThreads, a.H, frames), block(kConvThreads);
	if (vec) hipLaunchKernelGGL((convert_kernel<IN, OUT, true>), grid, block, 0, stream, a);
	else hipLaunchKernelGGL((convert_kernel<IN, OUT, false>), grid, block, 0, stream, a);
	return hipGetLastError();
}

// at most kMaxFramesPerLaunch frames (blockIdx.z), at most 65 535 rows (blockIdx.y)
static hipError_t launch_convert_slice(const ConvertArgs& a, int inFmt, int outFmt, bool vec, int frames, hipStream_t stream)
{
	switch (inFmt * kFormats + outFmt) {
#define CONV_CASE(I, O) case (I) * kFormats + (O): return launchPair<I, O>(a, vec, frames, stream)
#define CONV_FROM_YUV(O) CONV_CASE(kNV12, O); CONV_CASE(kNV21, O); CONV_CASE(kYUV420P, O); CONV_CASE(kYUV422P, O); CONV_CASE(kYUV444P, O); \
	CONV_CASE(kYUYV422, O); CONV_CASE(kUYVY422, O)
	CONV_FROM_YUV(kRGBA32); CONV_FROM_YUV(kRGB24); CONV_FROM_YUV(kHSV);
	CONV_CASE(kY, kRGBA32); CONV_CASE(kY, kRGB24);
	CONV_CASE(kRGBA32, kRGB24); CONV_CASE(kBGRA32, kRGB24); CONV_CASE(kBGR24, kRGB24); CONV_CASE(kRGBA32, kBGR24); CONV_CASE(kRGB24, kBGR24);
	CONV_CASE(kRGB24, kHSV); CONV_CASE(kRGBA32, kHSV);
	CONV_CASE(kRGBA32, kYUV444P); CONV_CASE(kARGB32, kYUV444P); CONV_CASE(kBGRA32, kYUV444P); CONV_CASE(kRGB24, kYUV444P); CONV_CASE(kBGR24, kYUV444P);
	CONV_CASE(kRGB565LE, kYUV444P); CONV_CASE(kRGB565BE, kYUV444P); CONV_CASE(kBGR565LE, kYUV444P); CONV_CASE(kBGR565BE, kYUV444P);
#undef CONV_FROM_YUV
#undef CONV_CASE
	default: return hipErrorInvalidValue;
	}
}

hipError_t launch_convert(const ConvertArgs& args, int inFmt, int outFmt, int frames, hipStream_t stream)
{
	if (!served(inFmt, outFmt) || args.W <= 0 || args.H <= 0 || args.H > 65535) return hipErrorInvalidValue;
	// the word path: every address a lane forms is base + multiples of its word size when all of these are multiples of 16
	uintptr_t bits = 0;
	for (int p = 0; p < 3; ++p) {
		if (args.in[p]) bits |= reinterpret_cast<uintptr_t>(args.in[p]) | args.inRow[p] | (frames > 1 ? args.inFrame[p] : 0);
		if (args.out[p]) bits |= reinterpret_cast<uintptr_t>(args.out[p]) | args.outRow[p] | (frames > 1 ? args.outFrame[p] : 0);
	}
	const bool vec = (bits & 15) == 0;
	return for_frame_slices(frames, [&](int f0, int nf) {
		ConvertArgs a = args;
		for (int p = 0; p < 3; ++p) {
			if (a.in[p]) a.in[p] += static_cast<size_t>(f0) * a.inFrame[p];
			if (a.out[p]) a.out[p] += static_cast<size_t>(f0) * a.outFrame[p];
		}
		return launch_convert_slice(a, inFmt, outFmt, vec, nf, stream);
	});
}

} // namespace compvhip
