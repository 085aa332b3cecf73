// remap_kernels.hip -- geometric resampling for gfx950: CompVImageRemap::process (base/image/compv_image_remap.cxx) and the inverse warp of
// CompVImage::warpInverse (base/image/compv_image.cxx:997-1195), which is the same gather behind a coordinate table.
// Definition: include/compv_hip.h (section "remap and inverse warp"), docs/kernels/remap.md.
//
//   remap_kernel<SRC, INTERP, OutT>   ONE kernel family, specialised at compile time over where the source coordinates come from (a float32 map, the
//                           running-sum tables of a 2 x 3 matrix, those of a 3 x 3 matrix with its one division per pixel, the lens model of a
//                           camera's 14-float coefficient record: include/compv_hip.h, "lens undistortion"), the interpolation (nearest,
//                           bilinear) and the output type (uint8, float32).  A workgroup owns a 256 x 4 tile of the destination, one wave per row; a lane
//                           produces 4 adjacent pixels and stores them as one dword (uint8) or one 16-byte vector (float32).  The group that crosses Wout,
//                           and every group of a destination that is not aligned, stores single elements, so stride padding is never written.
//                           The coordinates, the inside test, the four gather offsets and the four weights of a lane's pixels are worked out ONCE and kept
//                           in registers; the workgroup then loops over `framesPerGroup` frames (8 when the map or matrix is shared, 1 when every frame
//                           has its own), so a shared map is read once per 8 frames.  A pixel outside the ROI gathers from offset 0 and is replaced by
//                           the default value afterwards: no divergent branch.  The bilinear forms load the two neighbours of a row as one 2-byte pair: 8 loads per lane
//                           and frame in flight.  No LDS, no atomic.
//   remap_bicubic_kernel<SRC, OutT>   The same tile, coordinates (remap_coords, shared), stores and frame loop for the bicubic forms (paragraph F of the
//                           definition; the arithmetic is bicubic_math.hpp, unfused).  16 taps per pixel: a tap row is one unaligned 4-byte load whose bytes
//                           the four packed selectors pick: 4 loads per pixel and frame.
#include "bicubic_math.hpp"
#include "undistort_math.hpp"
#include "device.hpp"
#include "frame_slices.hpp"

namespace compvhip {
namespace {

constexpr int kRemapTileW = 256, kRemapTileH = 4;   // 64 lanes x 4 pixels, one wave per row
enum { kPairLoHi = 0, kPairHiHi = 1, kPairLoLo = 2, kPairLoFar = 3 };   // where I[.][x1] and I[.][x2] sit relative to the 2 bytes loaded: (0, 1), (1, 1), (0, 0), (0, 2)

// 2 adjacent bytes at any address, as one load (global memory takes unaligned accesses)
__device__ __forceinline__ uint32_t load_pair(const uint8_t* p)
{
	uint16_t v;
	__builtin_memcpy(&v, p, sizeof(v));
	return v;
}

// ---- source coordinates of the lane's pixels (pixels >= n keep a NaN: outside, and never stored): shared by every kernel of this file ----
template <int SRC>
__device__ __forceinline__ void remap_coords(const RemapArgs& a, int f0, int j, int i0, int n, float (&x)[4], float (&y)[4])
{
#pragma unroll
	for (int b = 0; b < 4; ++b) x[b] = y[b] = __builtin_nanf("");
	if (SRC == kRemapMap) {
		const size_t k = static_cast<size_t>(f0) * a.coordFrameStride + static_cast<size_t>(j) * a.Wout + i0;          // coordFrameStride: 0 for a shared map
		if (a.mapVec && n == 4) {
			const float4 vx = *reinterpret_cast<const float4*>(a.mapX + k), vy = *reinterpret_cast<const float4*>(a.mapY + k);
			x[0] = vx.x; x[1] = vx.y; x[2] = vx.z; x[3] = vx.w; y[0] = vy.x; y[1] = vy.y; y[2] = vy.z; y[3] = vy.w;
		}
		else {
#pragma unroll
			for (int b = 0; b < 4; ++b) if (b < n) { x[b] = a.mapX[k + b]; y[b] = a.mapY[k + b]; }
		}
	}
	else if (SRC == kRemapUndist) {
		// the lens model (undistort_math.hpp): the camera's 14-float record is wave-uniform, the coordinates are arithmetic in registers -- no map is read
		const float* __restrict__ rec = a.tables + static_cast<size_t>(f0) * a.coordFrameStride;          // coordFrameStride: 0 for a shared camera
		float c[undist::kCoeffs];
#pragma unroll
		for (int k = 0; k < undist::kCoeffs; ++k) c[k] = rec[k];
		const float Y = static_cast<float>(a.originY + j);          // exact: origin + size <= 32767
#pragma unroll
		for (int b = 0; b < 4; ++b) if (b < n) undist::map_entry(c, static_cast<float>(a.originX + i0 + b), Y, x[b], y[b]);
	}
	else {
		constexpr int R = SRC == kRemapWarp3 ? 3 : 2;          // table rows: ac, df[, gi] of Wout values, then by, ey[, hy] of Hout values
		const float* __restrict__ cols = a.tables + static_cast<size_t>(f0) * a.coordFrameStride;
		const float* __restrict__ rows = cols + static_cast<size_t>(R) * a.Wout;
		const float by = rows[j], ey = rows[a.Hout + j], hy = R == 3 ? rows[2 * a.Hout + j] : 0.f;
#pragma unroll
		for (int b = 0; b < 4; ++b) {
			if (b >= n) continue;
			const float X = cols[i0 + b] + by, Y = cols[a.Wout + i0 + b] + ey;
			if (R == 3) {
				const float Z = cols[2 * a.Wout + i0 + b] + hy;
				const float s = 1.f / Z;          // IEEE division, correctly rounded (the compiler's default for HIP: v_div_scale / v_div_fmas / v_div_fixup)
				x[b] = X * s; y[b] = Y * s;
			}
			else { x[b] = X; y[b] = Y; }
		}
	}
}

template <int SRC, int INTERP, typename OutT>
__global__ __launch_bounds__(256) void remap_kernel(RemapArgs a)
{
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const int ty = blockIdx.x / a.tilesX, tx = blockIdx.x - ty * a.tilesX;
	const int j = ty * kRemapTileH + wave, i0 = tx * kRemapTileW + 4 * lane;
	if (j >= a.Hout || i0 >= a.Wout) return;
	const int f0 = (a.group0 + static_cast<int>(blockIdx.y)) * a.framesPerGroup, nf = min(a.framesPerGroup, a.frames - f0);
	const int n = min(4, a.Wout - i0);          // pixels of this lane inside the row

	float x[4], y[4];
	remap_coords<SRC>(a, f0, j, i0, n, x, y);

	// ---- per pixel, once for all frames: inside, gather offsets, weights ----
	bool inside[4];
	int o11[4], dy[4], pick[4];          // offset of the pair (or, nearest, of the pixel) in the frame, (y2 - y1) * S, which bytes of the pair are I[.][x1], I[.][x2]
	float wA[4], wB[4], wC[4], wD[4];
#pragma unroll
	for (int b = 0; b < 4; ++b) {
		inside[b] = x[b] >= a.left && x[b] <= a.right && y[b] >= a.top && y[b] <= a.bottom;          // ordered compares: a NaN is outside
		o11[b] = dy[b] = 0; pick[b] = kPairLoHi; wA[b] = wB[b] = wC[b] = wD[b] = 0.f;
		if (!inside[b]) continue;          // 0 <= left <= x <= right <= W - 1 from here on (the launch function checks the ROI): every index below lies in the frame
		if (INTERP == kRemapNearest) {
			const int xi = static_cast<int>(static_cast<double>(x[b]) + 0.5), yi = static_cast<int>(static_cast<double>(y[b]) + 0.5);   // COMPV_MATH_ROUNDFU_2_NEAREST_INT
			o11[b] = min(yi, a.H - 1) * a.S + min(xi, a.W - 1);
		}
		else {
			const int x1 = min(static_cast<int>(x[b]), a.W - 1), x2 = min(static_cast<int>(x[b] + 1.f), a.W - 1);
			const int y1 = min(static_cast<int>(y[b]), a.H - 1), y2 = min(static_cast<int>(y[b] + 1.f), a.H - 1);
			const float xf = x[b] - static_cast<float>(x1), yf = y[b] - static_cast<float>(y1), xy = xf * yf;
			wA[b] = ((1.f - xf) - yf) + xy; wB[b] = xf - xy; wC[b] = yf - xy; wD[b] = xy;          // each operation rounds once (-ffp-contract=off)
			// x2 - x1 is 1, or 0 at the clamp (x1 == W - 1: the pair then starts one byte earlier), or 2 where x + 1.f rounds up to the next integer
			const int xb = x2 == x1 && x1 > 0 ? x1 - 1 : x1;
			pick[b] = x2 == x1 ? (xb != x1 ? kPairHiHi : kPairLoLo) : (x2 - x1 == 2 ? kPairLoFar : kPairLoHi);
			o11[b] = y1 * a.S + xb; dy[b] = (y2 - y1) * a.S;
		}
	}

	const float defF = static_cast<float>(a.defaultValue);
	for (int k = 0; k < nf; ++k) {
		const uint8_t* __restrict__ src = a.in + static_cast<size_t>(f0 + k) * a.inFrameStride;
		float p[4]; uint32_t q[4];
#pragma unroll
		for (int b = 0; b < 4; ++b) {
			if (INTERP == kRemapNearest) q[b] = inside[b] ? src[o11[b]] : static_cast<uint32_t>(a.defaultValue);
			else {
				// two loads of 2 bytes, not four of 1: the gathers are bound by the number of load instructions.  Both bytes of a pair lie in the row
				// (xb + 1 <= max(W - 1, 1) < S: launch_remap asks for S >= 2).
				const uint32_t r1 = load_pair(src + o11[b]), r2 = load_pair(src + o11[b] + dy[b]);
				uint32_t n11 = r1 & 0xffu, n12 = r1 >> 8, n21 = r2 & 0xffu, n22 = r2 >> 8;
				if (pick[b] == kPairHiHi) { n11 = n12; n21 = n22; }
				if (pick[b] == kPairLoLo) { n12 = n11; n22 = n21; }
				if (pick[b] == kPairLoFar) { n12 = src[o11[b] + 2]; n22 = src[o11[b] + dy[b] + 2]; }          // rare: x just below an integer
				const float i11 = static_cast<float>(n11), i12 = static_cast<float>(n12), i21 = static_cast<float>(n21), i22 = static_cast<float>(n22);
				// the reference's AVX2 leaf as its compiler contracts it: one product, three fused multiply-adds
				const float v = __fmaf_rn(i22, wD[b], __fmaf_rn(i21, wC[b], __fmaf_rn(i12, wB[b], i11 * wA[b])));
				p[b] = inside[b] ? v : defF;
				q[b] = inside[b] ? static_cast<uint32_t>(static_cast<int>(v)) & 0xffu : static_cast<uint32_t>(a.defaultValue);          // v in [0, 256): truncation
			}
		}
		const size_t at = static_cast<size_t>(f0 + k) * a.outFrameStride + static_cast<size_t>(j) * a.Sout + i0;          // in elements
		if (sizeof(OutT) == 1) {
			uint8_t* __restrict__ dst = static_cast<uint8_t*>(a.out) + at;
			if (a.wide && n == 4) *reinterpret_cast<uint32_t*>(dst) = q[0] | q[1] << 8 | q[2] << 16 | q[3] << 24;
			else {
#pragma unroll
				for (int b = 0; b < 4; ++b) if (b < n) dst[b] = static_cast<uint8_t>(q[b]);
			}
		}
		else {
			float* __restrict__ dst = static_cast<float*>(a.out) + at;
			if (a.wide && n == 4) *reinterpret_cast<float4*>(dst) = make_float4(p[0], p[1], p[2], p[3]);
			else {
#pragma unroll
				for (int b = 0; b < 4; ++b) if (b < n) dst[b] = p[b];
			}
		}
	}
}

// 4 adjacent bytes at any address, as one load
__device__ __forceinline__ uint32_t load_quad(const uint8_t* p)
{
	uint32_t v;
	__builtin_memcpy(&v, p, sizeof(v));
	return v;
}

// Paragraph F of the definition; the arithmetic is bicubic_math.hpp, which the host checker compiles too.  A tap row is ONE 4-byte load at
// base = quad_base(x_0, W) = min(x_0, max(W - 4, 0)) and tap k is byte x_k - base of it (0 .. 3 at both clamps); base + 3 stays inside the row because
// S >= 4 (launch_remap).
template <int SRC, typename OutT>
__global__ __launch_bounds__(256) void remap_bicubic_kernel(RemapArgs a)
{
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const int ty = blockIdx.x / a.tilesX, tx = blockIdx.x - ty * a.tilesX;
	const int j = ty * kRemapTileH + wave, i0 = tx * kRemapTileW + 4 * lane;
	if (j >= a.Hout || i0 >= a.Wout) return;
	const int f0 = (a.group0 + static_cast<int>(blockIdx.y)) * a.framesPerGroup, nf = min(a.framesPerGroup, a.frames - f0);
	const int n = min(4, a.Wout - i0);          // pixels of this lane inside the row

	float x[4], y[4];
	remap_coords<SRC>(a, f0, j, i0, n, x, y);

	// ---- per pixel, once for all frames: inside, the offset of tap row 0, the four tap selectors in one word, three row deltas, the fractions ----
	bool inside[4];
	int o0[4], d1[4], d2[4], d3[4];          // y_0 * S + base; (y_r - y_0) * S
	uint32_t sel[4];          // byte k: the bit shift 8 * (x_k - base) into the loaded word
	float xf[4], xf2[4], xf3[4], yf[4], yf2[4], yf3[4];
#pragma unroll
	for (int b = 0; b < 4; ++b) {
		inside[b] = x[b] >= a.left && x[b] <= a.right && y[b] >= a.top && y[b] <= a.bottom;          // ordered compares: a NaN is outside
		o0[b] = d1[b] = d2[b] = d3[b] = 0; sel[b] = 0; xf[b] = xf2[b] = xf3[b] = yf[b] = yf2[b] = yf3[b] = 0.f;
		if (!inside[b]) continue;          // 0 <= x <= W - 1 and 0 <= y <= H - 1 from here on (the launch function checks the ROI)
		int xi, yi;
		bicubic::split(x[b], xi, xf[b], xf2[b], xf3[b]);
		bicubic::split(y[b], yi, yf[b], yf2[b], yf3[b]);
		int xk[4], yk[4];
#pragma unroll
		for (int k = 0; k < 4; ++k) { xk[k] = bicubic::clamp_tap(xi - 1 + k, a.W - 1); yk[k] = bicubic::clamp_tap(yi - 1 + k, a.H - 1); }   // to the frame, not to the ROI
		const int base = bicubic::quad_base(xk[0], a.W);
		sel[b] = static_cast<uint32_t>(xk[0] - base) << 3 | static_cast<uint32_t>(xk[1] - base) << 11 | static_cast<uint32_t>(xk[2] - base) << 19 |
		         static_cast<uint32_t>(xk[3] - base) << 27;
		o0[b] = yk[0] * a.S + base;
		d1[b] = (yk[1] - yk[0]) * a.S; d2[b] = (yk[2] - yk[0]) * a.S; d3[b] = (yk[3] - yk[0]) * a.S;
	}

	const float defF = static_cast<float>(a.defaultValue);
	for (int k = 0; k < nf; ++k) {
		const uint8_t* __restrict__ src = a.in + static_cast<size_t>(f0 + k) * a.inFrameStride;
		float p[4]; uint32_t q[4];
#pragma unroll
		for (int b = 0; b < 4; ++b) {
			const uint8_t* const r0 = src + o0[b];          // an outside pixel gathers at offset 0 (bytes 0 .. 3 of the frame)
			const int dr[4] = { 0, d1[b], d2[b], d3[b] };
			const uint32_t s0 = sel[b] & 0xffu, s1 = sel[b] >> 8 & 0xffu, s2 = sel[b] >> 16 & 0xffu, s3 = sel[b] >> 24;
			float c[4];
#pragma unroll
			for (int r = 0; r < 4; ++r) {
				const uint32_t w = load_quad(r0 + dr[r]);
				const uint32_t t0 = w >> s0 & 0xffu, t1 = w >> s1 & 0xffu, t2 = w >> s2 & 0xffu, t3 = w >> s3 & 0xffu;
				c[r] = bicubic::hermite_row(static_cast<float>(t0), static_cast<float>(t1), static_cast<float>(t2), static_cast<float>(t3), xf[b], xf2[b], xf3[b]);
			}
			const float v = bicubic::clip255(bicubic::hermite_col(c[0], c[1], c[2], c[3], yf[b], yf2[b], yf3[b]));
			p[b] = inside[b] ? v : defF;
			q[b] = inside[b] ? static_cast<uint32_t>(bicubic::to_u8(v)) : static_cast<uint32_t>(a.defaultValue);
		}
		const size_t at = static_cast<size_t>(f0 + k) * a.outFrameStride + static_cast<size_t>(j) * a.Sout + i0;          // in elements
		if (sizeof(OutT) == 1) {
			uint8_t* __restrict__ dst = static_cast<uint8_t*>(a.out) + at;
			if (a.wide && n == 4) *reinterpret_cast<uint32_t*>(dst) = q[0] | q[1] << 8 | q[2] << 16 | q[3] << 24;
			else {
#pragma unroll
				for (int b = 0; b < 4; ++b) if (b < n) dst[b] = static_cast<uint8_t>(q[b]);
			}
		}
		else {
			float* __restrict__ dst = static_cast<float*>(a.out) + at;
			if (a.wide && n == 4) *reinterpret_cast<float4*>(dst) = make_float4(p[0], p[1], p[2], p[3]);
			else {
#pragma unroll
				for (int b = 0; b < 4; ++b) if (b < n) dst[b] = p[b];
			}
		}
	}
}

template <int SRC>
void launch_src(const RemapArgs& a, int interp, dim3 grid, hipStream_t stream)
{
	if (interp == kRemapNearest) hipLaunchKernelGGL((remap_kernel<SRC, kRemapNearest, uint8_t>), grid, dim3(256), 0, stream, a);
	else if (interp == kRemapBilinear) hipLaunchKernelGGL((remap_kernel<SRC, kRemapBilinear, uint8_t>), grid, dim3(256), 0, stream, a);
	else if (interp == kRemapBilinearF32) hipLaunchKernelGGL((remap_kernel<SRC, kRemapBilinear, float>), grid, dim3(256), 0, stream, a);
	else if (interp == kRemapBicubic) hipLaunchKernelGGL((remap_bicubic_kernel<SRC, uint8_t>), grid, dim3(256), 0, stream, a);
	else hipLaunchKernelGGL((remap_bicubic_kernel<SRC, float>), grid, dim3(256), 0, stream, a);
}

} // namespace

hipError_t launch_remap(const RemapArgs& args, int source, int interp, bool perFrame, hipStream_t stream)
{
	RemapArgs a = args;
	if (!a.in || !a.out || a.W < 1 || a.H < 1 || a.S < a.W || a.S < 2 || a.Wout < 1 || a.Hout < 1 || a.Sout < a.Wout || a.frames < 1) return hipErrorInvalidValue;
	const bool bicubic = interp == kRemapBicubic || interp == kRemapBicubicF32;
	if (source < kRemapMap || source > kRemapUndist || (interp != kRemapNearest && interp != kRemapBilinear && interp != kRemapBilinearF32 && !bicubic)) return hipErrorInvalidValue;
	if (bicubic && a.S < 4) return hipErrorInvalidValue;          // the 4-byte tap rows; no caller comes here: a plan's stride is a multiple of 8, the host calls stage at 64
	if (source == kRemapMap ? !a.mapX || !a.mapY : !a.tables) return hipErrorInvalidValue;
	// every offset of a frame fits an int; the ROI is empty or lies in the frame, so an inside pixel never gathers outside it
	if (static_cast<long long>(a.S) * a.H > INT32_MAX || a.W > (1 << 24) || a.H > (1 << 24)) return hipErrorInvalidValue;
	const bool empty = !(a.left <= a.right && a.top <= a.bottom);
	if (!empty && !(a.left >= 0.f && a.right <= static_cast<float>(a.W - 1) && a.top >= 0.f && a.bottom <= static_cast<float>(a.H - 1))) return hipErrorInvalidValue;
	if (a.defaultValue < 0 || a.defaultValue > 255) return hipErrorInvalidValue;
	const bool f32 = interp == kRemapBilinearF32 || interp == kRemapBicubicF32;
	const uintptr_t mask = f32 ? 15u : 3u, unit = f32 ? 4u : 1u;          // float32: 16-byte vectors, Sout and the frame stride count elements
	a.wide = !((reinterpret_cast<uintptr_t>(a.out) | static_cast<uintptr_t>(a.Sout) * unit | static_cast<uintptr_t>(a.outFrameStride) * unit) & mask);
	a.framesPerGroup = perFrame ? 1 : kRemapFramesPerGroup;
	if (!perFrame) a.coordFrameStride = 0;
	a.mapVec = source == kRemapMap && !(a.Wout & 3) && !((reinterpret_cast<uintptr_t>(a.mapX) | reinterpret_cast<uintptr_t>(a.mapY)) & 15) && !(a.coordFrameStride & 3);
	a.tilesX = (a.Wout + kRemapTileW - 1) / kRemapTileW;
	const long long tiles = static_cast<long long>(a.tilesX) * ((a.Hout + kRemapTileH - 1) / kRemapTileH);
	if (tiles > INT32_MAX) return hipErrorInvalidValue;
	const int groups = (a.frames + a.framesPerGroup - 1) / a.framesPerGroup;
	return for_frame_slices(groups, [&](int g0, int ng) {
		a.group0 = g0;
		const dim3 grid(static_cast<unsigned>(tiles), static_cast<unsigned>(ng));
		if (source == kRemapMap) launch_src<kRemapMap>(a, interp, grid, stream);
		else if (source == kRemapWarp2) launch_src<kRemapWarp2>(a, interp, grid, stream);
		else if (source == kRemapWarp3) launch_src<kRemapWarp3>(a, interp, grid, stream);
		else launch_src<kRemapUndist>(a, interp, grid, stream);
		return hipGetLastError();
	});
}

} // namespace compvhip
