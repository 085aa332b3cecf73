// scale_kernels.hip -- the fixed-point bilinear scaler of CompVImageScaleBilinear (base/image/compv_image_scale_bilinear.cxx:48-88,149-192) for gfx950.
// Definition: include/compv_hip.h (section "bilinear scale"), docs/kernels/scale.md.
//
//   scale_bilinear_kernel   ONE launch writes every destination of the argument block -- the non-empty levels of a pyramid, all scaled from the same
//                           source batch -- for all frames.  The grid's x axis is cut into per-level runs of workgroups (lv[l].blockEnd); a workgroup
//                           finds its level, then its 256 x 4 tile.  A lane produces 4 adjacent output bytes of one row and stores them as one dword;
//                           the group that crosses W (and every group of a destination that is not dword-aligned) stores bytes, so stride padding is
//                           never written.  Integer arithmetic only, no LDS, no atomic.
#include "device.hpp"

namespace compvhip {
namespace {

constexpr int kScaleTileW = 256, kScaleTileH = 4;   // 64 lanes x 4 pixels, one wave per row

__global__ __launch_bounds__(256) void scale_bilinear_kernel(ScaleArgs a)
{
	const int bid = blockIdx.x, f = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	int l = 0;          // workgroup-uniform: at most 15 scalar compares
#pragma unroll
	for (int k = 0; k < kPyrMaxLevels - 1; ++k) if (k + 1 < a.levels && bid >= a.lv[k].blockEnd) l = k + 1;
	const ScaleLevel& L = a.lv[l];
	const int local = bid - (l ? a.lv[l - 1].blockEnd : 0);
	const int ty = local / L.tilesX, tx = local - ty * L.tilesX;
	const int j = ty * kScaleTileH + wave, i0 = tx * kScaleTileW + 4 * lane;
	if (j >= L.H || i0 >= L.W) return;
	const uint8_t* __restrict__ src = a.in + static_cast<size_t>(f) * a.frameStride;
	uint8_t* __restrict__ dst = L.out + static_cast<size_t>(f) * L.frameStride + static_cast<size_t>(j) * L.S + i0;
	uint32_t px[4] = { 0u, 0u, 0u, 0u };
	if (L.copy) {
#pragma unroll
		for (int b = 0; b < 4; ++b) if (i0 + b < L.W) px[b] = src[static_cast<size_t>(j) * a.S + i0 + b];
	}
	else {
		const uint32_t y = static_cast<uint32_t>(j) * L.sy, y0 = y & 255u, y1 = 255u - y0;
		const int ny = static_cast<int>(y >> 8);
		const uint8_t* __restrict__ r0 = src + static_cast<size_t>(min(ny, a.H - 1)) * a.S;          // the clamp: a strict downscale never needs it
		const uint8_t* __restrict__ r1 = src + static_cast<size_t>(min(ny + 1, a.H - 1)) * a.S;
#pragma unroll
		for (int b = 0; b < 4; ++b) {
			if (i0 + b >= L.W) continue;
			const uint32_t x = static_cast<uint32_t>(i0 + b) * L.sx, x0 = x & 255u, x1 = 255u - x0;
			const int nx = static_cast<int>(x >> 8), c0 = min(nx, a.W - 1), c1 = min(nx + 1, a.W - 1);
			const uint32_t A = r0[c0] * x1 + r0[c1] * x0, B = r1[c0] * x1 + r1[c1] * x0;
			px[b] = (((y1 * A) >> 16) + ((y0 * B) >> 16)) & 0xffu;          // two shifts, as the reference's live branch
		}
	}
	if (L.dwords && i0 + 4 <= L.W) *reinterpret_cast<uint32_t*>(dst) = px[0] | px[1] << 8 | px[2] << 16 | px[3] << 24;
	else {
#pragma unroll
		for (int b = 0; b < 4; ++b) if (i0 + b < L.W) dst[b] = static_cast<uint8_t>(px[b]);
	}
}

} // namespace

bool scale_level_init(ScaleLevel& lv, int Win, int Hin)
{
	if (Win < 1 || Hin < 1 || lv.W < 1 || lv.H < 1) return false;
	const float fx = static_cast<float>(Win) / static_cast<float>(lv.W), fy = static_cast<float>(Hin) / static_cast<float>(lv.H);   // :167-170
	lv.copy = lv.W == Win && lv.H == Hin;          // CompVImage::scale clones (compv_image.cxx:852-905)
	if (!lv.copy && (fx <= 0.f || fx >= 256.f || fy <= 0.f || fy >= 256.f)) return false;          // :175, where the reference only warns
	lv.sx = static_cast<uint32_t>(static_cast<int>(fx * 256.f)); lv.sy = static_cast<uint32_t>(static_cast<int>(fy * 256.f));
	lv.dwords = !((reinterpret_cast<uintptr_t>(lv.out) | static_cast<uintptr_t>(lv.S) | lv.frameStride) & 3);
	lv.tilesX = (lv.W + kScaleTileW - 1) / kScaleTileW;
	return true;
}

hipError_t launch_scale_bilinear(ScaleArgs& a, int frames, hipStream_t stream)
{
	if (!a.in || a.W < 1 || a.H < 1 || a.S < a.W || a.levels < 1 || a.levels > kPyrMaxLevels || frames < 1 || frames > 65535) return hipErrorInvalidValue;
	long long blocks = 0;
	for (int l = 0; l < a.levels; ++l) {
		ScaleLevel& L = a.lv[l];
		if (!L.out || L.W < 1 || L.H < 1 || L.S < L.W || L.tilesX != (L.W + kScaleTileW - 1) / kScaleTileW) return hipErrorInvalidValue;
		// x = i * sx and y = j * sy stay below 2^32
		if (static_cast<unsigned long long>(L.W) * L.sx >= (1ull << 32) || static_cast<unsigned long long>(L.H) * L.sy >= (1ull << 32)) return hipErrorInvalidValue;
		blocks += static_cast<long long>(L.tilesX) * ((L.H + kScaleTileH - 1) / kScaleTileH);
		if (blocks > INT32_MAX) return hipErrorInvalidValue;
		L.blockEnd = static_cast<int>(blocks);
	}
	hipLaunchKernelGGL(scale_bilinear_kernel, dim3(static_cast<unsigned>(blocks), frames), dim3(256), 0, stream, a);
	return hipGetLastError();
}

} // namespace compvhip
