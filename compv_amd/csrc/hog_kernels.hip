// hog_kernels.hip -- HOG descriptors for gfx950: CompVHogStd::process (core/features/hog/compv_core_feature_hog_std.cxx) on a batch of gray frames.
// Definition: include/compv_hip.h (section "HOG descriptors"), docs/kernels/hog.md.  The arithmetic of a pixel and of a block's norm is hog_math.hpp's.
//
//   hog_cells_kernel<INTERP, DWORDS>   The histogram of a cell is a SEQUENTIAL float32 sum over its pixels, so one lane owns one cell and walks it row-major;
//                           the parallelism is the cells.  A workgroup is ONE wave that takes nx adjacent cells of ny cell rows (nx = min(64, cellsX),
//                           ny = 64 / nx: a narrow crop fills its lanes with several cell rows).  Per lane row it stages the cell rows plus one row above
//                           and below and one pixel left and right in LDS -- whole dwords where the frames are 4-byte aligned (DWORDS), single bytes
//                           otherwise; coordinates outside the frame are clamped, their values are never used: the border rule forces gx / gy to 0 there
//                           -- as many cell rows at a time as fit kHogTileBudget.  The histograms live in LDS as [bin][lane]: lane-consecutive words, no
//                           bank conflict whatever the bin.  gx, gy, magnitude and direction exist in registers only.  The map leaves through the
//                           histogram's LDS image: consecutive lanes write consecutive floats of a cell row.
//   hog_blocks_kernel       Four lanes per block, one for each accumulator lane of the reference's SSE2 sums (hog_math.hpp: lane_partial, ordered_sum):
//                           each sums its share of the block's cells straight from the map, three shuffles exchange the partials, every lane finishes the
//                           sum in the reference's order.  L2HYS reads the block three times (L2 cache).  The quad writes elements l, l + 4, ...
// No atomic, no float reordering anywhere: the result does not depend on the launch geometry.
#include "device.hpp"
#include "frame_slices.hpp"
#include "hog_math.hpp"

namespace compvhip {
namespace {

static_assert(COMPVHIP_HOG_NORM_NONE == hog::kNormNone && COMPVHIP_HOG_NORM_L1 == hog::kNormL1 && COMPVHIP_HOG_NORM_L1SQRT == hog::kNormL1Sqrt &&
              COMPVHIP_HOG_NORM_L2 == hog::kNormL2 && COMPVHIP_HOG_NORM_L2HYS == hog::kNormL2Hys && COMPVHIP_HOG_INTERP_NEAREST == hog::kInterpNearest &&
              COMPVHIP_HOG_INTERP_BILINEAR == hog::kInterpBilinear, "hog_math.hpp mirrors the header's constants");

struct LdsHist {          // the lane's histogram inside the wave's [bin][64] image
	float* h;
	__device__ __forceinline__ float& operator[](int b) { return h[b * 64]; }
};

template <int INTERP, bool DWORDS>
__global__ __launch_bounds__(64) void hog_cells_kernel(HogArgs a)
{
	extern __shared__ __attribute__((aligned(16))) uint8_t hog_smem[];
	float* const hist = reinterpret_cast<float*>(hog_smem);                       // [nbins][64]
	uint8_t* const tile = hog_smem + static_cast<size_t>(a.nbins) * 256;          // [ny][rowsPerChunk + 2][pitch]
	const int lane = threadIdx.x;
	const int ty = blockIdx.x / a.tilesX, tx = blockIdx.x - ty * a.tilesX;
	const int ly = lane / a.nx, lx = lane - ly * a.nx;
	const int cx0 = tx * a.nx, cy0 = ty * a.ny;
	const int cx = cx0 + lx, cy = cy0 + ly;
	const bool valid = ly < a.ny && cx < a.validX && cy < a.validY;
	const uint8_t* __restrict__ frame = a.gray + static_cast<size_t>(blockIdx.y) * a.frameStride;
	for (int b = 0; b < a.nbins; ++b) hist[b * 64 + lane] = 0.f;
	// LDS column 0 is frame column xs: the halo column cx0 * strideW - 1 rounded down to a dword (-4 for the first tile)
	const int xs = (cx0 * a.strideW - 1) & ~3;
	const int dwPerRow = a.pitch >> 2, band = a.rowsPerChunk + 2;
	const hog::Binning q = hog::binning(a.nbins, a.gradientSigned != 0);
	LdsHist h{hist + lane};

	for (int r0 = 0; r0 < a.cellH; r0 += a.rowsPerChunk) {
		const int rows = min(a.rowsPerChunk, a.cellH - r0);
		// ---- stage rows r0 - 1 .. r0 + rows of the cells of every lane row ----
		for (int by = 0; by < a.ny; ++by) {
			const int ytop = (cy0 + by) * a.strideH + r0 - 1;
			for (int t = 0; t < rows + 2; ++t) {
				const int y = min(max(ytop + t, 0), a.H - 1);
				const uint8_t* __restrict__ src = frame + static_cast<size_t>(y) * a.S;
				uint32_t* dst = reinterpret_cast<uint32_t*>(tile + static_cast<size_t>(by * band + t) * a.pitch);
				for (int d = lane; d < dwPerRow; d += 64) {
					uint32_t v = 0;
					if (DWORDS) v = reinterpret_cast<const uint32_t*>(src)[min(max((xs >> 2) + d, 0), (a.S >> 2) - 1)];   // S % 4 == 0: the dword lies in the row
					else {
#pragma unroll
						for (int b = 0; b < 4; ++b) v |= static_cast<uint32_t>(src[min(max(xs + 4 * d + b, 0), a.W - 1)]) << (8 * b);
					}
					dst[d] = v;
				}
			}
		}
		__syncthreads();
		// ---- the lane's cell, rows r0 .. r0 + rows - 1, row-major ----
		if (valid) {
			const int col0 = cx * a.strideW - xs;          // >= 1
			for (int jj = 0; jj < rows; ++jj) {
				const int y = cy * a.strideH + r0 + jj;
				const bool yb = y == 0 || y == a.H - 1;
				const uint8_t* c = tile + static_cast<size_t>(ly * band + jj + 1) * a.pitch + col0;
				int left = c[-1], mid = c[0];
				for (int i = 0; i < a.cellW; ++i) {
					const int x = cx * a.strideW + i;
					const int right = c[i + 1];
					float gx, gy;
					hog::gradient(left, right, c[i - a.pitch], c[i + a.pitch], x == 0 || x == a.W - 1, yb, gx, gy);
					hog::vote<INTERP>(h, q, hog::magnitude(gx, gy), hog::direction(gx, gy));
					left = mid; mid = right;
				}
			}
		}
		__syncthreads();          // the next chunk overwrites the rows; the histograms are complete behind the last one
	}

	// ---- the map: per lane row, the nbins floats of its adjacent cells are contiguous; a left-out cell writes its zeros ----
	float* __restrict__ map = a.cells + static_cast<size_t>(blockIdx.y) * a.cellsFrameStride;
	const int ncell = min(a.nx, a.cellsX - cx0);
	for (int r = 0; r < a.ny && cy0 + r < a.cellsY; ++r) {
		float* __restrict__ out = map + (static_cast<size_t>(cy0 + r) * a.cellsX + cx0) * a.nbins;
		for (int k = lane; k < ncell * a.nbins; k += 64) {
			const int cell = k / a.nbins, bin = k - cell * a.nbins;
			out[k] = hist[bin * 64 + r * a.nx + cell];
		}
	}
}

// the reference's sum of the block's terms: lane l of the quad holds accumulator lane l
template <typename Term>
__device__ __forceinline__ float quad_sum(const Term& t, int count, int l)
{
	const float p = hog::lane_partial(t, count, l);
	const float p1 = __shfl_xor(p, 1), p2 = __shfl_xor(p, 2), p3 = __shfl_xor(p, 3);          // of lanes l ^ 1, l ^ 2, l ^ 3
	const float l0 = l == 0 ? p : (l == 1 ? p1 : (l == 2 ? p2 : p3));
	const float l1 = l == 1 ? p : (l == 0 ? p1 : (l == 3 ? p2 : p3));
	const float l2 = l == 2 ? p : (l == 3 ? p1 : (l == 0 ? p2 : p3));
	const float l3 = l == 3 ? p : (l == 2 ? p1 : (l == 1 ? p2 : p3));
	return hog::ordered_sum(l0, l1, l2, l3, t, count);
}

__global__ __launch_bounds__(256) void hog_blocks_kernel(HogArgs a)
{
	const int t = blockIdx.x * 256 + threadIdx.x;
	const int block = t >> 2, l = t & 3;
	const bool active = block < a.blocksX * a.blocksY;          // whole quads: an idle quad computes block 0 and writes nothing
	const int bb = active ? block : 0;
	const int by = bb / a.blocksX, bx = bb - by * a.blocksX;
	const float* __restrict__ map = a.cells + static_cast<size_t>(blockIdx.y) * a.cellsFrameStride;
	const hog::BlockLoad v{map + (static_cast<size_t>(by) * a.stepY * a.cellsX + static_cast<size_t>(bx) * a.stepX) * a.nbins, a.cpbX * a.nbins, a.cellsX * a.nbins};
	float r = 0.f, r2 = 0.f;
	if (a.norm != hog::kNormNone) {
		if (hog::norm_is_l2(a.norm)) r = hog::norm_factor(quad_sum(hog::TermSquare<hog::BlockLoad>{v}, a.count, l), a.norm);
		else r = hog::norm_factor(quad_sum(hog::TermValue<hog::BlockLoad>{v}, a.count, l), a.norm);
		if (a.norm == hog::kNormL2Hys) r2 = hog::norm_factor(quad_sum(hog::TermClippedSquare<hog::BlockLoad>{v, r}, a.count, l), a.norm);
	}
	if (!active) return;
	float* __restrict__ out = a.desc + static_cast<size_t>(blockIdx.y) * a.descStride + static_cast<size_t>(block) * a.count;
	for (int i = l; i < a.count; i += 4) out[i] = hog::norm_value(v(i), a.norm, r, r2);
}

template <int INTERP, bool DWORDS>
hipError_t cells_attr()
{
	return hipFuncSetAttribute(reinterpret_cast<const void*>(hog_cells_kernel<INTERP, DWORDS>), hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(kHogLdsLimit));
}

} // namespace

bool hog_plan_launch(HogArgs& a)
{
	const size_t histBytes = static_cast<size_t>(a.nbins) * 256;
	// columns of a staged row: the cells' span, a halo pixel each side, up to 3 bytes of dword alignment in front; a multiple of 4
	auto pitchOf = [&](int nx) { return (static_cast<size_t>(nx - 1) * a.strideW + a.cellW + 5 + 3) & ~static_cast<size_t>(3); };
	int nx = a.cellsX < 64 ? a.cellsX : 64, ny = 64 / nx;
	if (ny > a.cellsY) ny = a.cellsY;
	// three rows per lane row must fit the budget: fewer lane rows first, then fewer cells across
	while (ny > 1 && 3 * ny * pitchOf(nx) > kHogTileBudget) ny = (ny + 1) / 2;
	while (nx > 1 && 3 * pitchOf(nx) > kHogTileBudget) nx = (nx + 1) / 2;
	const size_t pitch = pitchOf(nx);
	size_t rows = kHogTileBudget / (ny * pitch);
	if (rows < 3) {          // nx == ny == 1: one cell wider than the budget takes what the CU has left
		if (histBytes + 3 * pitch > kHogLdsLimit) return false;
		rows = 3;
	}
	a.nx = nx; a.ny = ny; a.pitch = static_cast<int>(pitch);
	a.rowsPerChunk = rows - 2 < static_cast<size_t>(a.cellH) ? static_cast<int>(rows - 2) : a.cellH;
	a.tilesX = (a.cellsX + nx - 1) / nx; a.tilesY = (a.cellsY + ny - 1) / ny;
	a.ldsBytes = static_cast<int>(histBytes + static_cast<size_t>(ny) * (a.rowsPerChunk + 2) * pitch);
	a.dwords = !((reinterpret_cast<uintptr_t>(a.gray) | static_cast<uintptr_t>(a.S) | a.frameStride) & 3);
	return true;
}

hipError_t launch_hog_cells(const HogArgs& args, int frames, hipStream_t stream)
{
	if (!args.gray || !args.cells || args.nx < 1 || args.ny < 1 || args.nx * args.ny > 64 || args.rowsPerChunk < 1 || static_cast<size_t>(args.ldsBytes) > kHogLdsLimit)
		return hipErrorInvalidValue;
	if (args.interp != hog::kInterpNearest && args.interp != hog::kInterpBilinear) return hipErrorInvalidValue;
	// the opt-in to > 64 KB of dynamic LDS (360 bins take 90 KB) is a per-device function attribute: remember it per device
	static bool attr_set[64] = {};
	int dev = 0;
	(void)hipGetDevice(&dev);
	dev = (dev >= 0 && dev < 64) ? dev : 0;
	if (!attr_set[dev]) {
		hipError_t e = cells_attr<hog::kInterpNearest, false>();
		if (e == hipSuccess) e = cells_attr<hog::kInterpNearest, true>();
		if (e == hipSuccess) e = cells_attr<hog::kInterpBilinear, false>();
		if (e == hipSuccess) e = cells_attr<hog::kInterpBilinear, true>();
		if (e != hipSuccess) return e;
		attr_set[dev] = true;
	}
	const long long tiles = static_cast<long long>(args.tilesX) * args.tilesY;
	if (tiles < 1 || tiles > INT32_MAX) return hipErrorInvalidValue;
	return for_frame_slices(frames, [&](int f0, int nf) {
		HogArgs a = args;
		a.gray += static_cast<size_t>(f0) * a.frameStride; a.cells += static_cast<size_t>(f0) * a.cellsFrameStride;
		const dim3 grid(static_cast<unsigned>(tiles), static_cast<unsigned>(nf));
		const size_t lds = static_cast<size_t>(a.ldsBytes);
		if (a.interp == hog::kInterpNearest) {
			if (a.dwords) hipLaunchKernelGGL((hog_cells_kernel<hog::kInterpNearest, true>), grid, dim3(64), lds, stream, a);
			else hipLaunchKernelGGL((hog_cells_kernel<hog::kInterpNearest, false>), grid, dim3(64), lds, stream, a);
		}
		else {
			if (a.dwords) hipLaunchKernelGGL((hog_cells_kernel<hog::kInterpBilinear, true>), grid, dim3(64), lds, stream, a);
			else hipLaunchKernelGGL((hog_cells_kernel<hog::kInterpBilinear, false>), grid, dim3(64), lds, stream, a);
		}
		return hipGetLastError();
	});
}

hipError_t launch_hog_blocks(const HogArgs& args, int frames, hipStream_t stream)
{
	if (!args.cells || !args.desc || args.count < 1 || args.norm < hog::kNormNone || args.norm > hog::kNormL2Hys) return hipErrorInvalidValue;
	const long long threads = 4ll * args.blocksX * args.blocksY;
	if (threads < 4 || (threads + 255) / 256 > INT32_MAX) return hipErrorInvalidValue;
	return for_frame_slices(frames, [&](int f0, int nf) {
		HogArgs a = args;
		a.cells += static_cast<size_t>(f0) * a.cellsFrameStride; a.desc += static_cast<size_t>(f0) * a.descStride;
		hipLaunchKernelGGL(hog_blocks_kernel, dim3(static_cast<unsigned>((threads + 255) / 256), static_cast<unsigned>(nf)), dim3(256), 0, stream, a);
		return hipGetLastError();
	});
}

} // namespace compvhip
