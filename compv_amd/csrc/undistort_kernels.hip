// undistort_kernels.hip -- the lens distortion model outside an image gather, for gfx950: CompVCalibUtils::initUndistMap, dist2DPoints and proj2D
// (core/calib/compv_core_calib_utils.cxx).  Definition: include/compv_hip.h ("lens undistortion"), docs/kernels/undistort.md; the arithmetic is
// undistort_math.hpp, unfused (-ffp-contract=off).  The fused image form is the fourth coordinate source of remap_kernels.hip.
//
//   undist_map_kernel<T>      the two map planes of 1 or `cameras` cameras.  The remap tile: a workgroup owns 256 x 4 map entries, one wave per row, a lane
//                             4 adjacent entries, stored as one 16-byte vector (float32) or two (float64) where the planes allow it, else element by
//                             element.  The camera's record is wave-uniform.  blockIdx.y is the camera.
//   undist_points_kernel<T>   one lane per point of [sets][n] {x, y}; blockIdx.y is the set.  Points behind a set's count are neither read nor written.
//   undist_project_kernel     the same over {x, y, z} float64 with a pose {R, t} per set.
// No LDS, no atomic; every output element has one writer; every store is a plain C++ store.
#include "kernels.hpp"
#include "frame_slices.hpp"
#include "undistort_math.hpp"

namespace compvhip {
namespace {

constexpr int kMapTileW = 256, kMapTileH = 4;   // 64 lanes x 4 entries, one wave per row
constexpr int kPointThreads = 256;

template <typename T>
__global__ __launch_bounds__(256) void undist_map_kernel(UndistMapArgs a, int cam0, int tilesX, int vec)
{
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const int ty = blockIdx.x / tilesX, tx = blockIdx.x - ty * tilesX;
	const int j = ty * kMapTileH + wave, i0 = tx * kMapTileW + 4 * lane;
	if (j >= a.Hout || i0 >= a.Wout) return;
	const int cam = cam0 + static_cast<int>(blockIdx.y);
	const int n = min(4, a.Wout - i0);
	const T* __restrict__ rec = static_cast<const T*>(a.coeffs) + static_cast<size_t>(cam) * a.coeffStride;
	T c[undist::kCoeffs];
#pragma unroll
	for (int k = 0; k < undist::kCoeffs; ++k) c[k] = rec[k];
	const T Y = static_cast<T>(a.originY + j);
	T u[4], v[4];
#pragma unroll
	for (int b = 0; b < 4; ++b) {
		u[b] = v[b] = static_cast<T>(0);
		if (b < n) undist::map_entry(c, static_cast<T>(a.originX + i0 + b), Y, u[b], v[b]);
	}
	const size_t at = static_cast<size_t>(cam) * a.Wout * a.Hout + static_cast<size_t>(j) * a.Wout + i0;
	T* __restrict__ mx = static_cast<T*>(a.mapX) + at;
	T* __restrict__ my = static_cast<T*>(a.mapY) + at;
	if (vec) {          // Wout % 4 == 0: n == 4 and `at` is a multiple of 4
		if (sizeof(T) == 4) {
			*reinterpret_cast<float4*>(mx) = make_float4(u[0], u[1], u[2], u[3]);
			*reinterpret_cast<float4*>(my) = make_float4(v[0], v[1], v[2], v[3]);
		}
		else {
			reinterpret_cast<double2*>(mx)[0] = make_double2(u[0], u[1]); reinterpret_cast<double2*>(mx)[1] = make_double2(u[2], u[3]);
			reinterpret_cast<double2*>(my)[0] = make_double2(v[0], v[1]); reinterpret_cast<double2*>(my)[1] = make_double2(v[2], v[3]);
		}
	}
	else {
#pragma unroll
		for (int b = 0; b < 4; ++b) if (b < n) { mx[b] = u[b]; my[b] = v[b]; }
	}
}

__device__ __forceinline__ int set_count(const int32_t* counts, int set, int n)
{
	return counts ? min(max(counts[set], 0), n) : n;
}

template <typename T>
__global__ __launch_bounds__(kPointThreads) void undist_points_kernel(UndistPointsArgs a, int set0)
{
	const int set = set0 + static_cast<int>(blockIdx.y);
	const int i = static_cast<int>(blockIdx.x) * kPointThreads + static_cast<int>(threadIdx.x);
	if (i >= set_count(a.counts, set, a.n)) return;
	const T* __restrict__ rec = static_cast<const T*>(a.coeffs) + static_cast<size_t>(set) * a.coeffStride;
	T c[undist::kCoeffs];
#pragma unroll
	for (int k = 0; k < undist::kCoeffs; ++k) c[k] = rec[k];
	const size_t at = 2 * (static_cast<size_t>(set) * a.n + i);
	const T* in = static_cast<const T*>(a.in) + at;          // (no __restrict__: in == out is served)
	T* out = static_cast<T*>(a.out) + at;
	const T X = in[0], Y = in[1];
	T u, v;
	undist::map_entry(c, X, Y, u, v);
	out[0] = u; out[1] = v;
}

__global__ __launch_bounds__(kPointThreads) void undist_project_kernel(UndistProjectArgs a, int set0)
{
	const int set = set0 + static_cast<int>(blockIdx.y);
	const int i = static_cast<int>(blockIdx.x) * kPointThreads + static_cast<int>(threadIdx.x);
	if (i >= set_count(a.counts, set, a.n)) return;
	const double* __restrict__ rec = a.coeffs + static_cast<size_t>(set) * a.coeffStride;
	const double* __restrict__ pose = a.poses + static_cast<size_t>(set) * undist::kPose;
	double c[undist::kCoeffs], Rt[undist::kPose];
#pragma unroll
	for (int k = 0; k < undist::kCoeffs; ++k) c[k] = rec[k];
#pragma unroll
	for (int k = 0; k < undist::kPose; ++k) Rt[k] = pose[k];
	const size_t p = static_cast<size_t>(set) * a.n + i;
	const double* __restrict__ in = a.in + 3 * p;
	double u, v;
	undist::project(c, Rt, in[0], in[1], in[2], u, v);
	a.out[2 * p] = u; a.out[2 * p + 1] = v;
}

} // namespace

hipError_t launch_undist_map(const UndistMapArgs& a, hipStream_t stream)
{
	if (!a.coeffs || !a.mapX || !a.mapY || a.Wout < 1 || a.Hout < 1 || a.cameras < 1 || a.originX < 0 || a.originY < 0) return hipErrorInvalidValue;
	if (a.originX + a.Wout > 32767 || a.originY + a.Hout > 32767 || (a.coeffStride != 0 && a.coeffStride != undist::kCoeffs)) return hipErrorInvalidValue;
	const uintptr_t elem = a.f64 ? 8 : 4;
	if ((reinterpret_cast<uintptr_t>(a.mapX) | reinterpret_cast<uintptr_t>(a.mapY) | reinterpret_cast<uintptr_t>(a.coeffs)) & (elem - 1)) return hipErrorInvalidValue;
	const int vec = !(a.Wout & 3) && !((reinterpret_cast<uintptr_t>(a.mapX) | reinterpret_cast<uintptr_t>(a.mapY)) & 15);
	const int tilesX = (a.Wout + kMapTileW - 1) / kMapTileW;
	const unsigned tiles = static_cast<unsigned>(tilesX) * static_cast<unsigned>((a.Hout + kMapTileH - 1) / kMapTileH);          // < 2^21
	return for_frame_slices(a.cameras, [&](int c0, int nc) {
		const dim3 grid(tiles, static_cast<unsigned>(nc));
		if (a.f64) hipLaunchKernelGGL(undist_map_kernel<double>, grid, dim3(256), 0, stream, a, c0, tilesX, vec);
		else hipLaunchKernelGGL(undist_map_kernel<float>, grid, dim3(256), 0, stream, a, c0, tilesX, vec);
		return hipGetLastError();
	});
}

hipError_t launch_undist_points(const UndistPointsArgs& a, hipStream_t stream)
{
	if (!a.coeffs || !a.in || !a.out || a.n < 1 || a.sets < 1 || (a.coeffStride != 0 && a.coeffStride != undist::kCoeffs)) return hipErrorInvalidValue;
	const uintptr_t elem = a.f64 ? 8 : 4;
	if ((reinterpret_cast<uintptr_t>(a.in) | reinterpret_cast<uintptr_t>(a.out) | reinterpret_cast<uintptr_t>(a.coeffs)) & (elem - 1)) return hipErrorInvalidValue;
	if (reinterpret_cast<uintptr_t>(a.counts) & 3) return hipErrorInvalidValue;
	const unsigned blocks = (static_cast<unsigned>(a.n) + kPointThreads - 1) / kPointThreads;
	return for_frame_slices(a.sets, [&](int s0, int ns) {
		const dim3 grid(blocks, static_cast<unsigned>(ns));
		if (a.f64) hipLaunchKernelGGL(undist_points_kernel<double>, grid, dim3(kPointThreads), 0, stream, a, s0);
		else hipLaunchKernelGGL(undist_points_kernel<float>, grid, dim3(kPointThreads), 0, stream, a, s0);
		return hipGetLastError();
	});
}

hipError_t launch_undist_project(const UndistProjectArgs& a, hipStream_t stream)
{
	if (!a.coeffs || !a.poses || !a.in || !a.out || a.n < 1 || a.sets < 1 || (a.coeffStride != 0 && a.coeffStride != undist::kCoeffs)) return hipErrorInvalidValue;
	if ((reinterpret_cast<uintptr_t>(a.in) | reinterpret_cast<uintptr_t>(a.out) | reinterpret_cast<uintptr_t>(a.coeffs) | reinterpret_cast<uintptr_t>(a.poses)) & 7)
		return hipErrorInvalidValue;
	if (reinterpret_cast<uintptr_t>(a.counts) & 3) return hipErrorInvalidValue;
	const unsigned blocks = (static_cast<unsigned>(a.n) + kPointThreads - 1) / kPointThreads;
	return for_frame_slices(a.sets, [&](int s0, int ns) {
		const dim3 grid(blocks, static_cast<unsigned>(ns));
		hipLaunchKernelGGL(undist_project_kernel, grid, dim3(kPointThreads), 0, stream, a, s0);
		return hipGetLastError();
	});
}

} // namespace compvhip
