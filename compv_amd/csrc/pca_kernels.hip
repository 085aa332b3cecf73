// pca_kernels.hip -- PCA projection (CompVMathPCA::project, base/math/compv_math_pca.cxx), CompVMath::mulABt (base/math/compv_math_op_mul.cxx) and
// the row-based front half of CompVMathPCA::compute (mean, covariance) for gfx950, in float32.  The definition is in include/compv_hip.h ("PCA
// projection", items A - G); the arithmetic is pca_math.hpp.
//
//   pca_project_kernel<CENTRE>    a workgroup of 256 lanes owns 32 rows x 32 components.  It stages 64 columns of both in the LDS, row-major with a
//                                 pitch of 68 floats: the 16 lanes that share a row read one address (a broadcast), the 16 that differ in their
//                                 component read 16-byte pieces 272 bytes apart, which fall into 16 different 4-bank slots of the 64 banks.  The
//                                 mean is subtracted as a row is staged (item B), so the centred matrix never goes to memory.  A lane keeps 2 x 2
//                                 outputs -- rows ty, ty + 16, components tx, tx + 16 -- with the sixteen accumulators of item C each, and feeds
//                                 them a quarter of a 16-group at a time (4 columns of 2 rows and 2 vectors: 16 operand registers beside the 64
//                                 accumulators).  A chunk is a multiple of 16 columns, so a 16-group never straddles two; the 4-groups, the fold
//                                 and the last columns run once behind the last whole group.  Optionally one more rounded multiply by `scale`.
//   pca_mean_kernel               a lane per dimension walks the observations in row order with a binary64 sum (item F): exact by construction,
//                                 coalesced across dimensions, and as slow as n dependent additions.
//   pca_centre_transpose_kernel   c[j][i] = obs[i][j] - mean[j] through a 32 x 33 LDS tile, into rows of nPad elements; the padding is not written.
// No atomics: every output element has one writer.  No FMA: the Makefile builds with -ffp-contract=off, and a contracted a * b + v would round once
// where the reference rounds twice.  No MFMA: v_mfma_f32 is an fmaf chain in an order of its own.  Every store is a plain C++ store.
#include "kernels.hpp"
#include "pca_math.hpp"

#include <type_traits>

namespace compvhip {
namespace {

using namespace pca;

constexpr int kTile = kPcaTile;               // rows and components of a workgroup
constexpr int kReg = 2;                       // per lane: kReg x kReg outputs
constexpr int kChunk = kPcaChunk;             // columns staged at a time: a multiple of 16
constexpr int kPitch = kChunk + 4;            // floats per staged row: 16-byte pieces of rows one apart land 4 banks apart
constexpr int kThreads = 256;                 // 16 x 16 lanes
static_assert(kTile == 16 * kReg && kChunk % 16 == 0 && kPitch % 4 == 0 && kPitch % 64 == 4, "pca_project_kernel: tile / staging geometry");

template <bool CENTRE>
__global__ __launch_bounds__(kThreads) void pca_project_kernel(PcaProjectArgs a)
{
	__shared__ __attribute__((aligned(16))) float s_mem[2 * kTile * kPitch];
	float* const s_a = s_mem;
	float* const s_b = s_mem + kTile * kPitch;
	const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
	const size_t r0 = static_cast<size_t>(blockIdx.x) * kTile;
	const int m0 = static_cast<int>(blockIdx.y) * kTile;

	Dot16 acc[kReg][kReg];
#pragma unroll
	for (int i = 0; i < kReg; ++i)
#pragma unroll
		for (int j = 0; j < kReg; ++j) acc[i][j].clear();

	// columns [k0, k0 + kc) of the tile's rows and vectors; rows behind n, vectors behind comps read nothing and stage 0; columns behind kc are not staged
	auto stage = [&](int k0, int kc) {
		for (int idx = tid; idx < kTile * kChunk; idx += kThreads) {
			const int r = idx / kChunk, c = idx % kChunk;
			if (c >= kc) continue;
			float av = 0.f, bv = 0.f;
			if (r0 + r < static_cast<size_t>(a.n)) {
				av = a.in[(r0 + r) * a.inStride + static_cast<size_t>(k0 + c)];
				if constexpr (CENTRE) av = centre(av, a.mean[k0 + c]);
			}
			if (m0 + r < a.comps) bv = a.vectors[static_cast<size_t>(m0 + r) * a.vecStride + static_cast<size_t>(k0 + c)];
			s_a[r * kPitch + c] = av;
			s_b[r * kPitch + c] = bv;
		}
	};

	const int d16 = a.dim & ~15;
	for (int k0 = 0; k0 < d16; k0 += kChunk) {
		const int kc = min(kChunk, d16 - k0);          // 16, 32, 48 or 64
		stage(k0, kc);
		__syncthreads();
		for (int g = 0; g < kc; g += 16) {
			auto quarter = [&](auto Q) {
				constexpr int q = decltype(Q)::value;
				float4 ra[kReg], rb[kReg];
#pragma unroll
				for (int i = 0; i < kReg; ++i) {
					ra[i] = *reinterpret_cast<const float4*>(s_a + (ty + 16 * i) * kPitch + g + 4 * q);
					rb[i] = *reinterpret_cast<const float4*>(s_b + (tx + 16 * i) * kPitch + g + 4 * q);
				}
#pragma unroll
				for (int i = 0; i < kReg; ++i)
#pragma unroll
					for (int j = 0; j < kReg; ++j) {
						const float pa[4] = { ra[i].x, ra[i].y, ra[i].z, ra[i].w }, pb[4] = { rb[j].x, rb[j].y, rb[j].z, rb[j].w };
						acc[i][j].template quarter<q>(pa, pb);
					}
			};
			quarter(std::integral_constant<int, 0>{}); quarter(std::integral_constant<int, 1>{});
			quarter(std::integral_constant<int, 2>{}); quarter(std::integral_constant<int, 3>{});
		}
		__syncthreads();          // the next chunk (or the tail) overwrites the staging
	}

	const int nt = a.dim - d16;          // 0 .. 15 columns behind the last whole group
	if (nt) {
		stage(d16, nt);
		__syncthreads();
	}
#pragma unroll
	for (int i = 0; i < kReg; ++i)
#pragma unroll
		for (int j = 0; j < kReg; ++j) {
			float v = acc[i][j].finish(s_a + (ty + 16 * i) * kPitch, s_b + (tx + 16 * j) * kPitch, static_cast<size_t>(nt));
			if (a.scaled) v = v * a.scale;
			const size_t r = r0 + ty + 16 * i;
			const int m = m0 + tx + 16 * j;
			if (r < static_cast<size_t>(a.n) && m < a.comps) a.out[r * a.outStride + m] = v;
		}
}

__global__ __launch_bounds__(256) void pca_mean_kernel(PcaMeanArgs a)
{
	const int j = static_cast<int>(blockIdx.x) * 256 + threadIdx.x;
	if (j < a.dim) a.mean[j] = mean(a.obs + j, static_cast<size_t>(a.n), a.obsStride);
}

__global__ __launch_bounds__(256) void pca_centre_transpose_kernel(PcaCentreArgs a)
{
	__shared__ float s_t[32][33];
	const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;          // 32 x 8
	const size_t i0 = static_cast<size_t>(blockIdx.x) * 32;          // observations
	const int j0 = static_cast<int>(blockIdx.y) * 32;                // dimensions
	const size_t n = static_cast<size_t>(a.n);
	for (int r = ty; r < 32; r += 8) {
		float v = 0.f;
		if (i0 + r < n && j0 + tx < a.dim) v = centre(a.obs[(i0 + r) * a.obsStride + static_cast<size_t>(j0 + tx)], a.mean[j0 + tx]);
		s_t[r][tx] = v;
	}
	__syncthreads();
	for (int r = ty; r < 32; r += 8)
		if (j0 + r < a.dim && i0 + tx < n) a.centred[static_cast<size_t>(j0 + r) * a.nPad + i0 + tx] = s_t[tx][r];
}

} // namespace

hipError_t launch_pca_project(const PcaProjectArgs& a, hipStream_t stream)
{
	if (a.n <= 0 || a.comps <= 0 || a.dim <= 0) return hipSuccess;
	const dim3 grid((static_cast<unsigned>(a.n) + kTile - 1) / kTile, (static_cast<unsigned>(a.comps) + kTile - 1) / kTile);          // y <= 2^20 / 32
	if (a.mean) hipLaunchKernelGGL(pca_project_kernel<true>, grid, dim3(kThreads), 0, stream, a);
	else hipLaunchKernelGGL(pca_project_kernel<false>, grid, dim3(kThreads), 0, stream, a);
	return hipGetLastError();
}

hipError_t launch_pca_mean(const PcaMeanArgs& a, hipStream_t stream)
{
	if (a.n <= 0 || a.dim <= 0) return hipSuccess;
	hipLaunchKernelGGL(pca_mean_kernel, dim3((static_cast<unsigned>(a.dim) + 255) / 256), dim3(256), 0, stream, a);
	return hipGetLastError();
}

hipError_t launch_pca_centre_transpose(const PcaCentreArgs& a, hipStream_t stream)
{
	if (a.n <= 0 || a.dim <= 0) return hipSuccess;
	const dim3 grid((static_cast<unsigned>(a.n) + 31) / 32, (static_cast<unsigned>(a.dim) + 31) / 32);          // y <= 2^20 / 32
	hipLaunchKernelGGL(pca_centre_transpose_kernel, grid, dim3(256), 0, stream, a);
	return hipGetLastError();
}

} // namespace compvhip
