// stats_kernels.hip -- per-image statistics for gfx950: CompVImage::integral (base/image/compv_image_integral.cxx), histogramBuild, histogramEqualiz,
// histogramBuildProjectionX / Y (base/image/compv_image.cxx, base/math/compv_math_histogram.cxx) on a batch of gray frames.
// Definition: include/compv_hip.h (section "image statistics"), docs/kernels/stats.md.  Everything is integer arithmetic (the look-up table: two float32
// operations on integers), no atomic touches global memory, no workgroup waits for another: the result does not depend on the launch geometry.
//
//   stats_band_sums_kernel<DWORDS>   A frame is cut into bands of kStatsBandRows rows.  One workgroup per (band, frame), four adjacent columns per thread,
//                            1024 columns at a time: the band's column sums of p and of p * p (u32 in registers, widened at the store) and, for the
//                            projections, the sum of every row of the band (one u32 per row and thread, v_sad_u8 per dword, reduced over the workgroup at
//                            the end).  The frame is read once.
//   stats_band_scan_kernel   One thread per column walks the bands top down: the column sums become, in place, the sums of all bands above (the integral's
//                            column increments at the band's upper edge) -- or, for projX, their total leaves as int32.
//   stats_integral_kernel<SUM, SQ>   The single-pass form of the issue's kernel note, not the separable one.  One wave per (band, frame) walks tiles of
//                            kStatsTile columns left to right, one column per lane.  Per row a u32 wave scan of the pixels (and of their squares; six DPP
//                            adds, device.hpp) plus the row's wave-uniform u32 carry gives the row's prefix; a u64 scan of the upper edge's column
//                            increments plus its carry gives the integral at the band's upper edge; the prefixes are accumulated down the column in u64
//                            registers and converted once at the store.  A store instruction writes 64 consecutive float64 of one row.  The frame is
//                            read a second time here (2 B / px in all), a byte per lane.
//   stats_hist_kernel<DWORDS>   A new kernel, not the one behind launch_otsu: that one loads 8-byte groups (per lane, so the hardware takes them at any
//                            address too, but a dword-aligned frame would pay for the split accesses), where these calls pick their arm by the pointer; launch_otsu and its kernels are untouched.  It keeps that kernel's LDS layout ([256 bins][32 columns],
//                            a lane always uses column lane % 32) with one wave per row and four pixels per lane; partial histograms per row chunk, no
//                            global atomic, no memset.
//   stats_hist_finish_kernel Sums the partial histograms of a frame (or takes the caller's), writes the histogram and / or the equalisation look-up table.
//   stats_equalize_kernel<DWORDS>   out = lut[in] with the frame's table in LDS, four pixels per lane; the lane that reads a pixel writes it, so out may be in.
// DWORDS: the frames (for the equalisation also the output) start on a dword and S % 4 == 0, so four pixels are one load (one store); otherwise bytes are
// loaded one by one and no alignment is asked of the frames.  No load reaches outside a row, no store outside the columns < W.
#include "device.hpp"
#include "frame_slices.hpp"

namespace compvhip {
namespace {

constexpr int kR = kStatsBandRows;

// Pixels x .. x + 3 of a row as one dword (x % 4 == 0, x < W), the bytes at columns >= W as 0.  DWORDS: the row starts on a dword and S % 4 == 0, so the
// dword at x lies inside the row; otherwise only the bytes that count are loaded, one by one.
template <bool DWORDS>
__device__ __forceinline__ uint32_t load4(const uint8_t* __restrict__ row, int x, int W)
{
	const int n = W - x;
	if (DWORDS) {
		const uint32_t d = *reinterpret_cast<const uint32_t*>(row + x);
		return n >= 4 ? d : d & ((1u << (8 * n)) - 1u);
	}
	uint32_t d = row[x];
	if (n > 1) d |= static_cast<uint32_t>(row[x + 1]) << 8;
	if (n > 2) d |= static_cast<uint32_t>(row[x + 2]) << 16;
	if (n > 3) d |= static_cast<uint32_t>(row[x + 3]) << 24;
	return d;
}

template <bool DWORDS>
__global__ __launch_bounds__(kStatsThreads) void stats_band_sums_kernel(StatsBandArgs a)
{
	__shared__ uint32_t s_row[kStatsThreads / 64][kR];
	const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
	const int band = blockIdx.x, y0 = band * kR, rows = min(kR, a.H - y0);
	const size_t f = blockIdx.y;
	const uint8_t* __restrict__ top = a.in + f * a.frameStride + static_cast<size_t>(y0) * a.S;
	const size_t colBase = (f * a.bands + band) * static_cast<size_t>(a.W);
	uint32_t rowAcc[kR];
#pragma unroll
	for (int r = 0; r < kR; ++r) rowAcc[r] = 0u;
	for (int x = 4 * tid; x < a.W; x += 4 * blockDim.x) {          // four adjacent columns per thread
		uint32_t c[4] = { 0u, 0u, 0u, 0u }, c2[4] = { 0u, 0u, 0u, 0u };
#pragma unroll
		for (int r = 0; r < kR; ++r) {
			if (r < rows) {
				const uint32_t d = load4<DWORDS>(top + static_cast<size_t>(r) * a.S, x, a.W);
#pragma unroll
				for (int k = 0; k < 4; ++k) {
					const uint32_t p = (d >> (8 * k)) & 0xffu;
					c[k] += p; c2[k] += p * p;          // a band: at most 255 * 255 * kStatsBandRows
				}
				rowAcc[r] = __builtin_amdgcn_sad_u8(d, 0u, rowAcc[r]);          // + the four bytes; a row: at most 255 * 32 767
			}
		}
#pragma unroll
		for (int k = 0; k < 4; ++k) {
			if (x + k < a.W) {
				if (a.colSum) a.colSum[colBase + x + k] = c[k];
				if (a.colSq) a.colSq[colBase + x + k] = c2[k];
			}
		}
	}
	if (!a.rowSum) return;
#pragma unroll
	for (int r = 0; r < kR; ++r) {
		const uint32_t t = wave_sum(rowAcc[r]);
		if (lane == 0) s_row[wv][r] = t;
	}
	__syncthreads();
	if (tid < rows) {
		uint32_t t = 0u;
		for (int w = 0; w < static_cast<int>(blockDim.x >> 6); ++w) t += s_row[w][tid];
		a.rowSum[f * a.H + y0 + tid] = static_cast<int32_t>(t);
	}
}

// colSum / colSq: [frames][bands][W], either may be null.  projX == nullptr: exclusive prefix sums down the bands, in place; otherwise the total of colSum.
__global__ __launch_bounds__(256) void stats_band_scan_kernel(uint64_t* __restrict__ colSum, uint64_t* __restrict__ colSq, int bands, int W, int32_t* __restrict__ projX)
{
	const int x = blockIdx.x * 256 + threadIdx.x;
	if (x >= W) return;
	const size_t f = blockIdx.y;
	const size_t base = f * bands * static_cast<size_t>(W) + x;
	if (projX) {
		uint64_t t = 0;
		for (int b = 0; b < bands; ++b) t += colSum[base + static_cast<size_t>(b) * W];
		projX[f * W + x] = static_cast<int32_t>(t);          // at most 255 * 32 767
		return;
	}
	uint64_t run = 0, run2 = 0;
	for (int b = 0; b < bands; ++b) {
		const size_t i = base + static_cast<size_t>(b) * W;
		if (colSum) { const uint64_t v = colSum[i]; colSum[i] = run; run += v; }
		if (colSq) { const uint64_t v = colSq[i]; colSq[i] = run2; run2 += v; }
	}
}

template <bool SUM, bool SQ>
__global__ __launch_bounds__(kStatsTile) void stats_integral_kernel(StatsIntegralArgs a)
{
	static_assert(kStatsTile == 64 && kR <= 64, "one wave per band, one lane per column of a tile; column 0 is written by one lane per row");
	const int lane = threadIdx.x;
	const int band = blockIdx.x, y0 = band * kR, rows = min(kR, a.H - y0);
	const size_t f = blockIdx.y;
	const uint8_t* __restrict__ top = a.in + f * a.frameStride + static_cast<size_t>(y0) * a.S;
	const size_t edgeBase = (f * a.bands + band) * static_cast<size_t>(a.W);
	const size_t frameOut = f * (static_cast<size_t>(a.H) + 1) * a.sumStride;
	const size_t bandOut = frameOut + (static_cast<size_t>(y0) + 1) * a.sumStride;          // output row y0 + 1: the integral behind the band's first row
	// row 0 (the first band) and column 0 are zeros
	if (band == 0) {
		for (int x = lane; x <= a.W; x += kStatsTile) {
			if (SUM) a.sum[frameOut + x] = 0.0;
			if (SQ) a.sumsq[frameOut + x] = 0.0;
		}
	}
	if (lane < rows) {
		if (SUM) a.sum[bandOut + static_cast<size_t>(lane) * a.sumStride] = 0.0;
		if (SQ) a.sumsq[bandOut + static_cast<size_t>(lane) * a.sumStride] = 0.0;
	}
	uint32_t carry[kR], carry2[kR];          // per row: the sum of the pixels (squares) of the tiles to the left; wave-uniform
#pragma unroll
	for (int r = 0; r < kR; ++r) { carry[r] = 0u; carry2[r] = 0u; }
	uint64_t edgeCarry = 0, edgeCarry2 = 0;
	for (int x0 = 0; x0 < a.W; x0 += kStatsTile) {
		const int x = x0 + lane;
		const bool in = x < a.W;
		uint32_t p[kR];
#pragma unroll
		for (int r = 0; r < kR; ++r) p[r] = (in && r < rows) ? top[static_cast<size_t>(r) * a.S + x] : 0u;
		uint64_t acc = 0, acc2 = 0;          // the integral at (y, x + 1), from the band's upper edge downwards
		if (SUM) {
			const uint64_t e = wave_incl_scan<uint64_t>(in ? a.edgeSum[edgeBase + x] : 0ull, lane);
			acc = edgeCarry + e;
			edgeCarry += __shfl(e, 63);
		}
		if (SQ) {
			const uint64_t e = wave_incl_scan<uint64_t>(in ? a.edgeSq[edgeBase + x] : 0ull, lane);
			acc2 = edgeCarry2 + e;
			edgeCarry2 += __shfl(e, 63);
		}
#pragma unroll
		for (int r = 0; r < kR; ++r) {
			if (r < rows) {
				const size_t o = bandOut + static_cast<size_t>(r) * a.sumStride + x + 1;
				if (SUM) {
					const uint32_t s = wave_incl_scan_dpp(p[r]);
					acc += carry[r] + s;          // a row's prefix: at most 255 * 32 767
					carry[r] += __builtin_amdgcn_readlane(s, 63);
					if (in) a.sum[o] = static_cast<double>(acc);
				}
				if (SQ) {
					const uint32_t s = wave_incl_scan_dpp(p[r] * p[r]);
					acc2 += carry2[r] + s;        // at most 255 * 255 * 32 767 < 2^32
					carry2[r] += __builtin_amdgcn_readlane(s, 63);
					if (in) a.sumsq[o] = static_cast<double>(acc2);
				}
			}
		}
	}
}

template <bool DWORDS>
__global__ __launch_bounds__(256) void stats_hist_kernel(const uint8_t* __restrict__ in, int W, int H, int S, size_t frameStride, uint32_t* __restrict__ part)
{
	__shared__ uint32_t s_hist[256 * 32];
	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	for (int i = tid; i < 256 * 32; i += 256) s_hist[i] = 0u;
	__syncthreads();
	const int rows = (H + static_cast<int>(gridDim.x) - 1) / static_cast<int>(gridDim.x);
	const int r0 = blockIdx.x * rows, r1 = min(H, r0 + rows);
	const uint8_t* __restrict__ base = in + static_cast<size_t>(blockIdx.y) * frameStride;
	uint32_t* col = s_hist + (tid & 31);
	for (int r = r0 + wave; r < r1; r += 4) {          // a wave per row, a lane per group of four pixels
		const uint8_t* __restrict__ row = base + static_cast<size_t>(r) * S;
		for (int x = 4 * lane; x < W; x += 256) {
			const uint32_t d = load4<DWORDS>(row, x, W);
			const int n = min(4, W - x);
#pragma unroll
			for (int k = 0; k < 4; ++k)
				if (k < n) atomicAdd(col + ((d >> (8 * k)) & 0xffu) * 32, 1u);
		}
	}
	__syncthreads();
	uint32_t sum = 0;
#pragma unroll 8
	for (int j = 0; j < 32; ++j) sum += s_hist[tid * 32 + ((j + tid) & 31)];          // rotated: the lanes of a wave read different banks
	part[(static_cast<size_t>(blockIdx.y) * gridDim.x + blockIdx.x) * 256 + tid] = sum;
}

// part: [frames][chunks][256].  hist (may be null): their sum.  lut (may be null): the equalisation table of the definition.
__global__ __launch_bounds__(256) void stats_hist_finish_kernel(const uint32_t* __restrict__ part, int chunks, uint32_t* __restrict__ hist, float scaleF,
                                                                uint8_t* __restrict__ lut)
{
	__shared__ uint32_t s_wave[4];
	const int i = threadIdx.x, lane = i & 63, wv = i >> 6;
	const size_t f = blockIdx.x;
	uint32_t h = 0;
	for (int c = 0; c < chunks; ++c) h += part[(f * chunks + c) * 256 + i];
	if (hist) hist[f * 256 + i] = h;
	if (!lut) return;
	const uint32_t incl = wave_incl_scan<uint32_t>(h, lane);          // modulo 2^32, like the reference's running sum
	if (lane == 63) s_wave[wv] = incl;
	__syncthreads();
	uint32_t run = incl;
	for (int k = 0; k < wv; ++k) run += s_wave[k];
	const float v = __fmul_rn(static_cast<float>(run), scaleF);       // u32 -> f32 rounds to nearest even; one rounding in the multiply
	lut[f * 256 + i] = v >= 255.f ? static_cast<uint8_t>(255) : static_cast<uint8_t>(static_cast<int>(v));
}

template <bool DWORDS>          // here: in AND out start on a dword, S % 4 == 0
__global__ __launch_bounds__(256) void stats_equalize_kernel(StatsEqualizeArgs a)
{
	__shared__ uint8_t s_lut[256];
	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	const size_t f = blockIdx.y;
	s_lut[tid] = a.lut[f * 256 + tid];
	__syncthreads();
	const int rows = (a.H + static_cast<int>(gridDim.x) - 1) / static_cast<int>(gridDim.x);
	const int r0 = blockIdx.x * rows, r1 = min(a.H, r0 + rows);
	for (int r = r0 + wave; r < r1; r += 4) {
		const size_t o = f * a.frameStride + static_cast<size_t>(r) * a.S;
		for (int x = 4 * lane; x < a.W; x += 256) {          // the lane that reads a pixel writes it: out may be in
			const uint32_t d = load4<DWORDS>(a.in + o, x, a.W);
			const int n = min(4, a.W - x);
			const uint32_t v = s_lut[d & 0xffu] | (static_cast<uint32_t>(s_lut[(d >> 8) & 0xffu]) << 8) | (static_cast<uint32_t>(s_lut[(d >> 16) & 0xffu]) << 16) |
			                   (static_cast<uint32_t>(s_lut[d >> 24]) << 24);
			if (DWORDS && n == 4) *reinterpret_cast<uint32_t*>(a.out + o + x) = v;
			else for (int k = 0; k < n; ++k) a.out[o + x + k] = static_cast<uint8_t>(v >> (8 * k));
		}
	}
}

// whole dwords can be loaded (stored): every pointer, the row stride and the frame stride are multiples of 4
template <typename... P>
bool dword_rows(int S, size_t frameStride, const P*... ptrs) { return (((reinterpret_cast<uintptr_t>(ptrs) | ...) | static_cast<uintptr_t>(S) | frameStride) & 3) == 0; }

} // namespace

int stats_bands(int H) { return (H + kStatsBandRows - 1) / kStatsBandRows; }

int stats_row_chunks(int H, int frames)
{
	int chunks = 1024 / (frames > 0 ? frames : 1);          // about four workgroups per CU in flight, at least 16 rows each; a large batch: one per frame
	chunks = chunks < 1 ? 1 : (chunks > kStatsMaxChunks ? kStatsMaxChunks : chunks);
	if (chunks > (H + 15) / 16) chunks = (H + 15) / 16;
	return chunks;
}

hipError_t launch_stats_band_sums(const StatsBandArgs& args, int frames, hipStream_t stream)
{
	if (!args.in || args.W < 1 || args.H < 1 || args.bands != stats_bands(args.H) || (!args.colSum && !args.colSq && !args.rowSum)) return hipErrorInvalidValue;
	const int threads = args.W <= 256 ? 64 : kStatsThreads;          // four columns per thread; a narrow crop: one wave
	const bool dwords = dword_rows(args.S, args.frameStride, args.in);
	return for_frame_slices(frames, [&](int f0, int nf) {
		StatsBandArgs a = args;
		a.in += static_cast<size_t>(f0) * a.frameStride;
		const size_t cols = static_cast<size_t>(f0) * a.bands * a.W;
		if (a.colSum) a.colSum += cols;
		if (a.colSq) a.colSq += cols;
		if (a.rowSum) a.rowSum += static_cast<size_t>(f0) * a.H;
		const dim3 grid(static_cast<unsigned>(a.bands), static_cast<unsigned>(nf));
		if (dwords) hipLaunchKernelGGL(stats_band_sums_kernel<true>, grid, dim3(threads), 0, stream, a);
		else hipLaunchKernelGGL(stats_band_sums_kernel<false>, grid, dim3(threads), 0, stream, a);
		return hipGetLastError();
	});
}

hipError_t launch_stats_band_scan(uint64_t* colSum, uint64_t* colSq, int bands, int W, int32_t* projX, int frames, hipStream_t stream)
{
	if ((!colSum && !colSq) || (projX && !colSum) || bands < 1 || W < 1) return hipErrorInvalidValue;
	return for_frame_slices(frames, [&](int f0, int nf) {
		const size_t cols = static_cast<size_t>(f0) * bands * W;
		hipLaunchKernelGGL(stats_band_scan_kernel, dim3(static_cast<unsigned>((W + 255) / 256), static_cast<unsigned>(nf)), dim3(256), 0, stream,
		                   colSum ? colSum + cols : nullptr, colSq ? colSq + cols : nullptr, bands, W, projX ? projX + static_cast<size_t>(f0) * W : nullptr);
		return hipGetLastError();
	});
}

hipError_t launch_stats_integral(const StatsIntegralArgs& args, int frames, hipStream_t stream)
{
	if (!args.in || args.W < 1 || args.H < 1 || args.bands != stats_bands(args.H) || args.sumStride < static_cast<size_t>(args.W) + 1) return hipErrorInvalidValue;
	if ((!args.sum && !args.sumsq) || (args.sum && !args.edgeSum) || (args.sumsq && !args.edgeSq)) return hipErrorInvalidValue;
	return for_frame_slices(frames, [&](int f0, int nf) {
		StatsIntegralArgs a = args;
		a.in += static_cast<size_t>(f0) * a.frameStride;
		const size_t cols = static_cast<size_t>(f0) * a.bands * a.W, outs = static_cast<size_t>(f0) * (static_cast<size_t>(a.H) + 1) * a.sumStride;
		if (a.sum) { a.edgeSum += cols; a.sum += outs; }
		if (a.sumsq) { a.edgeSq += cols; a.sumsq += outs; }
		const dim3 grid(static_cast<unsigned>(a.bands), static_cast<unsigned>(nf));
		if (a.sum && a.sumsq) hipLaunchKernelGGL((stats_integral_kernel<true, true>), grid, dim3(kStatsTile), 0, stream, a);
		else if (a.sum) hipLaunchKernelGGL((stats_integral_kernel<true, false>), grid, dim3(kStatsTile), 0, stream, a);
		else hipLaunchKernelGGL((stats_integral_kernel<false, true>), grid, dim3(kStatsTile), 0, stream, a);
		return hipGetLastError();
	});
}

hipError_t launch_stats_hist(const uint8_t* in, int W, int H, int S, size_t frameStride, int frames, int chunks, uint32_t* part, hipStream_t stream)
{
	if (!in || !part || W < 1 || H < 1 || chunks < 1 || chunks > kStatsMaxChunks) return hipErrorInvalidValue;
	return for_frame_slices(frames, [&](int f0, int nf) {
		const dim3 grid(static_cast<unsigned>(chunks), static_cast<unsigned>(nf));
		const uint8_t* const src = in + static_cast<size_t>(f0) * frameStride;
		uint32_t* const dst = part + static_cast<size_t>(f0) * chunks * 256;
		if (dword_rows(S, frameStride, in)) hipLaunchKernelGGL(stats_hist_kernel<true>, grid, dim3(256), 0, stream, src, W, H, S, frameStride, dst);
		else hipLaunchKernelGGL(stats_hist_kernel<false>, grid, dim3(256), 0, stream, src, W, H, S, frameStride, dst);
		return hipGetLastError();
	});
}

hipError_t launch_stats_hist_finish(const uint32_t* part, int chunks, uint32_t* hist, float scaleF, uint8_t* lut, int frames, hipStream_t stream)
{
	if (!part || chunks < 1 || (!hist && !lut) || frames < 1) return hipErrorInvalidValue;
	hipLaunchKernelGGL(stats_hist_finish_kernel, dim3(static_cast<unsigned>(frames)), dim3(256), 0, stream, part, chunks, hist, scaleF, lut);          // frames in x
	return hipGetLastError();
}

hipError_t launch_stats_equalize(const StatsEqualizeArgs& args, int frames, int chunks, hipStream_t stream)
{
	if (!args.in || !args.out || !args.lut || args.W < 1 || args.H < 1 || chunks < 1) return hipErrorInvalidValue;
	return for_frame_slices(frames, [&](int f0, int nf) {
		StatsEqualizeArgs a = args;
		a.in += static_cast<size_t>(f0) * a.frameStride; a.out += static_cast<size_t>(f0) * a.frameStride; a.lut += static_cast<size_t>(f0) * 256;
		const dim3 grid(static_cast<unsigned>(chunks), static_cast<unsigned>(nf));
		if (dword_rows(args.S, args.frameStride, args.in, args.out)) hipLaunchKernelGGL(stats_equalize_kernel<true>, grid, dim3(256), 0, stream, a);
		else hipLaunchKernelGGL(stats_equalize_kernel<false>, grid, dim3(256), 0, stream, a);
		return hipGetLastError();
	});
}

} // namespace compvhip
