// match_kernels.hip -- brute-force Hamming matching (CompVMatcherBruteForce, core/matchers/compv_core_matcher_bruteforce.cxx:81-228) for gfx950:
// k nearest train rows of every query row in (distance, train index) order, and the sample's good-match filter.  Definition: include/compv_hip.h,
// docs/kernels/match.md.
//
//   match_slice_kernel   one workgroup = kMatchQueryBlock queries (one per lane, the descriptor in registers) x one slice of kMatchTrainSlice train
//                        rows (staged once in LDS, read uniformly by the wave: a broadcast); per dword one XOR and one accumulating popcount, then
//                        a branch-free insertion of the key (distance << 16 | row within the slice) into a sorted register list.  The list goes
//                        to scratch: [pair][slice][k][queryCap] keys.
//   match_merge_kernel   one thread per query: merges the lists of the pair's slices by (distance, train index) and writes the records.
//   match_reference_kernel  the host entry point's kernel: one lane per query walks ALL train rows upward (slice after slice through the same LDS
//                        stage) and inserts as the reference does, comparing distances only -- which reproduces the reference's order among
//                        equal distances (it is NOT the (distance, index) order: see docs/kernels/match.md).
//   match_good_kernel    one workgroup per pair: flag -> rank by wave prefix sums -> emit, in ascending query order.
// Keys are unique (the train index is part of them), so every minimum is decided by comparison alone: no atomic anywhere.
#include "kernels.hpp"

namespace compvhip {
namespace {

constexpr int kQB = kMatchQueryBlock, kTS = kMatchTrainSlice;
constexpr uint32_t kEmptyKey = 0xffffffffu;          // above every real key: distance <= 1024, row < kTS

__device__ __forceinline__ int clipCount(const int32_t* counts, int idx, int cap)
{
	if (!counts) return cap;
	const int c = counts[idx];
	return c < 0 ? 0 : (c > cap ? cap : c);
}

// DW: descriptor dwords the registers and the LDS rows hold (the real count rounded up to a power of two; the padding is zero on both sides and
// adds nothing to a distance).  K: list length (knn rounded up to a power of two; only the first knn entries leave the kernel).
template <int DW, int K>
__global__ __launch_bounds__(kQB) void match_slice_kernel(MatchSliceArgs a)
{
	__shared__ __attribute__((aligned(16))) uint32_t sTrain[kTS * DW];
	const int tid = threadIdx.x, pair = blockIdx.z, slice = blockIdx.y;
	const int Q = clipCount(a.queryCounts, a.queryShared ? 0 : pair, a.queryCap);
	const int T = clipCount(a.trainCounts, a.trainShared ? 0 : pair, a.trainCap);
	const int q0 = blockIdx.x * kQB, t0 = slice * kTS;
	if (q0 >= Q || t0 >= T) return;          // workgroup-uniform, in front of every barrier
	const int nT = min(kTS, T - t0);
	const uint8_t* __restrict__ train = a.train + (a.trainShared ? 0 : static_cast<size_t>(pair) * a.trainCap * a.trainStride) + static_cast<size_t>(t0) * a.trainStride;
	for (int i = tid; i < nT * DW; i += kQB) {
		const int r = i / DW, w = i % DW;
		sTrain[i] = w < a.descDwords ? reinterpret_cast<const uint32_t*>(train + static_cast<size_t>(r) * a.trainStride)[w] : 0u;
	}
	const int q = q0 + tid;
	const bool valid = q < Q;
	uint32_t qd[DW];
	{
		const uint8_t* __restrict__ row = a.query + (a.queryShared ? 0 : static_cast<size_t>(pair) * a.queryCap * a.queryStride) + static_cast<size_t>(valid ? q : q0) * a.queryStride;
#pragma unroll
		for (int w = 0; w < DW; ++w) qd[w] = w < a.descDwords ? reinterpret_cast<const uint32_t*>(row)[w] : 0u;
	}
	__syncthreads();
	uint32_t best[K];
#pragma unroll
	for (int k = 0; k < K; ++k) best[k] = kEmptyKey;
	for (int t = 0; t < nT; ++t) {
		const uint32_t* __restrict__ row = sTrain + t * DW;          // wave-uniform address
		uint32_t d = 0;
		if (DW >= 4) {
#pragma unroll
			for (int w = 0; w < DW; w += 4) {
				const uint4 v = *reinterpret_cast<const uint4*>(row + w);
				d += __popc(qd[w] ^ v.x); d += __popc(qd[w + 1] ^ v.y); d += __popc(qd[w + 2] ^ v.z); d += __popc(qd[w + 3] ^ v.w);
			}
		}
		else {
#pragma unroll
			for (int w = 0; w < DW; ++w) d += __popc(qd[w] ^ row[w]);
		}
		uint32_t c = (d << 16) | static_cast<uint32_t>(t);
#pragma unroll
		for (int k = 0; k < K; ++k) {          // sorted insertion: the list keeps the K smallest keys seen
			const uint32_t lo = min(best[k], c);
			c = max(best[k], c);
			best[k] = lo;
		}
	}
	if (!valid) return;
	uint32_t* __restrict__ out = a.partial + (static_cast<size_t>(pair) * a.slices + slice) * a.knn * a.queryCap + q;
#pragma unroll
	for (int k = 0; k < K; ++k) if (k < a.knn) out[static_cast<size_t>(k) * a.queryCap] = best[k];
}

// The reference's insertion (compv_core_matcher_bruteforce.cxx:209-224), order included: the candidate walks down the list and swaps with every entry
// whose DISTANCE is larger; the displaced entry walks on.  An entry displaced from the head of a run of equal distances therefore lands behind the
// run (or falls off the list), so the order among equal distances depends on the arrival sequence and t has to walk upward through all rows.
template <int DW, int K>
__global__ __launch_bounds__(kQB) void match_reference_kernel(MatchSliceArgs a)
{
	__shared__ __attribute__((aligned(16))) uint32_t sTrain[kTS * DW];
	const int tid = threadIdx.x, pair = blockIdx.y;
	const int Q = clipCount(a.queryCounts, a.queryShared ? 0 : pair, a.queryCap);
	const int T = clipCount(a.trainCounts, a.trainShared ? 0 : pair, a.trainCap);
	const int q0 = blockIdx.x * kQB;
	if (q0 >= Q) return;          // workgroup-uniform, in front of every barrier
	const int q = q0 + tid;
	const bool valid = q < Q;
	uint32_t qd[DW];
	{
		const uint8_t* __restrict__ row = a.query + (a.queryShared ? 0 : static_cast<size_t>(pair) * a.queryCap * a.queryStride) + static_cast<size_t>(valid ? q : q0) * a.queryStride;
#pragma unroll
		for (int w = 0; w < DW; ++w) qd[w] = w < a.descDwords ? reinterpret_cast<const uint32_t*>(row)[w] : 0u;
	}
	int bd[K], bt[K];
#pragma unroll
	for (int k = 0; k < K; ++k) { bd[k] = 0x7fffffff; bt[k] = -1; }
	const uint8_t* __restrict__ trainBase = a.train + (a.trainShared ? 0 : static_cast<size_t>(pair) * a.trainCap * a.trainStride);
	for (int t0 = 0; t0 < T; t0 += kTS) {          // T is workgroup-uniform
		const int nT = min(kTS, T - t0);
		__syncthreads();          // the previous slice has been consumed
		for (int i = tid; i < nT * DW; i += kQB) {
			const int r = i / DW, w = i % DW;
			sTrain[i] = w < a.descDwords ? reinterpret_cast<const uint32_t*>(trainBase + static_cast<size_t>(t0 + r) * a.trainStride)[w] : 0u;
		}
		__syncthreads();
		for (int t = 0; t < nT; ++t) {
			const uint32_t* __restrict__ row = sTrain + t * DW;
			int cd = 0, ct = t0 + t;
#pragma unroll
			for (int w = 0; w < DW; ++w) cd += __popc(qd[w] ^ row[w]);
#pragma unroll
			for (int k = 0; k < K; ++k) {
				const bool lt = cd < bd[k];
				const int od = bd[k], ot = bt[k];
				bd[k] = lt ? cd : od; bt[k] = lt ? ct : ot;
				cd = lt ? od : cd; ct = lt ? ot : ct;
			}
		}
	}
	if (!valid) return;
	int4* __restrict__ out = reinterpret_cast<int4*>(a.matches) + static_cast<size_t>(pair) * a.knn * a.queryCap + q;
#pragma unroll
	for (int k = 0; k < K; ++k) if (k < a.knn) out[static_cast<size_t>(k) * a.queryCap] = make_int4(q, bt[k], 0, bd[k]);
}

template <int K>
__global__ __launch_bounds__(256) void match_merge_kernel(MatchSliceArgs a)
{
	const int pair = blockIdx.y, q = blockIdx.x * 256 + threadIdx.x;
	const int Q = clipCount(a.queryCounts, a.queryShared ? 0 : pair, a.queryCap);
	const int T = clipCount(a.trainCounts, a.trainShared ? 0 : pair, a.trainCap);
	if (q >= Q) return;
	const int slices = (T + kTS - 1) / kTS;          // the slices that ran
	unsigned long long best[K];
#pragma unroll
	for (int k = 0; k < K; ++k) best[k] = ~0ull;
	for (int s = 0; s < slices; ++s) {
		const uint32_t* __restrict__ in = a.partial + (static_cast<size_t>(pair) * a.slices + s) * a.knn * a.queryCap + q;
		for (int j = 0; j < a.knn; ++j) {
			const uint32_t key = in[static_cast<size_t>(j) * a.queryCap];
			if (key == kEmptyKey) break;          // the list is sorted: nothing behind an empty slot
			unsigned long long c = (static_cast<unsigned long long>(key >> 16) << 32) | static_cast<unsigned int>(s * kTS + static_cast<int>(key & 0xffffu));
#pragma unroll
			for (int k = 0; k < K; ++k) {
				const unsigned long long lo = best[k] < c ? best[k] : c;
				c = best[k] < c ? c : best[k];
				best[k] = lo;
			}
		}
	}
	int4* __restrict__ out = reinterpret_cast<int4*>(a.matches) + static_cast<size_t>(pair) * a.knn * a.queryCap + q;
#pragma unroll
	for (int k = 0; k < K; ++k) {
		if (k >= a.knn) break;
		const bool have = best[k] != ~0ull;
		out[static_cast<size_t>(k) * a.queryCap] = make_int4(q, have ? static_cast<int>(best[k] & 0xffffffffull) : -1, 0, have ? static_cast<int>(best[k] >> 32) : 0x7fffffff);
	}
}

// Per pair: good[i] = matches[0][q] of the i-th query (ascending q) that passes every enabled test; counts[pair] = their number before clipping.
__global__ __launch_bounds__(256) void match_good_kernel(MatchGoodArgs a)
{
	__shared__ int sWave[4];
	const int pair = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	const int Q = clipCount(a.queryCounts, pair, a.queryCap);
	const int T = clipCount(a.trainCounts, a.trainShared ? 0 : pair, a.trainCap);
	const int4* __restrict__ m0 = reinterpret_cast<const int4*>(a.matches) + static_cast<size_t>(pair) * a.knn * a.queryCap;
	const int4* __restrict__ rev = reinterpret_cast<const int4*>(a.reverse) + static_cast<size_t>(pair) * a.trainCap;
	int4* __restrict__ out = reinterpret_cast<int4*>(a.good) + static_cast<size_t>(pair) * a.goodCap;
	long long base = 0;
	for (int q0 = 0; q0 < Q && T > 0; q0 += 256) {          // Q and T are workgroup-uniform
		const int q = q0 + tid;
		bool ok = q < Q;
		int4 m = make_int4(0, 0, 0, 0);
		if (ok) {
			m = m0[q];
			if (a.ratio > 0.0) ok = T >= 2 && static_cast<double>(m.w) < a.ratio * static_cast<double>(m0[a.queryCap + q].w);
			if (a.maxDistance >= 0) ok = ok && m.w <= a.maxDistance;
			if (a.crossCheck) ok = ok && m.y >= 0 && m.y < T && rev[m.y].y == q;          // rev[t] = {t, best query of t, 0, distance}
		}
		const unsigned long long mask = __ballot(ok);
		const int before = __popcll(mask & ((1ull << lane) - 1ull));
		__syncthreads();          // the previous round's sWave has been read
		if (lane == 0) sWave[wave] = __popcll(mask);
		__syncthreads();
		int off = 0, total = 0;
#pragma unroll
		for (int w = 0; w < 4; ++w) { if (w < wave) off += sWave[w]; total += sWave[w]; }
		const long long idx = base + off + before;
		if (ok && idx < static_cast<long long>(a.goodCap)) out[idx] = m;
		base += total;
	}
	if (tid == 0) a.counts[pair] = static_cast<int32_t>(base);
}

template <int DW>
hipError_t launchSliceK(const MatchSliceArgs& a, int K, dim3 grid, hipStream_t stream)
{
	switch (K) {
	case 1: hipLaunchKernelGGL((match_slice_kernel<DW, 1>), grid, dim3(kQB), 0, stream, a); break;
	case 2: hipLaunchKernelGGL((match_slice_kernel<DW, 2>), grid, dim3(kQB), 0, stream, a); break;
	case 4: hipLaunchKernelGGL((match_slice_kernel<DW, 4>), grid, dim3(kQB), 0, stream, a); break;
	default: hipLaunchKernelGGL((match_slice_kernel<DW, 8>), grid, dim3(kQB), 0, stream, a); break;
	}
	return hipGetLastError();
}

template <int DW>
hipError_t launchReferenceK(const MatchSliceArgs& a, int K, dim3 grid, hipStream_t stream)
{
	switch (K) {
	case 1: hipLaunchKernelGGL((match_reference_kernel<DW, 1>), grid, dim3(kQB), 0, stream, a); break;
	case 2: hipLaunchKernelGGL((match_reference_kernel<DW, 2>), grid, dim3(kQB), 0, stream, a); break;
	case 4: hipLaunchKernelGGL((match_reference_kernel<DW, 4>), grid, dim3(kQB), 0, stream, a); break;
	default: hipLaunchKernelGGL((match_reference_kernel<DW, 8>), grid, dim3(kQB), 0, stream, a); break;
	}
	return hipGetLastError();
}

int pow2AtLeast(int v) { int p = 1; while (p < v) p <<= 1; return p; }

bool sliceArgsOk(const MatchSliceArgs& a, int pairs)
{
	if (pairs < 1 || a.queryCap < 1 || a.trainCap < 1 || a.knn < 1 || a.knn > kMatchMaxKnn || a.descDwords < 1 || a.descDwords > kMatchMaxDwords) return false;
	if (a.queryStride < a.descDwords * 4 || a.trainStride < a.descDwords * 4 || (a.queryStride & 3) || (a.trainStride & 3)) return false;
	if (a.slices != (a.trainCap + kTS - 1) / kTS || !a.query || !a.train || !a.partial || !a.matches) return false;
	return true;
}

} // namespace

hipError_t launch_match_slices(const MatchSliceArgs& a, int pairs, hipStream_t stream)
{
	if (!sliceArgsOk(a, pairs)) return hipErrorInvalidValue;
	const dim3 grid((a.queryCap + kQB - 1) / kQB, a.slices, pairs);
	const int K = pow2AtLeast(a.knn);
	switch (pow2AtLeast(a.descDwords)) {
	case 1: return launchSliceK<1>(a, K, grid, stream);
	case 2: return launchSliceK<2>(a, K, grid, stream);
	case 4: return launchSliceK<4>(a, K, grid, stream);
	case 8: return launchSliceK<8>(a, K, grid, stream);
	case 16: return launchSliceK<16>(a, K, grid, stream);
	default: return launchSliceK<32>(a, K, grid, stream);
	}
}

hipError_t launch_match_reference(const MatchSliceArgs& a, int pairs, hipStream_t stream)
{
	if (!sliceArgsOk(a, pairs)) return hipErrorInvalidValue;
	const dim3 grid((a.queryCap + kQB - 1) / kQB, pairs);
	const int K = pow2AtLeast(a.knn);
	switch (pow2AtLeast(a.descDwords)) {          // the dword widths a host descriptor comes in: up to 8 (32 bytes), 16, 32
	case 1: case 2: case 4: case 8: return launchReferenceK<8>(a, K, grid, stream);
	case 16: return launchReferenceK<16>(a, K, grid, stream);
	default: return launchReferenceK<32>(a, K, grid, stream);
	}
}

hipError_t launch_match_merge(const MatchSliceArgs& a, int pairs, hipStream_t stream)
{
	if (!sliceArgsOk(a, pairs)) return hipErrorInvalidValue;
	const dim3 grid((a.queryCap + 255) / 256, pairs);
	switch (pow2AtLeast(a.knn)) {
	case 1: hipLaunchKernelGGL(match_merge_kernel<1>, grid, dim3(256), 0, stream, a); break;
	case 2: hipLaunchKernelGGL(match_merge_kernel<2>, grid, dim3(256), 0, stream, a); break;
	case 4: hipLaunchKernelGGL(match_merge_kernel<4>, grid, dim3(256), 0, stream, a); break;
	default: hipLaunchKernelGGL(match_merge_kernel<8>, grid, dim3(256), 0, stream, a); break;
	}
	return hipGetLastError();
}

hipError_t launch_match_good(const MatchGoodArgs& a, int pairs, hipStream_t stream)
{
	if (pairs < 1 || a.queryCap < 1 || a.trainCap < 1 || a.knn < 1 || !a.matches || !a.counts || (a.goodCap && !a.good)) return hipErrorInvalidValue;
	if ((a.ratio > 0.0 && a.knn < 2) || (a.crossCheck && !a.reverse)) return hipErrorInvalidValue;
	hipLaunchKernelGGL(match_good_kernel, dim3(pairs), dim3(256), 0, stream, a);
	return hipGetLastError();
}

} // namespace compvhip
