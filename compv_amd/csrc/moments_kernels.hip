// moments_kernels.hip -- image moments per frame and per component (compvhip_moments_frames, _components, _shapes; definition in
// include/compv_hip.h, "image moments", and docs/kernels/moments.md).  Every raw moment is an integer sum, so the order of the adds is free: partial
// sums are folded in registers, across the wave and (frames) through LDS, and what is left goes into the caller's records with 64-bit atomic adds.
// The result is exact and the same from run to run.
//
// Launches:
//  moments_zero_kernel        the records a call serves := 0 (the call's own clear: nothing rests on what the caller's memory held)
//  moments_frames_kernel      one workgroup per kMomentsRows rows of a frame.  A row is cut into 16-byte chunks at 16-byte ADDRESSES, whatever the base
//                             and the stride: chunk c of a row whose address is a (mod 16) holds the columns 16 c - a .. 16 c - a + 15.  A chunk inside
//                             the row is one 16-byte load and twelve dot4 instructions (sum w, sum k w, sum k k w for the byte positions k = 0 .. 15, in
//                             32 bits); a chunk that crosses an end of the row is read byte by byte, guarded.  sum (i0 + k) w = i0 sum w + sum k w and its
//                             square form move the chunk to its column i0; j is constant in a row.  Six sums per lane in 64 bits, wave reduction, LDS,
//                             six atomics per workgroup.
//  moments_components_kernel  one wave per 512 columns of kMomentsCompRows label rows, 8 consecutive elements per lane and row.  A lane folds its
//                             elements of one id; the wave folds the lanes that share the first active lane's id, in two rounds (as comp_count_kernel
//                             does), and holds the sums of one id back -- on a fold about another id the heavier of the two (by m00) stays and the other
//                             goes out: six atomics then and at the end of the band, and per lane for what two rounds left.
//  moments_shapes_kernel      one thread per record: moments::shape.
#include "device.hpp"
#include "frame_slices.hpp"
#include "moments_math.hpp"

namespace compvhip {

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kCompElems = 8;                      // label elements of one lane
constexpr int kCompSpan = 64 * kCompElems;         // columns of one wave
constexpr unsigned kMaxBlocks = 1u << 20;          // of the grid-stride kernels

typedef unsigned long long u64;

__device__ __forceinline__ int served(const int32_t* counts, size_t g, int cap) { return counts ? min(max(counts[g], 0), cap) : cap; }

// 0x01 in every byte of d that is not zero
__device__ __forceinline__ uint32_t nonzero_bytes(uint32_t d) { return ((((d & 0x7f7f7f7fu) + 0x7f7f7f7fu) | d) & 0x80808080u) >> 7; }

__device__ __forceinline__ uint32_t dot4(uint32_t a, uint32_t b, uint32_t c) { return __builtin_amdgcn_udot4(a, b, c, false); }

// v[p] without a dynamic index: the array stays in registers
template <typename T>
__device__ __forceinline__ T pick(const T (&v)[kCompElems], int p)
{
	T r = v[0];
#pragma unroll
	for (int e = 1; e < kCompElems; ++e) r = p == e ? v[e] : r;
	return r;
}

// the six sums of pixels of row j with s0 = sum w, s1 = sum i w, s2 = sum i i w
__device__ __forceinline__ void add_row_sums(u64 (&m)[6], u64 j, u64 s0, u64 s1, u64 s2)
{
	m[0] += s0; m[1] += j * s0; m[2] += s1; m[3] += j * s1; m[4] += j * j * s0; m[5] += s2;
}

// the six sums of a record, added by this lane; sums of 0 are not sent
__device__ __forceinline__ void send(u64* dst, const u64 (&m)[6])
{
#pragma unroll
	for (int q = 0; q < 6; ++q) if (m[q]) atomicAdd(dst + q, m[q]);
}

__global__ __launch_bounds__(kThreads) void moments_zero_kernel(compvhip_moments* raw, size_t groups, int cap, const int32_t* counts)
{
	const size_t total = groups * (size_t)cap;
	for (size_t idx = (size_t)blockIdx.x * kThreads + threadIdx.x; idx < total; idx += (size_t)gridDim.x * kThreads) {
		const size_t g = idx / (size_t)cap;
		if ((int)(idx - g * (size_t)cap) >= served(counts, g, cap)) continue;
		compvhip_moments z = {};
		raw[idx] = z;
	}
}

__global__ __launch_bounds__(kThreads) void moments_frames_kernel(MomentsFramesArgs a)
{
	__shared__ u64 part[kWaves][6];
	const int f = a.frame0 + blockIdx.y;
	const uint8_t* frame = a.gray + (size_t)f * a.S * (size_t)a.H;
	const int row0 = blockIdx.x * kMomentsRows, rows = min(kMomentsRows, a.H - row0);
	const int cpr = (a.W + 30) >> 4;                 // chunks of a row at the worst address (a = 15)
	const int items = rows * cpr;
	const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
	u64 m[6] = {};
	for (int t = threadIdx.x; t < items; t += kThreads) {
		const int r = t / cpr, c = t - r * cpr, j = row0 + r;
		const uint8_t* row = frame + (size_t)j * a.S;
		const int i0 = c * 16 - (int)(reinterpret_cast<uintptr_t>(row) & 15);
		if (i0 >= a.W) continue;
		uint32_t s0 = 0, s1 = 0;
		u64 s2 = 0;
		if (i0 >= 0 && i0 + 16 <= a.W) {
			const uint4 v = *reinterpret_cast<const uint4*>(row + i0);
			uint32_t d[4] = { v.x, v.y, v.z, v.w };
			uint32_t k1 = 0, k2 = 0;
			// byte positions k = 4 q + b: k as 0x03020100 + q * 0x04040404, k * k spelled out (225 fits a byte)
			const uint32_t sq[4] = { 0x09040100u, 0x31241910u, 0x79645140u, 0xe1c4a990u };
#pragma unroll
			for (int q = 0; q < 4; ++q) {
				const uint32_t w = a.unit ? nonzero_bytes(d[q]) : d[q];
				s0 = dot4(w, 0x01010101u, s0);
				k1 = dot4(w, 0x03020100u + (uint32_t)q * 0x04040404u, k1);
				k2 = dot4(w, sq[q], k2);
			}
			// sum (i0 + k) w and sum (i0 + k)^2 w
			s1 = (uint32_t)i0 * s0 + k1;
			s2 = (u64)((uint32_t)i0 * (uint32_t)i0) * s0 + (u64)(2u * (uint32_t)i0) * k1 + k2;
		}
		else {
			for (int k = max(i0, 0); k < min(i0 + 16, a.W); ++k) {
				const uint32_t p = row[k], w = a.unit ? (p != 0) : p;
				s0 += w; s1 += (uint32_t)k * w; s2 += (u64)((uint32_t)k * (uint32_t)k) * w;
			}
		}
		add_row_sums(m, (u64)j, s0, s1, s2);
	}
#pragma unroll
	for (int k = 0; k < 6; ++k) {
		const u64 s = wave_sum(m[k]);
		if (lane == 0) part[wv][k] = s;
	}
	__syncthreads();
	if (threadIdx.x < 6) {
		u64 s = 0;
#pragma unroll
		for (int w = 0; w < kWaves; ++w) s += part[w][threadIdx.x];
		if (s) atomicAdd(reinterpret_cast<u64*>(a.raw + f) + threadIdx.x, s);
	}
}

__global__ __launch_bounds__(kThreads) void moments_components_kernel(MomentsCompArgs a)
{
	const int f = a.frame0 + blockIdx.y;
	const int spans = (a.W + kCompSpan - 1) / kCompSpan, bands = (a.H + kMomentsCompRows - 1) / kMomentsCompRows;
	const long long item = (long long)blockIdx.x * kWaves + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
	if (item >= (long long)spans * bands) return;          // (whole waves leave: the folds below need the wave's lanes together)
	const int band = (int)(item / spans), lane = threadIdx.x & 63;
	const int x0 = (int)(item - (long long)band * spans) * kCompSpan + lane * kCompElems;
	const int n = min(max(a.W - x0, 0), kCompElems);
	const int bound = served(a.counts, (size_t)f, a.compCap);
	const compvhip_component* comps = a.comps + (size_t)f * a.compCap;
	u64* out = reinterpret_cast<u64*>(a.raw + (size_t)f * a.compCap);
	// what the wave holds back, the same in every lane: the sums of the id its last fold was about.  Most folds of a wave are about one id (the benchmark
	// frames put 87 % of their edge pixels into one component), and every atomic of that id from every wave lands on the same 48 bytes.
	int held = 0;
	u64 hm[6] = {};
	const int rowEnd = min((band + 1) * kMomentsCompRows, a.H);
	for (int j = band * kMomentsCompRows; j < rowEnd; ++j) {
		const int32_t* lab = a.labels + ((size_t)f * a.H + j) * a.labelStride + x0;
		const uint8_t* g = a.gray ? a.gray + ((size_t)f * a.H + j) * a.S + x0 : nullptr;
		// the lane's elements and their gray bytes in registers; vm: the elements with a served id
		int32_t L[kCompElems];
		uint32_t G[kCompElems];
		uint32_t vm = 0;
#pragma unroll
		for (int e = 0; e < kCompElems; ++e) {
			L[e] = e < n ? lab[e] : 0;
			G[e] = g && e < n ? g[e] : 1u;
			if (L[e] > 0 && L[e] <= bound) vm |= 1u << e;
		}
		while (__any(vm != 0)) {
			// one (id, sums) per lane and turn: the lane's next elements of one id (elements without a served id between them do not part them)
			int id = 0, ox = 0, oy = 0;
			uint32_t s0 = 0;
			u64 s1 = 0, s2 = 0;
			while (vm) {
				const int e = __builtin_ctz(vm);
				const int l = pick(L, e);
				if (id && l != id) break;
				vm &= vm - 1;
				if (!id) {
					id = l;
					if (a.box) { ox = comps[id - 1].x0; oy = comps[id - 1].y0; }
				}
				const uint32_t p = pick(G, e), w = a.unit ? (p != 0) : p;          // (without gray planes p is 1)
				const uint32_t i = (uint32_t)(x0 + e - ox);          // (a record that does not hold its component wraps here: other numbers, no other address)
				s0 += w; s1 += (u64)i * w; s2 += (u64)(i * i) * w;
			}
			// two rounds of "everybody with the first active lane's id"
			for (int k = 0; k < 2; ++k) {
				const u64 act = __ballot(id > 0);
				if (!act) break;
				const int lead = __builtin_ctzll(act);
				const int lid = __shfl(id, lead);
				const uint32_t jr = (uint32_t)(j - __shfl(oy, lead));
				const bool mine = id == lid;
				const uint32_t t0 = wave_sum(mine ? s0 : 0u);
				const u64 t1 = wave_sum(mine ? s1 : (u64)0), t2 = wave_sum(mine ? s2 : (u64)0);
				if (lid == held) add_row_sums(hm, (u64)jr, t0, t1, t2);          // (the same in every lane)
				else {
					// the heavier of the two stays: the component everybody sends to is the one with the most pixels, and it is not put out
					// by every small one that crosses the band
					u64 m[6] = {};
					add_row_sums(m, (u64)jr, t0, t1, t2);
					if (held == 0 || hm[0] < m[0]) {
						if (held > 0 && lane == 0) send(out + (size_t)(held - 1) * 6, hm);
						held = lid;
#pragma unroll
						for (int q = 0; q < 6; ++q) hm[q] = m[q];
					}
					else if (lane == 0) send(out + (size_t)(lid - 1) * 6, m);
				}
				if (mine) id = 0;
			}
			if (id > 0) {
				u64 m[6] = {};
				add_row_sums(m, (u64)(uint32_t)(j - oy), s0, s1, s2);
				send(out + (size_t)(id - 1) * 6, m);
			}
		}
	}
	if (held > 0 && lane == 0) send(out + (size_t)(held - 1) * 6, hm);
}

__global__ __launch_bounds__(kThreads) void moments_shapes_kernel(MomentsShapeArgs a)
{
	const size_t total = a.groups * (size_t)a.cap;
	for (size_t idx = (size_t)blockIdx.x * kThreads + threadIdx.x; idx < total; idx += (size_t)gridDim.x * kThreads) {
		const size_t g = idx / (size_t)a.cap;
		if ((int)(idx - g * (size_t)a.cap) >= served(a.counts, g, a.cap)) continue;
		compvhip_moments_shape s;
		moments::shape(a.raw[idx], &s);
		a.shape[idx] = s;
	}
}

unsigned strideBlocks(size_t total) { return (unsigned)std::min<size_t>((total + kThreads - 1) / kThreads, kMaxBlocks); }

hipError_t launchZero(compvhip_moments* raw, size_t groups, int cap, const int32_t* counts, hipStream_t stream)
{
	hipLaunchKernelGGL(moments_zero_kernel, dim3(strideBlocks(groups * (size_t)cap)), dim3(kThreads), 0, stream, raw, groups, cap, counts);
	return hipGetLastError();
}

} // namespace

hipError_t launch_moments_frames(const MomentsFramesArgs& a0, hipStream_t stream)
{
	if (a0.frames <= 0) return hipSuccess;
	const hipError_t e = hipMemsetAsync(a0.raw, 0, (size_t)a0.frames * sizeof(compvhip_moments), stream);
	if (e != hipSuccess) return e;
	MomentsFramesArgs a = a0;
	const unsigned groups = (unsigned)((a.H + kMomentsRows - 1) / kMomentsRows);
	return for_frame_slices(a.frames, [&](int f0, int nf) {
		a.frame0 = f0;
		hipLaunchKernelGGL(moments_frames_kernel, dim3(groups, (unsigned)nf), dim3(kThreads), 0, stream, a);
		return hipGetLastError();
	});
}

hipError_t launch_moments_components(const MomentsCompArgs& a0, hipStream_t stream)
{
	if (a0.frames <= 0 || a0.compCap <= 0) return hipSuccess;
	const hipError_t e = launchZero(a0.raw, (size_t)a0.frames, a0.compCap, a0.counts, stream);
	if (e != hipSuccess) return e;
	MomentsCompArgs a = a0;
	const long long items = (long long)((a.W + kCompSpan - 1) / kCompSpan) * ((a.H + kMomentsCompRows - 1) / kMomentsCompRows);
	const unsigned blocks = (unsigned)((items + kWaves - 1) / kWaves);
	return for_frame_slices(a.frames, [&](int f0, int nf) {
		a.frame0 = f0;
		hipLaunchKernelGGL(moments_components_kernel, dim3(blocks, (unsigned)nf), dim3(kThreads), 0, stream, a);
		return hipGetLastError();
	});
}

hipError_t launch_moments_shapes(const MomentsShapeArgs& a, hipStream_t stream)
{
	const size_t total = a.groups * (size_t)a.cap;
	if (!total) return hipSuccess;
	hipLaunchKernelGGL(moments_shapes_kernel, dim3(strideBlocks(total)), dim3(kThreads), 0, stream, a);
	return hipGetLastError();
}

} // namespace compvhip
