// ransac_device.hpp -- the wave-level skeleton the RANSAC kernel files (homography_kernels.hip, curvefit_kernels.hip) share on top of device.hpp: the
// clamped set count, the fold of sum64, the selection of the best try, the compaction of its inliers and the staged walk over a set's points.  What a
// family adds is its model, its residual and its refit, handed in as functors.  Everything __device__ __forceinline__; the order of every addition
// and of every comparison is part of the bit-exact contract.
#pragma once
#include "device.hpp"
#include "ransac_math.hpp"

namespace compvhip {

// points of set s: the caller's count clamped to [0, cap]; no counts: cap
__device__ __forceinline__ int ransac_count(const int32_t* counts, int s, int cap) { return counts ? min(max(counts[s], 0), cap) : cap; }

// lane l holds partial l of a sum64: p[l] += p[l + stride], stride 32 .. 1 (ransac::fold64 is the array form).  Lane 0 ends with the fold and every
// lane returns it; what the other lanes add on the way down is garbage and is dropped.
__device__ __forceinline__ double wave_fold64(double v)
{
#pragma unroll
	for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
	return __shfl(v, 0);
}

__device__ __forceinline__ double wave_xor_variance(double v, int o) { return __shfl_xor(v, o); }
__device__ __forceinline__ ransac::NoVariance wave_xor_variance(ransac::NoVariance v, int) { return v; }

// The best of the tries [0, tries) of a model of m points by ransac::better, in every lane of the wave: a lane-strided scan, then a butterfly.
// load(t, &count, &variance) reads the score of try t.  No try has m inliers: count < m, tryIdx -1.  The running best stays three scalars: carried
// as one struct, the variance of a try was loaded only after its count had passed (two dependent loads per try; the homography's refit 3 % slower).
template <typename V>
struct BestTry { int count; V variance; int tryIdx; };
template <typename V, typename Load>
__device__ __forceinline__ BestTry<V> wave_best_try(int m, int tries, int lane, Load load)
{
	int bc = 0, bt = -1; V bv = V{};
	for (int t = lane; t < tries; t += 64) {
		int c; V v;
		load(t, &c, &v);
		if (ransac::better(m, c, v, t, bc, bv, bt)) { bc = c; bv = v; bt = t; }
	}
#pragma unroll
	for (int o = 32; o > 0; o >>= 1) {
		const int c = __shfl_xor(bc, o), t = __shfl_xor(bt, o); const V v = wave_xor_variance(bv, o);
		if (ransac::better(m, c, v, t, bc, bv, bt)) { bc = c; bv = v; bt = t; }
	}
	return { bc, bv, bt };
}

// The inliers among the points [0, k) compacted in index order by one wave: inlier(i) loads point i and tells; store(o) writes the point inlier() has
// just loaded to slot o.  mask, where there is one, gets a 0 / 1 byte per point.  Returns the number of inliers (the same in every lane).
template <typename Inlier, typename Store>
__device__ __forceinline__ int wave_compact_inliers(int k, int lane, uint8_t* mask, Inlier inlier, Store store)
{
	int n = 0;
	for (int base = 0; base < k; base += 64) {
		const int i = base + lane;
		bool inl = false;
		if (i < k) {
			inl = inlier(i);
			if (mask) mask[i] = inl ? 1 : 0;
		}
		const unsigned long long b = __ballot(inl);
		if (inl) store(n + __popcll(b & ((1ull << lane) - 1ull)));
		n += __popcll(b);
	}
	return n;
}

// One pass of a workgroup of THREADS over the points [0, k), THREADS at a time through LDS: stage(tid, i) copies point i to slot tid, visit(j) reads
// slot j of the round (0 <= j < the round's points) and runs in live threads only.  Every thread of the workgroup must call it with the same k: the
// barriers are outside everything that diverges.
template <int THREADS, typename Stage, typename Visit>
__device__ __forceinline__ void staged_points(int k, int tid, bool live, Stage stage, Visit visit)
{
	for (int base = 0; base < k; base += THREADS) {
		__syncthreads();
		if (base + tid < k) stage(tid, base + tid);
		__syncthreads();
		const int n = min(THREADS, k - base);
		if (live) {
			for (int j = 0; j < n; ++j) visit(j);
		}
	}
}

} // namespace compvhip
