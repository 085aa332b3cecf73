// homography_kernels.hip -- RANSAC homography (CompVHomography<double>::find, core/calib/compv_core_calib_homography.cxx) for gfx950: good matches to a
// 3 x 3 matrix without a host trip.  The definition is in include/compv_hip.h ("RANSAC homography", items A - H); the arithmetic is homography_math.hpp.
//
//   homography_points_kernel   one workgroup per pair: the good list's records become two float64 point arrays; records with an index outside
//                              its capacity are dropped by a block scan per 256 records, the order kept.
//   homography_solve_kernel    one LANE per try: quad (counter hash or the caller's), collinearity test, computeH of the four correspondences,
//                              the inverse.  The Jacobi pivot indexes the 9 x 9 matrices D and Qt dynamically, so they live in LDS -- 162 float64
//                              per lane, the lanes' words interleaved ([element][lane]: lane-consecutive, conflict-free for every pivot); one
//                              wave per workgroup (82 944 bytes of LDS), no barrier.  Lanes diverge on the rotation count.
//   homography_score_kernel    one lane per try, 256 tries per workgroup: the pair's points are staged in LDS 256 at a time and every lane walks
//                              them in index order twice (inlier count and sum, then the variance about the mean) -- the order of item E.
//   homography_refit_kernel    one wave per pair: selection over the tries (item F), the inlier mask of the best try, the inliers compacted in
//                              index order, computeH over them with lane l holding partial l of sum64, Jacobi by lane 0 in LDS, the record.
//   homography_project_kernel  one lane per point.
// The RANSAC skeleton (clamped count, fold of sum64, selection, compaction, staged walk) is ransac_device.hpp's, shared with curvefit_kernels.hip.
// No MFMA; every store is a plain C++ store.
#include "ransac_device.hpp"
#include "homography_math.hpp"

namespace compvhip {
namespace {

using namespace hg;

constexpr int kSolveThreads = kHomographySolveBlock;     // one wave
constexpr int kScoreThreads = kHomographyScoreBlock;
constexpr int kPointThreads = 256;

__global__ __launch_bounds__(kPointThreads) void homography_points_kernel(HomographyPointsArgs a)
{
	__shared__ int32_t s_flag[kPointThreads];
	const int p = blockIdx.x, tid = threadIdx.x;
	const int n = min(ransac_count(a.goodCounts, p, a.goodCap), a.pointCap);
	const compvhip_match* good = a.good + (size_t)p * a.goodCap;
	const compvhip_keypoint* query = a.query + (size_t)p * a.queryCap;
	const compvhip_keypoint* train = a.train + (a.trainShared ? 0 : (size_t)p * a.trainCap);
	double2* src = a.src + (size_t)p * a.pointCap;
	double2* dst = a.dst + (size_t)p * a.pointCap;
	int kept = 0;
	for (int base = 0; base < n; base += kPointThreads) {
		const int r = base + tid;
		int qi = -1, ti = -1;
		if (r < n) { qi = good[r].queryIdx; ti = good[r].trainIdx; }
		const bool ok = qi >= 0 && qi < a.queryCap && ti >= 0 && ti < a.trainCap;
		s_flag[tid] = ok ? 1 : 0;
		const int32_t total = block_excl_scan<kPointThreads>(s_flag, s_flag, kPointThreads);
		if (ok) {
			const int o = kept + s_flag[tid];
			src[o] = make_double2((double)train[ti].x, (double)train[ti].y);
			dst[o] = make_double2((double)query[qi].x, (double)query[qi].y);
		}
		kept += total;
		__syncthreads();          // s_flag is written again in the next round
	}
	if (tid == 0) a.counts[p] = kept;
}

__global__ __launch_bounds__(kSolveThreads) void homography_solve_kernel(HomographyFindArgs a)
{
	__shared__ double s_mat[162 * kSolveThreads];
	const int lane = threadIdx.x, p = blockIdx.y;
	const int t = blockIdx.x * kSolveThreads + lane;
	const int k = ransac_count(a.counts, p, a.pointCap);
	if (t >= a.tries || k < 4) return;
	const size_t slot = (size_t)p * a.maxTries + t;
	int32_t q[4];
	if (a.quads) {
		const int4 v = reinterpret_cast<const int4*>(a.quads)[(size_t)p * a.tries + t];
		q[0] = v.x; q[1] = v.y; q[2] = v.z; q[3] = v.w;
	}
	else quad(a.seed, (uint32_t)p, (uint32_t)t, (uint32_t)k, q);
	int32_t state = 0, rotations = 0;          // state 1: H and its inverse are valid
	double H[9], Hinv[9];
	const bool inRange = (uint32_t)q[0] < (uint32_t)k && (uint32_t)q[1] < (uint32_t)k && (uint32_t)q[2] < (uint32_t)k && (uint32_t)q[3] < (uint32_t)k;
	if (inRange) {
		const double2* src = a.src + (size_t)p * a.pointCap;
		const double2* dst = a.dst + (size_t)p * a.pointCap;
		double sx[4], sy[4], dx[4], dy[4];
#pragma unroll
		for (int i = 0; i < 4; ++i) {
			const double2 s = src[q[i]], d = dst[q[i]];
			sx[i] = s.x; sy[i] = s.y; dx[i] = d.x; dy[i] = d.y;
		}
		if (!collinear4(sx, sy)) {
			rotations = computeH4<kSolveThreads>(sx, sy, dx, dy, s_mat + lane, s_mat + 81 * kSolveThreads + lane, false, H);
			state = inverse3(H, Hinv) ? 1 : 0;
		}
	}
	a.state[slot] = state;
	a.rotations[slot] = rotations;
	if (state) {
		double* out = a.hyp + slot * 18;
#pragma unroll
		for (int j = 0; j < 9; ++j) { out[j] = H[j]; out[9 + j] = Hinv[j]; }
	}
}

__global__ __launch_bounds__(kScoreThreads) void homography_score_kernel(HomographyFindArgs a)
{
	__shared__ double2 s_src[kScoreThreads], s_dst[kScoreThreads];
	const int tid = threadIdx.x, p = blockIdx.y;
	const int t = blockIdx.x * kScoreThreads + tid;
	const int k = ransac_count(a.counts, p, a.pointCap);
	if (k < 4) return;          // (the whole workgroup: k is the pair's)
	const size_t slot = (size_t)p * a.maxTries + t;
	const bool live = t < a.tries && a.state[slot] != 0;
	double H[9], Hinv[9];
	if (live) {
		const double* in = a.hyp + slot * 18;
#pragma unroll
		for (int j = 0; j < 9; ++j) { H[j] = in[j]; Hinv[j] = in[9 + j]; }
	}
	const double2* src = a.src + (size_t)p * a.pointCap;
	const double2* dst = a.dst + (size_t)p * a.pointCap;
	int count = 0;
	double sum = 0.0, mean = 0.0, var = 0.0;
	for (int pass = 0; pass < 2; ++pass) {
		staged_points<kScoreThreads>(k, tid, live, [&](int slot, int i) { s_src[slot] = src[i]; s_dst[slot] = dst[i]; }, [&](int j) {
			const double d = distance(H, Hinv, s_src[j].x, s_src[j].y, s_dst[j].x, s_dst[j].y);
			if (d < a.threshold) {
				if (pass == 0) { ++count; sum += d; }
				else { const double dev = d - mean; var += dev * dev; }
			}
		});
		if (pass == 0 && count > 0) mean = ddiv(sum, (double)count);
	}
	if (t < a.tries) {
		a.scoreCount[slot] = count;
		a.scoreVar[slot] = count >= 2 ? ddiv(var, (double)(count - 1)) : DBL_MAX;
	}
}

// Hartley normalisation of n > 4 points, lane l holding partial l of every sum64
__device__ __forceinline__ Norm normWave(const double2* pts, int n, int lane)
{
	double sx = 0.0, sy = 0.0;
	for (int i = lane; i < n; i += 64) { const double2 v = pts[i]; sx += v.x; sy += v.y; }
	const double inv = ddiv(1.0, (double)n);
	Norm r;
	r.tx = wave_fold64(sx) * inv; r.ty = wave_fold64(sy) * inv;
	double mag = 0.0;
	for (int i = lane; i < n; i += 64) { const double2 v = pts[i]; mag += hypotNaive(v.x - r.tx, v.y - r.ty); }
	r.s = scaleOf(wave_fold64(mag) * inv);
	return r;
}

__global__ __launch_bounds__(64) void homography_refit_kernel(HomographyFindArgs a)
{
	__shared__ double s_mat[162];
	__shared__ double s_H[9];
	__shared__ int s_rot;
	const int lane = threadIdx.x, p = blockIdx.x;
	const int k = ransac_count(a.counts, p, a.pointCap);
	compvhip_homography_result* out = a.results + p;
	if (k < 4) {
		if (a.mask && lane < k) a.mask[(size_t)p * a.pointCap + lane] = 0;
		if (lane == 0) {
			for (int j = 0; j < 9; ++j) out->H[j] = 0.0;
			out->variance = DBL_MAX; out->inliers = 0; out->bestTry = -1; out->status = 2; out->rotations = 0;
		}
		return;
	}
	// F. selection
	const BestTry<double> best = wave_best_try<double>(4, a.tries, lane, [&](int t, int* count, double* variance) {
		const size_t slot = (size_t)p * a.maxTries + t;
		*count = a.scoreCount[slot]; *variance = a.scoreVar[slot];
	});
	const bool found = best.count >= 4;
	const double2* src = a.src + (size_t)p * a.pointCap;
	const double2* dst = a.dst + (size_t)p * a.pointCap;
	uint8_t* mask = a.mask ? a.mask + (size_t)p * a.pointCap : nullptr;
	int n = k;
	if (found) {          // the inliers of the best try, compacted in index order
		double H[9], Hinv[9];
		const double* in = a.hyp + ((size_t)p * a.maxTries + best.tryIdx) * 18;
#pragma unroll
		for (int j = 0; j < 9; ++j) { H[j] = in[j]; Hinv[j] = in[9 + j]; }
		double2* selSrc = a.selSrc + (size_t)p * a.pointCap;
		double2* selDst = a.selDst + (size_t)p * a.pointCap;
		double2 s = make_double2(0.0, 0.0), d = s;
		n = wave_compact_inliers(k, lane, mask, [&](int i) { s = src[i]; d = dst[i]; return distance(H, Hinv, s.x, s.y, d.x, d.y) < a.threshold; },
		                         [&](int o) { selSrc[o] = s; selDst[o] = d; });
		src = selSrc; dst = selDst;
		__syncthreads();          // one wave: the compacted points are visible to every lane
	}
	else if (mask) {
		for (int i = lane; i < k; i += 64) mask[i] = 0;
	}
	// G. computeH over the n points, promotion on
	if (n == 4) {
		if (lane == 0) {
			double sx[4], sy[4], dx[4], dy[4], H[9];
			for (int i = 0; i < 4; ++i) { sx[i] = src[i].x; sy[i] = src[i].y; dx[i] = dst[i].x; dy[i] = dst[i].y; }
			s_rot = computeH4<1>(sx, sy, dx, dy, s_mat, s_mat + 81, true, H);
			for (int j = 0; j < 9; ++j) s_H[j] = H[j];
		}
	}
	else {
		const Norm na = normWave(src, n, lane), nb = normWave(dst, n, lane);
		double acc[45];
#pragma unroll
		for (int e = 0; e < 45; ++e) acc[e] = 0.0;
		for (int i = lane; i < n; i += 64) {
			const double2 s = src[i], d = dst[i];
			double m0[9], m1[9];
			rowsOf(normalised(s.x, na.tx, na.s), normalised(s.y, na.ty, na.s), normalised(d.x, nb.tx, nb.s), normalised(d.y, nb.ty, nb.s), m0, m1);
			accumulateS(m0, m1, acc);
		}
#pragma unroll
		for (int e = 0; e < 45; ++e) acc[e] = wave_fold64(acc[e]);
		if (lane == 0) {
			double H[9];
			storeS<1>(acc, s_mat, s_mat + 81);
			s_rot = jacobi<1>(s_mat, s_mat + 81);
			finishH<1>(s_mat, s_mat + 81, na, nb, true, H);
			for (int j = 0; j < 9; ++j) s_H[j] = H[j];
		}
	}
	__syncthreads();
	if (lane < 9) out->H[lane] = s_H[lane];
	if (lane == 0) {
		out->variance = found ? best.variance : DBL_MAX;
		out->inliers = found ? best.count : 0;
		out->bestTry = found ? best.tryIdx : -1;
		out->status = found ? 0 : 1;
		out->rotations = s_rot;
	}
}

__global__ __launch_bounds__(256) void homography_project_kernel(HomographyProjectArgs a)
{
	const int i = blockIdx.x * 256 + threadIdx.x, p = blockIdx.y;
	if (i >= a.n) return;
	const compvhip_homography_result* r = a.results + p;
	double H[9];
#pragma unroll
	for (int j = 0; j < 9; ++j) H[j] = r->H[j];
	const double2 v = a.points[(a.shared ? 0 : (size_t)p * a.n) + i];
	double2 o;
	project(H, v.x, v.y, &o.x, &o.y);
	a.out[(size_t)p * a.n + i] = o;
}

} // namespace

hipError_t launch_homography_points(const HomographyPointsArgs& a, int pairs, hipStream_t stream)
{
	hipLaunchKernelGGL(homography_points_kernel, dim3(pairs), dim3(kPointThreads), 0, stream, a);
	return hipGetLastError();
}

hipError_t launch_homography_solve(const HomographyFindArgs& a, int pairs, hipStream_t stream)
{
	hipLaunchKernelGGL(homography_solve_kernel, dim3((a.tries + kSolveThreads - 1) / kSolveThreads, pairs), dim3(kSolveThreads), 0, stream, a);
	return hipGetLastError();
}

hipError_t launch_homography_score(const HomographyFindArgs& a, int pairs, hipStream_t stream)
{
	hipLaunchKernelGGL(homography_score_kernel, dim3((a.tries + kScoreThreads - 1) / kScoreThreads, pairs), dim3(kScoreThreads), 0, stream, a);
	return hipGetLastError();
}

hipError_t launch_homography_refit(const HomographyFindArgs& a, int pairs, hipStream_t stream)
{
	hipLaunchKernelGGL(homography_refit_kernel, dim3(pairs), dim3(64), 0, stream, a);
	return hipGetLastError();
}

hipError_t launch_homography_project(const HomographyProjectArgs& a, int pairs, hipStream_t stream)
{
	if (!a.n) return hipSuccess;
	hipLaunchKernelGGL(homography_project_kernel, dim3((a.n + 255) / 256, pairs), dim3(256), 0, stream, a);
	return hipGetLastError();
}

} // namespace compvhip
