// curvefit_kernels.hip -- RANSAC line and parabola fits (CompVMathStatsFit::line / ::parabola, base/math/compv_math_stats_fit.cxx, on
// CompVMathStatsRansac and CompVMathDistance) for gfx950: many point sets at once, from a label map's components to curves without a host trip.  The
// definition is in include/compv_hip.h ("RANSAC curve fitting", items A - G); the arithmetic is curvefit_math.hpp.
//
//   curvefit_gather_kernel    one workgroup per (component, frame): walks the record's box in raster order 256 pixels at a time, ranks the pixels that
//                             carry the id with a block scan and keeps every step-th one as a float64 point.  Its cost grows with the box AREA.
//   curvefit_score_kernel     one lane per try, 256 tries per workgroup: the lane builds its own model (a handful of operations); the set's points are
//                             staged in LDS 256 at a time and read as broadcasts; the inlier count is written per try.
//   curvefit_refit_kernel     one wave per set: selection over the tries by butterfly, the mask of the best try, its inliers compacted in index order
//                             by ballot, the refit's sums with lane l holding partial l of sum64 (a mean pass, then a moment pass), the closed-form
//                             solve, the record.
//   curvefit_distance_kernel  one lane per point: item C alone.
// The RANSAC skeleton (clamped count, fold of sum64, selection, compaction, staged walk) is ransac_device.hpp's, shared with homography_kernels.hip.
// No MFMA; every store is a plain C++ store.
#include "ransac_device.hpp"
#include "curvefit_math.hpp"

namespace compvhip {
namespace {

using namespace cf;

constexpr int kThreads = kCurvefitBlock;

__global__ __launch_bounds__(kThreads) void curvefit_gather_kernel(CurvefitGatherArgs a)
{
	__shared__ int32_t s_flag[kThreads];
	const int s = blockIdx.x, tid = threadIdx.x;
	const int f = s / a.compCap, c = s - f * a.compCap;
	const int count = min(max(a.compCounts[f], 0), a.compCap);
	int kept = 0;
	if (c < count) {          // (the whole workgroup: c and count are the set's)
		const compvhip_component rec = a.comps[(size_t)f * a.compCap + c];
		const int id = c + 1;
		const int x0 = max(rec.x0, 0), y0 = max(rec.y0, 0), x1 = min(rec.x1, a.W - 1), y1 = min(rec.y1, a.H - 1);
		if (rec.pixels > 0 && x0 <= x1 && y0 <= y1) {
			const int step = (int)(((long long)rec.pixels + a.pointCap - 1) / a.pointCap);
			const int bw = x1 - x0 + 1;
			const long long area = (long long)bw * (y1 - y0 + 1);
			const int32_t* labels = a.labels + (size_t)f * a.H * a.labelStride;
			double2* out = a.points + (size_t)s * a.pointCap;
			long long rank = 0;
			for (long long base = 0; base < area; base += kThreads) {
				const long long i = base + tid;
				int x = 0, y = 0;
				bool on = false;
				if (i < area) {
					y = y0 + (int)(i / bw); x = x0 + (int)(i % bw);
					on = labels[(size_t)y * a.labelStride + x] == id;
				}
				s_flag[tid] = on ? 1 : 0;
				const int32_t total = block_excl_scan<kThreads>(s_flag, s_flag, kThreads);
				if (on) {
					const long long r = rank + s_flag[tid];
					if (r % step == 0 && r / step < a.pointCap) out[r / step] = make_double2((double)x, (double)y);
				}
				rank += total;
				__syncthreads();          // s_flag is written again in the next round
			}
			kept = (int)min((rank + step - 1) / step, (long long)a.pointCap);
		}
	}
	if (tid == 0) a.counts[s] = kept;
}

// the model of try t of set s among its k > m points: false when the sample leaves [0, k) or the model is rejected
__device__ __forceinline__ bool tryCurve(const CurvefitFindArgs& a, int s, int t, int k, const double2* pts, Curve* c)
{
	const int m = modelPoints(a.model);
	int32_t q[3];
	if (a.samples) {
		const int32_t* in = a.samples + ((size_t)s * a.tries + t) * m;
		q[0] = in[0]; q[1] = in[1]; q[2] = m == 3 ? in[2] : 0;
	}
	else sample(a.model, a.seed, (uint32_t)s, (uint32_t)t, (uint32_t)k, q);
	if (!((uint32_t)q[0] < (uint32_t)k && (uint32_t)q[1] < (uint32_t)k && (uint32_t)q[2] < (uint32_t)k)) return false;
	double px[3], py[3];
#pragma unroll
	for (int i = 0; i < 3; ++i) { const double2 v = pts[q[i]]; px[i] = v.x; py[i] = v.y; }
	return curveOf(a.model, px, py, c);
}

__global__ __launch_bounds__(kThreads) void curvefit_score_kernel(CurvefitFindArgs a)
{
	__shared__ double2 s_pts[kThreads];
	const int tid = threadIdx.x, s = blockIdx.y;
	const int t = blockIdx.x * kThreads + tid;
	const int k = ransac_count(a.counts, s, a.pointCap);
	if (k <= modelPoints(a.model)) return;          // (the whole workgroup: k is the set's) no try runs on such a set
	const double2* pts = a.points + (size_t)s * a.pointCap;
	Curve c = { 0.0, 0.0, 0.0 };
	bool live = false;
	if (t < a.tries) {
		live = tryCurve(a, s, t, k, pts, &c);
		if (live) c = prepared(a.model, c);
	}
	int count = 0;
	staged_points<kThreads>(k, tid, live, [&](int slot, int i) { s_pts[slot] = pts[i]; },
	                        [&](int j) { count += residual(a.model, c, s_pts[j].x, s_pts[j].y) < a.threshold ? 1 : 0; });
	if (t < a.tries) a.scoreCount[(size_t)s * a.maxTries + t] = count;
}

__device__ __forceinline__ void writeRecord(compvhip_curvefit_result* out, Curve c, int inliers, int bestTry, int status, int k)
{
	out->A = c.A; out->B = c.B; out->C = c.C;
	out->inliers = inliers; out->bestTry = bestTry; out->status = status; out->k = k;
}

__global__ __launch_bounds__(64) void curvefit_refit_kernel(CurvefitFindArgs a)
{
	const int lane = threadIdx.x, s = blockIdx.x;
	const int k = ransac_count(a.counts, s, a.pointCap);
	const int model = a.model, m = modelPoints(model);
	compvhip_curvefit_result* out = a.results + s;
	const double2* pts = a.points + (size_t)s * a.pointCap;
	uint8_t* mask = a.mask ? a.mask + (size_t)s * a.pointCap : nullptr;
	const Curve zero = { 0.0, 0.0, 0.0 };
	if (k <= m) {          // k < m: status 2; k == m: the points themselves are the sample -- no generator, no refit
		Curve c = zero;
		bool ok = false;
		if (k == m) {
			double px[3] = { 0.0, 0.0, 0.0 }, py[3] = { 0.0, 0.0, 0.0 };
			for (int i = 0; i < m; ++i) { const double2 v = pts[i]; px[i] = v.x; py[i] = v.y; }
			ok = curveOf(model, px, py, &c);
		}
		if (mask && lane < k) mask[lane] = ok ? 1 : 0;
		if (lane == 0) writeRecord(out, ok ? c : zero, ok ? m : 0, ok ? 0 : -1, ok ? 0 : (k == m ? 1 : 2), k);
		return;
	}
	// D. selection
	const BestTry<ransac::NoVariance> best = wave_best_try<ransac::NoVariance>(m, a.tries, lane, [&](int t, int* count, ransac::NoVariance*) { *count = a.scoreCount[(size_t)s * a.maxTries + t]; });
	const int bt = best.tryIdx;
	if (best.count < m) {
		if (mask) for (int i = lane; i < k; i += 64) mask[i] = 0;
		if (lane == 0) writeRecord(out, zero, 0, -1, 1, k);
		return;
	}
	// the inliers of the best try, compacted in index order
	Curve own = zero;
	(void)tryCurve(a, s, bt, k, pts, &own);          // (it scored: the sample is in range and the model is not rejected)
	const Curve p = prepared(model, own);
	double2* sel = a.sel + (size_t)s * a.pointCap;
	double2 v = make_double2(0.0, 0.0);
	const int n = wave_compact_inliers(k, lane, mask, [&](int i) { v = pts[i]; return residual(model, p, v.x, v.y) < a.threshold; }, [&](int o) { sel[o] = v; });
	__syncthreads();          // one wave: the compacted points are visible to every lane
	// E. refit
	Curve fit = zero;
	bool ok;
	if (n == m) {
		double px[3] = { 0.0, 0.0, 0.0 }, py[3] = { 0.0, 0.0, 0.0 };
		for (int i = 0; i < m; ++i) { const double2 v = sel[i]; px[i] = v.x; py[i] = v.y; }
		ok = curveOf(model, px, py, &fit);
	}
	else if (model == kLine) {
		double sx = 0.0, sy = 0.0;
		for (int i = lane; i < n; i += 64) { const double2 v = sel[i]; sx += v.x; sy += v.y; }
		const double meanX = meanOf(wave_fold64(sx), n), meanY = meanOf(wave_fold64(sy), n);
		double sab = 0.0, sden = 0.0;
		for (int i = lane; i < n; i += 64) {
			const double2 v = sel[i];
			double ab, den;
			lineTerms(v.x, v.y, meanX, meanY, &ab, &den);
			sab += ab; sden += den;
		}
		fit = lineFromSums(meanX, meanY, wave_fold64(sab), wave_fold64(sden));
		ok = true;
	}
	else {
		double su = 0.0;
		for (int i = lane; i < n; i += 64) { const double2 v = sel[i]; su += xOf(model, v.x, v.y); }
		const double mean = meanOf(wave_fold64(su), n);
		double acc[7] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 };
		for (int i = lane; i < n; i += 64) {
			const double2 v = sel[i];
			double t[7];
			parabolaTerms(xOf(model, v.x, v.y), yOf(model, v.x, v.y), mean, t);
#pragma unroll
			for (int e = 0; e < 7; ++e) acc[e] += t[e];
		}
#pragma unroll
		for (int e = 0; e < 7; ++e) acc[e] = wave_fold64(acc[e]);
		ok = parabolaFromSums(n, mean, acc, &fit);
	}
	if (lane == 0) writeRecord(out, ok ? fit : own, n, bt, ok ? 0 : 3, k);
}

__global__ __launch_bounds__(256) void curvefit_distance_kernel(CurvefitDistanceArgs a)
{
	const int i = blockIdx.x * 256 + threadIdx.x, s = blockIdx.y;
	if (i >= ransac_count(a.counts, s, a.pointCap)) return;
	const double* in = a.params + (size_t)s * 3;
	Curve c;
	c.A = in[0]; c.B = in[1]; c.C = in[2];
	const double2 v = a.points[(size_t)s * a.pointCap + i];
	a.out[(size_t)s * a.pointCap + i] = residual(a.model, prepared(a.model, c), v.x, v.y);
}

} // namespace

hipError_t launch_curvefit_gather(const CurvefitGatherArgs& a, int sets, hipStream_t stream)
{
	hipLaunchKernelGGL(curvefit_gather_kernel, dim3(sets), dim3(kThreads), 0, stream, a);
	return hipGetLastError();
}

hipError_t launch_curvefit_score(const CurvefitFindArgs& a, int sets, hipStream_t stream)
{
	hipLaunchKernelGGL(curvefit_score_kernel, dim3((a.tries + kThreads - 1) / kThreads, sets), dim3(kThreads), 0, stream, a);
	return hipGetLastError();
}

hipError_t launch_curvefit_refit(const CurvefitFindArgs& a, int sets, hipStream_t stream)
{
	hipLaunchKernelGGL(curvefit_refit_kernel, dim3(sets), dim3(64), 0, stream, a);
	return hipGetLastError();
}

hipError_t launch_curvefit_distances(const CurvefitDistanceArgs& a, int sets, hipStream_t stream)
{
	hipLaunchKernelGGL(curvefit_distance_kernel, dim3((a.pointCap + 255) / 256, sets), dim3(256), 0, stream, a);
	return hipGetLastError();
}

} // namespace compvhip
