// sht_fit_kernels.hip -- Hough line REFINEMENT: a total-least-squares fit through the edge pixels in a band of rho cells around an SHT line
// (compvhip_plan_houghsht_fit, compvhip_houghsht_fit_u8; definition in docs/kernels/sht_fit.md and include/compv_hip.h).
//
// The band of a line (row, col) with half width b holds exactly the edge pixels that voted for the cells (row - b .. row + b, col):
//   | ((x * cosQ[col] + y * sinQ[col]) >> 16) - (barrier - row) | <= b      -- the vote's own expression, evaluated here as an int64 predicate:
//   0 <= x * cosQ + y * sinQ - (rho_i - b) * 65536 < (2 b + 1) * 65536.
//
// Shape: ONE WAVE PER RECORD (a line, or a segment of a line: the same band cut to a range of positions), four waves per workgroup, no LDS,
// nothing between the waves.  The 64 lanes take 64 consecutive positions p of the line's major axis (the walk of sht_segments_kernels.hip).
// Per position the minor coordinates of the band are an interval; its ends come from two f64 floor divisions (of the band's two bounds by the
// minor coefficient, |cm| >= 46340), widened by one on each side, and EVERY candidate in it is tested with the predicate -- cosQ is negative past
// 90 degrees and >> floors, so the predicate decides and the divisions only say where to look (<= 28 candidates at b = 8, <= 25 of them inside).
//
// Edge reads: on a y-major line the candidates of a position are adjacent bits of ONE mask row -- the one or two words that hold them are read
// once into a 64-bit window.  On an x-major line they sit in up to 25 different rows at the same column: one word (or byte) per candidate, but
// the 64 lanes of the wave read neighbouring columns of the same rows, i.e. two or three mask words (one or two 64-byte runs of bytes) per row.
//
// Sums: a position's partial sums (count, sum m, sum m^2 over <= 25 minor coordinates below 8192) fit int32; a lane keeps its six moments in
// int64; the wave adds them with a 64-bit xor butterfly (__shfl_xor on long long: two ds_bpermute_b32 per step, 72 for the record -- against
// the walk's loads that is noise, so no DPP form was written).  Lane 0 computes the central moments in int64 and the closed-form 2 x 2 eigen
// step in binary64 -- + - * / sqrt only, every operation rounded once (-ffp-contract=off), in the order of the definition -- and writes the
// 80-byte record.  One record per line or segment at a known index: no atomics, no second pass, no scan.
#include "device.hpp"
#include "frame_slices.hpp"

namespace compvhip {

namespace {

constexpr int kFitWaves = 4;      // waves (= records) per workgroup; the waves never synchronise
static_assert(sizeof(compvhip_line_fit) == 80, "compvhip_line_fit has no padding");

template <bool BITS>
__global__ __launch_bounds__(kFitWaves * 64) void sht_fit_kernel(ShtFitArgs a)
{
	const int lane = threadIdx.x & 63;
	const int ri = blockIdx.x * kFitWaves + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
	const int f = a.frame0 + blockIdx.y;
	const int nl = min(max(a.lineCounts[f], 0), a.nLines);   // line_count, written out
	const int nRec = a.segs ? (int)min((size_t)max(a.segCounts[f], 0), a.segCap) : nl;
	if (ri == 0 && lane == 0) a.fitCounts[f] = nRec;
	if (ri >= nRec) return;
	if ((size_t)ri >= a.fitCap && !a.refined) return;

	int li = ri, r0 = 0, r1 = 0x7fffffff;     // the line of the record; its range of positions
	int sx0 = 0, sy0 = 0, sx1 = 0, sy1 = 0;
	if (a.segs) {
		const compvhip_segment* sg = a.segs + (size_t)f * a.segCap + ri;
		li = __builtin_amdgcn_readfirstlane(sg->line);
		sx0 = __builtin_amdgcn_readfirstlane(sg->x0); sy0 = __builtin_amdgcn_readfirstlane(sg->y0);
		sx1 = __builtin_amdgcn_readfirstlane(sg->x1); sy1 = __builtin_amdgcn_readfirstlane(sg->y1);
	}
	// a segment whose line is not one of the lines considered, or a line that is not an accumulator cell, has an empty band (the host entry
	// point refuses both before it gets here)
	bool ok = li >= 0 && li < nl;
	int row = 0, col = 0;
	const compvhip_line* ln = a.lines + (size_t)f * a.lineCap + (ok ? li : 0);
	if (ok) {
		row = __builtin_amdgcn_readfirstlane(ln->row); col = __builtin_amdgcn_readfirstlane(ln->col);
		ok = row >= 0 && row < a.R && col >= 0 && col < a.T;
	}

	long long n = 0, sp = 0, sm = 0, spp = 0, spm = 0, smm = 0;   // moments over (position, minor coordinate)
	bool xMajor = true;
	if (ok) {
		const int sq = a.sinQ[col], cq = a.cosQ[col];
		xMajor = sq >= abs(cq);
		const int N = xMajor ? a.W : a.H, Nm = xMajor ? a.H : a.W;      // positions / minor coordinates
		const long long cp = xMajor ? cq : sq, cm = xMajor ? sq : cq;   // coefficient of the position / of the minor coordinate (|cm| >= 46340)
		const long long lo = (long long)(a.barrier - row - a.halfWidth) * 65536;   // band: 0 <= p * cp + m * cm - lo < span
		const long long span = (long long)(2 * a.halfWidth + 1) * 65536;
		const double den = (double)cm;
		const size_t frameBase = (size_t)f * (BITS ? a.bitsFrameStride : a.edgeFrameStride);
		if (a.segs) { r0 = xMajor ? sx0 : sy0; r1 = xMajor ? sx1 : sy1; }
		const int pa = max(r0, 0), pb = min(r1, N - 1);
		for (int b0 = pa & ~63; b0 <= pb; b0 += 64) {
			const int p = b0 + lane;
			if (p < pa || p > pb) continue;
			const long long base = (long long)p * cp;
			const long long Alo = lo - base;                            // band: Alo <= m * cm < Alo + span
			const int e0 = (int)floor((double)Alo / den), e1 = (int)floor((double)(Alo + span) / den);
			const int mlo = max(min(e0, e1) - 1, 0), mhi = min(max(e0, e1) + 1, Nm - 1);
			if (mlo > mhi) continue;
			long long d = (long long)mlo * cm - Alo;
			int np = 0, s1 = 0, s2 = 0;
			if (BITS && !xMajor) {
				// adjacent bits of one mask row: mhi - mlo <= 30, so the window starting at bit (mlo & 31) of word mlo >> 5 ends inside the next word
				const uint32_t* rw = a.ebits + frameBase + (size_t)p * a.wb;
				const int w = mlo >> 5;
				unsigned long long win = rw[w];
				if ((mhi >> 5) != w) win |= (unsigned long long)rw[w + 1] << 32;
				win >>= (mlo & 31);
				for (int m = mlo; m <= mhi; ++m, d += cm, win >>= 1)
					if ((unsigned long long)d < (unsigned long long)span && (win & 1ull)) { ++np; s1 += m; s2 += m * m; }
			}
			else {
				for (int m = mlo; m <= mhi; ++m, d += cm) {
					if ((unsigned long long)d >= (unsigned long long)span) continue;
					bool e;      // line_edge<BITS>, written out: with BITS only x-major lines get here
					if (BITS) e = (a.ebits[frameBase + (size_t)m * a.wb + (p >> 5)] >> (p & 31)) & 1u;      // x-major: pixel (p, m)
					else e = (xMajor ? a.edges[frameBase + (size_t)m * a.S + p] : a.edges[frameBase + (size_t)p * a.S + m]) != 0;
					if (e) { ++np; s1 += m; s2 += m * m; }
				}
			}
			n += np; sp += (long long)p * np; sm += s1;
			spp += (long long)p * p * np; spm += (long long)p * s1; smm += s2;
		}
	}
	n = wave_sum(n); sp = wave_sum(sp); sm = wave_sum(sm); spp = wave_sum(spp); spm = wave_sum(spm); smm = wave_sum(smm);
	if (lane != 0) return;

	compvhip_line_fit r;
	r.line = li; r.pixels = (int)n;
	r.sx = xMajor ? sp : sm; r.sy = xMajor ? sm : sp;
	r.sxx = xMajor ? spp : smm; r.sxy = spm; r.syy = xMajor ? smm : spp;
	// central moments, exact: |A|, |B|, |C| <= n^2 * 8191^2 < 2^63 for max(W, H) <= 8192 (n <= 25 * 8192)
	const long long A = n * r.sxx - r.sx * r.sx, B = n * r.sxy - r.sx * r.sy, C = n * r.syy - r.sy * r.sy;
	const double ad = (double)A, bd = (double)B, cd = (double)C;
	const double d = ad - cd;
	const double s = sqrt(d * d + 4.0 * (bd * bd));
	const bool valid = n >= 2 && s != 0.0;
	r.nx = r.ny = r.rho = r.rms2 = 0.0;
	if (valid) {
		// the eigenvector of the smaller eigenvalue of [[A, B], [B, C]], from the row that does not cancel
		double u, v;
		if (d >= 0.0) { u = -(2.0 * bd); v = d + s; }
		else { u = s - d; v = -(2.0 * bd); }
		const double h = sqrt(u * u + v * v);
		double nx = u / h, ny = v / h;
		if (ny < 0.0 || (ny == 0.0 && nx < 0.0)) { nx = -nx; ny = -ny; }
		const double nd = (double)n;
		const double t = (ad + cd) - s;
		r.nx = nx; r.ny = ny;
		r.rho = (nx * (double)r.sx + ny * (double)r.sy) / nd;
		r.rms2 = (t > 0.0 ? t : 0.0) / (2.0 * nd * nd);
	}
	if ((size_t)ri < a.fitCap) a.fits[(size_t)f * a.fitCap + ri] = r;
	if (a.refined) {     // per-line mode only: li == ri < nl, so ln is the record's line
		compvhip_line o = *ln;
		if (valid) { o.rho = (float)r.rho; o.theta = (float)atan2(r.ny, r.nx); o.strength = r.pixels; }
		a.refined[(size_t)f * a.lineCap + ri] = o;
	}
}

} // namespace

hipError_t launch_sht_fit(const ShtFitArgs& args, int frames, hipStream_t stream)
{
	const size_t recs = args.segs ? args.segCap : (size_t)args.nLines;
	const dim3 grid((unsigned)((recs + kFitWaves - 1) / kFitWaves > 0 ? (recs + kFitWaves - 1) / kFitWaves : 1), 1);
	// the frame index rides in blockIdx.y
	return for_frame_slices(frames, [&](int f0, int nf) {
		ShtFitArgs a = args;
		a.frame0 = f0;
		const dim3 g(grid.x, (unsigned)nf);
		if (a.edges) hipLaunchKernelGGL(sht_fit_kernel<false>, g, dim3(kFitWaves * 64), 0, stream, a);
		else hipLaunchKernelGGL(sht_fit_kernel<true>, g, dim3(kFitWaves * 64), 0, stream, a);
		return hipGetLastError();
	});
}

} // namespace compvhip
