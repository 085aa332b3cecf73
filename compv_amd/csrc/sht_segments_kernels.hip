// sht_segments_kernels.hip -- Hough line SEGMENTS: where along an SHT line its edge pixels are (compvhip_plan_houghsht_segments,
// compvhip_houghsht_segments_u8; definition in docs/kernels/sht_segments.md and include/compv_hip.h).
//
// The pixels of a line are exactly the edge pixels that voted for its accumulator cell (row, col):
//   (x * cosQ[col] + y * sinQ[col]) >> 16 == barrier - row        -- the vote's own expression, evaluated here as a predicate.
// The vote kernel works on image tiles with per-tile int32 constants computed in int64 on the host (api.cpp voteGridTables), i.e. it is
// the exact floor of the exact sum for every geometry the plan accepts (W, H <= 32767, where the sum needs 33 bits): the predicate below is
// evaluated in int64 for every geometry, so it cannot disagree with the accumulator.
//
// Shape: ONE WAVE PER (frame, line).  The 64 lanes take 64 consecutive positions p of the line's major axis (x when sinQ >= |cosQ|, y
// otherwise); a lane tests the <= 4 candidate minor coordinates est - 1 .. est + 2 (est = floor of the exact inverse, one f64 division: the
// quotient of two integers below 2^53 whose distance from an integer is 0 or >= 1 / 65535 floors exactly) and reads the edge bit / byte of the <= 2
// that satisfy the predicate and lie inside the image.  __ballot gives the 64-bit occupancy word of the chunk (and a second word: positions with two
// support edges); splitting the on-positions into groups whose gaps are <= maxGap is wave-uniform bit arithmetic on that word (ctz over its runs of
// ones) with four carried scalars -- run open, run start, last on-position, run support -- from chunk to chunk.  A 4K line is 64 chunks.
//
// Placement is count -> scan -> write (deterministic also when segCap clips): the walk runs twice, once counting the segments of every
// line, once writing them at the exclusive prefix sum of the counts of the frame's earlier lines (sht_segments_scan_kernel, one
// workgroup per frame).  A line may hold max(W, H) / 2 segments, so they cannot wait in registers or the LDS between the phases; the second walk
// skips the lines that start at or beyond segCap.
//
// Memory: an x-major line reads 64 nearly consecutive bits of one or two mask rows per chunk (one or two 128-byte lines for the whole wave).  A
// y-major line reads one mask word (or byte) per ROW per lane: 64 different cache lines per chunk for 64 bits of payload, the worst case of the
// kernel and what bounds it on frames whose lines are mostly vertical.  Neither a transposed copy of the masks (an extra pass over every
// frame for the few hundred lines that use it) nor an LDS-staged band (a y-major line is one pixel wide: staging does not create reuse inside
// one wave) was tried; lines of neighbouring waves share those cache lines in the L2 when they are close in rho.
#include "device.hpp"
#include "frame_slices.hpp"

namespace compvhip {

namespace {

constexpr int kSegWaves = 4;      // waves (= lines) per workgroup; the waves never synchronise
constexpr int kScanThreads = 1024;

// WRITE = false: perLine[frame][line] = number of segments of the line.  WRITE = true: perLine holds the exclusive prefix sums; the segments
// are written at perLine[frame][line] + k while that is below segCap.
template <bool BITS, bool WRITE>
__global__ __launch_bounds__(kSegWaves * 64) void sht_segments_kernel(ShtSegArgs a)
{
	const int lane = threadIdx.x & 63;
	const int li = blockIdx.x * kSegWaves + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
	const int f = a.frame0 + blockIdx.y;
	if (li >= a.nLines) return;
	if (li >= line_count(a, f)) return;
	int32_t* slot = a.perLine + (size_t)f * a.nLines + li;
	const compvhip_line* ln = a.lines + (size_t)f * a.lineCap + li;
	const int row = __builtin_amdgcn_readfirstlane(ln->row), col = __builtin_amdgcn_readfirstlane(ln->col);
	if (row < 0 || row >= a.R || col < 0 || col >= a.T) {   // not an accumulator cell (the host entry point refuses such lines before it gets here)
		if (!WRITE && lane == 0) *slot = 0;
		return;
	}
	int base = 0;
	if (WRITE) {
		base = __builtin_amdgcn_readfirstlane(*slot);
		if ((size_t)base >= a.segCap) return;
	}
	const int sq = a.sinQ[col], cq = a.cosQ[col];
	const bool xMajor = sq >= abs(cq);
	const int N = xMajor ? a.W : a.H, Nm = xMajor ? a.H : a.W;      // positions / minor coordinates
	const long long cp = xMajor ? cq : sq, cm = xMajor ? sq : cq;   // coefficient of the position / of the minor coordinate (|cm| >= 46340)
	const long long rhoQ = (long long)(a.barrier - row) * 65536;
	const double invDen = (double)cm;
	const size_t frameBase = (size_t)f * (BITS ? a.bitsFrameStride : a.edgeFrameStride);
	compvhip_segment* out = a.segs + (size_t)f * a.segCap;

	// the open run (wave-uniform): [p0, last], its support so far, the minor coordinates of its first pixel and of the pixel at `last`
	bool open = false;
	int p0 = 0, last = 0, sup = 0, nseg = 0;
	int p0m = 0, lastM = 0;
	auto closeRun = [&](int p1m) {
		if (last - p0 + 1 >= a.minLength) {
			if (WRITE) {
				const size_t idx = (size_t)base + nseg;
				if (idx < a.segCap && lane == 0) {
					compvhip_segment s;
					s.line = li;
					s.x0 = xMajor ? p0 : p0m; s.y0 = xMajor ? p0m : p0;
					s.x1 = xMajor ? last : p1m; s.y1 = xMajor ? p1m : last;
					s.support = sup;
					out[idx] = s;
				}
			}
			++nseg;
		}
	};

	for (int b = 0; b < N; b += 64) {
		const int p = b + lane;
		int cnt = 0, mf = 0;
		if (p < N) {
			const long long A = rhoQ - (long long)p * cp;           // support: 0 <= m * cm - A < 65536
			const int est = (int)floor((double)A / invDen);
			long long d = (long long)(est - 1) * cm - A;
#pragma unroll
			for (int k = 0; k < 4; ++k, d += cm) {
				const int m = est - 1 + k;
				if ((unsigned long long)d < 65536ull && (unsigned)m < (unsigned)Nm) {
					if (xMajor ? line_edge<BITS>(a, frameBase, p, m) : line_edge<BITS>(a, frameBase, m, p)) {
						if (!cnt) mf = m;
						++cnt;
					}
				}
			}
		}
		const unsigned long long on = __ballot(cnt > 0), two = __ballot(cnt > 1);
		unsigned long long w = on;
		while (w) {
			const int first = __builtin_ctzll(w);
			const unsigned long long inv = ~(w >> first);
			const int len = inv ? __builtin_ctzll(inv) : 64;        // the run of ones that starts at `first`
			const unsigned long long m = (len == 64 ? ~0ull : ((1ull << len) - 1ull)) << first;
			const int pos = b + first;
			if (open && pos - last - 1 > a.maxGap) {
				closeRun(last >= b ? __shfl(mf, last - b) : lastM);
				open = false;
			}
			if (!open) { open = true; p0 = pos; sup = 0; p0m = __shfl(mf, first); }
			sup += len + __popcll(two & m);
			last = pos + len - 1;
			w &= ~m;
		}
		if (open && last >= b) lastM = __shfl(mf, last - b);
	}
	if (open) closeRun(lastM);
	if (!WRITE && lane == 0) *slot = nseg;
}

// exclusive prefix sum of a frame's per-line segment counts, in place; segCounts[frame] = their total
__global__ __launch_bounds__(kScanThreads) void sht_segments_scan_kernel(ShtSegArgs a)
{
	const int f = a.frame0 + blockIdx.x;
	int32_t* v = a.perLine + (size_t)f * a.nLines;
	const int32_t total = block_excl_scan<kScanThreads>(v, v, line_count(a, f));
	if (threadIdx.x == 0) a.segCounts[f] = total;
}

template <bool WRITE>
void launch_walk(const ShtSegArgs& a, int frames, hipStream_t stream)
{
	const dim3 grid((unsigned)((a.nLines + kSegWaves - 1) / kSegWaves), (unsigned)frames);
	if (a.edges) hipLaunchKernelGGL((sht_segments_kernel<false, WRITE>), grid, dim3(kSegWaves * 64), 0, stream, a);
	else hipLaunchKernelGGL((sht_segments_kernel<true, WRITE>), grid, dim3(kSegWaves * 64), 0, stream, a);
}

} // namespace

hipError_t launch_sht_segments(const ShtSegArgs& args, int frames, int phase, hipStream_t stream)
{
	// the frame index rides in blockIdx.y
	return for_frame_slices(frames, [&](int f0, int nf) {
		ShtSegArgs a = args;
		a.frame0 = f0;
		if (phase == 1) {
			hipLaunchKernelGGL(sht_segments_scan_kernel, dim3((unsigned)nf), dim3(kScanThreads), 0, stream, a);
		}
		else if (a.nLines > 0) {
			if (phase == 0) launch_walk<false>(a, nf, stream); else launch_walk<true>(a, nf, stream);
		}
		return hipGetLastError();
	});
}

} // namespace compvhip
