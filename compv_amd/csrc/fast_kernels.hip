// fast_kernels.hip -- FAST corner detection on u8 planes: scores, non-maximum suppression, raster-ordered corner lists (definition in
// include/compv_hip.h and docs/kernels/fast.md).
//
// Replaces, behind compvhip_fast_u8 / compvhip_plan_fast:
//   CompVCornerDeteFAST::process      core/features/fast/compv_core_feature_fast_dete.cxx:163-422
//   CompVFastDataRow_C                :658-771 (ring :221-238; the early exits :679-688, :729, :748 are necessary conditions only)
//   CompVFastNmsGather_C / Apply_C    :773-831
//   CompVFastBuildInterestPoints      :490-585 (strength = score + t - 1)
//   CompVInterestPoint::selectBest    base/include/compv/base/compv_common.h:641-656 -- as the canonical cut: every corner at or above the
//                                     maxFeatures-th largest strength
//
// For a pixel I with b = min(255, I + t), d = max(0, I - t) and ring pixels p_0 .. p_15 (clockwise from the top):
//   D_k = max(0, d - p_k), B_k = max(0, p_k - b);  score = max over the 16 arcs of N consecutive k of min(D_k over the arc), and of min(B_k).
// Integer arithmetic only.  Frames are a grid dimension (blockIdx.z); frame bases are 8-byte aligned (compvhip_plan_fast and the pyramid refuse
// anything else before they enqueue) and S % 8 == 0 (plan contract), so every
// row starts on a dword.  Columns >= W are read (they only ever feed pixels within 3 of the right edge, whose score is 0 by definition) and
// never written.
//
// Stages of one call (all on the caller's stream; no atomic decides where a record goes):
//   fast_score_kernel   tile + halo in the LDS -> scores of the tile and of the 1-pixel ring around it -> NMS -> score map, corners per row
//                       (integer atomic adds: a sum), strength histogram when a cut was asked for
//   fast_cut_kernel     per frame: the score of the maxFeatures-th strongest corner            } only with maxFeatures > 1
//   fast_rows_kernel<0> per row: corners at or above that score                                }
//   fast_scan_kernel    per frame: exclusive scan of the row counts, the frame's count
//   fast_rows_kernel<1> per row with corners: walk the score map row in x order, write the records at their final index
#include "device.hpp"

namespace compvhip {

namespace {

// Byte lanes through the packed 16-bit ALU (device.hpp).  Sums and differences of the 16-bit halves stay within 16 bits here (<= 510, >= 0), so
// plain 32-bit add / sub serve.
// 0xff in the low byte of every half that is not zero (halves <= 255)
__device__ __forceinline__ uint32_t nzMask(uint32_t h) { return (((h + kLo) >> 8) & 0x00010001u) * 0xffu; }

// ---- tile geometry ---------------------------------------------------------------------------------------------------------------------------
// One workgroup = one 128 x 32 tile of the output.  Scores are needed for the tile and the 1-pixel ring around it (NMS), in whole dwords: 34 rows
// of 34 dword groups (columns tx0 - 4 .. tx0 + 132).  Their rings reach 3 further: the raw plane holds 40 rows of 36 dwords (columns tx0 - 8 ..
// tx0 + 136).  Both pitches are odd numbers of dwords.
constexpr int kTW = 128, kTH = 32;
constexpr int kScoreRows = kTH + 2, kScoreGroups = kTW / 4 + 2, kScorePitch = kScoreGroups + 1;          // 34, 34, 35
constexpr int kRawRows = kTH + 8, kRawWords = kTW / 4 + 4, kRawPitch = kRawWords + 1;                     // 40, 36, 37

// the four pixels `dx` columns from those of word `w` of an LDS row (dx is a constant after unrolling)
__device__ __forceinline__ uint32_t shifted4(const uint32_t* row, int w, int dx)
{
	const int q = dx >> 2, s = dx & 3;          // floor division: dx = -3 -> word -1, byte 1
	const uint32_t lo = row[w + q];
	return s ? __builtin_amdgcn_alignbyte(row[w + q + 1], lo, static_cast<uint32_t>(s)) : lo;
}

// max over the 16 arcs of N consecutive ring positions of the arc's minimum, for two pixels at once
template <int N>
__device__ __forceinline__ uint32_t arcMax(const uint32_t (&v)[16])
{
	uint32_t m2[16], m4[16], m8[16];
#pragma unroll
	for (int k = 0; k < 16; ++k) m2[k] = pk_min_u16(v[k], v[(k + 1) & 15]);
#pragma unroll
	for (int k = 0; k < 16; ++k) m4[k] = pk_min_u16(m2[k], m2[(k + 2) & 15]);
#pragma unroll
	for (int k = 0; k < 16; ++k) m8[k] = pk_min_u16(m4[k], m4[(k + 4) & 15]);
	uint32_t best = 0;
#pragma unroll
	for (int k = 0; k < 16; ++k) best = pk_max_u16(best, pk_min_u16(m8[k], N == 9 ? v[(k + 8) & 15] : m4[(k + 8) & 15]));   // positions k .. k + 8 / k .. k + 11
	return best;
}

// scores of the four pixels of word `w` of raw row `r` (no interior test: the caller zeroes what lies outside)
template <int N>
__device__ __forceinline__ uint32_t score4(const uint32_t* sRaw, int r, int w, uint32_t t2)
{
	constexpr int kDx[16] = { 0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1 };
	constexpr int kDy[16] = { -3, -3, -2, -1, 0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3 };
	const uint32_t c = sRaw[r * kRawPitch + w];
	const uint32_t cE = c & kLo, cO = (c >> 8) & kLo;
	const uint32_t bE = pk_min_u16(cE + t2, kLo), bO = pk_min_u16(cO + t2, kLo);          // min(255, I + t)
	const uint32_t dE = pk_max_u16(cE, t2) - t2, dO = pk_max_u16(cO, t2) - t2;            // max(0, I - t)
	uint32_t DE[16], DO[16], BE[16], BO[16];
	auto ring = [&](int k) {
		const uint32_t p = shifted4(sRaw + (r + kDy[k]) * kRawPitch, w, kDx[k]);
		const uint32_t pE = p & kLo, pO = (p >> 8) & kLo;
		DE[k] = dE - pk_min_u16(pE, dE); DO[k] = dO - pk_min_u16(pO, dO);                 // max(0, d - p)
		BE[k] = pk_max_u16(pE, bE) - bE; BO[k] = pk_max_u16(pO, bO) - bO;                 // max(0, p - b)
	};
	// An arc of 9 or more holds one position of every opposite pair: no darker (brighter) pixel in {0, 8} or in {4, 12} rules a darker (brighter) arc
	// out.  Most pixels of a natural image end here.
	ring(0); ring(8); ring(4); ring(12);
	const uint32_t maybe = pk_min_u16(pk_max_u16(DE[0], DE[8]), pk_max_u16(DE[4], DE[12])) | pk_min_u16(pk_max_u16(DO[0], DO[8]), pk_max_u16(DO[4], DO[12])) |
	                       pk_min_u16(pk_max_u16(BE[0], BE[8]), pk_max_u16(BE[4], BE[12])) | pk_min_u16(pk_max_u16(BO[0], BO[8]), pk_max_u16(BO[4], BO[12]));
	if (!maybe) return 0u;
#pragma unroll
	for (int k = 0; k < 16; ++k) if (k & 3) ring(k);
	const uint32_t e = pk_max_u16(arcMax<N>(DE), arcMax<N>(BE)), o = pk_max_u16(arcMax<N>(DO), arcMax<N>(BO));
	return e | (o << 8);
}

template <int N, bool NMS>
__global__ __launch_bounds__(256) void fast_score_kernel(FastArgs a)
{
	__shared__ uint32_t sRaw[kRawRows * kRawPitch];
	__shared__ uint32_t sScore[kScoreRows * kScorePitch];
	__shared__ int sHist[256];
	const int tid = threadIdx.x, frame = blockIdx.z;
	const int tx0 = blockIdx.x * kTW, ty0 = blockIdx.y * kTH;
	const uint8_t* __restrict__ src = a.in + static_cast<size_t>(frame) * a.frameStride;
	sHist[tid] = 0;
	// tile + halo, dword by dword; outside the plane: 0 (only pixels whose score is 0 by definition see those cells)
	for (int i = tid; i < kRawRows * kRawWords; i += 256) {
		const int row = i / kRawWords, w = i - row * kRawWords;
		const int y = ty0 - 4 + row, x = tx0 - 8 + 4 * w;
		uint32_t v = 0;
		if (y >= 0 && y < a.H && x >= 0 && x < a.S) v = *reinterpret_cast<const uint32_t*>(src + static_cast<size_t>(y) * a.S + x);
		sRaw[row * kRawPitch + w] = v;
	}
	__syncthreads();
	// scores: without NMS the tile's own 32 x 32 groups, with it the ring of groups around them as well
	const uint32_t t2 = static_cast<uint32_t>(a.t) * 0x00010001u;
	constexpr int kLo0 = NMS ? 0 : 1, kSpan = NMS ? kScoreGroups : kTW / 4, kRowsN = NMS ? kScoreRows : kTH;
	for (int i = tid; i < kRowsN * kSpan; i += 256) {
		const int sr = i / kSpan + kLo0, sg = i - (i / kSpan) * kSpan + kLo0;
		const int gy = ty0 - 1 + sr, gx = tx0 - 4 + 4 * sg;
		uint32_t s = 0;
		if (gy >= 3 && gy < a.H - 3 && gx + 3 >= 3 && gx < a.W - 3) {
			s = score4<N>(sRaw, sr + 3, sg + 1, t2);
			if (gx < 3 || gx + 3 >= a.W - 3) {          // the interior's first and last group: pixels outside 3 <= x < W - 3 score 0
				uint32_t m = 0;
				for (int b = 0; b < 4; ++b) if (gx + b >= 3 && gx + b < a.W - 3) m |= 0xffu << (8 * b);
				s &= m;
			}
		}
		sScore[sr * kScorePitch + sg] = s;
	}
	__syncthreads();
	// NMS, score map, survivors per row: a thread owns one dword group of four rows; the 32 groups of a tile row are one half of a wave
	const int g = tid & 31;
	uint8_t* __restrict__ dst = a.scores + static_cast<size_t>(frame) * a.frameStride;
	for (int r = tid >> 5; r < kTH; r += 8) {
		const uint32_t* row = sScore + (r + 1) * kScorePitch;
		uint32_t s = row[g + 1];
		if (NMS && s) {
			// largest of the 8 neighbours, then keep where s > it: a neighbour >= s suppresses, so two equal neighbours both go
			uint32_t mE = 0, mO = 0;
			auto add = [&](uint32_t w) { mE = pk_max_u16(mE, w & kLo); mO = pk_max_u16(mO, (w >> 8) & kLo); };
			add(shifted4(row - kScorePitch, g + 1, -1)); add(row[g + 1 - kScorePitch]); add(shifted4(row - kScorePitch, g + 1, 1));
			add(shifted4(row, g + 1, -1)); add(shifted4(row, g + 1, 1));
			add(shifted4(row + kScorePitch, g + 1, -1)); add(row[g + 1 + kScorePitch]); add(shifted4(row + kScorePitch, g + 1, 1));
			const uint32_t sE = s & kLo, sO = (s >> 8) & kLo;
			s &= nzMask(pk_max_u16(sE, mE) - mE) | (nzMask(pk_max_u16(sO, mO) - mO) << 8);
		}
		const int gy = ty0 + r, gx = tx0 + 4 * g;
		if (gy < a.H) storeRow4(dst + static_cast<size_t>(gy) * a.S, gx, a.W, s);
		int n = __popc((nzMask(s & kLo) | (nzMask((s >> 8) & kLo) << 8)) & 0x01010101u);
		if (a.hist && n) {
			for (int b = 0; b < 4; ++b) {
				const uint32_t v = (s >> (8 * b)) & 0xffu;
				if (v) atomicAdd(&sHist[v], 1);
			}
		}
		for (int d = 16; d; d >>= 1) n += __shfl_xor(n, d);          // stays inside the half wave (wave_sum over 32 lanes)
		if (g == 0 && n) atomicAdd(a.rowCounts + static_cast<size_t>(frame) * a.H + gy, n);          // n > 0 implies gy < H: rows outside the plane score 0
	}
	if (a.hist) {
		__syncthreads();
		if (sHist[tid]) atomicAdd(a.hist + frame * 256 + tid, sHist[tid]);
	}
}

// per frame: minScore = the score of the maxFeatures-th strongest corner when the frame has more than maxFeatures corners, else 1 (every corner)
__global__ __launch_bounds__(256) void fast_cut_kernel(FastArgs a)
{
	__shared__ int sHist[256];
	const int frame = blockIdx.x;
	sHist[threadIdx.x] = a.hist[frame * 256 + threadIdx.x];
	__syncthreads();
	if (threadIdx.x) return;
	int level = 1, seen = 0;
	for (int s = 255; s >= 1; --s) {
		seen += sHist[s];
		if (seen >= a.maxFeatures) { level = s; break; }
	}
	a.minScore[frame] = level;
}

// per frame: exclusive scan of the row counts -> row offsets; the total -> counts[frame]
// (Its own algorithm, not block_excl_scan: a thread sums its share of the rows, one scan round over the 256 sums.  block_excl_scan's nine rounds
// for 2160 rows measured 3.5 us slower per launch, docs/experiments.md.)
__global__ __launch_bounds__(256) void fast_scan_kernel(FastArgs a)
{
	__shared__ int sPart[256];
	const int frame = blockIdx.x, tid = threadIdx.x;
	const int* __restrict__ rc = a.rowCounts + static_cast<size_t>(frame) * a.H;
	int* __restrict__ ro = a.rowOffsets + static_cast<size_t>(frame) * a.H;
	const int per = (a.H + 255) / 256, y0 = tid * per, y1 = min(y0 + per, a.H);
	int sum = 0;
	for (int y = y0; y < y1; ++y) sum += rc[y];
	sPart[tid] = sum;
	__syncthreads();
	for (int d = 1; d < 256; d <<= 1) {          // inclusive scan of the 256 partial sums
		const int v = tid >= d ? sPart[tid - d] : 0;
		__syncthreads();
		sPart[tid] += v;
		__syncthreads();
	}
	int run = sPart[tid] - sum;
	for (int y = y0; y < y1; ++y) { ro[y] = run; run += rc[y]; }
	if (tid == 255) a.counts[frame] = sPart[255];
}

// One wave per row, in x order.  EMIT = false: recount the row against the frame's cut level.  EMIT = true: write the row's records at
// rowOffsets[y] + their rank within the row, up to cornerCap.  Rows without corners end at once, so only rows that hold corners are read.
template <bool EMIT>
__global__ __launch_bounds__(256) void fast_rows_kernel(FastArgs a)
{
	const int lane = threadIdx.x & 63, y = blockIdx.x * 4 + (threadIdx.x >> 6), frame = blockIdx.z;
	if (y >= a.H) return;
	int* rowCount = a.rowCounts + static_cast<size_t>(frame) * a.H + y;
	const int want = *rowCount;
	const int level = a.minScore ? a.minScore[frame] : 1;
	if (!want || (!EMIT && level <= 1)) return;
	long long base = 0;
	if (EMIT) {
		base = a.rowOffsets[static_cast<size_t>(frame) * a.H + y];
		if (base >= static_cast<long long>(a.cornerCap)) return;
	}
	const uint8_t* __restrict__ row = a.scores + static_cast<size_t>(frame) * a.frameStride + static_cast<size_t>(y) * a.S;
	compvhip_corner* __restrict__ out = a.corners + static_cast<size_t>(frame) * a.cornerCap;
	int found = 0;
	for (int x0 = 0; x0 < a.W; x0 += 512) {          // 64 lanes x 8 pixels; x + 8 <= S because S % 8 == 0
		const int x = x0 + 8 * lane;
		uint32_t w[2] = { 0u, 0u };
		if (x < a.W) { const uint2 v = *reinterpret_cast<const uint2*>(row + x); w[0] = v.x; w[1] = v.y; }
		int n = 0;
		uint32_t keep = 0;          // bit b: pixel x + b is a corner of the list
		for (int b = 0; b < 8; ++b) {
			const int v = (w[b >> 2] >> (8 * (b & 3))) & 0xff;
			if (x + b < a.W && v >= level) { keep |= 1u << b; ++n; }          // level >= 1: zero scores never pass
		}
		int incl = n;          // inclusive prefix sum over the wave (wave_incl_scan, written out)
		for (int d = 1; d < 64; d <<= 1) {
			const int v = __shfl_up(incl, d);
			if (lane >= d) incl += v;
		}
		const int total = __shfl(incl, 63);
		if (EMIT && n) {
			long long idx = base + found + incl - n;
			for (int b = 0; b < 8; ++b) {
				if (!(keep >> b & 1u)) continue;
				if (idx < static_cast<long long>(a.cornerCap)) {
					compvhip_corner c;
					c.x = x + b; c.y = y; c.strength = static_cast<int>((w[b >> 2] >> (8 * (b & 3))) & 0xff) + a.t - 1;
					out[idx] = c;
				}
				++idx;
			}
		}
		found += total;
		if (EMIT && found >= want) break;          // the row's corners are out (wave-uniform)
	}
	if (!EMIT && lane == 0) *rowCount = found;
}

} // namespace

hipError_t launch_fast(const FastArgs& a, int frames, int stage, hipStream_t stream)
{
	if (a.W < 7 || a.H < 7 || (a.N != 9 && a.N != 12) || a.t < 0 || a.t > 255 || (a.S & 7) || a.S < a.W || frames < 1) return hipErrorInvalidValue;
	if (!a.in || !a.scores || !a.rowCounts || !a.rowOffsets || !a.counts || (a.cornerCap && !a.corners)) return hipErrorInvalidValue;
	const bool cut = a.maxFeatures > 1;
	if (cut && (!a.hist || !a.minScore)) return hipErrorInvalidValue;
	FastArgs k = a;
	if (!cut) { k.hist = nullptr; k.minScore = nullptr; }
	const dim3 block(256);
	if (stage == 0) {
		const dim3 grid((a.W + kTW - 1) / kTW, (a.H + kTH - 1) / kTH, frames);
		if (a.N == 9) {
			if (a.nonmax) hipLaunchKernelGGL((fast_score_kernel<9, true>), grid, block, 0, stream, k);
			else hipLaunchKernelGGL((fast_score_kernel<9, false>), grid, block, 0, stream, k);
		}
		else {
			if (a.nonmax) hipLaunchKernelGGL((fast_score_kernel<12, true>), grid, block, 0, stream, k);
			else hipLaunchKernelGGL((fast_score_kernel<12, false>), grid, block, 0, stream, k);
		}
		return hipGetLastError();
	}
	const dim3 rows((a.H + 3) / 4, 1, frames);
	if (cut) {
		hipLaunchKernelGGL(fast_cut_kernel, dim3(frames), block, 0, stream, k);
		hipLaunchKernelGGL((fast_rows_kernel<false>), rows, block, 0, stream, k);
	}
	hipLaunchKernelGGL(fast_scan_kernel, dim3(frames), block, 0, stream, k);
	if (a.cornerCap) hipLaunchKernelGGL((fast_rows_kernel<true>), rows, block, 0, stream, k);
	return hipGetLastError();
}

} // namespace compvhip
