// sht_sort_kernels.hip -- the line sort of the device-resident SHT, sized by the lines that exist (gfx950, hand-written HIP).
//
// Replaces the tail of CompVHoughSht::process: std::sort(lines, strength descending) + the maxLines cut, core/features/hough/compv_core_feature_houghsht.cxx:241-249
// (canonical order of the plan API: strength descending, ties in nms_apply's emission order = accumulator (row, col) ascending, :546-562).
//
// Why not the library sort: rocPRIM's device radix sort takes its size from the HOST and costs 35-50 us whatever the size (histogram + two onesweep passes
// + their fills: 0.050 ms for 75 000 keys, 0.076 ms for 1.96 M; tools/microbench/sort_bench) -- at 1080p the sort of 75 000 real keys was 22 % of a step.
// The line keys have structure a general sort cannot use: a strength has at most 13 bits (a cell never exceeds 2 max(W, H)), the emission order inside a frame
// is the wanted tie order, frames are independent.  So the sort is a counting sort on the strength, per frame.  What a line needs for its slot is the number of
// EARLIER lines of the frame with its strength; inside a CHUNK of 8192 consecutive lines that number is counted in order, nothing is sorted or moved, and every
// size is read on the device: the three launches cover the capacity, a chunk without lines returns at once.
//   1. sht_chunk_rank_kernel   one workgroup per chunk: per line, at its own position, its rank among the chunk's lines of equal strength (ordered counting:
//                              wave ballots inside a row of 64 lines, one returning LDS add per group of equal strengths, rows committed in emission order);
//                              the counters left behind are the chunk's strength histogram (u16 [8192], written whole: nothing to clear)
//   2. sht_strength_scan_kernel  one workgroup per frame: lines per strength over the frame's chunks, exclusive scan in descending strength order
//   3. sht_place_lines_kernel  one thread per line: slot = start[strength] + lines of that strength in the frame's earlier chunks + rank; the slot's
//                              compvhip_line is written directly (rho, theta, strength, row, col: what sht_decode_kernel did behind the library sort)
// Larger strengths (max(W, H) > 4095) or line capacities beyond 16 chunks per frame keep the library sort (sht_kernels.hip).
#include "device.hpp"

#include <algorithm>

namespace compvhip {

namespace {

constexpr int kChunk = kShtSortChunk;        // lines per chunk
constexpr int kChunkBits = __builtin_ctz(kChunk);   // bits of a rank inside a chunk, of a position inside a chunk
constexpr int kChunkRows = kChunk / 64;      // rows of 64 consecutive lines, one line per lane
constexpr int kRankWaves = 16;               // waves of a rank workgroup, each owning kChunkRows / kRankWaves consecutive rows
constexpr int kSortThreads = 1024;           // the scan kernel's workgroup: 8 strengths per thread
constexpr int kBins = 1 << kShtSortMaxStrengthBits;   // 8192 strengths
static_assert(kChunk == 1 << kChunkBits && kShtSortMaxStrengthBits + kChunkBits <= 32, "rank word: the inverted strength above the rank");
static_assert(kBins == 8 * kSortThreads, "the scan kernel's thread owns 8 strengths");
static_assert(kChunk < 65536, "a chunk's histogram is u16");
static_assert(kChunkRows % kRankWaves == 0 && kRankWaves <= 16, "whole rows per wave; dense_frame_base's partial sums have 16 slots");

} // namespace

// ---------------------------------------------------------------------------------------------------------------
// rank(i) = number of j < i in the chunk with strength(j) == strength(i), for every line i of the chunk at its own position.
// Row = 64 consecutive lines, one per lane.  Inside a row the lanes of equal strength find each other by one ballot per strength bit; a lane's rank inside the
// row is the number of lower lanes of its group, and the group's first lane adds the group's size to count[strength] in the LDS with ONE returning add: what
// comes back is the number of equal strengths in all earlier rows -- provided the rows are committed in emission order.  (64 lanes adding 1 each in one
// instruction would not do: the order of same-address LDS atomics inside an instruction is not specified, and the order among equal strengths is the product's
// contract.)  A wave commits its own rows in order (LDS operations of a wave are executed in issue order); the waves take turns in wave order, one barrier
// per turn, and every wave has done its ballots -- the bulk of the instructions -- before the first turn.  (One wave per chunk, looping over the rows with
// the next rows' keys in flight and no barrier at all, was twice as slow alone and slower in the two-lane step: docs/kernels/sht_line_stage.md.)
// count[] holds two u16 counters per word, chunkHist's own layout (a chunk has 8192 lines: no carry from the low half; the leaders of strengths 2k and 2k+1
// may add to one word in one instruction in either order, the half a leader reads back is not touched by the other), and only 2^strengthBits of them.
// LDS: 384 B + 2 B per strength = 16.4 KB at 13 strength bits (4K), 8.4 KB at 12 (1080p).  Beside a 4K voting workgroup's 155.6 KB a CU has 4.4 KB left: none
// of these workgroups fits there at 4K or 1080p (8192 counters in 4.4 KB would be 4 bits each), they run on the CUs the vote has left.  On a CU without a voting
// workgroup the wave slots bound them: two workgroups of 16 waves (the sort this replaces: 52 KB, 1024 threads, ~20 barriers).
__global__ __launch_bounds__(kRankWaves * 64) void sht_chunk_rank_kernel(ShtArgs a, ShtSortArgs q)
{
	constexpr int THREADS = kRankWaves * 64, B = kChunkRows / kRankWaves;   // B consecutive rows per wave, all of them kept in registers until the wave's turn
	extern __shared__ __attribute__((aligned(16))) uint32_t s_rank[];
	unsigned long long* s_part = reinterpret_cast<unsigned long long*>(s_rank);   // [16]
	uint32_t* s_idle = s_rank + 32;                                                // [64] a word per lane for the lanes with nothing to add
	uint32_t* s_cnt = s_rank + 96;                                                 // [max(2^strengthBits / 2, 4)]
	const int frame = blockIdx.y, chunk = blockIdx.x, t = threadIdx.x;
	const size_t nf = min((size_t)max(a.lineCounts[frame], 0), a.lineCap);
	const size_t c0 = (size_t)chunk * kChunk;
	if (c0 >= nf) return;   // uniform: a chunk without lines
	const int m = (int)min((size_t)kChunk, nf - c0);
	const int lane = t & 63, wave = t >> 6;
	const int bits = a.strengthBits;
	const uint32_t mask = (1u << bits) - 1u;
	const int words = max((1 << bits) >> 1, 4);
	for (int w = t; w < words; w += THREADS) s_cnt[w] = 0u;
	const size_t base = dense_frame_base<THREADS>(a.lineCounts, frame, a.lineCap, s_part) + c0;   // (its barrier is also the one behind the zeroes)
	const uint32_t* __restrict__ kin = a.lineKeys + base;
	uint32_t* __restrict__ kout = q.rankKeys + base;
	const int row0 = wave * B;

	struct Row { uint32_t inv, rank, size; int first; bool valid; };
	// clamped, unconditional loads, all in flight: a load written under `i < m` is compiled into branch -> load -> s_waitcnt, one memory latency each
	auto load_rows = [&](uint32_t (&k)[B], int r0) {
#pragma unroll
		for (int j = 0; j < B; ++j) k[j] = kin[min((r0 + j) * 64 + lane, m - 1)];
	};
	auto ballot_rows = [&](const uint32_t (&k)[B], int r0, Row (&row)[B]) {
		uint64_t same[B];
#pragma unroll
		for (int j = 0; j < B; ++j) {
			row[j].valid = (r0 + j) * 64 + lane < m;
			row[j].inv = mask - (k[j] & mask);
			same[j] = __ballot(row[j].valid);   // lines past the chunk's end (the highest lanes of its last row) join no group
		}
		for (int b = 0; b < bits; ++b) {
#pragma unroll
			for (int j = 0; j < B; ++j) {
				const bool bit = (row[j].inv >> b) & 1u;
				const uint64_t bal = __ballot(bit);
				same[j] &= bit ? bal : ~bal;
			}
		}
#pragma unroll
		for (int j = 0; j < B; ++j) {
			row[j].rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(same[j] >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)same[j], 0u));
			row[j].size = (uint32_t)__popcll(same[j]);
			row[j].first = __ffsll((unsigned long long)same[j]) - 1;   // (a valid lane is in its own group: never -1)
		}
	};
	// The adds of a wave's rows, in row order and all in flight: every lane adds, so that no add sits behind a branch and a wait of its own -- a group's first
	// lane its group's size to the strength's counter, every other lane nothing to a word of its own.
	auto commit_rows = [&](const Row (&row)[B], uint32_t (&old)[B]) {
#pragma unroll
		for (int j = 0; j < B; ++j) {
			const bool first = row[j].valid && row[j].rank == 0u;
			old[j] = atomicAdd(first ? &s_cnt[row[j].inv >> 1] : &s_idle[lane], first ? row[j].size << ((row[j].inv & 1u) << 4) : 0u);
		}
	};
	auto store_rows = [&](int r0, const Row (&row)[B], const uint32_t (&old)[B]) {
#pragma unroll
		for (int j = 0; j < B; ++j) {
			const uint32_t before = (__shfl(old[j], row[j].first) >> ((row[j].inv & 1u) << 4)) & 0xffffu;   // equal strengths in the earlier rows
			if (row[j].valid) kout[(r0 + j) * 64 + lane] = (row[j].inv << kChunkBits) | (before + row[j].rank);
		}
	};

	uint32_t k[B], old[B];
	Row row[B];
	load_rows(k, row0);
	ballot_rows(k, row0, row);
	const int turns = (m + B * 64 - 1) / (B * 64);   // waves that have lines
	for (int turn = 0; turn < turns; ++turn) {
		if (wave == turn) commit_rows(row, old);
		__syncthreads();
	}
	if (wave < turns) store_rows(row0, row, old);
	// the chunk's histogram, whole: the counters, and zeroes for the strengths this plan cannot have
	uint4* __restrict__ hout = reinterpret_cast<uint4*>(q.chunkHist + ((size_t)frame * q.chunks + chunk) * kBins);
	const uint4* cnt4 = reinterpret_cast<const uint4*>(s_cnt);
	for (int v = t; v < kBins / 8; v += THREADS) hout[v] = 4 * v < words ? cnt4[v] : make_uint4(0u, 0u, 0u, 0u);
}

// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kSortThreads) void sht_strength_scan_kernel(ShtArgs a, ShtSortArgs q)
{
	__shared__ uint32_t s_wave[kSortThreads / 64];
	const int frame = blockIdx.x, t = threadIdx.x;
	const size_t nf = min((size_t)max(a.lineCounts[frame], 0), a.lineCap);
	if (nf == 0) return;
	const int nch = (int)((nf + kChunk - 1) / kChunk);
	// lines per inverted strength 8 t .. 8 t + 7 over the frame's chunks
	uint32_t tot[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
	const uint4* __restrict__ h = reinterpret_cast<const uint4*>(q.chunkHist + (size_t)frame * q.chunks * kBins) + t;
	auto add8 = [](uint32_t (&d)[8], const uint4& v) {
		d[0] += v.x & 0xffffu; d[1] += v.x >> 16; d[2] += v.y & 0xffffu; d[3] += v.y >> 16;
		d[4] += v.z & 0xffffu; d[5] += v.z >> 16; d[6] += v.w & 0xffffu; d[7] += v.w >> 16;
	};
	const uint4 zero4 = make_uint4(0u, 0u, 0u, 0u);
	for (int c0 = 0; c0 < nch; c0 += 4) {   // four chunks' histograms in flight (clamped, unconditional loads)
		uint4 v[4];
#pragma unroll
		for (int u = 0; u < 4; ++u) v[u] = h[(size_t)min(c0 + u, nch - 1) * (kBins / 8)];
#pragma unroll
		for (int u = 0; u < 4; ++u) add8(tot, (c0 + u < nch) ? v[u] : zero4);
	}
	uint32_t sum = 0;
#pragma unroll
	for (int u = 0; u < 8; ++u) { const uint32_t c = tot[u]; tot[u] = sum; sum += c; }   // exclusive inside the thread
	// exclusive scan of the thread sums over the block (ascending inverted strength = descending strength)
	uint32_t incl = sum;
	const int lane = t & 63, wave = t >> 6;
#pragma unroll
	for (int o = 1; o < 64; o <<= 1) {   // wave_incl_scan, written out
		const uint32_t n = __shfl_up(incl, o);
		if (lane >= o) incl += n;
	}
	if (lane == 63) s_wave[wave] = incl;
	__syncthreads();
	uint32_t before = 0;
#pragma unroll
	for (int w = 0; w < kSortThreads / 64; ++w) before += (w < wave) ? s_wave[w] : 0u;
	const uint32_t excl = before + incl - sum;
	uint4* __restrict__ out = reinterpret_cast<uint4*>(q.strengthStart + (size_t)frame * kBins) + 2 * t;
	out[0] = make_uint4(excl + tot[0], excl + tot[1], excl + tot[2], excl + tot[3]);
	out[1] = make_uint4(excl + tot[4], excl + tot[5], excl + tot[6], excl + tot[7]);
}

// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sht_place_lines_kernel(ShtArgs a, ShtSortArgs q, float thetaStep, int maxLines, compvhip_line* __restrict__ lines, size_t outCap)
{
	__shared__ unsigned long long s_part[4];
	const int frame = blockIdx.y;
	const size_t nf = min((size_t)max(a.lineCounts[frame], 0), a.lineCap);
	const size_t i0 = (size_t)blockIdx.x * 256;
	if (i0 >= nf) return;   // uniform
	const size_t base = dense_frame_base<256>(a.lineCounts, frame, a.lineCap, s_part);
	const size_t i = i0 + threadIdx.x;
	if (i >= nf) return;
	size_t limit = nf;      // slots of the frame that are written: min(lines, lineCap, maxLines, outCap)
	if (maxLines > 0 && limit > (size_t)maxLines) limit = (size_t)maxLines;
	if (limit > outCap) limit = outCap;
	const uint32_t kv = q.rankKeys[base + i];
	const uint32_t cell = a.lineVals[base + i];   // emission order: the line was never moved.  Loaded with its rank word, ahead of the cut below: nothing has
	                                              // read the cells since sht_lines_kernel wrote them, and behind the histogram loads the miss cost 1.5 us
	const uint32_t inv = kv >> kChunkBits, rank = kv & (uint32_t)(kChunk - 1);
	const int c = (int)(i >> kChunkBits);
	// slot = first slot of the strength in the frame + its lines in the frame's earlier chunks + rank inside the chunk.  The lines of a wave have unrelated
	// strengths (emission order), so these loads and the store below are gathers and a scatter: 23 us per 32 x 4K launch, 19 while the chunks were sorted.
	// (Per-chunk starts written by the scan kernel instead: 15 MB more traffic from 32 workgroups, 20 + 16 us against 8 + 18 for this loop at 4K with sorted
	// chunks of 4096.)  Four histograms in flight, clamped loads.
	size_t pos = (size_t)q.strengthStart[(size_t)frame * kBins + inv] + rank;
	const uint16_t* __restrict__ h = q.chunkHist + (size_t)frame * q.chunks * kBins + inv;
	for (int c0 = 0; c0 < c; c0 += 4) {
		uint32_t v[4];
#pragma unroll
		for (int u = 0; u < 4; ++u) v[u] = h[(size_t)min(c0 + u, c) * kBins];   // chunk c itself is a valid address (its histogram exists): masked below
#pragma unroll
		for (int u = 0; u < 4; ++u) pos += (c0 + u < c) ? v[u] : 0u;
	}
	if (pos >= limit) return;
	const int row = (int)(cell / (uint32_t)a.T), col = (int)(cell - (uint32_t)row * (uint32_t)a.T);
	compvhip_line o;
	o.rho = (float)(a.barrier - row);            // static_cast<float>(barrier - row), houghsht.cxx:661
	o.theta = __fmul_rn((float)col, thetaStep);  // col * theta (f32), houghsht.cxx:662
	o.strength = (int32_t)(((1u << a.strengthBits) - 1u) - inv);
	o.row = row; o.col = col;
	lines[(size_t)frame * outCap + pos] = o;
}

// ---------------------------------------------------------------------------------------------------------------
hipError_t launch_sht_sort_lines(const ShtArgs& a, const ShtSortArgs& q, int frames, float thetaStep, int maxLines, void* lines, size_t outCap, hipStream_t stream)
{
	if (!lines || !outCap) return hipSuccess;
	const size_t rankLds = 384 + sizeof(uint32_t) * (size_t)std::max((1 << a.strengthBits) >> 1, 4);
	hipLaunchKernelGGL(sht_chunk_rank_kernel, dim3((unsigned)q.chunks, (unsigned)frames), dim3(kRankWaves * 64), rankLds, stream, a, q);
	hipLaunchKernelGGL(sht_strength_scan_kernel, dim3((unsigned)frames), dim3(kSortThreads), 0, stream, a, q);
	hipLaunchKernelGGL(sht_place_lines_kernel, dim3((unsigned)(q.chunks * (kChunk / 256)), (unsigned)frames), dim3(256), 0, stream, a, q, thetaStep, maxLines,
	                   reinterpret_cast<compvhip_line*>(lines), outCap);
	return hipGetLastError();
}

} // namespace compvhip
