// device.hpp -- the device primitives the kernel files share (gfx950, wave64): wave reductions and scans, the per-frame block scan, the dense key
// array's frame offset, byte lanes through the packed 16-bit ALU, one-instruction asm wrappers, the XCD-aware tile placement and the line
// count / edge probe of the line-band walks.  Header-only, everything __device__ __forceinline__.
#pragma once
#include "kernels.hpp"

namespace compvhip {

// ---- wave reductions and scans ---------------------------------------------------------------------------------------------------------
// xor butterflies: every lane gets the result
template <typename T>
__device__ __forceinline__ T wave_sum(T v)
{
#pragma unroll
	for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
	return v;
}
template <typename T>
__device__ __forceinline__ T wave_min(T v)
{
#pragma unroll
	for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o));
	return v;
}
template <typename T>
__device__ __forceinline__ T wave_max(T v)
{
#pragma unroll
	for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o));
	return v;
}
// inclusive prefix sum over the wave; lane = threadIdx.x & 63.  The wave's total is __shfl(result, 63).
template <typename T>
__device__ __forceinline__ T wave_incl_scan(T x, int lane)
{
#pragma unroll
	for (int o = 1; o < 64; o <<= 1) {
		const T y = __shfl_up(x, o);
		if (lane >= o) x += y;
	}
	return x;
}

// The same for uint32 on the vector ALU alone: six v_add_u32 with a DPP operand (row_shr 1, 2, 4, 8 inside the rows of 16 lanes, then row_bcast:15 into
// rows 1 and 3 and row_bcast:31 into rows 2 and 3), no trip through the LDS crossbar.  All 64 lanes must be active.  The total is readlane(result, 63).
template <int CTRL, int ROWS>
__device__ __forceinline__ uint32_t dpp_or_zero(uint32_t v)          // the value of the lane CTRL names; 0 for a lane without a source or in a row outside ROWS
{
	return static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(v), CTRL, ROWS, 0xf, false));
}
__device__ __forceinline__ uint32_t wave_incl_scan_dpp(uint32_t x)
{
	x += dpp_or_zero<0x111, 0xf>(x);          // row_shr:1
	x += dpp_or_zero<0x112, 0xf>(x);          // row_shr:2
	x += dpp_or_zero<0x114, 0xf>(x);          // row_shr:4
	x += dpp_or_zero<0x118, 0xf>(x);          // row_shr:8
	x += dpp_or_zero<0x142, 0xa>(x);          // row_bcast:15
	x += dpp_or_zero<0x143, 0xc>(x);          // row_bcast:31
	return x;
}

// Exclusive prefix sum of src[0 .. n) into dst[0 .. n) by one workgroup of THREADS threads (all of them call it); src may be dst.  n > THREADS goes in
// rounds, the total of the earlier rounds carried in a register.  Every thread gets the total.
template <int THREADS>
__device__ __forceinline__ int32_t block_excl_scan(const int32_t* src, int32_t* dst, int n)
{
	__shared__ int32_t waveSum[THREADS / 64];
	const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
	int32_t carry = 0;
	for (int b = 0; b < n; b += THREADS) {
		const int i = b + tid;
		const int32_t x = i < n ? src[i] : 0;
		const int32_t incl = wave_incl_scan(x, lane);
		if (lane == 63) waveSum[wv] = incl;
		__syncthreads();
		int32_t before = 0, round = 0;
#pragma unroll
		for (int k = 0; k < THREADS / 64; ++k) {
			const int32_t s = waveSum[k];
			before += k < wv ? s : 0;
			round += s;
		}
		if (i < n) dst[i] = carry + before + incl - x;
		carry += round;
		__syncthreads();   // waveSum is written again in the next round
	}
	return carry;
}

// lines of the earlier frames (clamped to lineCap): where frame `frame` starts in the dense key array.  Every thread of the block gets the sum.
template <int THREADS>
__device__ __forceinline__ size_t dense_frame_base(const int* __restrict__ counts, int frame, size_t lineCap, unsigned long long* s_part)
{
	unsigned long long before = 0;
	for (int g = threadIdx.x; g < frame; g += THREADS) {
		const size_t cg = (size_t)max(counts[g], 0);
		before += cg < lineCap ? cg : lineCap;
	}
#pragma unroll
	for (int d = 32; d > 0; d >>= 1) before += __shfl_xor(before, d);   // wave_sum, written out
	if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = before;
	__syncthreads();
	unsigned long long sum = 0;
#pragma unroll
	for (int w = 0; w < THREADS / 64; ++w) sum += s_part[w];
	return (size_t)sum;
}

// ---- byte lanes through the packed 16-bit ALU ----------------------------------------------------------------------------------------
// The ISA has no byte-wise min / max.  A dword of four pixels is split once into its even and odd bytes, each zero-extended to a 16-bit
// half (E = b0 | b2 << 16, O = b1 | b3 << 16); v_pk_min_u16 / v_pk_max_u16 then work on two pixels per instruction.
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
constexpr uint32_t kLo = 0x00ff00ffu;

__device__ __forceinline__ uint32_t pk_min_u16(uint32_t a, uint32_t b)
{
	return __builtin_bit_cast(uint32_t, __builtin_elementwise_min(__builtin_bit_cast(u16x2, a), __builtin_bit_cast(u16x2, b)));
}
__device__ __forceinline__ uint32_t pk_max_u16(uint32_t a, uint32_t b)
{
	return __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(u16x2, a), __builtin_bit_cast(u16x2, b)));
}
// rows of a tile are stored only for columns < W: whole dwords where they fit, single bytes at the ragged end
__device__ __forceinline__ void storeRow4(uint8_t* dst, int gx, int W, uint32_t v)
{
	if (gx + 4 <= W) *reinterpret_cast<uint32_t*>(dst + gx) = v;
	else for (int b = 0; b < 4 && gx + b < W; ++b) dst[gx + b] = static_cast<uint8_t>(v >> (8 * b));
}

// ---- three-operand forms, one instruction each (the constants ride in SGPRs: VOP3 takes no literal on gfx9) ----------------------------
// (v_pk_max_u16 as an instruction the optimiser does not look into, for the gradient kernels whose schedule was tuned around it; pk_max_u16 elsewhere)
__device__ __forceinline__ uint32_t v_pk_max_u16(uint32_t a, uint32_t b) { uint32_t d; asm("v_pk_max_u16 %0, %1, %2" : "=v"(d) : "v"(a), "v"(b)); return d; }
// (a << SHIFT) + b.  The shift is spelled in the instruction text, one specialisation per shift in use: as an "n" operand it changed the register
// allocation of the edge-detector kernels.
template <int SHIFT> __device__ __forceinline__ uint32_t lshl_add(uint32_t a, uint32_t b);
#define COMPVHIP_LSHL_ADD(N) \
	template <> __device__ __forceinline__ uint32_t lshl_add<N>(uint32_t a, uint32_t b) { uint32_t d; asm("v_lshl_add_u32 %0, %1, " #N ", %2" : "=v"(d) : "v"(a), "v"(b)); return d; }
COMPVHIP_LSHL_ADD(1)
COMPVHIP_LSHL_ADD(3)
#undef COMPVHIP_LSHL_ADD
__device__ __forceinline__ uint32_t xad(uint32_t a, uint32_t sk, uint32_t c) { uint32_t d; asm("v_xad_u32 %0, %1, %2, %3" : "=v"(d) : "v"(a), "s"(sk), "v"(c)); return d; }   // (a ^ k) + c
__device__ __forceinline__ uint32_t add3(uint32_t a, uint32_t b, uint32_t sk) { uint32_t d; asm("v_add3_u32 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "s"(sk)); return d; }

// ---- XCD-aware tile mapping --------------------------------------------------------------------------------------------------------------
// Workgroup b is observed to run on XCD b % 8, each XCD with a private L2.  Horizontally adjacent
// tiles share their 4-byte column halos (one extra 128-byte line each side per row), so all tilesX tiles of one "row group"
// (same frame, same block-row) are given to the SAME XCD, consecutively: the halo lines then hit in that XCD's L2 instead
// of being fetched from the fabric twice.  A pure performance remap: any placement is correct.
// grid = 8 * ceil(groups/8) * tilesX workgroups (1-D); returns false for padding workgroups.
__device__ __forceinline__ bool xcd_tile_map(int b, int tilesX, int groups, int& tileX, int& group)
{
	const int xcd = b & 7;
	const int k = b >> 3;             // index of this workgroup inside its XCD's queue
	group = (k / tilesX) * 8 + xcd;
	tileX = k - (k / tilesX) * tilesX;
	return group < groups;
}

// ---- the line-band walks (sht_segments_kernels.hip, sht_fit_kernels.hip) -------------------------------------------------------------
// lines of frame f that are considered
__device__ __forceinline__ int line_count(const ShtLineSetArgs& a, int f) { return min(max(a.lineCounts[f], 0), a.nLines); }

// is pixel (x, y) of the frame an edge
template <bool BITS>
__device__ __forceinline__ bool line_edge(const ShtLineSetArgs& a, size_t frameBase, int x, int y)
{
	if (BITS) return (a.ebits[frameBase + (size_t)y * a.wb + (x >> 5)] >> (x & 31)) & 1u;
	return a.edges[frameBase + (size_t)y * a.S + x] != 0;
}

} // namespace compvhip
