// orb_kernels.hip -- ORB for gfx950, one pyramid level at a time: the intensity-centroid orientation of CompVCornerDeteORB::processLevelAt
// (core/features/orb/compv_core_feature_orb_dete.cxx:281-358, CompVPatch::moments0110 base/compv_patch.cxx:106-165) and the rotated BRIEF-256/31 of
// CompVCornerDescORB (core/features/orb/compv_core_feature_orb_desc.cxx:206-319, the AVX2 leaf intrin/x86/..._orb_desc_intrin_avx2.cxx:45-128).
// Definition: include/compv_hip.h, docs/kernels/orb.md.
//
//   orb_select_kernel   one workgroup per frame, 256 corners per round: flag (18 pixels from every border) -> rank by ballot prefix and the wave
//                       totals in the LDS -> the survivor's SOURCE INDEX goes to slot rank (the scheme of match_good_kernel); keyCounts[f].
//   orb_orient_kernel   one wave per surviving keypoint: the two halves of the wave walk the disc rows -15..0 and 1..15 (lane = column, a row
//                       is one coalesced read of at most 31 bytes of the RAW plane), a wave reduction gives m10 and m01 (|sum| <= 255 * sum |i|
//                       < 2^21: exact in int32), lane 0 does the binary64 atan2 and writes the record and the optional moments.
//   orb_brief_kernel    one wave per keypoint, four passes: in pass k lane j evaluates test 64 k + j, and __ballot(a < b) IS the k-th
//                       little-endian 64-bit word of the descriptor.  <true>: the 37 x 37 blurred patch is staged in the LDS by coalesced dword
//                       loads (10 dwords cover a row from the dword boundary at or below xi - 18) and the tests read bytes from there;
//                       <false>: the tests read their bytes from global memory.  Lanes 0 and 1 store the row, 16 bytes each.
//   orb_brief_pyramid_kernel   the same wave over the concatenated list of a pyramid: plane, size, stride and scale come from a level table in the
//                       argument block, chosen by the keypoint's own `level`.  orb_select_kernel / orb_orient_kernel take an optional per-frame
//                       offset from device memory (keyBase), so the levels' lists are written one behind the other without a host round trip.
// No atomic anywhere: every slot is decided by a rank, every word by a ballot.
#include "device.hpp"

namespace compvhip {
namespace {

// The rBRIEF pattern of the ORB method (256 tests on a 31 x 31 patch, coordinates -13 .. 12), one dword per test: int8 AX | AY << 8 | BX << 16 | BY << 24.
__device__ const uint32_t kOrbPattern[256] = {
	0x0509fd08u, 0xf4070204u, 0x02f809f5u, 0xf30cf407u, 0x0c02f302u, 0x0601f901u, 0xfcfef6feu, 0xf8f5f3f3u,
	0xf7f4fdf3u, 0x090b040au, 0xf7f8f8f3u, 0x0cf707f5u, 0x060c0707u, 0x00fdfbfcu, 0xfdf402f3u, 0x05f900f7u,
	0xff0cfa0cu, 0x0cfe06fdu, 0xf8fcf3fau, 0xf80cf30bu, 0x01050704u, 0xfd0afd05u, 0x0c06f903u, 0xfefaf9f8u,
	0xf6ff0bfeu, 0x0af80cf3u, 0xfdfb03f9u, 0x07fd02fcu, 0x0bfaf4f6u, 0xf906f405u, 0xff07fa05u, 0xfb040001u,
	0xf30b0b09u, 0x0c040704u, 0x0404ff02u, 0x07fef4fcu, 0xf6f9fbf8u, 0x0c090b04u, 0xf301f800u, 0x02f8fef3u,
	0x03fefefdu, 0xf7fc09fau, 0x070a0c08u, 0x03010900u, 0xf60bfb07u, 0x00f5faf3u, 0x010c070au, 0x0cfafdfau,
	0xfc0cf70au, 0xf4f808f3u, 0xfcf800f3u, 0x08070303u, 0xf90a0705u, 0xf40107ffu, 0x0605f603u, 0xf603fc02u,
	0x05f300f3u, 0x0cf4f9f3u, 0x08f503f3u, 0x07fc0cf9u, 0x080cf606u, 0xfaf9fff7u, 0x0c00fbfeu, 0x05f905f4u,
	0xf308f603u, 0x05fcf9f9u, 0xf9fffefdu, 0xf5050902u, 0xf3fbf3f5u, 0xff0006ffu, 0x0205fd05u, 0x0cfcf3fcu,
	0x06f7faf7u, 0xfcf8f6f4u, 0xfd0c020au, 0x0c0c0c07u, 0x05faf3f9u, 0x04fd09fcu, 0x020cff07u, 0x01fb06f9u,
	0x05f40bf3u, 0xfafe07fdu, 0xf90cf807u, 0xf4f5f9f3u, 0x0c0cfd01u, 0x0003fa02u, 0xf3fe03fcu, 0x0901f3ffu,
	0xfa080107u, 0x0c03ff01u, 0x060c0109u, 0x03fff7ffu, 0x05f6f3f3u, 0x0c0a0707u, 0x090cfb0cu, 0x0b070306u,
	0x0a06f305u, 0x0302f402u, 0xfa040803u, 0xf30c0602u, 0x030af409u, 0x09f904f8u, 0xfafc0cf5u, 0xf8020c01u,
	0xfc07f706u, 0xfe030302u, 0x000b0306u, 0xf808fd03u, 0x03090807u, 0xfcfafbf5u, 0x0afb0bf6u, 0x0cfdf8fbu,
	0x00f705f6u, 0xfa0cff08u, 0xf506fa04u, 0x07f80cf6u, 0x0706fe04u, 0x0cfe00feu, 0x02fbf8fbu, 0x0c0afa07u,
	0xf8f8f3f7u, 0xfefbf3fbu, 0xf309f808u, 0x00f7f5f7u, 0xfe01f801u, 0x0109fc07u, 0xfcff01feu, 0xf50cfa0bu,
	0x04faf7f4u, 0x0c070703u, 0x080a0505u, 0x0802fc00u, 0xf3fb0cf7u, 0x0c020700u, 0x070102ffu, 0xf7070b05u,
	0xf8060503u, 0x09f8fcf3u, 0xfdfd09fbu, 0xf4fdf9fcu, 0x00080506u, 0x0cfa06f9u, 0xfefb06f3u, 0x0a03f601u,
	0xfc080104u, 0xf302fefeu, 0x0c0cf402u, 0xfa00f3feu, 0x03090104u, 0xfbfdf6fau, 0x01fff3fdu, 0xf50c0507u,
	0xf905fe04u, 0xfbf709f3u, 0x06080107u, 0x0607f807u, 0x01f9fcf9u, 0xf8f90bf8u, 0xf8f406f3u, 0x09030402u,
	0x030cfb0au, 0x07fafbfau, 0xf809fd08u, 0x0802f402u, 0x03f6fef5u, 0xf7f9f3f4u, 0xfbf600f5u, 0x080bfd05u,
	0x0cfff3feu, 0x0900f8ffu, 0xfbf4f5f3u, 0x0bf6fef6u, 0xf3fe09fdu, 0x0203fd02u, 0x00fcf3f7u, 0xf6fd06fcu,
	0xf9fe0cfcu, 0x09fcf5fau, 0x0b06fd06u, 0x05fb0bf3u, 0x060c0b0bu, 0xfe0cfb07u, 0x07000cffu, 0xfefdf8fcu,
	0x07fa01f9u, 0xf3f8f4f3u, 0xf8fafef9u, 0xf7fa05f8u, 0x05fcfffbu, 0x0af807f3u, 0xf3050501u, 0xf30a0001u,
	0xff0a0c09u, 0xf70af805u, 0xf3010bffu, 0x02fafdf7u, 0x0c01f6ffu, 0xf6f801f3u, 0xfa0af508u, 0xfa03f302u,
	0xf70cf307u, 0xf9fbf6f6u, 0xf3f8f8f6u, 0x0508fa04u, 0xf3080c03u, 0xfdfd02fcu, 0xf40af305u, 0xff05f304u,
	0x03fc09f7u, 0xf7030300u, 0x01fa01f4u, 0xf8040203u, 0x09f6f6f6u, 0x0c0cf308u, 0xfbfaf4f8u, 0x07030202u,
	0xf80b060au, 0xf4080806u, 0x05fa0af9u, 0x09fdf7fdu, 0x05fff3ffu, 0x04fdf9fdu, 0x03f8fef8u, 0x0c0c0204u,
	0x0b03fb02u, 0xf30bf706u, 0x0c07ff03u, 0x040cff0bu, 0x06fd00fdu, 0x0c04f504u, 0x0102fc02u, 0x01f8faf6u,
	0x01f507f3u, 0xf3f50cf3u, 0xf30b0006u, 0x0401ff00u, 0xfef703f3u, 0xfdfa08f7u, 0xfef8faf3u, 0x0a08f705u,
	0xf7030702u, 0xfffffaffu, 0xfe0b0509u, 0xf80cfd0bu, 0x05030003u, 0x0a0004ffu, 0x0504fa03u, 0x05f600f3u,
	0x0b0c0805u, 0xfa090908u, 0xf408fc07u, 0x09f604f6u, 0x040c0307u, 0xfe0af909u, 0xfe0c0007u, 0xf500faffu,
};

// dX[k] = (int)sqrt(15^2 - k^2), the half width of disc row |j| = k, one nibble each (k = 0 in the lowest)
constexpr unsigned long long kOrbDiscHalfWidths = 0x0579abccddeeeeefull;

constexpr float kOrb180OverPi = 180.f / 3.1415926535897932384626433f;   // base/math/compv_math.cxx:27,31: a float32 quotient
constexpr float kOrbPiOver180 = 3.1415926535897932384626433f / 180.f;   // :30

typedef uint32_t u32x4a4 __attribute__((ext_vector_type(4), aligned(4)));   // a 16-byte store to a dword-aligned row

__device__ __forceinline__ int usedCount(const int32_t* counts, int f, size_t cap)
{
	const int c = counts[f];
	return c < 0 ? 0 : (static_cast<size_t>(c) > cap ? static_cast<int>(cap) : c);
}

__global__ __launch_bounds__(256) void orb_select_kernel(OrbKeyArgs a)
{
	__shared__ int sWave[4];
	const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	const int n = usedCount(a.cornerCounts, f, a.cornerCap);
	const compvhip_corner* __restrict__ in = a.corners + static_cast<size_t>(f) * a.cornerCap;
	int32_t* __restrict__ out = a.index + static_cast<size_t>(f) * a.keyCap;
	const long long before0 = a.keyBase ? a.keyBase[f] : 0;          // records of the pyramid levels before this one
	long long base = 0;
	for (int c0 = 0; c0 < n; c0 += 256) {          // n is workgroup-uniform
		const int c = c0 + tid;
		bool ok = c < n;
		if (ok) {
			const int x = in[c].x, y = in[c].y;
			ok = x >= kOrbBorder && x < a.W - kOrbBorder && y >= kOrbBorder && y < a.H - kOrbBorder;
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
		if (ok && before0 + idx < static_cast<long long>(a.keyCap)) out[idx] = c;
		base += total;
	}
	if (tid == 0) {
		a.keyCounts[f] = static_cast<int32_t>(base);
		if (a.keyTotal) a.keyTotal[f] = static_cast<int32_t>(before0 + base);
	}
}

__global__ __launch_bounds__(256) void orb_orient_kernel(OrbKeyArgs a)
{
	const int f = blockIdx.y, lane = threadIdx.x & 63, q = blockIdx.x * 4 + (threadIdx.x >> 6);
	if (q >= usedCount(a.keyCounts, f, a.keyCap)) return;          // wave-uniform; no barrier in this kernel
	const long long place = (a.keyBase ? a.keyBase[f] : 0) + static_cast<long long>(q);          // behind the levels before
	if (place >= static_cast<long long>(a.keyCap)) return;
	const compvhip_corner c = a.corners[static_cast<size_t>(f) * a.cornerCap + a.index[static_cast<size_t>(f) * a.keyCap + q]];
	const uint8_t* __restrict__ centre = a.gray + static_cast<size_t>(f) * a.frameStride + static_cast<size_t>(c.y) * a.S + c.x;   // 18 pixels inside: orb_select_kernel
	const int half = lane >> 5, col = lane & 31;
	int m10 = 0, m01 = 0;
#pragma unroll
	for (int t = 0; t < 16; ++t) {
		const int j = t - 15 + 16 * half;          // rows -15 .. 0 and 1 .. 16 (16: no row)
		const int dX = static_cast<int>((kOrbDiscHalfWidths >> (4 * (j < 0 ? -j : j))) & 15u);
		if (j <= 15 && col <= 2 * dX) {
			const int i = col - dX;
			const int v = centre[j * a.S + i];
			m10 += i * v; m01 += j * v;
		}
	}
	m10 = wave_sum(m10); m01 = wave_sum(m01);
	if (lane != 0) return;
	const float rad = static_cast<float>(atan2(static_cast<double>(m01), static_cast<double>(m10)));
	float orient = __fmul_rn(rad, kOrb180OverPi);
	if (orient < 0.f) orient = __fadd_rn(orient, 360.f);
	float x = static_cast<float>(c.x), y = static_cast<float>(c.y);
	if (a.level != 0) { const float sfi = 1.f / a.scale; x = __fmul_rn(x, sfi); y = __fmul_rn(y, sfi); }
	compvhip_keypoint k;
	k.x = x; k.y = y; k.strength = static_cast<float>(c.strength); k.orient = orient; k.level = a.level; k.size = 31.f / a.scale;
	const size_t slot = static_cast<size_t>(f) * a.keyCap + static_cast<size_t>(place);
	a.keys[slot] = k;
	if (a.moments) { a.moments[2 * slot] = m01; a.moments[2 * slot + 1] = m10; }
}

constexpr int kPatchSide = 2 * kOrbBorder + 1;   // 37
constexpr int kPatchDwords = 10;                  // a patch row in the LDS: 40 bytes from the dword boundary at or below xi - 18

// The descriptor of one keypoint by one wave (4 waves a workgroup; every wave of the workgroup calls this: the LDS variant has a barrier).  plane: the
// blurred plane of the keypoint's frame and level, W x H, stride S; nullptr = no such plane, a zero row.  have: this wave has a keypoint (*key, row).
template <bool LDS>
__device__ __forceinline__ void brief_wave(const uint8_t* __restrict__ plane, int W, int H, int S, float scale, bool have, const compvhip_keypoint* key, uint8_t* row,
                                           uint32_t* sPatch)
{
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	int xi = 0, yi = 0;
	float fcos = 1.f, fsin = 0.f;
	if (have) {
		const compvhip_keypoint k = *key;
		xi = static_cast<int>(static_cast<double>(__fmul_rn(k.x, scale)) + 0.5);          // :279-288
		yi = static_cast<int>(static_cast<double>(__fmul_rn(k.y, scale)) + 0.5);
		const float rad = __fmul_rn(k.orient, kOrbPiOver180);
		fcos = static_cast<float>(cos(static_cast<double>(rad))); fsin = static_cast<float>(sin(static_cast<double>(rad)));
	}
	// (compared without adding to xi: a caller's record may hold anything)
	const bool inside = have && plane && xi >= kOrbBorder && xi < W - kOrbBorder && yi >= kOrbBorder && yi < H - kOrbBorder;
	const int x0 = (xi - kOrbBorder) & ~3, y0 = yi - kOrbBorder;
	const uint8_t* patch = nullptr;
	if (LDS) {
		uint32_t* sP = sPatch + wave * (kPatchSide * kPatchDwords);
		if (inside) {
			for (int i = lane; i < kPatchSide * kPatchDwords; i += 64) {
				const int r = i / kPatchDwords, d = i - r * kPatchDwords;
				const int x = x0 + 4 * d;          // S % 4 == 0: a dword that starts inside the row ends inside it
				sP[i] = x < S ? *reinterpret_cast<const uint32_t*>(plane + static_cast<size_t>(y0 + r) * S + x) : 0u;
			}
		}
		__syncthreads();
		patch = reinterpret_cast<const uint8_t*>(sP);
	}
	if (!have) return;
	unsigned long long word[4] = { 0ull, 0ull, 0ull, 0ull };
	if (inside) {
#pragma unroll
		for (int k = 0; k < 4; ++k) {
			const uint32_t t = kOrbPattern[64 * k + lane];
			const float ax = static_cast<float>(static_cast<int8_t>(t)), ay = static_cast<float>(static_cast<int8_t>(t >> 8));
			const float bx = static_cast<float>(static_cast<int8_t>(t >> 16)), by = static_cast<float>(static_cast<int8_t>(t >> 24));
			// two products and one sum each, never fused; ties to even
			const int xa = __float2int_rn(__fsub_rn(__fmul_rn(ax, fcos), __fmul_rn(ay, fsin))), ya = __float2int_rn(__fadd_rn(__fmul_rn(ax, fsin), __fmul_rn(ay, fcos)));
			const int xb = __float2int_rn(__fsub_rn(__fmul_rn(bx, fcos), __fmul_rn(by, fsin))), yb = __float2int_rn(__fadd_rn(__fmul_rn(bx, fsin), __fmul_rn(by, fcos)));
			int va, vb;          // |x|, |y| <= 18 (13 * sqrt 2 = 18.38 rounds to 18): inside the patch and, as the point is 18 pixels inside, the plane
			if (LDS) {
				va = patch[(ya + kOrbBorder) * (4 * kPatchDwords) + (xi + xa - x0)];
				vb = patch[(yb + kOrbBorder) * (4 * kPatchDwords) + (xi + xb - x0)];
			}
			else {
				va = plane[static_cast<size_t>(yi + ya) * S + (xi + xa)];
				vb = plane[static_cast<size_t>(yi + yb) * S + (xi + xb)];
			}
			word[k] = __ballot(va < vb);
		}
	}
	if (lane < 2) {
		const unsigned long long lo = word[2 * lane], hi = word[2 * lane + 1];
		u32x4a4 v;
		v.x = static_cast<uint32_t>(lo); v.y = static_cast<uint32_t>(lo >> 32); v.z = static_cast<uint32_t>(hi); v.w = static_cast<uint32_t>(hi >> 32);
		*reinterpret_cast<u32x4a4*>(row + 16 * lane) = v;
	}
}

template <bool LDS>
__global__ __launch_bounds__(256) void orb_brief_kernel(OrbDescArgs a)
{
	__shared__ uint32_t sPatch[LDS ? 4 * kPatchSide * kPatchDwords : 1];
	const int f = blockIdx.y, q = blockIdx.x * 4 + (threadIdx.x >> 6);
	const bool have = q < usedCount(a.keyCounts, f, a.keyCap);          // not a return: the LDS variant has a barrier
	const size_t slot = static_cast<size_t>(f) * a.keyCap + (have ? q : 0);
	brief_wave<LDS>(a.blurred + static_cast<size_t>(f) * a.frameStride, a.W, a.H, a.S, a.scale, have, a.keys + slot, a.desc + slot * a.descStride, sPatch);
}

// The same over the concatenated list of a pyramid: the wave takes plane, size, stride and scale from the level table by its keypoint's `level`
// (wave-uniform, so the table is read with scalar loads).  A level outside the table or without a plane: a zero row.
template <bool LDS>
__global__ __launch_bounds__(256) void orb_brief_pyramid_kernel(OrbPyrDescArgs a)
{
	__shared__ uint32_t sPatch[LDS ? 4 * kPatchSide * kPatchDwords : 1];
	const int f = blockIdx.y, q = blockIdx.x * 4 + (threadIdx.x >> 6);
	const bool have = q < usedCount(a.keyCounts, f, a.keyCap);
	const size_t slot = static_cast<size_t>(f) * a.keyCap + (have ? q : 0);
	const int level = __builtin_amdgcn_readfirstlane(have ? a.keys[slot].level : -1);
	const bool known = level >= 0 && level < a.levels;
	const OrbLevelPlane& L = a.lv[known ? level : 0];
	const uint8_t* plane = known && L.blurred ? L.blurred + static_cast<size_t>(f) * L.frameStride : nullptr;
	brief_wave<LDS>(plane, L.W, L.H, L.S, L.scale, have, a.keys + slot, a.desc + slot * a.descStride, sPatch);
}

// counts of the pyramid's own, [active][frames], into the caller's arrays: one lane per (frame, level)
__global__ __launch_bounds__(256) void orb_pyramid_counts_kernel(OrbPyrCountArgs a)
{
	const int i = blockIdx.x * 256 + threadIdx.x;
	if (i >= a.frames * a.levels) return;
	const int f = i / a.levels, l = i - f * a.levels;
	if (l == 0) a.keyCounts[f] = a.totals[f];
	if (a.levelCounts) a.levelCounts[i] = l < a.active ? a.lvKeys[l * a.frames + f] : 0;
	if (a.levelCorners) a.levelCorners[i] = l < a.active ? a.lvCorners[l * a.frames + f] : 0;
}

} // namespace

hipError_t launch_orb_select(const OrbKeyArgs& a, int frames, hipStream_t stream)
{
	if (frames < 1 || a.W < kPatchSide || a.H < kPatchSide || !a.corners || !a.cornerCounts || !a.keyCounts || (a.keyCap && !a.index)) return hipErrorInvalidValue;
	if (a.cornerCap > static_cast<size_t>(INT32_MAX) || a.keyCap > static_cast<size_t>(INT32_MAX)) return hipErrorInvalidValue;
	hipLaunchKernelGGL(orb_select_kernel, dim3(frames), dim3(256), 0, stream, a);
	return hipGetLastError();
}

hipError_t launch_orb_orient(const OrbKeyArgs& a, int frames, hipStream_t stream)
{
	if (frames < 1 || frames > 65535 || !a.keyCap || a.keyCap > static_cast<size_t>(INT32_MAX) || !a.gray || !a.corners || !a.index || !a.keys || !a.keyCounts || !(a.scale > 0.f))
		return hipErrorInvalidValue;
	hipLaunchKernelGGL(orb_orient_kernel, dim3(static_cast<unsigned>((a.keyCap + 3) / 4), frames), dim3(256), 0, stream, a);
	return hipGetLastError();
}

hipError_t launch_orb_brief(const OrbDescArgs& a, int frames, bool lds, hipStream_t stream)
{
	if (frames < 1 || frames > 65535 || !a.keyCap || a.keyCap > static_cast<size_t>(INT32_MAX) || !a.blurred || !a.keys || !a.keyCounts || !a.desc) return hipErrorInvalidValue;
	if (a.W < kPatchSide || a.H < kPatchSide || a.S < a.W || (a.S & 3) || a.descStride < 32 || (a.descStride & 3)) return hipErrorInvalidValue;
	const dim3 grid(static_cast<unsigned>((a.keyCap + 3) / 4), frames);
	if (lds) hipLaunchKernelGGL(orb_brief_kernel<true>, grid, dim3(256), 0, stream, a);
	else hipLaunchKernelGGL(orb_brief_kernel<false>, grid, dim3(256), 0, stream, a);
	return hipGetLastError();
}

hipError_t launch_orb_brief_pyramid(const OrbPyrDescArgs& a, int frames, bool lds, hipStream_t stream)
{
	if (frames < 1 || frames > 65535 || !a.keyCap || a.keyCap > static_cast<size_t>(INT32_MAX) || !a.keys || !a.keyCounts || !a.desc) return hipErrorInvalidValue;
	if (a.levels < 1 || a.levels > kPyrMaxLevels || a.descStride < 32 || (a.descStride & 3)) return hipErrorInvalidValue;
	for (int l = 0; l < a.levels; ++l) {
		const OrbLevelPlane& L = a.lv[l];
		if (L.blurred && (L.W < kPatchSide || L.H < kPatchSide || L.S < L.W || (L.S & 3) || (L.frameStride & 3) || (reinterpret_cast<uintptr_t>(L.blurred) & 3))) return hipErrorInvalidValue;
	}
	const dim3 grid(static_cast<unsigned>((a.keyCap + 3) / 4), frames);
	if (lds) hipLaunchKernelGGL(orb_brief_pyramid_kernel<true>, grid, dim3(256), 0, stream, a);
	else hipLaunchKernelGGL(orb_brief_pyramid_kernel<false>, grid, dim3(256), 0, stream, a);
	return hipGetLastError();
}

hipError_t launch_orb_pyramid_counts(const OrbPyrCountArgs& a, hipStream_t stream)
{
	if (a.frames < 1 || a.levels < 1 || a.levels > kPyrMaxLevels || a.active < 1 || a.active > a.levels || !a.totals || !a.lvKeys || !a.lvCorners || !a.keyCounts) return hipErrorInvalidValue;
	hipLaunchKernelGGL(orb_pyramid_counts_kernel, dim3((a.frames * a.levels + 255) / 256), dim3(256), 0, stream, a);
	return hipGetLastError();
}

} // namespace compvhip
