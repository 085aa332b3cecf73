// morph_kernels.hip -- global / adaptive thresholding and mathematical morphology on u8 planes: the step between a gray frame and the
// connected components of its text blobs (definitions in include/compv_hip.h and docs/kernels/morph.md).
//
// Replaces, behind compvhip_threshold_u8 / compvhip_threshold_adaptive_u8 / compvhip_morph_u8 and their plan twins:
//   CompVImageThreshold::global      base/image/compv_image_threshold.cxx:118-180 (entry), 320-347 (leaf: in > t ? 0xff : 0)
//   CompVImageThreshold::adaptive    base/image/compv_image_threshold.cxx:183-317 (mean kernel, hz + vt fixed-point passes, 768-entry LUT)
//   CompVMathMorph::process          base/math/compv_math_morph.cxx:95-123 (ops), 125-247 (basicOper), 542-674 (borders), 676-692 (leaf)
//
// Integer arithmetic only.  Frames are a grid dimension (blockIdx.z); S % 8 == 0 (plan contract), so every row starts a whole number of
// 8-byte groups behind the frame base.  The base itself may sit at any byte (include/compv_hip.h: ANY BYTE): every access to the caller's
// planes is a per-lane global load or store of 4 or 8 bytes at base + a multiple of its size, which the hardware takes at any address and
// which stays inside the frame span; nothing rounds an address down, and no atomic touches a plane
// (tests/test_gpu_pointer_alignment.py runs every kernel of this file off alignment).  Columns >= W are read (they only ever feed
// border cells, whose value does not depend on them) and never written.
#include "device.hpp"
#include "frame_slices.hpp"

namespace compvhip {

// byte lanes through the packed 16-bit ALU (device.hpp)
template <bool MAX>
__device__ __forceinline__ uint32_t pk(uint32_t a, uint32_t b) { return MAX ? pk_max_u16(a, b) : pk_min_u16(a, b); }
template <bool MAX>
struct Acc {   // running min / max of four pixels in split form
	uint32_t e = MAX ? 0u : kLo, o = MAX ? 0u : kLo;
	__device__ __forceinline__ void add(uint32_t w) { e = pk<MAX>(e, w & kLo); o = pk<MAX>(o, (w >> 8) & kLo); }
	__device__ __forceinline__ uint32_t packed() const { return e | (o << 8); }
};

// ---- global threshold ----------------------------------------------------------------------------------------------------------------
// one thread = 8 adjacent pixels of one row.  x > t per 16-bit half: (x + (255 - t)) carries into bit 8 exactly when x > t.
__global__ __launch_bounds__(256) void threshold_kernel(ThreshArgs a)
{
	const int groups = (a.W + 7) >> 3;
	const int idx = blockIdx.x * 256 + threadIdx.x, frame = blockIdx.z;
	if (idx >= groups * a.H) return;
	const int y = idx / groups, x0 = (idx - y * groups) * 8;
	int t = a.t8;
	if (a.levels) t = min(max(a.levels[frame], 0), 255);
	const uint32_t k = static_cast<uint32_t>(255 - t) * 0x00010001u;
	const size_t off = static_cast<size_t>(frame) * a.frameStride + static_cast<size_t>(y) * a.S + x0;
	const uint2 v = *reinterpret_cast<const uint2*>(a.in + off);
	auto bin = [k](uint32_t w) {
		const uint32_t e = (((w & kLo) + k) >> 8) & 0x00010001u, o = ((((w >> 8) & kLo) + k) >> 8) & 0x00010001u;
		return (e * 0xffu) | ((o * 0xffu) << 8);
	};
	const uint2 q = make_uint2(bin(v.x), bin(v.y));
	uint8_t* row = a.out + static_cast<size_t>(frame) * a.frameStride + static_cast<size_t>(y) * a.S;
	if (x0 + 8 <= a.W) *reinterpret_cast<uint2*>(row + x0) = q;
	else { storeRow4(row, x0, a.W, q.x); storeRow4(row, x0 + 4, a.W, q.y); }
}

hipError_t launch_threshold(const ThreshArgs& args, int frames, hipStream_t stream)
{
	const int groups = (args.W + 7) >> 3;
	const long long total = static_cast<long long>(groups) * args.H;
	if ((total + 255) / 256 > INT32_MAX) return hipErrorInvalidValue;
	// the frame index rides in blockIdx.z: a slice starts at its own frame's planes and level
	return for_frame_slices(frames, [&](int f0, int nf) {
		ThreshArgs a = args;
		a.in += static_cast<size_t>(f0) * a.frameStride; a.out += static_cast<size_t>(f0) * a.frameStride;
		if (a.levels) a.levels += f0;
		hipLaunchKernelGGL(threshold_kernel, dim3(static_cast<unsigned>((total + 255) / 256), 1, nf), dim3(256), 0, stream, a);
		return hipGetLastError();
	});
}

// ---- adaptive threshold ---------------------------------------------------------------------------------------------------------------
// All taps of the mean kernel are equal, so a tap's (p * k) >> 16 depends on the pixel alone: a pass is a sliding-window SUM of that per-pixel
// value, saturated once.  One workgroup = one 128 x 32 tile: the tile and its halo (blockSize / 2 <= 15 either side) go to the LDS once, as raw
// bytes and as tap values; the horizontal sums run along the rows (one lane per row: the row pitch is an odd number of banks), the vertical
// ones down the columns, and the comparison with the raw pixel follows in the same thread.  The mean never reaches memory.
constexpr int kAdTW = 128, kAdTH = 32, kAdHalo = 16;
constexpr int kAdRows = kAdTH + 2 * 15;                 // tile rows with the largest halo
constexpr int kAdPitch = kAdTW + 2 * kAdHalo + 4;       // 164 bytes = 41 banks
constexpr int kAdHPitch = kAdTW + 4;                    // 132 bytes = 33 banks
constexpr int kAdSeg = 16;                              // outputs a lane produces from one window start

__global__ __launch_bounds__(256) void threshold_adaptive_kernel(AdaptArgs a)
{
	__shared__ __attribute__((aligned(4))) uint8_t sRaw[kAdRows * kAdPitch];
	__shared__ __attribute__((aligned(4))) uint8_t sTap[kAdRows * kAdPitch];
	__shared__ uint8_t sHz[kAdRows * kAdHPitch];
	const int tid = threadIdx.x, r = a.r, rows = kAdTH + 2 * r;
	const int tx0 = blockIdx.x * kAdTW, ty0 = blockIdx.y * kAdTH;
	const uint32_t k = a.k;
	const uint8_t* __restrict__ src = a.in + static_cast<size_t>(blockIdx.z) * a.frameStride;
	uint8_t* __restrict__ dst = a.out + static_cast<size_t>(blockIdx.z) * a.frameStride;
	// tile + halo, dword by dword: columns tx0 - 16 .. tx0 + 144, rows ty0 - r .. ty0 + 32 + r; outside the plane: 0
	constexpr int kWords = (kAdTW + 2 * kAdHalo) / 4;
	for (int i = tid; i < rows * kWords; i += 256) {
		const int row = i / kWords, w = i - row * kWords;
		const int y = ty0 - r + row, x = tx0 - kAdHalo + 4 * w;
		uint32_t v = 0;
		if (y >= 0 && y < a.H && x >= 0 && x < a.S) v = *reinterpret_cast<const uint32_t*>(src + static_cast<size_t>(y) * a.S + x);
		const uint32_t q = ((v & 0xffu) * k >> 16) | (((v >> 8) & 0xffu) * k >> 16) << 8 | (((v >> 16) & 0xffu) * k >> 16) << 16 | ((v >> 24) * k >> 16) << 24;
		*reinterpret_cast<uint32_t*>(sRaw + row * kAdPitch + 4 * w) = v;
		*reinterpret_cast<uint32_t*>(sTap + row * kAdPitch + 4 * w) = q;
	}
	__syncthreads();
	// horizontal pass: hz = min(255, window sum) inside [r, W - r), 0 on the border; stored as ITS tap value (hz * k) >> 16 for the vertical pass
	for (int u = tid; u < rows * (kAdTW / kAdSeg); u += 256) {
		const int row = u % rows, xs = (u / rows) * kAdSeg;
		const uint8_t* q = sTap + row * kAdPitch + kAdHalo + xs;
		int sum = 0;
		for (int t = -r; t < r; ++t) sum += q[t];
		for (int c = 0; c < kAdSeg; ++c) {
			sum += q[c + r];
			const int gx = tx0 + xs + c;
			const uint32_t hz = (gx >= r && gx < a.W - r) ? static_cast<uint32_t>(min(sum, 255)) : 0u;
			sHz[row * kAdHPitch + xs + c] = static_cast<uint8_t>((hz * k) >> 16);
			sum -= q[c - r];
		}
	}
	__syncthreads();
	// vertical pass + decision: thread = one column, 16 rows
	const int c = tid & (kAdTW - 1), ys = (tid >> 7) * kAdSeg, gx = tx0 + c;
	const uint8_t* h = sHz + c;                    // sHz row 0 is plane row ty0 - r: output row yl sums sHz rows yl .. yl + 2r
	int sum = 0;
	for (int t = 0; t < 2 * r; ++t) sum += h[(ys + t) * kAdHPitch];
	for (int j = 0; j < kAdSeg; ++j) {
		const int yl = ys + j, gy = ty0 + yl;
		sum += h[(yl + 2 * r) * kAdHPitch];
		if (gx < a.W && gy < a.H) {
			const int mean = (gy >= r && gy < a.H - r) ? min(sum, 255) : 0;
			const int p = sRaw[(yl + r) * kAdPitch + kAdHalo + c];
			const bool hit = (p - mean + 255) >= (256 - a.delta);      // the reference's LUT index against its first `maxVal` slot (:223-226,287)
			dst[static_cast<size_t>(gy) * a.S + gx] = static_cast<uint8_t>((hit != (a.invert != 0)) ? a.maxVal : 0);
		}
		sum -= h[yl * kAdHPitch];
	}
}

hipError_t launch_threshold_adaptive(const AdaptArgs& args, int frames, hipStream_t stream)
{
	if (args.r < 1 || args.r > 15) return hipErrorInvalidValue;
	return for_frame_slices(frames, [&](int f0, int nf) {   // (blockIdx.z, as above)
		AdaptArgs a = args;
		a.in += static_cast<size_t>(f0) * a.frameStride; a.out += static_cast<size_t>(f0) * a.frameStride;
		hipLaunchKernelGGL(threshold_adaptive_kernel, dim3((a.W + kAdTW - 1) / kAdTW, (a.H + kAdTH - 1) / kAdTH, nf), dim3(256), 0, stream, a);
		return hipGetLastError();
	});
}

// ---- morphology ----------------------------------------------------------------------------------------------------------------------
// One workgroup = one 256 x 32 tile of the output; the tile and its halo (16 columns either side, sh / 2 rows above and below) sit in the
// LDS; a thread owns one dword column (four pixels) of eight rows.  Cells outside the plane are 0 in the LDS: only border cells could see
// them, and those take in(y, x) or 0.
constexpr int kMoTW = 256, kMoTH = 32, kMoHalo = 16;
constexpr int kMoRows = kMoTH + 2 * 15;
constexpr int kMoPitchW = (kMoTW + 2 * kMoHalo) / 4 + 1;   // 73 dwords (odd)
constexpr int kMoRowPitchW = kMoTW / 4 + 1;                 // 65 dwords (odd)

__device__ __forceinline__ void morphLoadTile(uint32_t* sRaw, const uint8_t* __restrict__ src, const MorphArgs& a, int tx0, int ty0, int hd)
{
	constexpr int kWords = (kMoTW + 2 * kMoHalo) / 4;
	const int rows = kMoTH + 2 * hd;
	for (int i = threadIdx.x; i < rows * kWords; i += 256) {
		const int row = i / kWords, w = i - row * kWords;
		const int y = ty0 - hd + row, x = tx0 - kMoHalo + 4 * w;
		uint32_t v = 0;
		if (y >= 0 && y < a.H && x >= 0 && x < a.S) v = *reinterpret_cast<const uint32_t*>(src + static_cast<size_t>(y) * a.S + x);
		sRaw[row * kMoPitchW + w] = v;
	}
}

// the four pixels at byte offset `b` of an LDS row (any alignment)
__device__ __forceinline__ uint32_t ldsBytes4(const uint32_t* row, int b)
{
	const int w = b >> 2, s = b & 3;
	const uint32_t lo = row[w];
	return s ? __builtin_amdgcn_alignbyte(row[w + 1], lo, static_cast<uint32_t>(s)) : lo;
}

// addBordersVt, then addBordersHz (compv_math_morph.cxx:542-674): rows y < hb and y >= H - hb (hb = (sh + 1) >> 1: one row MORE than the
// interior leaves uncomputed), then columns x < wd and x >= W - wd, take in(y, x) (REPLICATE) or 0 (ZERO)
__device__ __forceinline__ void morphStore(uint8_t* __restrict__ dst, const MorphArgs& a, int gx, int gy, uint32_t res, uint32_t centre)
{
	if (gx >= a.W || gy >= a.H) return;
	const int wd = a.sw >> 1, hb = (a.sh + 1) >> 1;
	const uint32_t edge = a.replicate ? centre : 0u;
	if (gy < hb || gy >= a.H - hb) res = edge;
	else if (gx < wd || gx + 3 >= a.W - wd) {
		uint32_t m = 0;
		for (int b = 0; b < 4; ++b) if (gx + b < wd || gx + b >= a.W - wd) m |= 0xffu << (8 * b);
		res = (res & ~m) | (edge & m);
	}
	storeRow4(dst + static_cast<size_t>(gy) * a.S, gx, a.W, res);
}

// (a) any structuring element: the member list is the bit mask of every strel row, walked in raster order
template <bool MAX>
__global__ __launch_bounds__(256) void morph_general_kernel(MorphArgs a)
{
	__shared__ uint32_t sRaw[kMoRows * kMoPitchW];
	const int wd = a.sw >> 1, hd = a.sh >> 1;
	const int tx0 = blockIdx.x * kMoTW, ty0 = blockIdx.y * kMoTH;
	const uint8_t* __restrict__ src = a.in + static_cast<size_t>(blockIdx.z) * a.frameStride;
	uint8_t* __restrict__ dst = a.out + static_cast<size_t>(blockIdx.z) * a.frameStride;
	morphLoadTile(sRaw, src, a, tx0, ty0, hd);
	__syncthreads();
	const int g = threadIdx.x & 63, y0 = (threadIdx.x >> 6) * 8;
	const int b0 = kMoHalo + 4 * g - wd;             // byte offset of member column 0 for this thread's first pixel
	for (int yl = y0; yl < y0 + 8; ++yl) {
		Acc<MAX> acc;
		for (int j = 0; j < a.sh; ++j) {
			const uint32_t* row = sRaw + (yl + j) * kMoPitchW;
			for (uint32_t m = a.rows[j]; m; m &= m - 1) acc.add(ldsBytes4(row, b0 + __builtin_ctz(m)));
		}
		morphStore(dst, a, tx0 + 4 * g, ty0 + yl, acc.packed(), sRaw[(yl + hd) * kMoPitchW + (kMoHalo >> 2) + g]);
	}
}

// (b) full rectangle: a row pass over every tile row (halo rows included) into the LDS, then a column pass over its result;
// (c) cross: OP(row run through the centre row, column run through the centre column) -- the row pass for the tile's own rows only, the column
//     pass over the raw tile.
template <bool MAX, bool CROSS>
__global__ __launch_bounds__(256) void morph_separable_kernel(MorphArgs a)
{
	__shared__ uint32_t sRaw[kMoRows * kMoPitchW];
	__shared__ uint32_t sRow[kMoRows * kMoRowPitchW];
	const int wd = a.sw >> 1, hd = a.sh >> 1;
	const int tx0 = blockIdx.x * kMoTW, ty0 = blockIdx.y * kMoTH;
	const uint8_t* __restrict__ src = a.in + static_cast<size_t>(blockIdx.z) * a.frameStride;
	uint8_t* __restrict__ dst = a.out + static_cast<size_t>(blockIdx.z) * a.frameStride;
	morphLoadTile(sRaw, src, a, tx0, ty0, hd);
	__syncthreads();
	const int g = threadIdx.x & 63, q = threadIdx.x >> 6;
	// row pass: LDS rows [r0, r1), four per round of the workgroup
	const int r0 = CROSS ? hd : 0, r1 = CROSS ? hd + kMoTH : kMoTH + 2 * hd;
	for (int row = r0 + q; row < r1; row += 4) {
		const uint32_t* rp = sRaw + row * kMoPitchW;
		Acc<MAX> acc;
		int b = kMoHalo + 4 * g - wd;
		uint32_t lo = rp[b >> 2], hi = rp[(b >> 2) + 1];
		for (int t = 0; t < a.sw; ++t, ++b) {
			const int s = b & 3;
			acc.add(s ? __builtin_amdgcn_alignbyte(hi, lo, static_cast<uint32_t>(s)) : lo);
			if (s == 3) { lo = hi; hi = rp[(b >> 2) + 2]; }
		}
		sRow[row * kMoRowPitchW + g] = acc.packed();
	}
	__syncthreads();
	const int y0 = q * 8;
	for (int yl = y0; yl < y0 + 8; ++yl) {
		Acc<MAX> acc;
		const uint32_t centre = sRaw[(yl + hd) * kMoPitchW + (kMoHalo >> 2) + g];
		if (CROSS) {
			acc.add(sRow[(yl + hd) * kMoRowPitchW + g]);
			for (int j = 0; j < a.sh; ++j) acc.add(sRaw[(yl + j) * kMoPitchW + (kMoHalo >> 2) + g]);
		}
		else {
			for (int j = 0; j < a.sh; ++j) acc.add(sRow[(yl + j) * kMoRowPitchW + g]);
		}
		morphStore(dst, a, tx0 + 4 * g, ty0 + yl, acc.packed(), centre);
	}
}

// at most kMaxFramesPerLaunch frames: the frame index rides in blockIdx.z
static hipError_t launch_morph_slice(const MorphArgs& a, int frames, hipStream_t stream)
{
	const dim3 grid((a.W + kMoTW - 1) / kMoTW, (a.H + kMoTH - 1) / kMoTH, frames), block(256);
	if (a.kind == kMorphRect) {
		if (a.dilate) hipLaunchKernelGGL((morph_separable_kernel<true, false>), grid, block, 0, stream, a);
		else hipLaunchKernelGGL((morph_separable_kernel<false, false>), grid, block, 0, stream, a);
	}
	else if (a.kind == kMorphCross) {
		if (a.dilate) hipLaunchKernelGGL((morph_separable_kernel<true, true>), grid, block, 0, stream, a);
		else hipLaunchKernelGGL((morph_separable_kernel<false, true>), grid, block, 0, stream, a);
	}
	else {
		if (a.dilate) hipLaunchKernelGGL((morph_general_kernel<true>), grid, block, 0, stream, a);
		else hipLaunchKernelGGL((morph_general_kernel<false>), grid, block, 0, stream, a);
	}
	return hipGetLastError();
}

hipError_t launch_morph(const MorphArgs& args, int frames, hipStream_t stream)
{
	if (args.sw < 1 || args.sw > kMorphMaxStrel || args.sh < 1 || args.sh > kMorphMaxStrel || !(args.sw & 1) || !(args.sh & 1)) return hipErrorInvalidValue;
	return for_frame_slices(frames, [&](int f0, int nf) {
		MorphArgs a = args;
		a.in += static_cast<size_t>(f0) * a.frameStride; a.out += static_cast<size_t>(f0) * a.frameStride;
		return launch_morph_slice(a, nf, stream);
	});
}

} // namespace compvhip
