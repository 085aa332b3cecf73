// components_kernels.hip -- connected-component labelling of 1-bit edge maps with per-component records (compvhip_plan_components,
// compvhip_components_u8; definition in include/compv_hip.h and docs/kernels/components.md).
//
// Everything works on the plan's mask layout (u32 [frames][H][wb], bit i of word k = pixel 32 k + i); mask bits at columns >= W are cut off by
// comp_word() before anything looks at them.  A component is named by its ROOT, the pixel with the smallest raster index r = y * W + x, so a
// union-find that always links the larger root below the smaller one (atomicMin) ends in the same forest of roots whatever the order of the
// unions.  The parent words live in the caller's label map when there is one (element (y, x) at y * stride + x, labelled in place), otherwise in
// the plan's scratch; a parent word holds a raster index, which orders pixels exactly as their addresses do.
//
// Launches (one grid each over all frames of the plan; what one workgroup writes and another reads crosses a kernel boundary, except for the
// agent-scope atomics named below):
//  1 comp_tile     one workgroup per 128 x 64 tile: runs of a row are found with bit arithmetic (a pixel is represented by the first pixel of
//                  its run inside the tile), vertical / diagonal contacts are united in an LDS union-find (ds atomicMin), every foreground
//                  pixel's parent word := the root of its piece of the tile.  Contacts that other unions already imply are skipped.
//  2 comp_border   the contacts across tile borders (the row above every tile row, the column left of every tile column): global union-find,
//                  atomicMin on root words, parent words read with agent-scope atomic loads.  Only border pixels work here.
//  3 comp_flatten  every pixel's parent word := its root (agent-scope atomic stores: the words are read by the walks of other workgroups);
//                  a root's word := -1.  From here on a NEGATIVE word marks a root.
//  4 comp_count    pixel counts: a root's word becomes -1 - pixels (atomicAdd; runs, then lanes of a wave with the same root, are summed first).
//  5 comp_rows<false>  survivors (roots with pixels >= minPixels) per image row, one wave per row  -- count
//  6 comp_scan     exclusive prefix over the rows of a frame, total -> compCounts              -- scan
//  7 comp_rows<true>   root words := -1 - id (id 0: dropped), records of the ids <= compCap        -- write (no atomic cursor: ids are ordered)
//  8 comp_boxes    non-root pixels: word := id; bounding boxes by atomicMin / atomicMax on the records, after a wave-level reduction and
//                  only where the box read back is still too small
//  9 comp_finish   label map only: root words := id, background := 0
// Without a label map 8 only runs when records are wanted and 9 never.
#include "device.hpp"
#include "frame_slices.hpp"

namespace compvhip {

namespace {

constexpr int kTileWords = 4;                  // 128 columns
constexpr int kTileW = kTileWords * 32;
constexpr int kTileH = 64;
constexpr int kCompThreads = 256;

__device__ __forceinline__ uint32_t comp_word(const CompArgs& a, const uint32_t* bits, int y, int w)
{
	if ((unsigned)y >= (unsigned)a.H || (unsigned)w >= (unsigned)a.words) return 0u;
	const uint32_t m = bits[(size_t)y * a.wb + w];
	return w == a.words - 1 ? m & a.lastMask : m;
}

// raster index -> element of the parent array
__device__ __forceinline__ size_t comp_slot(const CompArgs& a, int r)
{
	if (a.ps == a.W) return (size_t)r;
	const int y = r / a.W;
	return (size_t)y * a.ps + (r - y * a.W);
}

__device__ __forceinline__ int comp_load(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void comp_store(int32_t* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// root of raster index r: the walk ends at a word that names itself or is negative (a root that comp_flatten has already marked)
__device__ __forceinline__ int comp_find(const CompArgs& a, const int32_t* P, int r)
{
	for (;;) {
		const int v = comp_load(P + comp_slot(a, r));
		if (v == r || v < 0) return r;
		r = v;
	}
}

__device__ __forceinline__ void comp_union(const CompArgs& a, int32_t* P, int x, int y)
{
	for (;;) {
		x = comp_find(a, P, x); y = comp_find(a, P, y);
		if (x == y) return;
		if (x < y) { const int t = x; x = y; y = t; }
		const int old = atomicMin(P + comp_slot(a, x), y);   // device scope
		if (old == x) return;                                // x was still a root: linked
		x = old;                                             // somebody linked x meanwhile: its word is min(old, y) now, unite the other two
	}
}

// the run of ones of m that starts at its lowest set bit: length
__device__ __forceinline__ int run_len(uint32_t m, int b)
{
	const uint32_t inv = ~(m >> b);
	return inv ? __builtin_ctz(inv) : 32;
}
__device__ __forceinline__ uint32_t run_mask(int b, int len) { return (len >= 32 ? ~0u : ((1u << len) - 1u)) << b; }

// ---- 1: tiles --------------------------------------------------------------------------------------------------------------------
// first pixel (tile column) of the run that holds tile pixel (row, lx)
__device__ __forceinline__ int tile_run_start(const uint32_t (*sb)[kTileWords], int row, int lx)
{
	int k = lx >> 5;
	const int bit = lx & 31;
	const uint32_t zerosBelow = ~sb[row][k] & ((1u << bit) - 1u);
	if (zerosBelow) return k * 32 + 32 - __clz((int)zerosBelow);
	int s = k * 32;
	while (k > 0) {
		--k;
		const int ones = __clz((int)~sb[row][k]);   // leading ones of the word to the left (32 when it is full)
		s -= ones;
		if (ones < 32) break;
	}
	return s;
}

__device__ __forceinline__ int tile_find(int* lab, int x)
{
	for (;;) {
		const int v = __hip_atomic_load(lab + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
		if (v == x) return x;
		x = v;
	}
}

__device__ __forceinline__ void tile_union(int* lab, int x, int y)
{
	for (;;) {
		x = tile_find(lab, x); y = tile_find(lab, y);
		if (x == y) return;
		if (x < y) { const int t = x; x = y; y = t; }
		const int old = atomicMin(lab + x, y);
		if (old == x) return;
		x = old;
	}
}

__global__ __launch_bounds__(kCompThreads) void comp_tile_kernel(CompArgs a)
{
	__shared__ uint32_t sb[kTileH][kTileWords];
	__shared__ int lab[kTileH * kTileW];          // valid at run starts only: every pixel is represented by the start of its run
	const int f = a.frame0 + blockIdx.z;
	const uint32_t* bits = a.bits + (size_t)f * a.bitsFrameStride;
	int32_t* P = a.parent + (size_t)f * a.parentFrameStride;
	const int tw = threadIdx.x & (kTileWords - 1), ty = threadIdx.x / kTileWords;
	const int w = blockIdx.x * kTileWords + tw, y = blockIdx.y * kTileH + ty;
	const uint32_t m = comp_word(a, bits, y, w);
	sb[ty][tw] = m;
	__syncthreads();
	// run starts inside this word name themselves
	{
		const uint32_t leftIn = tw > 0 ? sb[ty][tw - 1] >> 31 : 0u;
		uint32_t starts = m & ~((m << 1) | leftIn);
		while (starts) {
			const int b = __builtin_ctz(starts);
			starts &= starts - 1;
			lab[ty * kTileW + tw * 32 + b] = ty * kTileW + tw * 32 + b;
		}
	}
	__syncthreads();
	if (ty > 0 && m) {
		const uint32_t up = sb[ty - 1][tw];
		const uint32_t upL = tw > 0 ? sb[ty - 1][tw - 1] : 0u, upR = tw < kTileWords - 1 ? sb[ty - 1][tw + 1] : 0u;
		const uint32_t lw = tw > 0 ? sb[ty][tw - 1] : 0u, rw = tw < kTileWords - 1 ? sb[ty][tw + 1] : 0u;
		const uint32_t L = (m << 1) | (lw >> 31), R = (m >> 1) | (rw << 31);          // left / right neighbour is foreground
		const uint32_t UL = (up << 1) | (upL >> 31), UR = (up >> 1) | (upR << 31);    // upper-left / upper-right neighbour is foreground
		// up: unless the left neighbour and the upper-left one are both set (the left neighbour makes that contact, and runs connect the rest)
		uint32_t nu = m & up & ~(L & UL);
		while (nu) {
			const int b = __builtin_ctz(nu);
			nu &= nu - 1;
			const int lx = tw * 32 + b;
			tile_union(lab, ty * kTileW + tile_run_start(sb, ty, lx), (ty - 1) * kTileW + tile_run_start(sb, ty - 1, lx));
		}
		if (a.conn8) {
			// diagonals only matter under a background pixel; the left (right) neighbour, when set, is right below that diagonal pixel itself
			uint32_t nl = m & ~up & UL & ~L;
			while (nl) {
				const int b = __builtin_ctz(nl);
				nl &= nl - 1;
				const int lx = tw * 32 + b;
				tile_union(lab, ty * kTileW + tile_run_start(sb, ty, lx), (ty - 1) * kTileW + tile_run_start(sb, ty - 1, lx - 1));
			}
			uint32_t nr = m & ~up & UR & ~R;
			while (nr) {
				const int b = __builtin_ctz(nr);
				nr &= nr - 1;
				const int lx = tw * 32 + b;
				tile_union(lab, ty * kTileW + tile_run_start(sb, ty, lx), (ty - 1) * kTileW + tile_run_start(sb, ty - 1, lx + 1));
			}
		}
	}
	__syncthreads();
	if (m) {
		const int x0 = blockIdx.x * kTileW, y0 = blockIdx.y * kTileH;
		int32_t* row = P + (size_t)y * a.ps + (size_t)w * 32;
		uint32_t r = m;
		while (r) {
			const int b = __builtin_ctz(r);
			const int len = run_len(r, b);
			r &= ~run_mask(b, len);
			const int root = tile_find(lab, ty * kTileW + tile_run_start(sb, ty, tw * 32 + b));
			const int v = (y0 + root / kTileW) * a.W + x0 + (root & (kTileW - 1));
			for (int i = b; i < b + len; ++i) row[i] = v;
		}
	}
}

// ---- 2: tile borders -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kCompThreads) void comp_border_kernel(CompArgs a)
{
	const int f = a.frame0 + blockIdx.y;
	const uint32_t* bits = a.bits + (size_t)f * a.bitsFrameStride;
	int32_t* P = a.parent + (size_t)f * a.parentFrameStride;
	const long long idx = (long long)blockIdx.x * kCompThreads + threadIdx.x;
	const int tilesY = (a.H + kTileH - 1) / kTileH, tilesX = (a.words + kTileWords - 1) / kTileWords;
	const long long nRow = (long long)(tilesY - 1) * a.words;
	if (idx < nRow) {
		// the first row of a tile row against the row above it
		const int y = ((int)(idx / a.words) + 1) * kTileH, w = (int)(idx % a.words);
		const uint32_t m = comp_word(a, bits, y, w);
		if (!m) return;
		const uint32_t up = comp_word(a, bits, y - 1, w), upL = comp_word(a, bits, y - 1, w - 1), upR = comp_word(a, bits, y - 1, w + 1);
		const uint32_t lw = comp_word(a, bits, y, w - 1), rw = comp_word(a, bits, y, w + 1);
		const uint32_t L = (m << 1) | (lw >> 31), R = (m >> 1) | (rw << 31);
		const uint32_t UL = (up << 1) | (upL >> 31), UR = (up >> 1) | (upR << 31);
		const int r0 = y * a.W + w * 32;
		uint32_t nu = m & up & ~(L & UL);
		while (nu) {
			const int b = __builtin_ctz(nu);
			nu &= nu - 1;
			comp_union(a, P, r0 + b, r0 + b - a.W);
		}
		if (a.conn8) {
			uint32_t nl = m & ~up & UL & ~L;
			while (nl) {
				const int b = __builtin_ctz(nl);
				nl &= nl - 1;
				comp_union(a, P, r0 + b, r0 + b - a.W - 1);
			}
			uint32_t nr = m & ~up & UR & ~R;
			while (nr) {
				const int b = __builtin_ctz(nr);
				nr &= nr - 1;
				comp_union(a, P, r0 + b, r0 + b - a.W + 1);
			}
		}
		return;
	}
	const long long j = idx - nRow;
	if (j >= (long long)(tilesX - 1) * a.H) return;
	// the first column of a tile column against the column left of it
	const int w = ((int)(j / a.H) + 1) * kTileWords, y = (int)(j % a.H);
	if (!(comp_word(a, bits, y, w) & 1u)) return;
	const int r = y * a.W + w * 32;
	const bool left = comp_word(a, bits, y, w - 1) >> 31;
	if (left) comp_union(a, P, r, r - 1);
	else if (a.conn8) {
		// with the left neighbour set, it touches both diagonal pixels itself; with the pixel above (below) set, that one touches the diagonal one
		if ((comp_word(a, bits, y - 1, w - 1) >> 31) && !(comp_word(a, bits, y - 1, w) & 1u)) comp_union(a, P, r, r - a.W - 1);
		if ((comp_word(a, bits, y + 1, w - 1) >> 31) && !(comp_word(a, bits, y + 1, w) & 1u)) comp_union(a, P, r, r + a.W - 1);
	}
}

// ---- 3: flatten ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kCompThreads) void comp_flatten_kernel(CompArgs a)
{
	const int f = a.frame0 + blockIdx.y;
	const uint32_t* bits = a.bits + (size_t)f * a.bitsFrameStride;
	int32_t* P = a.parent + (size_t)f * a.parentFrameStride;
	const long long idx = (long long)blockIdx.x * kCompThreads + threadIdx.x;
	if (idx >= (long long)a.words * a.H) return;
	const int y = (int)(idx / a.words), w = (int)(idx % a.words);
	uint32_t r = comp_word(a, bits, y, w);
	int32_t* row = P + (size_t)y * a.ps + (size_t)w * 32;
	const int r0 = y * a.W + w * 32;
	while (r) {
		// the pixels of a run inside a word left the tile kernel with one parent: one walk serves them all
		const int b = __builtin_ctz(r);
		const int len = run_len(r, b);
		r &= ~run_mask(b, len);
		const int root = comp_find(a, P, r0 + b);
		for (int i = b; i < b + len; ++i) comp_store(row + i, r0 + i == root ? -1 : root);
	}
}

// ---- 4: pixel counts -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kCompThreads) void comp_count_kernel(CompArgs a)
{
	const int f = a.frame0 + blockIdx.y;
	const uint32_t* bits = a.bits + (size_t)f * a.bitsFrameStride;
	int32_t* P = a.parent + (size_t)f * a.parentFrameStride;
	const long long idx = (long long)blockIdx.x * kCompThreads + threadIdx.x;
	const bool inside = idx < (long long)a.words * a.H;
	const int y = inside ? (int)(idx / a.words) : 0, w = inside ? (int)(idx % a.words) : 0;
	uint32_t r = inside ? comp_word(a, bits, y, w) : 0u;
	const int32_t* row = P + (size_t)y * a.ps + (size_t)w * 32;
	const int r0 = y * a.W + w * 32;
	const int lane = threadIdx.x & 63;
	// every lane brings one (root, pixels) pair per turn -- consecutive runs of its word with one root already summed -- and the wave stays whole
	while (__any(r != 0)) {
		int root = -1, n = 0;
		while (r) {
			const int b = __builtin_ctz(r);
			const int len = run_len(r, b);
			const int v = comp_load(row + b);
			const int rt = v < 0 ? r0 + b : v;
			if (root >= 0 && rt != root) break;
			root = rt; n += len;
			r &= ~run_mask(b, len);
		}
		// two rounds of "everybody with the first lane's root": one atomic for a wave inside one component
		for (int k = 0; k < 2; ++k) {
			const unsigned long long act = __ballot(root >= 0);
			if (!act) break;
			const int lead = __builtin_ctzll(act);
			const int lr = __shfl(root, lead);
			const bool mine = root == lr;
			const int s = wave_sum(mine ? n : 0);
			if (lane == lead) atomicAdd(P + comp_slot(a, lr), -s);
			if (mine) root = -1;
		}
		if (root >= 0) atomicAdd(P + comp_slot(a, root), -n);
	}
}

// ---- 5 / 7: survivors per row, ids and records --------------------------------------------------------------------------------------
// one wave per image row; WRITE = false: rowCounts[f][y] = survivors whose root is in row y; WRITE = true: rowCounts holds the exclusive prefix
template <bool WRITE>
__global__ __launch_bounds__(kCompThreads) void comp_rows_kernel(CompArgs a)
{
	const int f = a.frame0 + blockIdx.y;
	const uint32_t* bits = a.bits + (size_t)f * a.bitsFrameStride;
	int32_t* P = a.parent + (size_t)f * a.parentFrameStride;
	const int lane = threadIdx.x & 63;
	const int y = blockIdx.x * (kCompThreads / 64) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
	if (y >= a.H) return;
	int32_t* row = P + (size_t)y * a.ps;
	int base = WRITE ? a.rowCounts[(size_t)f * a.H + y] : 0;
	compvhip_component* out = a.comps + (size_t)f * a.compCap;
	for (int w0 = 0; w0 < a.words; w0 += 64) {
		const int w = w0 + lane;
		const uint32_t m = comp_word(a, bits, y, w);
		// a root has no foreground pixel to its left: only run starts are looked at
		uint32_t starts = m & ~((m << 1) | (comp_word(a, bits, y, w - 1) >> 31));
		uint32_t surv = 0, roots = 0;
		for (uint32_t s = starts; s; s &= s - 1) {
			const int b = __builtin_ctz(s);
			const int v = row[w * 32 + b];
			if (v < 0) {
				roots |= 1u << b;
				if (-(v + 1) >= a.minPixels) surv |= 1u << b;
			}
		}
		const int c = __popc(surv);
		if (!WRITE) { base += c; continue; }
		int incl = c;
#pragma unroll
		for (int o = 1; o < 64; o <<= 1) {   // wave_incl_scan, written out
			const int t = __shfl_up(incl, o);
			if (lane >= o) incl += t;
		}
		int id = base + incl - c;                 // survivors in front of this word
		for (uint32_t s = roots; s; s &= s - 1) {
			const int b = __builtin_ctz(s);
			const int x = w * 32 + b;
			if (!((surv >> b) & 1u)) { row[x] = -1; continue; }      // dropped: id 0
			const int pixels = -(row[x] + 1);
			++id;
			row[x] = -1 - id;
			if ((size_t)id <= a.compCap) {
				compvhip_component c8;
				c8.x = x; c8.y = y; c8.x0 = x; c8.y0 = y; c8.x1 = x; c8.y1 = y; c8.pixels = pixels;
				out[id - 1] = c8;
			}
		}
		base += __shfl(incl, 63);
	}
	if (!WRITE) {
		base = wave_sum(base);
		if (lane == 0) a.rowCounts[(size_t)f * a.H + y] = base;
	}
}

// ---- 6: exclusive prefix over the rows of a frame ---------------------------------------------------------------------------------
constexpr int kScanThreads = 1024;
__global__ __launch_bounds__(kScanThreads) void comp_scan_kernel(CompArgs a)
{
	const int f = a.frame0 + blockIdx.x;
	int32_t* v = a.rowCounts + (size_t)f * a.H;
	const int32_t total = block_excl_scan<kScanThreads>(v, v, a.H);
	if (threadIdx.x == 0) a.compCounts[f] = total;
}

// ---- 8: labels of the non-root pixels, bounding boxes ---------------------------------------------------------------------------------
__device__ __forceinline__ void box_update(compvhip_component* c, int xa, int xb, int yb)
{
	// y0 is the root's row already; a box only grows, so a stale read can only ask for an atomic that changes nothing
	if (xa < comp_load(&c->x0)) atomicMin(&c->x0, xa);
	if (xb > comp_load(&c->x1)) atomicMax(&c->x1, xb);
	if (yb > comp_load(&c->y1)) atomicMax(&c->y1, yb);
}

__global__ __launch_bounds__(kCompThreads) void comp_boxes_kernel(CompArgs a)
{
	const int f = a.frame0 + blockIdx.y;
	const uint32_t* bits = a.bits + (size_t)f * a.bitsFrameStride;
	int32_t* P = a.parent + (size_t)f * a.parentFrameStride;
	compvhip_component* out = a.comps + (size_t)f * a.compCap;
	const long long idx = (long long)blockIdx.x * kCompThreads + threadIdx.x;
	const bool inside = idx < (long long)a.words * a.H;
	const int y = inside ? (int)(idx / a.words) : 0, w = inside ? (int)(idx % a.words) : 0;
	uint32_t r = inside ? comp_word(a, bits, y, w) : 0u;
	int32_t* row = P + (size_t)y * a.ps + (size_t)w * 32;
	const int lane = threadIdx.x & 63;
	while (__any(r != 0)) {
		// one (id, x range) per lane and turn: consecutive runs of the word with one id are merged
		int id = 0, xa = 0, xb = 0;
		while (r) {
			const int b = __builtin_ctz(r);
			const int len = run_len(r, b);
			const int v = row[b];
			const int enc = v < 0 ? v : P[comp_slot(a, v)];      // root words are not written in this launch
			const int rid = -(enc + 1);
			const bool rec = rid > 0 && (size_t)rid <= a.compCap;     // has a record to grow
			if (rec && id > 0 && rid != id) break;                    // next turn
			r &= ~run_mask(b, len);
			if (a.wantLabels)
				for (int i = v < 0 ? b + 1 : b; i < b + len; ++i) row[i] = rid;   // a root keeps its word for the other pixels to read
			if (rec) {
				if (id == 0) { id = rid; xa = w * 32 + b; }
				xb = w * 32 + b + len - 1;
			}
		}
		const unsigned long long act = __ballot(id > 0);
		if (act) {
			const int lead = __builtin_ctzll(act);
			const int lid = __shfl(id, lead);
			const bool mine = id == lid;
			const int mxa = wave_min(mine ? xa : 0x7fffffff), mxb = wave_max(mine ? xb : -1), myb = wave_max(mine ? y : -1);
			if (lane == lead) box_update(out + (lid - 1), mxa, mxb, myb);
			if (mine) id = 0;
		}
		if (id > 0) box_update(out + (id - 1), xa, xb, y);
	}
}

// ---- 9: roots and background of the label map ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(kCompThreads) void comp_finish_kernel(CompArgs a)
{
	const int f = a.frame0 + blockIdx.z;
	const uint32_t* bits = a.bits + (size_t)f * a.bitsFrameStride;
	int32_t* P = a.parent + (size_t)f * a.parentFrameStride;
	const int x = blockIdx.x * kCompThreads + threadIdx.x, y = blockIdx.y;
	if (x >= a.W) return;
	const uint32_t m = comp_word(a, bits, y, x >> 5);
	int32_t* q = P + (size_t)y * a.ps + x;
	if (!((m >> (x & 31)) & 1u)) { *q = 0; return; }
	const bool leftSet = (x & 31) ? (m >> ((x & 31) - 1)) & 1u : comp_word(a, bits, y, (x >> 5) - 1) >> 31;
	if (leftSet) return;
	const int v = *q;
	if (v < 0) *q = -(v + 1);
}

// the frame index rides in grid dimension frameDim
template <typename K>
hipError_t launch_sliced(K kernel, dim3 grid, int frameDim, int frames, CompArgs a, int threads, hipStream_t stream)
{
	return for_frame_slices(frames, [&](int f0, int nf) {
		a.frame0 = f0;
		(frameDim == 0 ? grid.x : frameDim == 1 ? grid.y : grid.z) = (unsigned)nf;
		hipLaunchKernelGGL(kernel, grid, dim3((unsigned)threads), 0, stream, a);
		return hipGetLastError();
	});
}

} // namespace

hipError_t launch_components(const CompArgs& a, int frames, int phase, hipStream_t stream)
{
	const int tilesX = (a.words + kTileWords - 1) / kTileWords, tilesY = (a.H + kTileH - 1) / kTileH;
	const long long items = (long long)a.words * a.H;
	const unsigned itemBlocks = (unsigned)((items + kCompThreads - 1) / kCompThreads);
	const unsigned rowBlocks = (unsigned)((a.H + kCompThreads / 64 - 1) / (kCompThreads / 64));
	switch (phase) {
	case 0: return launch_sliced(comp_tile_kernel, dim3((unsigned)tilesX, (unsigned)tilesY, 1), 2, frames, a, kCompThreads, stream);
	case 1: {
		const long long n = (long long)(tilesY - 1) * a.words + (long long)(tilesX - 1) * a.H;
		if (n <= 0) return hipSuccess;
		return launch_sliced(comp_border_kernel, dim3((unsigned)((n + kCompThreads - 1) / kCompThreads), 1, 1), 1, frames, a, kCompThreads, stream);
	}
	case 2: return launch_sliced(comp_flatten_kernel, dim3(itemBlocks, 1, 1), 1, frames, a, kCompThreads, stream);
	case 3: return launch_sliced(comp_count_kernel, dim3(itemBlocks, 1, 1), 1, frames, a, kCompThreads, stream);
	case 4: return launch_sliced(comp_rows_kernel<false>, dim3(rowBlocks, 1, 1), 1, frames, a, kCompThreads, stream);
	case 5: return launch_sliced(comp_scan_kernel, dim3(1, 1, 1), 0, frames, a, kScanThreads, stream);
	case 6: return launch_sliced(comp_rows_kernel<true>, dim3(rowBlocks, 1, 1), 1, frames, a, kCompThreads, stream);
	case 7: return launch_sliced(comp_boxes_kernel, dim3(itemBlocks, 1, 1), 1, frames, a, kCompThreads, stream);
	case 8: return launch_sliced(comp_finish_kernel, dim3((unsigned)((a.W + kCompThreads - 1) / kCompThreads), (unsigned)a.H, 1), 2, frames, a, kCompThreads, stream);
	default: return hipErrorInvalidValue;
	}
}

} // namespace compvhip
