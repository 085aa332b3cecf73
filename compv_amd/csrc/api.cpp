// api.cpp -- host side of the C ABI declared in include/compv_hip.h (compiled with hipcc, no torch types).
//
// Host-pointer entry points mirror the reference's process() contract (synchronous, results in host memory):
//   compvhip_canny_u8     <- CompVEdgeDeteCanny::process   core/features/edges/compv_core_feature_canny_dete.cxx:123-331
//   compvhip_edge_dete_u8 <- CompVCornerDeteEdgeBase::process core/features/edges/compv_core_feature_edge_dete.cxx:55-206
//   compvhip_houghsht_u8  <- CompVHoughSht::process        core/features/hough/compv_core_feature_houghsht.cxx:96-262
// Device-pointer ("plan") entry points run the same kernels on batches of frames resident in HBM.
#include "api_internal.hpp"

namespace {
// ---- thresholds: core/features/edges/compv_core_feature_canny_dete.cxx:251-266 (COMPARE_TO_GRADIENT branch) ----
// cosf / sinf exactly as the reference's scalar calls resolve them (never merged into sincosf)
__attribute__((noinline, optnone)) float libmCosf(float x) { return cosf(x); }
__attribute__((noinline, optnone)) float libmSinf(float x) { return sinf(x); }

void gradientThresholds(float fLow, float fHigh, int* tLow, int* tHigh)
{
	const float l = fLow < 1.f ? 1.f : (fLow > 65535.f ? 65535.f : fLow);
	const float h = fHigh < 1.f ? 1.f : (fHigh > 65535.f ? 65535.f : fHigh);
	uint16_t lo = static_cast<uint16_t>(l), hi = static_cast<uint16_t>(h);
	lo = static_cast<uint16_t>(std::max<int>(1, lo));
	hi = static_cast<uint16_t>(std::max<int>(lo + 2, hi));
	*tLow = lo; *tHigh = hi;
}

// ---- column coverage of the reference's SIMD + scalar-remainder dispatch (quirk Q3) ----
// ...canny_dete.cxx:362-412 (nms_gather) and :483-527 (hysteresis): the row leaves cover col = 1, 1+mpw, ... while
// col < (W-1)-(mpw-1); the scalar remainder restarts at (W-1) & -(mpw-1).
void cannyCoverage(size_t W, int* simdEnd, int* cStart)
{
	const size_t maxCols = W - 1;
	size_t mpw = 1;
	if (maxCols >= 16) mpw = 16; else if (maxCols >= 8) mpw = 8;
	if (mpw == 1) { *simdEnd = 1; *cStart = 1; return; }
	size_t col = 1;
	while (col + (mpw - 1) < maxCols) col += mpw;
	*simdEnd = static_cast<int>(col);
	*cStart = static_cast<int>(maxCols & static_cast<size_t>(-static_cast<ptrdiff_t>(mpw - 1)));
}

// ---- SHT geometry/tables: core/features/hough/compv_core_feature_houghsht.cxx:42-52,318-348 ----
const float kPiF = 3.1415926535897932384626433f;   // kfMathTrigPi (base/math/compv_math.cxx:27)
float piOver180() { return kPiF / 180.f; }         // kfMathTrigPiOver180 (:30)

void shtTables(float thetaDeg, size_t T, std::vector<int32_t>& sinQ, std::vector<int32_t>& cosQ)
{
	// float32 running angle and libm sinf/cosf on the HOST, exactly as initCoords (:335-339); never device sinf.
	const float fTheta = thetaDeg * piOver180();
	const float fRho = 1.f;
	sinQ.resize(T); cosQ.resize(T);
	float tt = 0.f;
	for (size_t t = 0; t < T; ++t, tt += fTheta) {
		sinQ[t] = static_cast<int32_t>((libmSinf(tt) * fRho) * 65535.f);
		cosQ[t] = static_cast<int32_t>((libmCosf(tt) * fRho) * 65535.f);
	}
}

// ---- tiles of the second-generation vote kernel (sht_tiles_kernels.hip) ----
// Grid of equal tiles (width a multiple of 32 px) whose rho windows -- per theta, the span of (lx cosQ + ly sinQ + Clo) >> 16 over the tile -- have at
// most kShtMaxWindow rows; fills the [tiles][T] tables K and rowBase (int64 arithmetic here, int32 on the device).  Grids are tried in order of tile
// count (split the dimension with the longer tile side) and the smallest one that fits is taken -- except when it leaves the chip nearly empty (fewer
// than 64 workgroups = frames x tiles x theta groups: the single-frame plans of the host entry points): then the next four grids are priced with a model
// calibrated on the 4K benchmark (a workgroup: 67 us per 960 x 720 pixels of tile + 9.3 us per 1208 window rows; the reduce kernel: 36 us per
// 32 x 12 x 1208 partial-window rows) and the cheapest is taken: 7 x 4 instead of 4 x 3 tiles for one 4K frame, 0.349 -> 0.320 ms per compvhip_houghsht_u8
// call.  Measured and NOT done: the same model for batches (round 4: 32 x 1080p on 4 x 2 instead of 2 x 2 tiles = three full rounds of the 256 CUs instead
// of one and a half: no change, that step is bound by the launch chain; 32 x 720p on 4 x 2 instead of 2 x 1: 0.180 against 0.170 ms per step).
// Lab knob (like COMPVHIP_RESOLVE_WRAP): COMPVHIP_VOTE_MAX_WINDOW=<rows> caps a voting workgroup's window below the 1264 rows the LDS holds, i.e. forces a
// finer tile grid that leaves LDS free beside a voting workgroup (co-residency experiments, profiles/r06/coresidency.md).  Results are identical for any
// grid (tests/test_gpu_plan_geometry.py::test_vote_window_knob_is_bit_exact); unset = the product's choice.
static size_t voteMaxWindow()   // read whenever a plan is made: one process can hold plans on different grids (tools/coresidency/grid_ab.py)
{
	const char* e = getenv("COMPVHIP_VOTE_MAX_WINDOW");
	const long n = e ? atol(e) : 0;
	return (n >= 64 && n <= kShtMaxWindow) ? static_cast<size_t>(n) : static_cast<size_t>(kShtMaxWindow);
}

static bool voteGridTables(size_t W, size_t H, const std::vector<int32_t>& sinQ, const std::vector<int32_t>& cosQ, int split, int& nx, int& ny, int& TW, int& TH, long long& worst,
                           std::vector<int32_t>* kt, std::vector<int32_t>* rowBase)
{
	const size_t T = sinQ.size();
	const long long barrier = static_cast<long long>(W + H);
	nx = 1; ny = 1;
	for (int k = 0; k < split; ++k) {
		const double tw = static_cast<double>(W) / nx, th = static_cast<double>(H) / ny;
		if (tw >= th) ++nx; else ++ny;
	}
	TW = static_cast<int>(alignUp((W + nx - 1) / nx, 32)); TH = static_cast<int>((H + ny - 1) / ny);
	nx = static_cast<int>((W + TW - 1) / TW); // the rounding to 32 columns may save a column of tiles
	const int tiles = nx * ny;
	if (kt) { kt->assign(static_cast<size_t>(tiles) * T, 0); rowBase->assign(static_cast<size_t>(tiles) * T, 0); }
	worst = 0;
	for (int ty = 0; ty < ny; ++ty) for (int tx = 0; tx < nx; ++tx) {
		const long long x0 = static_cast<long long>(tx) * TW, y0 = static_cast<long long>(ty) * TH;
		const long long mx = TW - 1, my = TH - 1; // largest local coordinates (tiles at the image border are not clipped: simpler, still exact)
		for (size_t t = 0; t < T; ++t) {
			const long long c = cosQ[t], sn = sinQ[t];
			const long long C = x0 * c + y0 * sn;
			long long Chi = C / 65536; if (C - Chi * 65536 < 0) --Chi; // floor
			const long long Clo = C - Chi * 65536;
			const long long corners[4] = { Clo, mx * c + Clo, my * sn + Clo, mx * c + my * sn + Clo };
			long long qmin = 0, qmax = 0;
			for (int k = 0; k < 4; ++k) {
				long long q = corners[k] / 65536; if (corners[k] - q * 65536 < 0) --q;
				if (k == 0 || q < qmin) qmin = q;
				if (k == 0 || q > qmax) qmax = q;
			}
			// the window starts on a multiple of 16 accumulator rows (d extra rows at its top): the reduce kernel adds whole 16-byte groups of count bytes
			const long long base = barrier - Chi - qmax;
			const long long d = ((base % 16) + 16) % 16;
			worst = std::max(worst, qmax - qmin + 1 + d);
			if (kt) {
				(*kt)[(static_cast<size_t>(ty) * nx + tx) * T + t] = static_cast<int32_t>((qmax + d) * 65536 + 65535 - Clo);
				(*rowBase)[(static_cast<size_t>(ty) * nx + tx) * T + t] = static_cast<int32_t>(base - d);
			}
		}
	}
	return alignUp(static_cast<size_t>(worst), 16) <= voteMaxWindow() && TW <= 1280 &&
	       static_cast<long long>(TW - 1) * 65535 + static_cast<long long>(TH - 1) * 65535 < 0x7f000000LL;
}

bool planVoteTiles(size_t W, size_t H, size_t frames, const std::vector<int32_t>& sinQ, const std::vector<int32_t>& cosQ, ShtTileArgs& v, std::vector<int32_t>& kt,
                   std::vector<int32_t>& rowBase)
{
	const size_t T = sinQ.size();
	const int groups = static_cast<int>((T + 63) / 64);
	int first = -1;
	for (int split = 0; split < 512 && first < 0; ++split) {
		int nx, ny, TW, TH; long long worst;
		if (voteGridTables(W, H, sinQ, cosQ, split, nx, ny, TW, TH, worst, nullptr, nullptr)) first = split;
	}
	if (first < 0) return false;
	int best = first; double bestCost = 0.0;
	int nx0, ny0, TW0, TH0; long long worst0;
	(void)voteGridTables(W, H, sinQ, cosQ, first, nx0, ny0, TW0, TH0, worst0, nullptr, nullptr);
	const bool starved = static_cast<double>(frames) * nx0 * ny0 * groups < 64.0;   // a quarter of the CUs at most: single frames (the host entry points)
	for (int split = first; starved && split <= first + 4; ++split) {
		int nx, ny, TW, TH; long long worst;
		if (!voteGridTables(W, H, sinQ, cosQ, split, nx, ny, TW, TH, worst, nullptr, nullptr)) continue;
		const double rw = static_cast<double>(alignUp(static_cast<size_t>(worst), 16));
		const double wgs = static_cast<double>(frames) * nx * ny * groups;
		const double rounds = wgs <= 1024.0 ? std::ceil(wgs / 256.0) : wgs / 256.0;   // a few rounds are quantised, many level out (the dispatcher hands workgroups out as CUs free up)
		const double perWg = 67.0 * (static_cast<double>(TW) * TH) / (960.0 * 720.0) + 9.3 * rw / 1208.0;
		const double reduce = 36.0 * (static_cast<double>(frames) * nx * ny * rw) / (32.0 * 12.0 * 1208.0);
		const double cost = rounds * perWg + reduce;
		if (split == first || cost < bestCost * 0.97) { best = split; bestCost = cost; }   // a finer grid has to win by 3 % (more partial windows, more memory)
	}
	int nx, ny, TW, TH; long long worst;
	if (!voteGridTables(W, H, sinQ, cosQ, best, nx, ny, TW, TH, worst, &kt, &rowBase)) return false;
	v.nx = nx; v.ny = ny; v.TW = TW; v.TH = TH; v.tiles = nx * ny;
	v.Rw = static_cast<int>(alignUp(static_cast<size_t>(worst), 16)); v.rwPitch = v.Rw;
	v.groups = groups; v.Tpad = v.groups * 64;
	v.tileCap = static_cast<size_t>(TW) * TH;
	return true;
}

ShtArgs shtArgs(compvhip_plan* p, int threshold)
{
	ShtArgs a;
	a.ebits = p->ebits; a.edges = p->edges; a.edgeCounts = p->edgeCounts; a.acc = p->acc;
	a.sinQ = p->sinQ; a.cosQ = p->cosQ; a.lineKeys = p->keysA; a.lineVals = p->valsA; a.lineCounts = p->lineCounts;
	a.frameTotals = p->frameTotals; a.lineTotal = p->lineTotal; a.sortN = 0; a.outCounts = nullptr; a.stepFlags = nullptr; a.hostStep = nullptr;
	a.nmsRange = p->nmsRange; a.blockCounts = p->blockCounts; a.lineBlocks = p->lineBlocks; a.nmsFlags = p->nmsFlags; a.nmsRows = static_cast<int>(sht_nms_rows(static_cast<int>(p->R))); a.nmsGroups = sht_nms_groups(static_cast<int>(p->T));
	a.bitsFrameStride = p->bitsFrameStride; a.edgeCap = p->edgeCap; a.accFrameStride = p->accFrameStride; a.lineCap = p->lineCap;
	a.W = static_cast<int>(p->W); a.H = static_cast<int>(p->H); a.wb = p->wb;
	a.R = static_cast<int>(p->R); a.T = static_cast<int>(p->T); a.accPitch = p->accPitch; a.barrier = static_cast<int>(p->W + p->H);
	a.threshold = threshold;
	a.nmsLastCol = static_cast<int>((p->T - 1) & ~static_cast<size_t>(3)); // quirk Q2: NMS covers theta columns [1, (T-1)&~3]
	a.frames = static_cast<int>(p->frames);
	a.strengthBits = p->strengthBits;
	return a;
}

// What one step carries from the function that decides it to the ones that use it.  The entry point (or runStepSync / runStepAsync) owns it; nothing of it
// outlives the call.
struct StepRun {
	uint8_t* patchOut = nullptr;   // (a view: the caller's edge buffer or tmpOut) the byte map the tile kernel writes and the resolve rounds patch
	uint8_t* copyBack = nullptr;   // in-place Canny (patchOut is tmpOut): the caller's buffer the finished map is copied to; nullptr otherwise
	int roundsUsed = 0;            // resolve rounds enqueued so far = the flag slot of the next one
	int* hostSlot = nullptr;       // asynchronous step: the ticket's pinned slot as the device sees it (ShtOpts::hostSlot); nullptr otherwise
};

int ensurePreproc(compvhip_plan* p)
{
	compvhip_ctx* ctx = p->ctx;
	HIPCHK(ctx, p->hist.reserve(ctx, static_cast<size_t>(256) * kOtsuMaxChunks * p->frames));
	HIPCHK(ctx, p->otsu.reserve(ctx, p->frames));
	return COMPVHIP_OK;
}

// thrMode: COMPVHIP_CANNY_THRESHOLD_* (per-frame device thresholds for PERCENT_OF_MEAN and OTSU)
int enqueueCanny(compvhip_plan* p, StepRun& run, const uint8_t* d_in, int tLow, int tHigh, int ksize, int thrMode, float fLow, float fHigh, hipStream_t st)
{
	compvhip_ctx* ctx = p->ctx;
	CannyArgs a;
	a.zero = nullptr; a.nZero = 0;
	a.in = d_in; a.out = run.patchOut; a.ebits = p->ebits; a.ubits = p->ubits; a.thrDev = (thrMode != COMPVHIP_CANNY_THRESHOLD_COMPARE_TO_GRADIENT) ? p->thrDev : nullptr;
	a.inFrameStride = p->S * p->H; a.outFrameStride = p->S * p->H; a.bitsFrameStride = p->bitsFrameStride;
	a.W = static_cast<int>(p->W); a.H = static_cast<int>(p->H); a.S = static_cast<int>(p->S); a.So = static_cast<int>(p->S);
	a.wb = p->wb; a.tilesX = p->tilesX; a.tilesY = p->tilesY; a.tLow = tLow; a.tHigh = tHigh; a.ksize = ksize;
	cannyCoverage(p->W, &a.simdEnd, &a.cStart);
	// coverage [1,simdEnd) U [cStart,W-1) equals the whole interior unless the two pieces leave a hole (W = 1 mod 16 ...)
	const bool gap = !((a.simdEnd >= a.W - 1) || (a.cStart <= a.simdEnd));
	if (thrMode == COMPVHIP_CANNY_THRESHOLD_OTSU) {
		int rc = ensurePreproc(p);
		if (rc) return rc;
		Stamp s(p, st, "otsu_kernels");
		HIPCHK(ctx, launch_otsu(d_in, a.W, a.H, a.S, a.inFrameStride, static_cast<int>(p->frames), fLow, fHigh, p->hist, p->otsu, p->thrDev, st));
	}
	if (thrMode == COMPVHIP_CANNY_THRESHOLD_PERCENT_OF_MEAN) {
		Stamp s(p, st, "canny_mean_thresholds");
		HIPCHK(ctx, launch_mean_thresholds(d_in, a.W, a.H, a.S, a.inFrameStride, static_cast<int>(p->frames), fLow, fHigh, p->sums, p->thrDev, st));
	}
	// ONE fill per step -- edge counts, line counts and the hysteresis round flags live in one allocation --, done by the first workgroups of the tile kernel
	// (round 6: the hipMemsetAsync it replaces was a launch of its own on the lane's chain)
	a.zero = p->counters; a.nZero = static_cast<int>(p->nCounts + kMaxRounds);
	p->countersFresh = true;
	run.roundsUsed = 0;
	{
		Stamp s(p, st, "canny_tile_kernel");
		HIPCHK(ctx, launch_canny_tiles(a, static_cast<int>(p->frames), gap, st));
	}
	return COMPVHIP_OK;
}

// `rounds` more resolve rounds, starting at run.roundsUsed; they patch the promoted pixels into run.patchOut
int enqueueResolve(compvhip_plan* p, StepRun& run, int rounds, hipStream_t st)
{
	compvhip_ctx* ctx = p->ctx;
	ResolveArgs r;
	r.ebits = p->ebits; r.ubits = p->ubits; r.out = run.patchOut; r.flags = p->flags; r.dirty = p->dirty;
	r.outFrameStride = p->S * p->H; r.bitsFrameStride = p->bitsFrameStride;
	r.H = static_cast<int>(p->H); r.So = static_cast<int>(p->S); r.wb = p->wb;
	for (int i = 0; i < rounds; ++i) {
		if (run.roundsUsed >= p->maxRounds) {
			// More border crossings than flag slots (a weak chain that zigzags across a band border needs one round per crossing): the
			// slots are reused.  The flood only ever adds pixels, so it terminates however many rounds that takes.  The sequence
			// continues as round 4 -- same dirty-flag generation as round maxRounds, a multiple of 4 -- behind a "changed" in slot 3.
			HIPCHK(ctx, hipMemsetAsync(p->flags + 3, 0, sizeof(int) * (p->maxRounds - 3), st));
			HIPCHK(ctx, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(p->flags + 3), 1, 1, st));
			run.roundsUsed = 4;
		}
		r.round = run.roundsUsed++;
		Stamp s(p, st, "canny_resolve_kernel");
		HIPCHK(ctx, launch_canny_resolve(r, static_cast<int>(p->frames), st));
	}
	return COMPVHIP_OK;
}

// true when the last enqueued round changed nothing (fixed point reached). Synchronises the stream.
int resolveConverged(compvhip_plan* p, const StepRun& run, hipStream_t st, bool* done)
{
	compvhip_ctx* ctx = p->ctx;
	const int last = run.roundsUsed - 1;
	HIPCHK(ctx, hipMemcpyAsync(p->hFlags, p->flags + last, sizeof(int), hipMemcpyDeviceToHost, st));
	HIPCHK(ctx, hipStreamSynchronize(st));
	*done = (p->hFlags[0] == 0);
	return COMPVHIP_OK;
}

} // namespace

int compvhip_api::shtDims(size_t W, size_t H, float thetaDeg, size_t* R, size_t* T, float* step)
{
	if (!W || !H || !(thetaDeg > 0.f)) return COMPVHIP_E_INVALID_PARAMETER;
	const float fTheta = thetaDeg * piOver180();
	const float fRho = 1.f;
	*R = static_cast<size_t>((static_cast<float>(((W + H) << 1) + 1) / fRho) + 0.5);
	*T = static_cast<size_t>((kPiF / fTheta) + 0.5);
	if (step) *step = fTheta;
	return COMPVHIP_OK;
}

int compvhip_api::ensureSht(compvhip_plan* p)
{
	if (p->shtReady) return COMPVHIP_OK;
	compvhip_ctx* ctx = p->ctx;
	// (a previous attempt may have failed half way, out of memory: shtReady is still false, and reserve reuses what that attempt allocated)
	size_t R, T; float step;
	int rc = shtDims(p->W, p->H, p->thetaDeg, &R, &T, &step);
	if (rc) return fail(ctx, rc, "invalid SHT geometry");
	if (T < 5) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "theta step too large (fewer than 5 theta bins)");
	if (!p->voteTiles) return fail(ctx, COMPVHIP_E_NOT_IMPLEMENTED, "no tile grid fits the vote windows of this geometry");
	p->R = R; p->T = T; p->thetaStep = step;
	p->accPitch = static_cast<int>(alignUp(R, 64));
	p->accFrameStride = static_cast<size_t>(p->accPitch) * T;
	std::vector<int32_t> s, c;
	shtTables(p->thetaDeg, T, s, c);
	HIPCHK(ctx, p->sinQ.reserve(ctx, T));
	HIPCHK(ctx, p->cosQ.reserve(ctx, T));
	HIPCHK(ctx, hipMemcpy(p->sinQ, s.data(), T * sizeof(int32_t), hipMemcpyHostToDevice));
	HIPCHK(ctx, hipMemcpy(p->cosQ, c.data(), T * sizeof(int32_t), hipMemcpyHostToDevice));
	{
		// toCartesian (houghsht.cxx:582): a = std::cos(theta), b = 1.f / std::sin(theta) with theta = col * thetaStep in f32
		// (separate libm calls: a compiler that fuses them into sincosf() changes cos by an ulp for some arguments)
		std::vector<float> ct(T), ist(T);
		for (size_t t = 0; t < T; ++t) {
			const float theta = static_cast<float>(t) * step;
			ct[t] = libmCosf(theta);
			ist[t] = 1.f / libmSinf(theta);
		}
		HIPCHK(ctx, p->cosT.reserve(ctx, T));
		HIPCHK(ctx, p->invSinT.reserve(ctx, T));
		HIPCHK(ctx, hipMemcpy(p->cosT, ct.data(), T * sizeof(float), hipMemcpyHostToDevice));
		HIPCHK(ctx, hipMemcpy(p->invSinT, ist.data(), T * sizeof(float), hipMemcpyHostToDevice));
	}
	{
		if (p->vt.tiles <= 0 || p->vtKt.size() != static_cast<size_t>(p->vt.tiles) * T) return fail(ctx, COMPVHIP_E_INVALID_STATE, "vote tiles were not planned");
		{
			// accumulator rows the NMS has to look at, per group of 8 theta columns (+ the column either side): the union of the tiles' windows
			const int tiles = p->vt.tiles, Rw = p->vt.Rw, groups = sht_nms_groups(static_cast<int>(T));
			std::vector<int2> range(static_cast<size_t>(groups));
			for (int g = 0; g < groups; ++g) {
				int lo = INT32_MAX, hi = INT32_MIN;
				for (int c = 8 * g - 1; c <= 8 * g + 8; ++c) {
					if (c < 0 || c >= static_cast<int>(T)) continue;
					for (int i = 0; i < tiles; ++i) {
						const int b = p->vtRowBase[static_cast<size_t>(i) * T + c];
						lo = std::min(lo, b); hi = std::max(hi, b + Rw);
					}
				}
				range[g] = make_int2(lo - 1, hi + 1);
			}
			std::vector<int2> reach(T);
			for (size_t t = 0; t < T; ++t) {
				int lo = INT32_MAX, hi = INT32_MIN;
				for (int i = 0; i < tiles; ++i) {
					const int b = p->vtRowBase[static_cast<size_t>(i) * T + t];
					lo = std::min(lo, b); hi = std::max(hi, b + Rw);
				}
				reach[t] = make_int2(lo, hi);
			}
			HIPCHK(ctx, p->reach.reserve(ctx, reach.size()));
			HIPCHK(ctx, hipMemcpy(p->reach, reach.data(), reach.size() * sizeof(int2), hipMemcpyHostToDevice));
			HIPCHK(ctx, p->nmsRange.reserve(ctx, range.size()));
			HIPCHK(ctx, hipMemcpy(p->nmsRange, range.data(), range.size() * sizeof(int2), hipMemcpyHostToDevice));
		}
		HIPCHK(ctx, p->dKt.reserve(ctx, p->vtKt.size()));
		HIPCHK(ctx, p->dRowBase.reserve(ctx, p->vtRowBase.size()));
		HIPCHK(ctx, hipMemcpy(p->dKt, p->vtKt.data(), p->vtKt.size() * sizeof(int32_t), hipMemcpyHostToDevice));
		HIPCHK(ctx, hipMemcpy(p->dRowBase, p->vtRowBase.data(), p->vtRowBase.size() * sizeof(int32_t), hipMemcpyHostToDevice));
		{
			// partial windows: one byte plane for the low bytes of the counts, one for the high bytes (only written / read for the few columns
			// that hold a count >= 256: a tile's share of a strong line), one flag byte per column
			const size_t cols = p->frames * p->vt.tiles * static_cast<size_t>(p->vt.Tpad);
			HIPCHK(ctx, p->partLo.reserve(ctx, cols * p->vt.rwPitch));
			HIPCHK(ctx, p->partHi.reserve(ctx, cols * p->vt.rwPitch));
			HIPCHK(ctx, p->colFlag.reserve(ctx, cols));
		}
		p->vt.kt = p->dKt; p->vt.rowBase = p->dRowBase; p->vt.partLo = p->partLo; p->vt.partHi = p->partHi; p->vt.colFlag = p->colFlag; p->vt.reach = p->reach; p->vt.tileCounts = p->tileCounts;
		p->edgeCap = static_cast<size_t>(p->vt.tiles) * p->vt.tileCap; // per frame: one list of TW * TH entries per tile
	}
	HIPCHK(ctx, p->edges.reserve(ctx, p->edgeCap * p->frames));
	HIPCHK(ctx, p->acc.reserve(ctx, p->accFrameStride * p->frames));
	HIPCHK(ctx, hipMemset(p->acc, 0, sizeof(uint16_t) * p->accFrameStride * p->frames)); // rows [Rp, accPitch) stay zero for ever
	// line key = frameTag | strength (strengthBits); the accumulator cell rides as the sort value (sht_nms / rank / emit kernels).  A cell of
	// column theta counts the pixels with (x*cosQ + y*sinQ) in one 65536-wide interval; max(|cosQ|,|sinQ|) >= 46340 so every x (or every y)
	// contributes at most 2 pixels: count <= 2*max(W,H).  Fewer key bits = fewer radix-sort passes.
	p->strengthBits = 1;
	while ((static_cast<size_t>(1) << p->strengthBits) <= 2 * (p->W > p->H ? p->W : p->H)) p->strengthBits++;
	if (p->strengthBits > 16) p->strengthBits = 16; // the accumulator itself is u16
	int frameBits = 0;
	while ((static_cast<size_t>(1) << frameBits) < p->frames) frameBits++;
	p->keyBits = frameBits + p->strengthBits;
	if (R * T >= (static_cast<size_t>(1) << 32)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "theta step too small: the accumulator has 2^32 cells or more"); // 32-bit cell values
	if (p->keyBits > 32) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "too many frames for a 32-bit line key");
	{
		const size_t frows = sht_nms_rows(static_cast<int>(R)), fgroups = static_cast<size_t>(sht_nms_groups(static_cast<int>(T)));
		HIPCHK(ctx, p->nmsFlags.reserve(ctx, frows * fgroups * p->frames));
		HIPCHK(ctx, hipMemset(p->nmsFlags, 0, frows * fgroups * p->frames)); // the NMS kernel skips the blocks no window reaches
		if (sht_lines_blocks(static_cast<int>(R)) != p->lineBlocks) return fail(ctx, COMPVHIP_E_INVALID_STATE, "row-block counters were sized for another accumulator");
	}
	p->shtReady = true;
	return COMPVHIP_OK;
}

int compvhip_api::ensureLineCap(compvhip_plan* p, size_t cap)
{
	compvhip_ctx* ctx = p->ctx;
	cap = std::min(cap, p->R * p->T);
	if (cap <= p->lineCap) return COMPVHIP_OK;
	p->lineCap = 0; p->deviceSort = false;   // (until everything below is there: a failed attempt runs again)
	// Each reserve replaces one buffer: while the keys grow, the smaller values, sort scratch and histograms of the old capacity are still there (the hand-written
	// version freed all seven first).  Same allocations, same sizes; the peak during a regrow is higher by at most the old capacity's buffers.
	HIPCHK(ctx, p->keysA.reserve(ctx, cap * p->frames));
	HIPCHK(ctx, p->keysB.reserve(ctx, cap * p->frames));
	HIPCHK(ctx, p->valsA.reserve(ctx, cap * p->frames));
	HIPCHK(ctx, p->valsB.reserve(ctx, cap * p->frames));
	size_t tb = 0;
	hipError_t e = sht_sort_pairs(nullptr, tb, p->keysA, p->keysB, p->valsA, p->valsB, cap * p->frames, p->keyBits, nullptr);
	if (e != hipSuccess) return fail(ctx, COMPVHIP_E_HIP, "radix sort size query", e);
	p->sortTempBytes = tb;
	HIPCHK(ctx, p->sortTemp.reserve(ctx, std::max<size_t>(tb, 16)));
	p->sortChunks = static_cast<int>((cap + kShtSortChunk - 1) / kShtSortChunk);
	if (p->strengthBits <= kShtSortMaxStrengthBits && p->sortChunks <= kShtSortMaxChunks) {
		HIPCHK(ctx, p->chunkHist.reserve(ctx, p->frames * static_cast<size_t>(p->sortChunks) << kShtSortMaxStrengthBits));
		HIPCHK(ctx, p->strengthStart.reserve(ctx, p->frames << kShtSortMaxStrengthBits));
		p->deviceSort = true;
	}
	else { p->chunkHist.release(); p->strengthStart.release(); }   // grown past the device sort: its tables are of no use any more
	p->lineCap = cap;
	p->recentTotals.reset();   // totals clamped to another capacity
	return COMPVHIP_OK;
}

int compvhip_api::validateCannyParams(compvhip_ctx* ctx, float tLow, float tHigh, int ksize, int type, int* lo, int* hi)
{
	if (ksize != 3 && ksize != 5) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "kernel size must be 3 or 5"); // canny_dete.cxx:101
	if (type != COMPVHIP_CANNY_THRESHOLD_COMPARE_TO_GRADIENT && type != COMPVHIP_CANNY_THRESHOLD_PERCENT_OF_MEAN && type != COMPVHIP_CANNY_THRESHOLD_OTSU)
		return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "invalid threshold type"); // :83
	if (type == COMPVHIP_CANNY_THRESHOLD_OTSU && !(tLow > 0.f)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "Otsu threshold factors must be > 0");
	if (tLow >= tHigh) return fail(ctx, COMPVHIP_E_INVALID_STATE, "tLow >= tHigh"); // :126
	*lo = 0; *hi = 0;
	if (type == COMPVHIP_CANNY_THRESHOLD_COMPARE_TO_GRADIENT) {
		gradientThresholds(tLow, tHigh, lo, hi);
		// the reference's SIMD leaves compare as signed int16 (intrin_avx2.cxx:144-147): thresholds above 32767 are an
		// artefact regime (g <= 24480) that this implementation rejects instead of reproducing
		if (*hi > 32767) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "thresholds above 32767 are not supported");
	}
	else if (type == COMPVHIP_CANNY_THRESHOLD_OTSU) { if (!(tHigh * 255.f < 32767.f)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "thresholds above 32767 are not supported"); }
	else if (!(tHigh * 255.f < 32767.f)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "thresholds above 32767 are not supported");
	return COMPVHIP_OK;
}

int compvhip_device_count(void)
{
	int n = 0;
	if (hipGetDeviceCount(&n) != hipSuccess) return 0;
	return n;
}

int compvhip_ctx_create(compvhip_ctx** out, int device)
{
	if (!out) return COMPVHIP_E_INVALID_PARAMETER;
	*out = nullptr;
	int n = 0;
	if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return COMPVHIP_E_NOT_INITIALIZED; // no GPU: fail loudly, no CPU fallback
	if (device < 0) { if (hipGetDevice(&device) != hipSuccess) return COMPVHIP_E_HIP; }
	if (device >= n) return COMPVHIP_E_INVALID_PARAMETER;
	if (hipSetDevice(device) != hipSuccess) return COMPVHIP_E_HIP;
	compvhip_ctx* ctx = new (std::nothrow) compvhip_ctx();
	if (!ctx) return COMPVHIP_E_OUT_OF_MEMORY;
	ctx->device = device;
	if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) { delete ctx; return COMPVHIP_E_HIP; }
	*out = ctx;
	return COMPVHIP_OK;
}

void compvhip_ctx_destroy(compvhip_ctx* ctx)
{
	if (!ctx) return;
	(void)hipSetDevice(ctx->device);
	if (ctx->hostPlan) compvhip_plan_destroy(ctx->hostPlan);   // first: it counts in ctx->live
	// the stream goes before the buffers do (by hand it went after them): every host entry point has drained it, hipStreamDestroy defers, hipFree synchronises
	if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
	delete ctx;   // the staging buffers and the KHT group state free themselves (the state borrowed the stream: it destroys none)
}

const char* compvhip_last_error(const compvhip_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }
long compvhip_live_allocations(const compvhip_ctx* ctx) { return ctx ? ctx->live.load() : 0; }
int compvhip_debug_alloc_fill(int byte)   // test hook: device_memory.hpp, allocFill
{
	if (byte < -1 || byte > 255) return COMPVHIP_E_INVALID_PARAMETER;
	return allocFill.exchange(byte);
}

int compvhip_houghsht_to_cartesian(size_t W, size_t H, const compvhip_line* lines, size_t n, float* out)
{
	if (!W || !H || (n && (!lines || !out))) return COMPVHIP_E_INVALID_PARAMETER; // houghsht.cxx:268
	const float widthF = static_cast<float>(W), heightF = static_cast<float>(H);
	const float r = std::sqrt((widthF * widthF) + (heightF * heightF));
	for (size_t i = 0; i < n; ++i, out += 4) {
		const float rho = lines[i].rho, theta = lines[i].theta;
		if (theta == 0.f) { out[0] = rho; out[1] = r; out[2] = rho; out[3] = -r; continue; }
		const float c = libmCosf(theta), inv = 1.f / libmSinf(theta);
		out[0] = 0.f; out[1] = rho * inv;
		out[2] = widthF; out[3] = (rho - (widthF * c)) * inv;
	}
	return COMPVHIP_OK;
}

int compvhip_houghkht_to_cartesian(size_t W, size_t H, const compvhip_line* lines, size_t n, float* out)
{
	if (!W || !H || (n && (!lines || !out))) return COMPVHIP_E_INVALID_PARAMETER; // houghkht.cxx:453
	const float widthF = static_cast<float>(W), heightF = static_cast<float>(H);
	const float r = std::sqrt((widthF * widthF) + (heightF * heightF));
	const float halfW = widthF * 0.5f, halfH = heightF * 0.5f;
	for (size_t i = 0; i < n; ++i, out += 4) {
		const float rho = lines[i].rho, theta = lines[i].theta;
		if (theta == 0.f) { out[0] = rho + halfW; out[1] = r; out[2] = rho + halfW; out[3] = -r; continue; }
		const float c = libmCosf(theta) * halfW, inv = 1.f / libmSinf(theta);
		out[0] = 0.f; out[1] = ((rho + c) * inv) + halfH;
		out[2] = widthF; out[3] = ((rho - c) * inv) + halfH;
	}
	return COMPVHIP_OK;
}

int compvhip_houghsht_vote_grid(size_t W, size_t H, float thetaDeg, size_t frames, int* nx, int* ny, int* windowRows)
{
	size_t R = 0, T = 0; float st = 0.f;
	if (!nx || !ny || !windowRows || !frames) return COMPVHIP_E_INVALID_PARAMETER;
	const int rc = shtDims(W, H, thetaDeg, &R, &T, &st);
	if (rc) return rc;
	if (T < 5) return COMPVHIP_E_NOT_IMPLEMENTED;
	std::vector<int32_t> sq, cq, kt, rb;
	shtTables(thetaDeg, T, sq, cq);
	ShtTileArgs v = {};
	if (!planVoteTiles(W, H, frames, sq, cq, v, kt, rb)) return COMPVHIP_E_NOT_IMPLEMENTED;
	*nx = v.nx; *ny = v.ny; *windowRows = v.Rw;
	return COMPVHIP_OK;
}

int compvhip_host_cpu_budget(void)
{
	return static_cast<int>(std::min<size_t>(hostCpuBudget(), 0x7fffffff));
}

int compvhip_houghsht_dims(size_t W, size_t H, float thetaDeg, size_t* R, size_t* T, float* step)
{
	if (!R || !T) return COMPVHIP_E_INVALID_PARAMETER;
	return shtDims(W, H, thetaDeg, R, T, step);
}

int compvhip_houghkht_dims(size_t W, size_t H, float rho, float thetaDeg, size_t* rhoN, size_t* T)
{
	KhtAxes ax;
	if (!rhoN || !T || !khtAxes(W, H, rho, thetaDeg, ax)) return COMPVHIP_E_INVALID_PARAMETER;
	*rhoN = ax.rhoN; *T = ax.T;
	return COMPVHIP_OK;
}

// ---- plans -------------------------------------------------------------------------------------------------------
int compvhip_plan_create(compvhip_ctx* ctx, size_t W, size_t H, size_t S, size_t frames, float thetaDeg, compvhip_plan** out)
{
	if (!ctx || !out) return COMPVHIP_E_INVALID_PARAMETER;
	*out = nullptr;
	// W,H >= 3: the convolution rejects images smaller than the kernel (compv_math_convlt.h:100); int16 coordinates in
	// the reference's hysteresis stack bound W,H <= 32767 (canny_dete.cxx:617-621)
	if (W < 3 || H < 3 || W > 32767 || H > 32767 || S < W || (S & 7) || !frames || !(thetaDeg > 0.f))
		return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "plan geometry (need 3 <= W,H <= 32767, S >= W, S % 8 == 0, frames > 0)");
	HIPCHK(ctx, hipSetDevice(ctx->device));
	compvhip_plan* p = new (std::nothrow) compvhip_plan();
	if (!p) return fail(ctx, COMPVHIP_E_OUT_OF_MEMORY, "plan");
	p->ctx = ctx; p->W = W; p->H = H; p->S = S; p->frames = frames; p->thetaDeg = thetaDeg;
	p->tilesX = static_cast<int>((W + 511) / 512);
	p->tilesY = static_cast<int>((H + 63) / 64);
	p->wb = p->tilesX * 16;
	p->bitsFrameStride = static_cast<size_t>(p->wb) * H;
	// one way out of a failure: the half-built plan is deleted, its buffers free themselves
	auto failed = [&](int rc) { compvhip_plan_destroy(p); return fail(ctx, rc, "plan allocation"); };
	if (p->ebits.reserve(ctx, p->bitsFrameStride * frames) != hipSuccess) return failed(COMPVHIP_E_OUT_OF_MEMORY);
	if (p->ubits.reserve(ctx, p->bitsFrameStride * frames) != hipSuccess) return failed(COMPVHIP_E_OUT_OF_MEMORY);
	// mask words past the last 496-column tile of a row are never written by the Canny kernel: they stay zero for ever
	if (hipMemset(p->ebits, 0, sizeof(uint32_t) * p->bitsFrameStride * frames) != hipSuccess) return failed(COMPVHIP_E_HIP);
	if (hipMemset(p->ubits, 0, sizeof(uint32_t) * p->bitsFrameStride * frames) != hipSuccess) return failed(COMPVHIP_E_HIP);
	// the fills run on the null stream; the plan's kernels may be enqueued on non-blocking streams that do not wait for it
	if (hipDeviceSynchronize() != hipSuccess) return failed(COMPVHIP_E_HIP);
	{
		p->voteTiles = true;
		size_t R = 0, T = 0; float step = 0.f;
		if (p->voteTiles && shtDims(W, H, thetaDeg, &R, &T, &step) == COMPVHIP_OK && T >= 5) {
			std::vector<int32_t> sq, cq;
			shtTables(thetaDeg, T, sq, cq);
			if (!planVoteTiles(W, H, frames, sq, cq, p->vt, p->vtKt, p->vtRowBase)) p->voteTiles = false;
		}
		else p->voteTiles = false;
		p->lineBlocks = p->voteTiles ? sht_lines_blocks(static_cast<int>(R)) : 0;
		p->nCounts = (2 + static_cast<size_t>(p->voteTiles ? p->vt.tiles : 0) + static_cast<size_t>(p->lineBlocks)) * frames + (frames + 1) * kFrameSlot;
	}
	if (p->counters.reserve(ctx, p->nCounts + kMaxRounds) != hipSuccess) return failed(COMPVHIP_E_OUT_OF_MEMORY);
	p->edgeCounts = p->counters; p->lineCounts = p->counters + frames; p->tileCounts = p->counters + 2 * frames; p->blockCounts = p->counters + (2 + static_cast<size_t>(p->voteTiles ? p->vt.tiles : 0)) * frames; p->flags = p->counters + p->nCounts;
	p->frameTotals = p->blockCounts + static_cast<size_t>(p->lineBlocks) * frames; p->lineTotal = reinterpret_cast<unsigned int*>(p->frameTotals + frames * kFrameSlot);
	if (const char* e = getenv("COMPVHIP_RESOLVE_WRAP")) { const int v = atoi(e); if (v >= 8 && v <= kMaxRounds && (v & 3) == 0) p->maxRounds = v; }
	p->traceRounds = getenv("COMPVHIP_TRACE_ROUNDS") != nullptr;
	if (hipMemset(p->counters, 0, sizeof(int) * (p->nCounts + kMaxRounds)) != hipSuccess) return failed(COMPVHIP_E_HIP);
	if (p->thrDev.reserve(ctx, frames) != hipSuccess) return failed(COMPVHIP_E_OUT_OF_MEMORY);
	if (p->dirty.reserve(ctx, canny_resolve_dirty_bytes(static_cast<int>(H), p->wb, static_cast<int>(frames))) != hipSuccess) return failed(COMPVHIP_E_OUT_OF_MEMORY);
	if (p->sums.reserve(ctx, frames * kFrameSlot) != hipSuccess) return failed(COMPVHIP_E_OUT_OF_MEMORY);
	if (p->hFlags.reserve(2) != hipSuccess) return failed(COMPVHIP_E_OUT_OF_MEMORY);
	p->hTotals = reinterpret_cast<unsigned int*>(p->hFlags + 1);
	if (p->hRounds.reserve(kSlotStride * kAsyncDepth, hipHostMallocMapped) != hipSuccess) return failed(COMPVHIP_E_OUT_OF_MEMORY);
	if (hipHostGetDevicePointer(reinterpret_cast<void**>(&p->hRoundsDev), p->hRounds, 0) != hipSuccess) return failed(COMPVHIP_E_HIP);
	*out = p;
	return COMPVHIP_OK;
}

void compvhip_plan_destroy(compvhip_plan* p)
{
	if (!p) return;
	compvhip_ctx* ctx = p->ctx;
	(void)hipSetDevice(ctx->device);
	timingTeardown(p);
	for (auto& stp : p->steps) if (stp.done) (void)hipEventDestroy(stp.done);
	delete p;   // every buffer frees itself; the batched KHT's states destroy their streams and events
}

int compvhip_plan_set_timing(compvhip_plan* p, int enabled)
{
	if (!p) return COMPVHIP_E_INVALID_PARAMETER;
	p->timing = (enabled >= 2 && enabled <= 4) ? enabled : (enabled != 0 ? 1 : 0);
	return COMPVHIP_OK;
}

int compvhip_plan_get_timing(compvhip_plan* p, const char** names, float* ms, int cap)
{
	if (!p) return COMPVHIP_E_INVALID_PARAMETER;
	return timingRead(p, p->ctx->device, names, ms, cap);
}

// The tile kernel writes E (edges so far), U (weak, unresolved) and the bytes of E; the resolve rounds finish the hysteresis on the
// masks and patch the promoted pixels into the byte map (run.patchOut; when in and out alias it is a scratch copy: a tile may still
// read the row halo a neighbour has overwritten).
static int planCannyImpl(compvhip_plan* p, StepRun& run, const uint8_t* d_in, float tLow, float tHigh, int ksize, int type, uint8_t* d_edges, hipStream_t st,
                         bool waitConverged, bool clearTimeline = true)
{
	compvhip_ctx* ctx = p->ctx;
	if (!d_in || !d_edges) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "null frame pointer");
	int lo, hi;
	int rc = validateCannyParams(ctx, tLow, tHigh, ksize, type, &lo, &hi);
	if (rc) return rc;
	HIPCHK(ctx, hipSetDevice(ctx->device));
	if (p->timing && clearTimeline) timelineClear(p);
	const size_t bytes = p->S * p->H * p->frames;
	const bool alias = overlaps(d_in, bytes, d_edges, bytes);
	if (alias) HIPCHK(ctx, p->tmpOut.reserve(ctx, bytes));
	run.patchOut = alias ? p->tmpOut : d_edges;
	run.copyBack = alias ? d_edges : nullptr;
	if (p->W < static_cast<size_t>(ksize) || p->H < static_cast<size_t>(ksize)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "image smaller than the kernel"); // compv_math_convlt.h:100
	rc = enqueueCanny(p, run, d_in, lo, hi, ksize, type, tLow, tHigh, st);
	if (rc) return rc;
	rc = enqueueResolve(p, run, waitConverged ? kSpecRounds : p->specRounds, st);
	if (rc) return rc;
	if (waitConverged) {
		for (;;) {
			bool done = false;
			rc = resolveConverged(p, run, st, &done);
			if (rc) return rc;
			if (done) break;
			rc = enqueueResolve(p, run, kSpecRounds, st);
			if (rc) return rc;
		}
	}
	if (run.copyBack) HIPCHK(ctx, hipMemcpyAsync(run.copyBack, run.patchOut, bytes, hipMemcpyDeviceToDevice, st));
	p->bitsValid = true;
	return COMPVHIP_OK;
}

int compvhip_plan_canny(compvhip_plan* p, const uint8_t* d_in, float tLow, float tHigh, int ksize, int type, uint8_t* d_edges, void* stream)
{
	if (!p) return COMPVHIP_E_INVALID_PARAMETER;
	if (int rc = refuseBeyondLaunchLimit(p->ctx, p->frames, "compvhip_plan_canny")) return rc;
	StepRun run;
	return planCannyImpl(p, run, d_in, tLow, tHigh, ksize, type, d_edges, static_cast<hipStream_t>(stream), true);
}

int compvhip_api::pixfmtBytes(int fmt)
{
	if (fmt < COMPVHIP_FMT_RGBA32 || fmt > COMPVHIP_FMT_Y) return 0;
	return fmt <= COMPVHIP_FMT_BGRA32 ? 4 : (fmt <= COMPVHIP_FMT_BGR24 ? 3 : (fmt == COMPVHIP_FMT_Y ? 1 : 2));
}

int compvhip_api::checkPixfmt(compvhip_ctx* ctx, int fmt, size_t W)
{
	if (fmt > COMPVHIP_FMT_Y && fmt <= COMPVHIP_FMT_HSV) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "a format of the colour conversion calls only (compvhip_convert_frames)");
	if (!pixfmtBytes(fmt)) return fail(ctx, COMPVHIP_E_NOT_IMPLEMENTED, "pixel format without a grayscale conversion"); // conv_to_grayscale.cxx:86-88
	if ((fmt == COMPVHIP_FMT_YUYV422 || fmt == COMPVHIP_FMT_UYVY422) && (W & 1)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "packed 4:2:2 needs an even width");
	return COMPVHIP_OK;
}

int compvhip_plan_grayscale(compvhip_plan* p, const uint8_t* d_in, int pixfmt, uint8_t* d_gray, void* stream)
{
	if (!p) return COMPVHIP_E_INVALID_PARAMETER;
	compvhip_ctx* ctx = p->ctx;
	if (!d_in || !d_gray) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "null frame pointer");
	const int rc = checkPixfmt(ctx, pixfmt, p->W);
	if (rc) return rc;
	HIPCHK(ctx, hipSetDevice(ctx->device));
	hipStream_t st = static_cast<hipStream_t>(stream);
	if (p->timing) timelineClear(p);
	GrayArgs a;
	a.in = d_in; a.out = d_gray; a.W = static_cast<int>(p->W); a.H = static_cast<int>(p->H); a.S = static_cast<int>(p->S); a.So = static_cast<int>(p->S);
	Stamp s(p, st, "gray_kernel");
	HIPCHK(ctx, launch_gray(a, pixfmt, static_cast<int>(p->frames), st));
	return COMPVHIP_OK;
}

int compvhip_plan_otsu(compvhip_plan* p, const uint8_t* d_gray, int32_t* d_thresholds, void* stream)
{
	if (!p) return COMPVHIP_E_INVALID_PARAMETER;
	compvhip_ctx* ctx = p->ctx;
	if (!d_gray || !d_thresholds) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "null pointer");
	if (misaligned(3, d_thresholds)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "levels must be 4-byte aligned");
	HIPCHK(ctx, hipSetDevice(ctx->device));
	int rc = ensurePreproc(p);
	if (rc) return rc;
	hipStream_t st = static_cast<hipStream_t>(stream);
	if (p->timing) timelineClear(p);
	Stamp s(p, st, "otsu_kernels");
	HIPCHK(ctx, launch_otsu(d_gray, static_cast<int>(p->W), static_cast<int>(p->H), static_cast<int>(p->S), p->S * p->H, static_cast<int>(p->frames), 0.5f, 1.f,
	                        p->hist, d_thresholds, nullptr, st));
	return COMPVHIP_OK;
}

int compvhip_api::checkFxpKernel(compvhip_ctx* ctx, size_t W, size_t H, const uint16_t* vt, const uint16_t* hz, size_t k)
{
	if (!vt || !hz || !(k & 1) || W < k || H < k) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "convolution kernel: null, even size or larger than the image"); // compv_math_convlt.h:100
	if (k < 3 || k > static_cast<size_t>(kFxpMaxTaps)) return fail(ctx, COMPVHIP_E_NOT_IMPLEMENTED, "fixed-point convolution supports kernel sizes 3..15");
	return COMPVHIP_OK;
}

int compvhip_plan_convlt1_fixedpoint(compvhip_plan* p, const uint8_t* d_in, const uint16_t* vtKern, const uint16_t* hzKern, size_t kernSize, uint8_t* d_out,
                                     void* stream)
{
	if (!p) return COMPVHIP_E_INVALID_PARAMETER;
	compvhip_ctx* ctx = p->ctx;
	if (!d_in || !d_out) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "null frame pointer");
	int rc = refuseBeyondLaunchLimit(ctx, p->frames, "compvhip_plan_convlt1_fixedpoint");
	if (rc) return rc;
	rc = checkFxpKernel(ctx, p->W, p->H, vtKern, hzKern, kernSize);
	if (rc) return rc;
	HIPCHK(ctx, hipSetDevice(ctx->device));
	const size_t span = p->S * p->H * p->frames;
	const bool alias = overlaps(d_in, span, d_out, span);
	if (alias) HIPCHK(ctx, p->blurTmp.reserve(ctx, span)); // only the in-place call needs the two-pass path
	hipStream_t st = static_cast<hipStream_t>(stream);
	if (p->timing) timelineClear(p);
	Stamp s(p, st, "convlt_fxp_kernels");
	HIPCHK(ctx, launch_convlt_fxp(d_in, p->blurTmp, d_out, static_cast<int>(p->W), static_cast<int>(p->H), static_cast<int>(p->S), p->S * p->H,
	                              static_cast<int>(p->frames), vtKern, hzKern, static_cast<int>(kernSize), st));
	return COMPVHIP_OK;
}

int compvhip_plan_edge_dete(compvhip_plan* p, const uint8_t* d_in, int op, uint8_t* d_out, void* stream)
{
	if (!p) return COMPVHIP_E_INVALID_PARAMETER;
	compvhip_ctx* ctx = p->ctx;
	if (!d_in || !d_out) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "null frame pointer");
	if (op != COMPVHIP_OP_SOBEL && op != COMPVHIP_OP_SCHARR && op != COMPVHIP_OP_PREWITT)
		return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "invalid detector id"); // edge_dete.cxx:246
	const size_t bytes = p->S * p->H * p->frames;
	if (overlaps(d_in, bytes, d_out, bytes)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "d_in and d_out must not alias");
	HIPCHK(ctx, hipSetDevice(ctx->device));
	hipStream_t st = static_cast<hipStream_t>(stream);
	if (p->timing) timelineClear(p);
	EdgeDeteArgs a;
	a.in = d_in; a.out = d_out; a.gmax = p->sums;
	a.inFrameStride = p->S * p->H; a.outFrameStride = p->S * p->H;
	a.W = static_cast<int>(p->W); a.H = static_cast<int>(p->H); a.S = static_cast<int>(p->S); a.So = static_cast<int>(p->S);
	a.tilesX = p->tilesX; a.tilesY = p->tilesY;
	Stamp s(p, st, "edge_dete_kernels");
	HIPCHK(ctx, launch_edge_dete(a, op, static_cast<int>(p->frames), st));
	return COMPVHIP_OK;
}

// o.sortN: kSortAll, kSortExact or a number of key slots (api_internal.hpp)
int compvhip_api::planShtImpl(compvhip_plan* p, const uint8_t* d_edges, int threshold, int maxLines, compvhip_line* d_lines, size_t lineCap, int32_t* d_counts,
                              hipStream_t st, const ShtOpts& o)
{
	compvhip_ctx* ctx = p->ctx;
	if (threshold <= 0) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "threshold must be > 0"); // houghsht.cxx:82
	if (misaligned(3, d_lines, d_counts)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "lines and counts must be 4-byte aligned");
	if (!d_edges && !p->bitsValid) return fail(ctx, COMPVHIP_E_INVALID_STATE, "no edge masks: run compvhip_plan_canny first or pass d_edges");
	HIPCHK(ctx, hipSetDevice(ctx->device));
	int rc = ensureSht(p);
	if (rc) return rc;
	rc = ensureLineCap(p, std::max(lineCap, kMinLineCap));
	if (rc) return rc;
	if (p->timing && o.clearTimeline) timelineClear(p);
	const int frames = static_cast<int>(p->frames);
	size_t sortN = o.sortN;
	if (d_edges) {
		Stamp s(p, st, "bytes_to_bits_kernel");
		HIPCHK(ctx, launch_bytes_to_bits(d_edges, static_cast<int>(p->W), static_cast<int>(p->H), static_cast<int>(p->S), p->S * p->H, p->ebits, p->wb,
		                                 p->bitsFrameStride, frames, st));
		p->bitsValid = false; // U masks no longer match
	}
	ShtArgs a = shtArgs(p, threshold);
	a.outCounts = d_counts;   // written by sht_lines_kernel together with the plan's own counts (was a device copy behind the sort)
	a.hostStep = o.hostSlot; a.stepFlags = p->flags;   // asynchronous steps: line total + round flags straight into the ticket's pinned slot
	const size_t capAll = p->lineCap * p->frames;
	const bool deviceSort = p->deviceSort && !o.pairsOnly;   // every size read on the device: nothing to predict, nothing to pad
	if (sortN != kSortExact) sortN = std::min(sortN, capAll);
	a.sortN = (o.pairsOnly || deviceSort || sortN == kSortExact) ? 0 : sortN;
	if (!p->countersFresh) HIPCHK(ctx, hipMemsetAsync(p->counters, 0, sizeof(int) * p->nCounts, st)); // edge, line and tile counts
	p->countersFresh = false;
	{ Stamp s(p, st, "sht_compact_kernel"); HIPCHK(ctx, launch_sht_compact_tiles(a, p->vt, frames, st)); }
	{ Stamp s(p, st, "sht_vote_kernel"); HIPCHK(ctx, launch_sht_vote_tiles(a, p->vt, frames, st)); }
	{ Stamp s(p, st, "sht_reduce_kernel"); HIPCHK(ctx, launch_sht_reduce_tiles(a, p->vt, frames, st)); }
	{ Stamp s(p, st, "sht_lines_kernel"); HIPCHK(ctx, launch_sht_lines(a, frames, st)); }
	// pairsOnly (the host entry point): stop at the (key, cell) pairs in emission order -- the caller orders them itself (referenceLineOrder)
	if (o.pairsOnly) {
		return COMPVHIP_OK;
	}
	if (deviceSort) {
		if (d_lines && lineCap) {
			Stamp s(p, st, "sht_sort_lines");
			ShtSortArgs q;
			q.rankKeys = p->keysB; q.chunkHist = p->chunkHist; q.strengthStart = p->strengthStart; q.chunks = p->sortChunks;
			HIPCHK(ctx, launch_sht_sort_lines(a, q, frames, p->thetaStep, maxLines, d_lines, lineCap, st));
		}
		return COMPVHIP_OK;
	}
	// Invariant of the library-sort fallback: nothing reads keysB / valsB beyond lineTotal (the decode kernel stops at the clamped per-frame counts), so the
	// slots [sortN, capAll) are neither sorted nor cleared and may hold a previous step's pairs.
	if (sortN == kSortExact) {
		HIPCHK(ctx, hipMemcpyAsync(p->hTotals, p->lineTotal, sizeof(unsigned int), hipMemcpyDeviceToHost, st));
		HIPCHK(ctx, hipStreamSynchronize(st));
		sortN = std::min(static_cast<size_t>(p->hTotals[0]), capAll);
	}
	if (sortN) {
		Stamp s(p, st, "sht_sort_lines");
		size_t tb = p->sortTempBytes;
		hipError_t e = sht_sort_pairs(p->sortTemp, tb, p->keysA, p->keysB, p->valsA, p->valsB, sortN, p->keyBits, st);
		if (e != hipSuccess) return fail(ctx, COMPVHIP_E_HIP, "radix sort", e);
	}
	if (d_lines && lineCap) {
		Stamp s(p, st, "sht_decode_kernel");
		HIPCHK(ctx, launch_sht_decode(p->keysB, p->valsB, p->lineCounts, p->lineCap, frames, static_cast<int>(p->T), static_cast<int>(p->W + p->H), p->thetaStep, maxLines,
		                              p->strengthBits, d_lines, lineCap, st));
	}
	return COMPVHIP_OK;
}

int compvhip_plan_houghsht(compvhip_plan* p, const uint8_t* d_edges, int threshold, int maxLines, compvhip_line* d_lines, size_t lineCap,
                           int32_t* d_counts, void* stream)
{
	if (!p) return COMPVHIP_E_INVALID_PARAMETER;
	if (int rc = refuseBeyondLaunchLimit(p->ctx, p->frames, "compvhip_plan_houghsht")) return rc;
	return planShtImpl(p, d_edges, threshold, maxLines, d_lines, lineCap, d_counts, static_cast<hipStream_t>(stream), ShtOpts());
}

// ---- the step: [grayscale ->] Canny (any kernel size / threshold mode) -> SHT [-> toCartesian], one enqueue ----------------------
static int checkStep(compvhip_plan* p, const StepParams& sp)
{
	compvhip_ctx* ctx = p->ctx;
	int rc = refuseBeyondLaunchLimit(ctx, p->frames, "compvhip_plan_pipeline");   // the Canny resolve and the SHT stage are not sliced
	if (rc) return rc;
	if (!sp.d_in || !sp.d_edges) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "null frame pointer");
	rc = checkPixfmt(ctx, sp.pixfmt, p->W);   // (COMPVHIP_FMT_Y passes: one byte, any width)
	if (rc) return rc;
	if (sp.d_cart && (!sp.d_lines || !sp.d_counts)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "toCartesian needs the line and count buffers");
	if (misaligned(3, sp.d_lines, sp.d_counts, sp.d_otsu, sp.d_cart)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "lines, counts, levels and endpoints must be 4-byte aligned");
	return COMPVHIP_OK;
}

// everything up to (not including) the convergence check, on `st`
static int enqueueStep(compvhip_plan* p, StepRun& run, const StepParams& sp, hipStream_t st, bool clearTimeline)
{
	compvhip_ctx* ctx = p->ctx;
	HIPCHK(ctx, hipSetDevice(ctx->device));   // before the scratch allocation below: the caller's current device may be another GPU
	const uint8_t* luma = sp.d_in;
	if (sp.pixfmt != COMPVHIP_FMT_Y) {
		// samples/hough_lines/main.cxx:102: CompVImage::convertGrayscale in front of everything else
		uint8_t* gray = sp.d_gray;
		if (!gray) {
			HIPCHK(ctx, p->grayTmp.reserve(ctx, p->S * p->H * p->frames));
			gray = p->grayTmp;
		}
		if (p->timing && clearTimeline) timelineClear(p);
		clearTimeline = false;
		GrayArgs a;
		a.in = sp.d_in; a.out = gray; a.W = static_cast<int>(p->W); a.H = static_cast<int>(p->H); a.S = static_cast<int>(p->S); a.So = static_cast<int>(p->S);
		Stamp s(p, st, "gray_kernel");
		HIPCHK(ctx, launch_gray(a, sp.pixfmt, static_cast<int>(p->frames), st));
		luma = gray;
	}
	int rc = planCannyImpl(p, run, luma, sp.tLow, sp.tHigh, sp.ksize, sp.thresholdType, sp.d_edges, st, false, clearTimeline);
	if (rc) return rc;
	if (sp.d_otsu && sp.thresholdType == COMPVHIP_CANNY_THRESHOLD_OTSU)
		HIPCHK(ctx, hipMemcpyAsync(sp.d_otsu, p->otsu, sizeof(int32_t) * p->frames, hipMemcpyDeviceToDevice, st));
	return COMPVHIP_OK;
}

static int toCartesianImpl(compvhip_plan* p, const compvhip_line* d_lines, const int32_t* d_counts, size_t lineCap, int maxLines, float* d_cart, void* stream);

static int enqueueStepTail(compvhip_plan* p, const StepRun& run, const StepParams& sp, hipStream_t st, size_t sortN)
{
	ShtOpts o;
	o.clearTimeline = false; o.sortN = sortN; o.hostSlot = run.hostSlot;
	int rc = planShtImpl(p, nullptr, sp.threshold, sp.maxLines, sp.d_lines, sp.lineCap, sp.d_counts, st, o);
	if (rc) return rc;
	if (sp.d_cart) {
		rc = toCartesianImpl(p, sp.d_lines, sp.d_counts, sp.lineCap, sp.maxLines, sp.d_cart, st);   // d_counts = the UNCUT counts; only min(count, lineCap, maxLines) slots were decoded
		if (rc) return rc;
	}
	return COMPVHIP_OK;
}

static int runStepSync(compvhip_plan* p, const StepParams& sp, hipStream_t st)
{
	// Everything is enqueued back to back (speculative resolve rounds included); the convergence flag is checked once at the end and,
	// in the rare case the hysteresis needed more rounds, the tail is replayed.
	StepRun run;
	int rc = enqueueStep(p, run, sp, st, true);
	if (rc) return rc;
	const size_t bytes = p->S * p->H * p->frames;
	for (;;) {
		rc = enqueueStepTail(p, run, sp, st, kSortExact);
		if (rc) return rc;
		bool done = false;
		rc = resolveConverged(p, run, st, &done);
		if (rc) return rc;
		if (done) break;
		do {
			rc = enqueueResolve(p, run, kSpecRounds, st);
			if (rc) return rc;
			rc = resolveConverged(p, run, st, &done);
			if (rc) return rc;
		} while (!done);
		if (run.copyBack) HIPCHK(p->ctx, hipMemcpyAsync(run.copyBack, run.patchOut, bytes, hipMemcpyDeviceToDevice, st));
		// replay of the Hough stage on the now final masks
	}
	return COMPVHIP_OK;
}

// The step without its host round trip.  What compvhip_plan_wait() needs -- the step's line total and its first four round flags -- is written by
// sht_lines_kernel straight into the ticket's pinned, device-mapped slot and looked at there, normally while the NEXT step is already running: no copy behind
// the step's kernels (rounds 2-5: three device-to-host copies, a device copy of the counts and a fill per step -- 30 us of stream operations between the last
// kernel of a step and the first of the next on a lane, 5 now).
static int runStepAsync(compvhip_plan* p, const StepParams& sp, hipStream_t st, int* ticket)
{
	compvhip_ctx* ctx = p->ctx;
	*ticket = -1;
	int slot = -1;
	for (int i = 0; i < kAsyncDepth; ++i) if (!p->steps[i].used) { slot = i; break; }
	if (slot < 0) return fail(ctx, COMPVHIP_E_INVALID_STATE, "too many steps in flight: call compvhip_plan_wait first");
	const size_t bytes = p->S * p->H * p->frames;
	const size_t inBytes = bytes * static_cast<size_t>(sp.pixfmt == COMPVHIP_FMT_Y ? 1 : pixfmtBytes(sp.pixfmt));
	if (overlaps(sp.d_in, inBytes, sp.d_edges, bytes))
		return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "the asynchronous step needs distinct input and edge buffers"); // a replay re-reads d_in
	compvhip_plan::AsyncStep& stp = p->steps[slot];
	HIPCHK(ctx, hipSetDevice(ctx->device));
	if (!stp.done) HIPCHK(ctx, hipEventCreateWithFlags(&stp.done, hipEventDisableTiming));
	// timing events of asynchronous steps accumulate until compvhip_plan_get_timing reads them; beyond kMaxTimeline entries the oldest go
	if (p->timeline.size() > kMaxTimeline) timelineClear(p);
	// The slot belongs to no step in flight.  Until this step's sht_lines_kernel writes it, it says "replay" (stepVerdict): a step whose lines kernel never ran
	// is run again by compvhip_plan_wait, not accepted with the previous step's numbers.
	int* slotHost = p->hRounds + kSlotStride * slot;
	slotHost[kSlotTotal] = ~0;
	for (int i = 0; i < 4; ++i) slotHost[kSlotFlags + i] = 1;
	StepRun run;
	run.hostSlot = p->hRoundsDev + kSlotStride * slot;
	int rc = enqueueStep(p, run, sp, st, false);
	if (rc) return rc;
	// (capacities first: ensureLineCap may grow the key buffers and reset recentTotals -- totals clamped to the old capacity predict nothing)
	rc = ensureSht(p);
	if (rc) return rc;
	rc = ensureLineCap(p, std::max(sp.lineCap, kMinLineCap));
	if (rc) return rc;
	const size_t capAll = p->lineCap * p->frames;
	const size_t sortN = p->deviceSort ? capAll : asyncSortRange(p->recentTotals, capAll);   // (sized on the device: no prediction to check)
	static_assert(kMaxRounds >= 4 && kSpecRounds <= 4, "the round flags compvhip_plan_wait looks at");
	if (run.roundsUsed > 4) return fail(ctx, COMPVHIP_E_INVALID_STATE, "more speculative rounds than flags the step reports");
	rc = enqueueStepTail(p, run, sp, st, sortN);
	if (rc) return rc;
	HIPCHK(ctx, hipEventRecord(stp.done, st));
	stp.used = true; stp.replay = false; stp.seq = ++p->stepSeq; stp.stream = st; stp.sp = sp; stp.sortN = sortN; stp.rounds = run.roundsUsed;
	*ticket = slot;
	return COMPVHIP_OK;
}

static StepParams classicStep(const uint8_t* d_in, float tLow, float tHigh, int threshold, int maxLines, uint8_t* d_edges, compvhip_line* d_lines, size_t lineCap,
                              int32_t* d_counts)
{
	StepParams sp;
	sp.d_in = d_in; sp.tLow = tLow; sp.tHigh = tHigh; sp.threshold = threshold; sp.maxLines = maxLines; sp.d_edges = d_edges; sp.d_lines = d_lines;
	sp.lineCap = lineCap; sp.d_counts = d_counts;
	return sp;
}

int compvhip_plan_pipeline(compvhip_plan* p, const uint8_t* d_in, float tLow, float tHigh, int threshold, int maxLines, uint8_t* d_edges,
                           compvhip_line* d_lines, size_t lineCap, int32_t* d_counts, void* stream)
{
	if (!p) return COMPVHIP_E_INVALID_PARAMETER;
	const StepParams sp = classicStep(d_in, tLow, tHigh, threshold, maxLines, d_edges, d_lines, lineCap, d_counts);
	int rc = checkStep(p, sp);
	if (rc) return rc;
	return runStepSync(p, sp, static_cast<hipStream_t>(stream));
}

int compvhip_plan_pipeline_async(compvhip_plan* p, const uint8_t* d_in, float tLow, float tHigh, int threshold, int maxLines, uint8_t* d_edges,
                                 compvhip_line* d_lines, size_t lineCap, int32_t* d_counts, void* stream, int* ticket)
{
	if (!p || !ticket) return COMPVHIP_E_INVALID_PARAMETER;
	const StepParams sp = classicStep(d_in, tLow, tHigh, threshold, maxLines, d_edges, d_lines, lineCap, d_counts);
	*ticket = -1;
	int rc = checkStep(p, sp);
	if (rc) return rc;
	return runStepAsync(p, sp, static_cast<hipStream_t>(stream), ticket);
}

int compvhip_plan_pipeline_ex(compvhip_plan* p, const uint8_t* d_in, const compvhip_pipeline_opts* o, uint8_t* d_edges, compvhip_line* d_lines, size_t lineCap,
                              int32_t* d_counts, void* stream, int* ticket)
{
	if (!p) return COMPVHIP_E_INVALID_PARAMETER;
	if (ticket) *ticket = -1;
	if (!o) return fail(p->ctx, COMPVHIP_E_INVALID_PARAMETER, "null options");
	StepParams sp = classicStep(d_in, o->tLow, o->tHigh, o->threshold, o->maxLines, d_edges, d_lines, lineCap, d_counts);
	sp.ksize = o->ksize ? o->ksize : 3; sp.thresholdType = o->thresholdType; sp.pixfmt = o->pixfmt;
	sp.d_gray = o->d_gray; sp.d_otsu = o->d_otsu; sp.d_cart = o->d_cart;
	int rc = checkStep(p, sp);
	if (rc) return rc;
	return ticket ? runStepAsync(p, sp, static_cast<hipStream_t>(stream), ticket) : runStepSync(p, sp, static_cast<hipStream_t>(stream));
}

int compvhip_plan_wait(compvhip_plan* p, int ticket)
{
	if (!p || ticket < 0 || ticket >= kAsyncDepth || !p->steps[ticket].used) return COMPVHIP_E_INVALID_PARAMETER;
	compvhip_ctx* ctx = p->ctx;
	compvhip_plan::AsyncStep& stp = p->steps[ticket];
	HIPCHK(ctx, hipSetDevice(ctx->device));
	HIPCHK(ctx, hipEventSynchronize(stp.done));
	stp.used = false;
	const int* stepOut = p->hRounds + kSlotStride * ticket;   // what the step's sht_lines_kernel wrote into the ticket's pinned slot (or, if it never ran, runStepAsync's reset)
	const unsigned int total = static_cast<unsigned int>(stepOut[kSlotTotal]);
	const int* rf = stepOut + kSlotFlags;
	const StepVerdict v = stepVerdict(stp.rounds, rf, total, stp.sortN, stp.replay);
	p->recentTotals.push(total);
	p->recentRounds.push(static_cast<unsigned int>(v.needed));
	p->specRounds = nextSpecRounds(p->recentRounds);
	if (p->traceRounds) fprintf(stderr, "plan %p ticket %d: rounds enqueued %d, flags %d %d %d %d, needed %d -> next %d\n", (void*)p, ticket, stp.rounds, rf[0], rf[1], rf[2], rf[3], v.needed, p->specRounds);
	if (!v.replay) return COMPVHIP_OK; // the speculative rounds reached the fixed point and the sort covered the lines (the usual case)
	// Rare: the hysteresis of this step needed more rounds than were enqueued (or it produced more lines than the sorted range held), and a later step may
	// already have reused the plan's masks.  Let the stream drain and run the step again, synchronously, from its (unmodified) input.  The replay writes this
	// step's output buffers AFTER the later steps of the plan ran: if they share those buffers (a caller that only consumes the newest
	// result), their results are gone -- every step enqueued after this one is therefore replayed as well when it is waited for, in order.
	HIPCHK(ctx, hipStreamSynchronize(stp.stream));
	for (int i = 0; i < kAsyncDepth; ++i)
		if (p->steps[i].used && p->steps[i].seq > stp.seq) p->steps[i].replay = true;
	stp.replay = false;
	return runStepSync(p, stp.sp, stp.stream);
}

int compvhip_plan_to_cartesian(compvhip_plan* p, const compvhip_line* d_lines, const int32_t* d_counts, size_t lineCap, float* d_cart, void* stream)
{
	return toCartesianImpl(p, d_lines, d_counts, lineCap, 0, d_cart, stream);
}

// maxLines > 0: d_counts holds the uncut line counts of a step that decoded only the first maxLines lines of every frame
static int toCartesianImpl(compvhip_plan* p, const compvhip_line* d_lines, const int32_t* d_counts, size_t lineCap, int maxLines, float* d_cart, void* stream)
{
	if (!p) return COMPVHIP_E_INVALID_PARAMETER;
	compvhip_ctx* ctx = p->ctx;
	if (!d_lines || !d_counts || !d_cart) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "null pointer");
	if (misaligned(3, d_lines, d_counts, d_cart)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "lines, counts and endpoints must be 4-byte aligned");
	int rc = refuseBeyondLaunchLimit(ctx, p->frames, "compvhip_plan_to_cartesian");
	if (rc) return rc;
	HIPCHK(ctx, hipSetDevice(ctx->device));
	rc = ensureSht(p);
	if (rc) return rc;
	const float widthF = static_cast<float>(p->W), heightF = static_cast<float>(p->H);
	const float r = std::sqrt((widthF * widthF) + (heightF * heightF)); // houghsht.cxx:570
	HIPCHK(ctx, launch_sht_cartesian(d_lines, d_counts, lineCap, maxLines, static_cast<int>(p->frames), static_cast<int>(p->T), p->cosT, p->invSinT, p->thetaStep, widthF, r, d_cart,
	                                 static_cast<hipStream_t>(stream)));
	return COMPVHIP_OK;
}

int compvhip_plan_acc(compvhip_plan* p, size_t frame, const uint16_t** d_acc, size_t* R, size_t* T, size_t* accPitch)
{
	if (!p || !p->shtReady || frame >= p->frames) return COMPVHIP_E_INVALID_PARAMETER;
	if (d_acc) *d_acc = p->acc + frame * p->accFrameStride;
	if (R) *R = p->R;
	if (T) *T = p->T;
	if (accPitch) *accPitch = static_cast<size_t>(p->accPitch);
	return COMPVHIP_OK;
}

int compvhip_plan_acc_export(compvhip_plan* p, size_t frame, int32_t* d_out, size_t outStride, void* stream)
{
	if (!p) return COMPVHIP_E_INVALID_PARAMETER;
	compvhip_ctx* ctx = p->ctx;
	// (a single frame, no frame index in the grid; but no call that fills the accumulators accepts such a plan: there is nothing to export)
	if (int rc = refuseBeyondLaunchLimit(ctx, p->frames, "compvhip_plan_acc_export")) return rc;
	if (misaligned(3, d_out)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "the accumulator copy must be 4-byte aligned");
	if (!p->shtReady || frame >= p->frames || !d_out || outStride < p->T) return COMPVHIP_E_INVALID_PARAMETER;
	HIPCHK(ctx, hipSetDevice(ctx->device));
	HIPCHK(ctx, launch_sht_acc_transpose(p->acc + frame * p->accFrameStride, static_cast<int>(p->R), static_cast<int>(p->T), p->accPitch, d_out, outStride,
	                                     static_cast<hipStream_t>(stream)));
	return COMPVHIP_OK;
}

int compvhip_plan_edge_counts(compvhip_plan* p, const int32_t** d_edge_counts)
{
	if (!p || !p->shtReady || !d_edge_counts) return COMPVHIP_E_INVALID_PARAMETER;
	*d_edge_counts = p->edgeCounts;
	return COMPVHIP_OK;
}
