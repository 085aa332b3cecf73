// api_host.cpp -- the host-pointer (`*_u8`) entry points: one frame in host memory in, results in host memory out, synchronous
// (KHT: api_kht.cpp; the RANSAC families' host forms: api_ransac.cpp).  They run the plan-level calls on a single-frame plan and staging buffers
// cached in the context.
#include "api_internal.hpp"

// ---- host entry points -------------------------------------------------------------------------------------------
namespace {
constexpr float kAnyTheta = 0.f;   // hostPlan: any theta serves, keep the cached plan when it fits

// the single-frame plan cached for the host entry points (rebuilt for another size, or another theta when the call's result depends on it), dIn / dOut sized for it
int hostPlan(compvhip_ctx* ctx, size_t W, size_t H, float thetaDeg, compvhip_plan** out)
{
	const size_t S = alignUp(W, 64);
	compvhip_plan* p = ctx->hostPlan;
	if (p && (p->W != W || p->H != H || (thetaDeg != kAnyTheta && p->thetaDeg != thetaDeg))) { compvhip_plan_destroy(p); ctx->hostPlan = p = nullptr; }
	if (!p) {
		int rc = compvhip_plan_create(ctx, W, H, S, 1, thetaDeg != kAnyTheta ? thetaDeg : 1.f, &p);
		if (rc) return rc;
		ctx->hostPlan = p;
	}
	HIPCHK(ctx, ctx->dIn.reserve(ctx, S * H));
	HIPCHK(ctx, ctx->dOut.reserve(ctx, S * H));
	*out = p;
	return COMPVHIP_OK;
}

// The host calls on the cached plan: select the device, get the plan (thetaDeg or kAnyTheta), the plane into dIn, run; with `out`, dOut into it and the
// stream waited for (without, `run` ends in a wait of its own: takeList).  The copies of `run` go through the call's frame, which drains on every way out.
template <typename Run>   // int run(compvhip_plan*, HostCall&)
int hostPlaneOp(compvhip_ctx* ctx, const uint8_t* in, size_t W, size_t H, size_t S, float thetaDeg, uint8_t* out, size_t So, const Run& run)
{
	HIPCHK(ctx, hipSetDevice(ctx->device));
	compvhip_plan* p = nullptr;
	int rc = hostPlan(ctx, W, H, thetaDeg, &p);
	if (rc) return rc;
	HostCall hc(ctx->stream);
	stagePlane(ctx, hc, ctx->dIn, in, W, H, S);
	if (!hc.ok()) return hostStatus(ctx, hc);
	rc = run(p, hc);
	if (rc || !out) return rc;
	hc.download2D(out, So, ctx->dOut, p->S, W, H);
	return hostWait(ctx, hc);
}

// The caller's lines with their number into dSegLines / dCounts and, with segs, its segments into dSegs / dSegCount (dSegCount is the caller's to allocate).
int stageLists(compvhip_ctx* ctx, HostCall& hc, const compvhip_line* lines, size_t n, const compvhip_segment* segs, size_t nSegs)
{
	const int32_t nLines = static_cast<int32_t>(n), nS = static_cast<int32_t>(nSegs);
	stageArray(ctx, hc, ctx->dSegLines, lines, n);
	stageArray(ctx, hc, ctx->dCounts, &nLines, 1);
	if (segs) { stageArray(ctx, hc, ctx->dSegs, segs, nSegs); hc.upload(ctx->dSegCount, &nS, sizeof(int32_t)); }
	return hostWait(ctx, hc);   // the counts live on this stack frame; pageable copies may still be staged
}

// Waits for the stream, stores the int32 record count in *n and copies the first min(count, cap) records; COMPVHIP_E_OUT_OF_BOUND (`what`) when they did not all fit.
template <typename T>
int takeList(compvhip_ctx* ctx, HostCall& hc, const int32_t* dCount, const T* dRecs, T* recs, size_t cap, size_t* n, const char* what)
{
	int32_t found = 0;
	hc.download(&found, dCount, sizeof(int32_t), "record count");
	if (!hc.wait()) return hostStatus(ctx, hc);
	*n = static_cast<size_t>(found);
	const size_t ncopy = std::min(*n, cap);
	if (ncopy && !hc.downloadNow(recs, dRecs, ncopy * sizeof(T), "record download")) return hostStatus(ctx, hc);
	if (*n > cap) return fail(ctx, COMPVHIP_E_OUT_OF_BOUND, what);
	return COMPVHIP_OK;
}

int checkImage(compvhip_ctx* ctx, const uint8_t* in, size_t W, size_t H, size_t S, const void* out, size_t So)
{
	if (!ctx) return COMPVHIP_E_INVALID_PARAMETER;
	if (!in || !out || S < W || So < W) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "null image or stride < width");
	if (W < 3 || H < 3 || W > 32767 || H > 32767) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "image size out of range (3..32767)");
	return COMPVHIP_OK;
}
} // namespace

int compvhip_canny_u8(compvhip_ctx* ctx, const uint8_t* in, size_t W, size_t H, size_t S, float tLow, float tHigh, int ksize, int type,
                      uint8_t* out, size_t So)
{
	int rc = checkImage(ctx, in, W, H, S, out, So);
	if (rc) return rc;
	int lo, hi;
	rc = validateCannyParams(ctx, tLow, tHigh, ksize, type, &lo, &hi);
	if (rc) return rc;
	return hostPlaneOp(ctx, in, W, H, S, kAnyTheta, out, So, [&](compvhip_plan* p, HostCall&) { return compvhip_plan_canny(p, ctx->dIn, tLow, tHigh, ksize, type, ctx->dOut, ctx->stream); });
}

int compvhip_edge_dete_u8(compvhip_ctx* ctx, const uint8_t* in, size_t W, size_t H, size_t S, int op, uint8_t* out, size_t So)
{
	int rc = checkImage(ctx, in, W, H, S, out, So);
	if (rc) return rc;
	if (op != COMPVHIP_OP_SOBEL && op != COMPVHIP_OP_SCHARR && op != COMPVHIP_OP_PREWITT)
		return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "invalid detector id"); // edge_dete.cxx:246
	return hostPlaneOp(ctx, in, W, H, S, kAnyTheta, out, So, [&](compvhip_plan* p, HostCall& hc) -> int {
		EdgeDeteArgs a;
		a.in = ctx->dIn; a.out = ctx->dOut; a.gmax = p->sums;
		a.inFrameStride = p->S * H; a.outFrameStride = p->S * H;
		a.W = static_cast<int>(W); a.H = static_cast<int>(H); a.S = static_cast<int>(p->S); a.So = static_cast<int>(p->S);
		a.tilesX = p->tilesX; a.tilesY = p->tilesY;
		HOSTSTEP(ctx, hc, launch_edge_dete(a, op, 1, ctx->stream));
		return hostStatus(ctx, hc);
	});
}

int compvhip_gauss_kernel_fixedpoint(size_t size, float sigma, uint16_t* kernel)
{
	// compv_math_gauss.h:24-55 with T = float (note the float/double mix), then compv_math_convlt.h:88
	if (!kernel || !(size & 1) || size > 255 || !(sigma > 0.f)) return COMPVHIP_E_INVALID_PARAMETER;
	float f[255];
	const size_t half = size >> 1;
	const float sigma2_times2 = static_cast<float>(2 * (sigma * sigma));
	const float a = static_cast<float>(1 / std::sqrt(3.14159265358979323846 * sigma2_times2));
	float sum = a;
	f[half] = a;
	for (size_t x = 1; x <= half; ++x) {
		const float k = static_cast<float>(a * std::exp(-static_cast<double>((x * x) / sigma2_times2)));
		f[x + half] = k; f[half - x] = k;
		sum += (k + k);
	}
	sum = 1 / sum;
	for (size_t x = 0; x < size; ++x) { f[x] *= sum; kernel[x] = static_cast<uint16_t>(f[x] * 0xffff); }
	return COMPVHIP_OK;
}

int compvhip_convlt1_fixedpoint_u8(compvhip_ctx* ctx, const uint8_t* in, size_t W, size_t H, size_t S, const uint16_t* vtKern, const uint16_t* hzKern,
                                   size_t kernSize, uint8_t* out, size_t So)
{
	if (!ctx) return COMPVHIP_E_INVALID_PARAMETER;
	if (!in || !out || S < W || So < W || !W || !H || W > 32767 || H > 32767) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "null image, stride < width or size out of range");
	int rc = checkFxpKernel(ctx, W, H, vtKern, hzKern, kernSize);
	if (rc) return rc;
	HIPCHK(ctx, hipSetDevice(ctx->device));
	HostCall hc(ctx->stream);
	const size_t Sd = stagePlane(ctx, hc, ctx->dIn, in, W, H, S), bytes = Sd * H;
	HOSTSTEP(ctx, hc, ctx->dOut.reserve(ctx, bytes));
	// dIn -> dOut with the fused kernel (no intermediate: the two staging buffers never alias)
	HOSTSTEP(ctx, hc, launch_convlt_fxp(ctx->dIn, nullptr, ctx->dOut, static_cast<int>(W), static_cast<int>(H), static_cast<int>(Sd), bytes, 1, vtKern, hzKern,
	                               static_cast<int>(kernSize), ctx->stream));
	hc.download2D(out, So, ctx->dOut, Sd, W, H);
	return hostWait(ctx, hc);
}

// CompVMathConvlt::convlt1<uint8_t | int16_t, int16_t, int16_t> (compv_math_convlt.h:26-28,37-39,98-292): the separable integer correlation the
// gradient is made of, stand-alone.  The device buffers are private to the call (the operator is not on the per-frame hot path: there it is
// fused into the tile kernels); S, So in elements.
static int convlt1I16(compvhip_ctx* ctx, const void* in, bool inIsU8, size_t W, size_t H, size_t S, const int16_t* vtKern, const int16_t* hzKern, size_t kernSize,
                      int16_t* out, size_t So)
{
	if (!ctx) return COMPVHIP_E_INVALID_PARAMETER;
	if (!in || !out || !vtKern || !hzKern || S < W || So < W || !(kernSize & 1) || W < kernSize || H < kernSize)
		return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "convolution: null pointer, stride < width, even kernel size or image smaller than the kernel"); // compv_math_convlt.h:100
	if (kernSize > static_cast<size_t>(kFxpMaxTaps)) return fail(ctx, COMPVHIP_E_NOT_IMPLEMENTED, "integer convolution supports kernel sizes 1..15");
	if (W > 32767 || H > 32767) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "image size out of range");
	HIPCHK(ctx, hipSetDevice(ctx->device));
	DevBuf<uint8_t> dIn; DevBuf<int16_t> dTmp, dOut;   // freed on the way out, behind the drain of the frame
	HostCall hc(ctx->stream);
	const size_t Sd = stagePlane(ctx, hc, dIn, in, W, H, S, inIsU8 ? 1 : 2);
	HOSTSTEP(ctx, hc, dTmp.reserve(ctx, Sd * H));
	HOSTSTEP(ctx, hc, dOut.reserve(ctx, Sd * H));
	HOSTSTEP(ctx, hc, launch_convlt_i16(dIn, inIsU8, dTmp, dOut, static_cast<int>(W), static_cast<int>(H), static_cast<int>(Sd), static_cast<int>(Sd), vtKern, hzKern,
	                               static_cast<int>(kernSize), ctx->stream));
	hc.download2D(out, So * 2, dOut, Sd * 2, W * 2, H);
	return hostWait(ctx, hc);
}

int compvhip_convlt1_8u16s16s(compvhip_ctx* ctx, const uint8_t* in, size_t W, size_t H, size_t S, const int16_t* vtKern, const int16_t* hzKern, size_t kernSize,
                              int16_t* out, size_t So)
{
	return convlt1I16(ctx, in, true, W, H, S, vtKern, hzKern, kernSize, out, So);
}

int compvhip_convlt1_16s16s16s(compvhip_ctx* ctx, const int16_t* in, size_t W, size_t H, size_t S, const int16_t* vtKern, const int16_t* hzKern, size_t kernSize,
                               int16_t* out, size_t So)
{
	return convlt1I16(ctx, in, false, W, H, S, vtKern, hzKern, kernSize, out, So);
}

int compvhip_grayscale_u8(compvhip_ctx* ctx, const uint8_t* in, int pixfmt, size_t W, size_t H, size_t S, uint8_t* out, size_t So)
{
	if (!ctx) return COMPVHIP_E_INVALID_PARAMETER;
	if (!in || !out || S < W || So < W || !W || !H || W > 32767 || H > 32767) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "null image, stride < width or size out of range");
	const int rc = checkPixfmt(ctx, pixfmt, W);
	if (rc) return rc;
	const int bpp = pixfmtBytes(pixfmt);
	HIPCHK(ctx, hipSetDevice(ctx->device));
	HostCall hc(ctx->stream);
	const size_t Sd = stagePlane(ctx, hc, ctx->dPacked, in, W, H, S, static_cast<size_t>(bpp));
	HOSTSTEP(ctx, hc, ctx->dOut.reserve(ctx, Sd * H));
	GrayArgs a;
	a.in = ctx->dPacked; a.out = ctx->dOut; a.W = static_cast<int>(W); a.H = static_cast<int>(H); a.S = static_cast<int>(Sd); a.So = static_cast<int>(Sd);
	HOSTSTEP(ctx, hc, launch_gray(a, pixfmt, 1, ctx->stream));
	hc.download2D(out, So, ctx->dOut, Sd, W, H);
	return hostWait(ctx, hc);
}

int compvhip_otsu_u8(compvhip_ctx* ctx, const uint8_t* in, size_t W, size_t H, size_t S, double* threshold)
{
	if (!ctx) return COMPVHIP_E_INVALID_PARAMETER;
	if (!in || !threshold || S < W || !W || !H || W > 32767 || H > 32767) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "null image, stride < width or size out of range"); // threshold.cxx:54
	HIPCHK(ctx, hipSetDevice(ctx->device));
	int32_t t = 0;
	HostCall hc(ctx->stream);
	const size_t Sd = stagePlane(ctx, hc, ctx->dIn, in, W, H, S), bytes = Sd * H;
	HOSTSTEP(ctx, hc, ctx->dHist.reserve(ctx, static_cast<size_t>(256) * kOtsuMaxChunks + 1));
	int32_t* dT = reinterpret_cast<int32_t*>(ctx->dHist + static_cast<size_t>(256) * kOtsuMaxChunks);
	HOSTSTEP(ctx, hc, launch_otsu(ctx->dIn, static_cast<int>(W), static_cast<int>(H), static_cast<int>(Sd), bytes, 1, 0.5f, 1.f, ctx->dHist, dT, nullptr, ctx->stream));
	hc.download(&t, dT, sizeof(t));
	if (!hc.wait()) return hostStatus(ctx, hc);
	*threshold = static_cast<double>(t);
	return COMPVHIP_OK;
}

// CompVHoughSht::process ends with std::sort(lines, strength >) and keeps the first maxLines (houghsht.cxx:241-249).  std::sort is
// unstable, but deterministic for one libstdc++ and one input order, and the input order is nms_apply's emission order: accumulator
// rows ascending, columns ascending (:546-562; per-thread vectors are concatenated in row order, :228-234).  Re-creating that order
// and calling the same std::sort gives the reference's list element by element -- callers such as CompVCalibCamera (line grouping,
// core/calib/compv_core_calib_camera.cxx:200-) depend on the order inside equal-strength groups.  The permutation only depends on
// the strengths, so it is computed on (strength, index) pairs.
static void referenceLineOrder(const std::vector<uint32_t>& keys, const std::vector<uint32_t>& cells, uint32_t strengthMask, size_t T, long long barrier, float thetaStep,
                               std::vector<compvhip_line>& lines)
{
	// keys / cells arrive in emission order (ascending cell): exactly the array the reference sorts
	const size_t n = keys.size();
	struct Item { int32_t strength; uint32_t idx; };
	std::vector<Item> items(n);
	for (size_t i = 0; i < n; ++i) { items[i].strength = static_cast<int32_t>(keys[i] & strengthMask); items[i].idx = static_cast<uint32_t>(i); }
	std::sort(items.begin(), items.end(), [](const Item& a, const Item& b) { return a.strength > b.strength; });
	lines.resize(n);
	for (size_t i = 0; i < n; ++i) {
		const uint32_t cell = cells[items[i].idx];
		const uint32_t row = cell / static_cast<uint32_t>(T), col = cell - row * static_cast<uint32_t>(T);
		compvhip_line& l = lines[i];
		l.rho = static_cast<float>(barrier - static_cast<long long>(row));   // houghsht.cxx:661
		l.theta = static_cast<float>(col) * thetaStep;                       // houghsht.cxx:662 (one rounded f32 product: -ffp-contract=off)
		l.strength = items[i].strength; l.row = static_cast<int32_t>(row); l.col = static_cast<int32_t>(col);
	}
}

int compvhip_houghsht_u8(compvhip_ctx* ctx, const uint8_t* edges, size_t W, size_t H, size_t S, float rho, float thetaDeg, int threshold, int maxLines,
                         compvhip_line* lines, size_t cap, size_t* n, int32_t* acc, size_t accStride)
{
	if (!ctx) return COMPVHIP_E_INVALID_PARAMETER;
	if (!edges || !n || (cap && !lines) || S < W || !W || !H) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "null/invalid argument"); // houghsht.cxx:98
	if (rho != 1.f) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "SHT requires rho == 1 (use KHT for fractional rho)"); // :306-316
	if (!(thetaDeg > 0.f) || threshold <= 0) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "theta and threshold must be > 0");
	if (W < 3 || H < 3 || W > 32767 || H > 32767) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "image size out of range (3..32767)");
	*n = 0;
	HIPCHK(ctx, hipSetDevice(ctx->device));
	compvhip_plan* p = nullptr;
	int rc = hostPlan(ctx, W, H, thetaDeg, &p);
	if (rc) return rc;
	rc = ensureSht(p);
	if (rc) return rc;
	if (acc && accStride < p->T) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "accStride < theta bins");
	int32_t count = 0;
	std::vector<uint32_t> hk, hv;          // (with `count`, targets of copies: in front of the frame, which drains before they go)
	HostCall hc(ctx->stream);
	stagePlane(ctx, hc, ctx->dIn, edges, W, H, S);
	HOSTSTEP(ctx, hc, ctx->dCounts.reserve(ctx, 1));
	// ALL candidate lines of the frame come back as (strength, cell) pairs in emission order -- the sort and the decode kernel are skipped:
	// the order the reference returns them in, and which equal-strength lines survive maxLines, is decided by its unstable std::sort
	for (int attempt = 0; attempt < 2; ++attempt) {
		ShtOpts o;
		o.pairsOnly = true;
		rc = planShtImpl(p, ctx->dIn, threshold, 0, nullptr, 0, ctx->dCounts, ctx->stream, o);
		if (rc) return rc;
		hc.download(&count, ctx->dCounts, sizeof(int32_t), "line count");
		if (!hc.wait()) return hostStatus(ctx, hc);
		if (static_cast<size_t>(count) <= p->lineCap) break;
		// more candidate lines than the device key buffer holds: grow it and redo the line stage
		rc = ensureLineCap(p, static_cast<size_t>(count));
		if (rc) return rc;
	}
	hk.resize(static_cast<size_t>(count)); hv.resize(static_cast<size_t>(count));
	if (count) {
		hc.download(hk.data(), p->keysA, hk.size() * sizeof(uint32_t), "line keys");
		hc.download(hv.data(), p->valsA, hv.size() * sizeof(uint32_t), "line cells");
		if (!hc.wait()) return hostStatus(ctx, hc);
	}
	std::vector<compvhip_line> all;
	referenceLineOrder(hk, hv, (1u << p->strengthBits) - 1u, p->T, static_cast<long long>(p->W + p->H), p->thetaStep, all);
	size_t found = all.size();
	if (maxLines > 0 && found > static_cast<size_t>(maxLines)) found = static_cast<size_t>(maxLines);
	*n = found;
	const size_t ncopy = std::min(found, cap);
	if (ncopy) memcpy(lines, all.data(), ncopy * sizeof(compvhip_line));
	if (acc) {
		HOSTSTEP(ctx, hc, ctx->dAccOut.reserve(ctx, p->R * p->T));
		HOSTSTEP(ctx, hc, launch_sht_acc_transpose(p->acc, static_cast<int>(p->R), static_cast<int>(p->T), p->accPitch, ctx->dAccOut, p->T, ctx->stream));
		hc.download2D(acc, accStride * sizeof(int32_t), ctx->dAccOut, p->T * sizeof(int32_t), p->T * sizeof(int32_t), p->R, "accumulator download");
		if (!hc.wait()) return hostStatus(ctx, hc);
	}
	if (found > cap) return fail(ctx, COMPVHIP_E_OUT_OF_BOUND, "line buffer too small");
	return COMPVHIP_OK;
}

int compvhip_houghsht_segments_u8(compvhip_ctx* ctx, const uint8_t* edges, size_t W, size_t H, size_t S, float thetaDeg, const compvhip_line* lines, size_t n,
                                  int minLength, int maxGap, compvhip_segment* segs, size_t cap, size_t* nSegs)
{
	if (!ctx) return COMPVHIP_E_INVALID_PARAMETER;
	if (!edges || !nSegs || (n && !lines) || (cap && !segs) || S < W) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "null/invalid argument");
	if (!(thetaDeg > 0.f) || minLength < 1 || maxGap < 0) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "theta must be > 0, minLength >= 1, maxGap >= 0");
	if (W < 3 || H < 3 || W > 32767 || H > 32767) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "image size out of range (3..32767)");
	*nSegs = 0;
	size_t R, T;
	int rc = shtDims(W, H, thetaDeg, &R, &T, nullptr);
	if (rc) return fail(ctx, rc, "invalid SHT geometry");
	if (n > static_cast<size_t>(INT32_MAX)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "too many lines");
	for (size_t i = 0; i < n; ++i)
		if (lines[i].row < 0 || static_cast<size_t>(lines[i].row) >= R || lines[i].col < 0 || static_cast<size_t>(lines[i].col) >= T)
			return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "a line's (row, col) is not a cell of the R x T accumulator");
	if (!n) return COMPVHIP_OK;
	return hostPlaneOp(ctx, edges, W, H, S, thetaDeg, nullptr, 0, [&](compvhip_plan* p, HostCall& hc) -> int {
		HOSTSTEP(ctx, hc, ctx->dSegs.reserve(ctx, cap));
		HOSTSTEP(ctx, hc, ctx->dSegCount.reserve(ctx, 1));
		int rc = stageLists(ctx, hc, lines, n, nullptr, 0);
		if (rc) return rc;
		rc = segmentsImpl(p, ctx->dIn, p->S, ctx->dSegLines, ctx->dCounts, n, 0, minLength, maxGap, ctx->dSegs, cap, ctx->dSegCount, ctx->stream);
		if (rc) return rc;
		return takeList(ctx, hc, ctx->dSegCount.ptr, ctx->dSegs.ptr, segs, cap, nSegs, "segment buffer too small");
	});
}

int compvhip_houghsht_fit_u8(compvhip_ctx* ctx, const uint8_t* edges, size_t W, size_t H, size_t S, float thetaDeg, const compvhip_line* lines, size_t n,
                             int halfWidth, const compvhip_segment* segs, size_t nSegs, compvhip_line_fit* fits, size_t cap, size_t* nFits, compvhip_line* refined)
{
	if (!ctx) return COMPVHIP_E_INVALID_PARAMETER;
	if (!edges || !nFits || (n && !lines) || (cap && !fits) || S < W) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "null/invalid argument");
	if (!(thetaDeg > 0.f) || halfWidth < 0 || halfWidth > kFitMaxHalfWidth) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "theta must be > 0, halfWidth 0 .. 8");
	if (segs && refined) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "refined lines are a per-line result: segs must be NULL");
	if (W < 3 || H < 3 || W > 32767 || H > 32767) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "image size out of range (3..32767)");
	if (std::max(W, H) > kFitMaxSide) return fail(ctx, COMPVHIP_E_NOT_IMPLEMENTED, "line fits need max(W, H) <= 8192 (int64 central moments)");
	*nFits = 0;
	size_t R, T;
	int rc = shtDims(W, H, thetaDeg, &R, &T, nullptr);
	if (rc) return fail(ctx, rc, "invalid SHT geometry");
	if (n > static_cast<size_t>(INT32_MAX) || (segs && nSegs > static_cast<size_t>(INT32_MAX))) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "too many lines / segments");
	for (size_t i = 0; i < n; ++i)
		if (lines[i].row < 0 || static_cast<size_t>(lines[i].row) >= R || lines[i].col < 0 || static_cast<size_t>(lines[i].col) >= T)
			return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "a line's (row, col) is not a cell of the R x T accumulator");
	if (segs)
		for (size_t j = 0; j < nSegs; ++j)
			if (segs[j].line < 0 || static_cast<size_t>(segs[j].line) >= n) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "a segment's line is not one of the n lines");
	const size_t nRec = segs ? nSegs : n;
	if (!n || !nRec) return COMPVHIP_OK;
	return hostPlaneOp(ctx, edges, W, H, S, thetaDeg, nullptr, 0, [&](compvhip_plan* p, HostCall& hc) -> int {
		HOSTSTEP(ctx, hc, ctx->dFits.reserve(ctx, cap));
		if (refined) HOSTSTEP(ctx, hc, ctx->dFitRefined.reserve(ctx, n));
		HOSTSTEP(ctx, hc, ctx->dSegCount.reserve(ctx, 1));
		HOSTSTEP(ctx, hc, ctx->dFitCount.reserve(ctx, 1));
		int rc = stageLists(ctx, hc, lines, n, segs, nSegs);
		if (rc) return rc;
		rc = fitImpl(p, ctx->dIn, p->S, ctx->dSegLines, ctx->dCounts, n, 0, halfWidth, segs ? ctx->dSegs.ptr : nullptr, ctx->dSegCount, nSegs, cap ? ctx->dFits.ptr : nullptr, cap,
		             ctx->dFitCount, refined ? ctx->dFitRefined.ptr : nullptr, ctx->stream);
		if (rc) return rc;
		if (refined) hc.download(refined, ctx->dFitRefined, n * sizeof(compvhip_line), "refined lines");
		return takeList(ctx, hc, ctx->dFitCount.ptr, ctx->dFits.ptr, fits, cap, nFits, "fit buffer too small");
	});
}

int compvhip_components_u8(compvhip_ctx* ctx, const uint8_t* edges, size_t W, size_t H, size_t S, int connectivity, int minPixels, int32_t* labels, size_t labelStride,
                           compvhip_component* comps, size_t cap, size_t* nComps)
{
	if (!ctx) return COMPVHIP_E_INVALID_PARAMETER;
	if (!edges || !nComps || (cap && !comps) || S < W || (labels && labelStride < W)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "null/invalid argument");
	if (W < 3 || H < 3 || W > 32767 || H > 32767) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "image size out of range (3..32767)");
	if ((connectivity != 4 && connectivity != 8) || minPixels < 1) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "connectivity must be 4 or 8, minPixels >= 1");
	*nComps = 0;
	return hostPlaneOp(ctx, edges, W, H, S, kAnyTheta, nullptr, 0, [&](compvhip_plan* p, HostCall& hc) -> int {
		if (labels) HOSTSTEP(ctx, hc, ctx->dCompLabels.reserve(ctx, W * H));
		HOSTSTEP(ctx, hc, ctx->dComps.reserve(ctx, cap));
		HOSTSTEP(ctx, hc, ctx->dCompCount.reserve(ctx, 1));
		int rc = componentsImpl(p, ctx->dIn, p->S, connectivity, minPixels, labels ? ctx->dCompLabels.ptr : nullptr, W, cap ? ctx->dComps.ptr : nullptr, cap, ctx->dCompCount, ctx->stream);
		if (rc) return rc;
		if (labels) hc.download2D(labels, labelStride * sizeof(int32_t), ctx->dCompLabels, W * sizeof(int32_t), W * sizeof(int32_t), H, "label download");
		return takeList(ctx, hc, ctx->dCompCount.ptr, ctx->dComps.ptr, comps, cap, nComps, "component buffer too small");
	});
}

int compvhip_fast_u8(compvhip_ctx* ctx, const uint8_t* gray, size_t W, size_t H, size_t S, int threshold, int fastType, int nonmax, int maxFeatures, uint8_t* scores,
                     size_t So, compvhip_corner* corners, size_t cap, size_t* n)
{
	if (!ctx) return COMPVHIP_E_INVALID_PARAMETER;
	if (!gray || !n || (cap && !corners) || S < W || (scores && So < W)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "null/invalid argument");
	*n = 0;
	int rc = checkFast(ctx, W, H, fastType);
	if (rc) return rc;
	if (W > 32767 || H > 32767) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "image size out of range (7..32767)");
	return hostPlaneOp(ctx, gray, W, H, S, kAnyTheta, nullptr, 0, [&](compvhip_plan* p, HostCall& hc) -> int {
		HOSTSTEP(ctx, hc, ctx->dFastCorners.reserve(ctx, cap));
		HOSTSTEP(ctx, hc, ctx->dFastCount.reserve(ctx, 1));
		int rc = compvhip_plan_fast(p, ctx->dIn, threshold, fastType, nonmax, maxFeatures, scores ? ctx->dOut.ptr : nullptr, cap ? ctx->dFastCorners.ptr : nullptr, cap, ctx->dFastCount, ctx->stream);
		if (rc) return rc;
		if (scores) hc.download2D(scores, So, ctx->dOut, p->S, W, H, "score download");
		return takeList(ctx, hc, ctx->dFastCount.ptr, ctx->dFastCorners.ptr, corners, cap, n, "corner buffer too small");
	});
}

int compvhip_orb_u8(compvhip_ctx* ctx, const uint8_t* gray, size_t W, size_t H, size_t S, const compvhip_corner* corners, size_t n, int level, float scale,
                    compvhip_keypoint* keypoints, uint8_t* desc, size_t descStride, size_t* kept)
{
	if (!ctx) return COMPVHIP_E_INVALID_PARAMETER;
	if (!gray || !kept || S < W || (n && (!corners || !keypoints || !desc))) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "null/invalid argument");
	*kept = 0;
	int rc = checkOrb(ctx, W, H, scale);
	if (rc) return rc;
	if (W > 32767 || H > 32767 || n > static_cast<size_t>(INT32_MAX)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "image size out of range (37..32767) or n beyond 2^31");
	if (descStride < 32 || (descStride & 3)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "descStride below 32 or no multiple of 4");
	if (!n) return COMPVHIP_OK;
	return hostPlaneOp(ctx, gray, W, H, S, kAnyTheta, nullptr, 0, [&](compvhip_plan* p, HostCall& hc) -> int {
		HOSTSTEP(ctx, hc, ctx->dOrbKeys.reserve(ctx, n));
		HOSTSTEP(ctx, hc, ctx->dOrbCount.reserve(ctx, 1));
		HOSTSTEP(ctx, hc, ctx->dOrbDesc.reserve(ctx, n * 32));
		const int32_t count = static_cast<int32_t>(n);
		stageArray(ctx, hc, ctx->dFastCorners, corners, n);
		stageArray(ctx, hc, ctx->dFastCount, &count, 1);
		if (!hc.wait()) return hostStatus(ctx, hc);   // the count lives on this stack frame; pageable copies may still be staged
		int rc = compvhip_plan_orb_keypoints(p, ctx->dIn, ctx->dFastCorners, n, ctx->dFastCount, level, scale, ctx->dOrbKeys, n, ctx->dOrbCount, nullptr, ctx->stream);
		if (rc) return rc;
		rc = compvhip_plan_orb_describe(p, ctx->dIn, ctx->dOrbKeys, n, ctx->dOrbCount, scale, 1, ctx->dOrbDesc, 32, ctx->stream);
		if (rc) return rc;
		rc = takeList(ctx, hc, ctx->dOrbCount.ptr, ctx->dOrbKeys.ptr, keypoints, n, kept, "keypoint buffer too small");
		if (rc || !*kept) return rc;
		hc.downloadNow2D(desc, descStride, ctx->dOrbDesc, 32, 32, *kept, "descriptor download");
		return hostStatus(ctx, hc);
	});
}

int compvhip_hog_u8(compvhip_ctx* ctx, const uint8_t* gray, size_t W, size_t H, size_t S, const compvhip_hog_opts* opts, float* desc, size_t cap, size_t* n)
{
	if (!ctx) return COMPVHIP_E_INVALID_PARAMETER;
	if (!gray || !n || (cap && !desc) || S < W) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "null/invalid argument");
	HogArgs a;
	int rc = hogGeometry(ctx, W, H, opts, &a);
	if (rc) return rc;
	if (W < 3 || H < 3) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "image size out of range (3..32767)");
	const size_t descLen = static_cast<size_t>(a.blocksX) * a.blocksY * a.count;
	*n = descLen;
	if (cap < descLen) return fail(ctx, COMPVHIP_E_OUT_OF_BOUND, "descriptor buffer too small");
	return hostPlaneOp(ctx, gray, W, H, S, kAnyTheta, nullptr, 0, [&](compvhip_plan* p, HostCall& hc) -> int {
		HOSTSTEP(ctx, hc, ctx->dHogDesc.reserve(ctx, descLen));
		const int rc = compvhip_plan_hog(p, ctx->dIn, opts, nullptr, ctx->dHogDesc, descLen, ctx->stream);
		if (rc) return rc;
		hc.download(desc, ctx->dHogDesc, descLen * sizeof(float), "descriptor download");
		return hostWait(ctx, hc);
	});
}

int compvhip_scale_u8(compvhip_ctx* ctx, const uint8_t* in, size_t W, size_t H, size_t S, uint8_t* out, size_t Wout, size_t Hout, size_t Sout)
{
	if (!ctx) return COMPVHIP_E_INVALID_PARAMETER;
	if (!in || !out || S < W || Sout < Wout) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "null image or stride < width");
	if (!W || !H || !Wout || !Hout || W > 32767 || H > 32767 || Wout > 32767 || Hout > 32767) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "image size out of range (1..32767)");
	HIPCHK(ctx, hipSetDevice(ctx->device));
	HostCall hc(ctx->stream);
	const size_t Sd = stagePlane(ctx, hc, ctx->dIn, in, W, H, S), Sod = alignUp(Wout, 64);          // no plan: a scale has no minimum size
	HOSTSTEP(ctx, hc, ctx->dOut.reserve(ctx, Sod * Hout));
	const int rc = scaleImpl(ctx, ctx->dIn, W, H, Sd, 1, ctx->dOut, Wout, Hout, Sod, ctx->stream);
	if (rc) return rc;
	hc.download2D(out, Sout, ctx->dOut, Sod, Wout, Hout);
	return hostWait(ctx, hc);
}

// remap and inverse warp of one host plane: the staging of both (no plan: neither has a minimum size).  `coords` enqueues the coordinate source into `a`.
template <typename Coords>   // int coords(RemapArgs*, HostCall&)
static int hostRemap(compvhip_ctx* ctx, const uint8_t* in, size_t W, size_t H, size_t S, int interp, const compvhip_roi* roi, uint8_t defaultValue, void* out, size_t Wout,
                     size_t Hout, size_t Sout, int source, const Coords& coords)
{
	if (!in || !out || S < W || Sout < Wout) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "null image or stride < width");
	if (!W || !H || !Wout || !Hout || W > 32767 || H > 32767 || Wout > 32767 || Hout > 32767) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "image size out of range (1..32767)");
	const size_t elem = interpElemBytes(interp), Sod = alignUp(Wout, 64);
	if (!elem) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "unknown interpolation");
	HIPCHK(ctx, hipSetDevice(ctx->device));
	HostCall hc(ctx->stream);
	const size_t Sd = stagePlane(ctx, hc, ctx->dIn, in, W, H, S);
	HOSTSTEP(ctx, hc, ctx->dOut.reserve(ctx, Sod * Hout * elem));
	RemapArgs a;
	int rc = remapPrepare(ctx, ctx->dIn, W, H, Sd, 1, interp, roi, ctx->dOut.ptr, Wout, Hout, Sod, defaultValue, &a);
	if (!rc) rc = coords(&a, hc);
	if (rc) return rc;
	HOSTSTEP(ctx, hc, launch_remap(a, source, interp, false, ctx->stream));
	hc.download2D(out, Sout * elem, ctx->dOut, Sod * elem, Wout * elem, Hout);
	return hostWait(ctx, hc);
}

int compvhip_remap_u8(compvhip_ctx* ctx, const uint8_t* in, size_t W, size_t H, size_t S, const float* mapX, const float* mapY, int interp, const compvhip_roi* roi,
                      uint8_t defaultValue, void* out, size_t Wout, size_t Hout, size_t Sout)
{
	if (!ctx) return COMPVHIP_E_INVALID_PARAMETER;
	if (!mapX || !mapY) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "null map");
	return hostRemap(ctx, in, W, H, S, interp, roi, defaultValue, out, Wout, Hout, Sout, kRemapMap, [&](RemapArgs* a, HostCall& hc) -> int {
		const size_t n = Wout * Hout;
		HOSTSTEP(ctx, hc, ctx->dMap.reserve(ctx, 2 * n));
		hc.upload(ctx->dMap, mapX, n * sizeof(float), "map upload");
		hc.upload(ctx->dMap + n, mapY, n * sizeof(float), "map upload");
		a->mapX = ctx->dMap; a->mapY = ctx->dMap + n; a->coordFrameStride = n;
		return hostStatus(ctx, hc);
	});
}

int compvhip_warp_inverse_u8(compvhip_ctx* ctx, const uint8_t* in, size_t W, size_t H, size_t S, const float* M, int rows, int interp, uint8_t defaultValue, void* out,
                             size_t Wout, size_t Hout, size_t Sout)
{
	if (!ctx) return COMPVHIP_E_INVALID_PARAMETER;
	if (!M || (rows != 2 && rows != 3)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "M must be a 2 x 3 or 3 x 3 float32 matrix");
	return hostRemap(ctx, in, W, H, S, interp, nullptr, defaultValue, out, Wout, Hout, Sout, rows == 3 ? kRemapWarp3 : kRemapWarp2,
	                 [&](RemapArgs* a, HostCall&) -> int { return warpUpload(ctx, &ctx->warp, M, rows, 1, a, ctx->stream); });
}

// the fused undistortion of one host plane (include/compv_hip.h, "lens undistortion"): the same staging, the camera's record through the context's ring
int compvhip_undistort_u8(compvhip_ctx* ctx, const uint8_t* in, size_t W, size_t H, size_t S, const float* K, const float* d, int nd, size_t x0, size_t y0, int interp,
                          const compvhip_roi* roi, uint8_t defaultValue, void* out, size_t Wout, size_t Hout, size_t Sout)
{
	if (!ctx) return COMPVHIP_E_INVALID_PARAMETER;
	if (!K || !d || nd < 2 || nd > 4) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "undistort: null K or d, or nd outside 2 .. 4");
	if (!undistWindowOk(x0, y0, Wout, Hout)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "undistort: an output size of 0 or beyond 32767, or x0 + Wout / y0 + Hout beyond 32767");
	float probe[14];
	if (compvhip_undistort_coeffs_f32(K, d, nd, probe)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "undistort: fx * fy == 0, the camera matrix is singular");
	return hostRemap(ctx, in, W, H, S, interp, roi, defaultValue, out, Wout, Hout, Sout, kRemapUndist,
	                 [&](RemapArgs* a, HostCall&) -> int { return undistCoords(ctx, &ctx->warp, K, d, nd, 1, x0, y0, a, ctx->stream); });
}

int compvhip_orb_pyramid_u8(compvhip_ctx* ctx, const uint8_t* gray, size_t W, size_t H, size_t S, const compvhip_orbpyr_opts* opts, compvhip_keypoint* keypoints,
                            uint8_t* desc, size_t descStride, size_t cap, size_t* n)
{
	if (!ctx) return COMPVHIP_E_INVALID_PARAMETER;
	if (!gray || !n || S < W || (cap && (!keypoints || !desc))) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "null/invalid argument");
	*n = 0;
	if (descStride < 32 || (descStride & 3)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "descStride below 32 or no multiple of 4");
	if (W > 32767 || H > 32767 || cap > static_cast<size_t>(INT32_MAX)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "image size out of range (37..32767) or cap beyond 2^31");
	const compvhip_orbpyr_opts defaults = { 8, 0.83f, 20, 9, 1, 2000 };
	if (!opts) opts = &defaults;
	HIPCHK(ctx, hipSetDevice(ctx->device));
	const size_t Sd = alignUp(W, 64);
	// with NMS no two corners are neighbours: every second pixel of every second row at most
	const size_t cornerCap = opts->nonmax ? ((W + 1) / 2) * ((H + 1) / 2) : W * H;
	compvhip_orbpyr* y = nullptr;
	int rc = compvhip_orbpyr_create(ctx, W, H, Sd, 1, opts, cornerCap, &y);
	if (rc) return rc;
	const TempHandle<compvhip_orbpyr> pyramid{ ctx, y, compvhip_orbpyr_destroy };
	HostCall hc(ctx->stream);
	stagePlane(ctx, hc, ctx->dIn, gray, W, H, S);
	HOSTSTEP(ctx, hc, ctx->dOrbKeys.reserve(ctx, cap));
	HOSTSTEP(ctx, hc, ctx->dOrbCount.reserve(ctx, 1));
	HOSTSTEP(ctx, hc, ctx->dOrbDesc.reserve(ctx, cap * 32));
	rc = compvhip_orbpyr_detect(y, ctx->dIn, cap ? ctx->dOrbKeys.ptr : nullptr, cap, ctx->dOrbCount, nullptr, nullptr, ctx->stream);
	if (!rc && cap) rc = compvhip_orbpyr_describe(y, ctx->dIn, 1, ctx->dOrbKeys, cap, ctx->dOrbCount, ctx->dOrbDesc, 32, ctx->stream);
	if (rc) return rc;
	rc = takeList(ctx, hc, ctx->dOrbCount.ptr, ctx->dOrbKeys.ptr, keypoints, cap, n, "keypoint buffer too small");
	const size_t rows = std::min(*n, cap);
	if ((rc == COMPVHIP_OK || rc == COMPVHIP_E_OUT_OF_BOUND) && rows && !hc.downloadNow2D(desc, descStride, ctx->dOrbDesc, 32, 32, rows, "descriptor download")) rc = hostStatus(ctx, hc);
	return rc;
}

int compvhip_threshold_u8(compvhip_ctx* ctx, const uint8_t* in, size_t W, size_t H, size_t S, double threshold, uint8_t* out, size_t So)
{
	int rc = checkImage(ctx, in, W, H, S, out, So);
	if (rc) return rc;
	if (!(threshold >= 0.0)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "threshold < 0"); // compv_image_threshold.cxx:120
	return hostPlaneOp(ctx, in, W, H, S, kAnyTheta, out, So, [&](compvhip_plan* p, HostCall&) { return compvhip_plan_threshold(p, ctx->dIn, threshold, nullptr, ctx->dOut, ctx->stream); });
}

int compvhip_threshold_adaptive_u8(compvhip_ctx* ctx, const uint8_t* in, size_t W, size_t H, size_t S, size_t blockSize, double delta, double maxVal, int invert,
                                   uint8_t* out, size_t So)
{
	int rc = checkImage(ctx, in, W, H, S, out, So);
	if (rc) return rc;
	rc = checkAdaptive(ctx, W, H, blockSize, delta, maxVal);
	if (rc) return rc;
	return hostPlaneOp(ctx, in, W, H, S, kAnyTheta, out, So,
	                   [&](compvhip_plan* p, HostCall&) { return compvhip_plan_threshold_adaptive(p, ctx->dIn, blockSize, delta, maxVal, invert, ctx->dOut, ctx->stream); });
}

int compvhip_morph_u8(compvhip_ctx* ctx, const uint8_t* in, size_t W, size_t H, size_t S, const uint8_t* strel, size_t sw, size_t sh, int op, int border, uint8_t* out,
                      size_t So)
{
	int rc = checkImage(ctx, in, W, H, S, out, So);
	if (rc) return rc;
	MorphArgs a;
	rc = morphPrepare(ctx, W, H, strel, sw, sh, op, border, COMPVHIP_MORPH_KERNEL_AUTO, &a);
	if (rc) return rc;
	// the host planes overlap when their byte ranges do (compv_math_morph.cxx:140-145: the reference reallocates; here the caller is told)
	const uint8_t* inEnd = in + (H - 1) * S + W; const uint8_t* outEnd = out + (H - 1) * So + W;
	if (in < outEnd && out < inEnd) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "input and output must not overlap");
	return hostPlaneOp(ctx, in, W, H, S, kAnyTheta, out, So, [&](compvhip_plan* p, HostCall&) { return compvhip_plan_morph(p, ctx->dIn, strel, sw, sh, op, border, ctx->dOut, ctx->stream); });
}

int compvhip_match_hamming_u8(compvhip_ctx* ctx, const uint8_t* query, size_t Q, size_t queryStride, const uint8_t* train, size_t T, size_t trainStride, size_t cols,
                              int knn, compvhip_match* matches, size_t matchStride, size_t* rows)
{
	if (!ctx) return COMPVHIP_E_INVALID_PARAMETER;
	if (!query || !train || !matches || !rows || !Q || !T || queryStride < cols || trainStride < cols || matchStride < Q) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "null/invalid argument");
	if (cols < 1 || cols > 4 * static_cast<size_t>(kMatchMaxDwords)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "cols must be in 1..128");
	*rows = 0;
	HIPCHK(ctx, hipSetDevice(ctx->device));
	const size_t S = alignUp(cols, 4);
	compvhip_matcher* m = nullptr;
	int rc = compvhip_matcher_create(ctx, S, Q, T, 1, knn, &m);
	if (rc) return rc;
	const TempHandle<compvhip_matcher> matcher{ ctx, m, compvhip_matcher_destroy };
	DevBuf<uint8_t> dDesc; DevBuf<compvhip_match> dMatches;
	const size_t nRows = std::min<size_t>(static_cast<size_t>(knn), T);
	HostCall hc(ctx->stream);
	HOSTSTEP(ctx, hc, dDesc.reserve(ctx, (Q + T) * S));
	HOSTSTEP(ctx, hc, dMatches.reserve(ctx, static_cast<size_t>(knn) * Q));
	HOSTSTEP(ctx, hc, hipMemsetAsync(dDesc, 0, (Q + T) * S, ctx->stream));          // the zero bytes that pad a row to a dword multiple
	hc.upload2D(dDesc, S, query, queryStride, cols, Q, "descriptor upload");
	hc.upload2D(dDesc + Q * S, S, train, trainStride, cols, T, "descriptor upload");
	// not compvhip_matcher_knn: the reference's order among equal distances is not the (distance, index) order of the device call
	const MatchSliceArgs a = matchForward(m, dDesc, S, nullptr, dDesc + Q * S, S, nullptr, 0, dMatches);
	HOSTSTEP(ctx, hc, launch_match_reference(a, 1, ctx->stream));
	hc.download2D(matches, matchStride * sizeof(compvhip_match), dMatches, Q * sizeof(compvhip_match), Q * sizeof(compvhip_match), nRows, "match download");
	if (!hc.wait()) return hostStatus(ctx, hc);
	*rows = nRows;
	return COMPVHIP_OK;
}

// ---- image statistics of one host frame (no plan: a plan has a minimum size, these calls have none) ------------------------------------------------------
namespace {
// the frame into dIn (rows of alignUp(W, 64) bytes), `run` on it (its copies through the call's frame), the stream waited for
template <typename Run>   // int run(const StatsFrames&, HostCall&): begins with a HOSTSTEP, so it does nothing behind a failed upload
int hostStats(compvhip_ctx* ctx, const uint8_t* in, size_t W, size_t H, size_t S, const Run& run)
{
	if (!in || S < W) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "null image or stride < width");
	if (!W || !H || W > 32767 || H > 32767) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "image size out of range (1..32767)");
	HIPCHK(ctx, hipSetDevice(ctx->device));
	HostCall hc(ctx->stream);
	const size_t Sd = stagePlane(ctx, hc, ctx->dIn, in, W, H, S);
	const int rc = run(StatsFrames{ ctx, nullptr, &ctx->stats, ctx->dIn, W, H, Sd, 1, ctx->stream }, hc);
	return rc ? rc : hostWait(ctx, hc);
}
} // namespace

int compvhip_integral_u8(compvhip_ctx* ctx, const uint8_t* in, size_t W, size_t H, size_t S, double* sum, double* sumsq, size_t sumStride)
{
	if (!ctx) return COMPVHIP_E_INVALID_PARAMETER;
	int rc = integralDims(ctx, W, H);
	if (rc) return rc;
	if (!sum && !sumsq) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "integral: both outputs are NULL");
	if (sumStride < W + 1) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "integral: sumStride below W + 1");
	return hostStats(ctx, in, W, H, S, [&](const StatsFrames& g, HostCall& hc) -> int {
		const size_t cols = W + 1, plane = (H + 1) * cols;
		HOSTSTEP(ctx, hc, ctx->dStatsF64.reserve(ctx, 2 * plane));
		double* const dSum = sum ? ctx->dStatsF64.ptr : nullptr;
		double* const dSq = sumsq ? ctx->dStatsF64.ptr + plane : nullptr;
		const int rc = integralImpl(g, dSum, dSq, cols);
		if (rc) return rc;
		if (sum) hc.download2D(sum, sumStride * sizeof(double), dSum, cols * sizeof(double), cols * sizeof(double), H + 1);
		if (sumsq) hc.download2D(sumsq, sumStride * sizeof(double), dSq, cols * sizeof(double), cols * sizeof(double), H + 1);
		return COMPVHIP_OK;
	});
}

int compvhip_histogram_u8(compvhip_ctx* ctx, const uint8_t* in, size_t W, size_t H, size_t S, uint32_t* hist)
{
	if (!ctx) return COMPVHIP_E_INVALID_PARAMETER;
	if (!hist) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "histogram: null output");
	return hostStats(ctx, in, W, H, S, [&](const StatsFrames& g, HostCall& hc) -> int {
		HOSTSTEP(ctx, hc, ctx->dStatsU32.reserve(ctx, 256));
		const int rc = histogramImpl(g, ctx->dStatsU32);
		if (rc) return rc;
		hc.download(hist, ctx->dStatsU32, 256 * sizeof(uint32_t));
		return COMPVHIP_OK;
	});
}

int compvhip_equalize_u8(compvhip_ctx* ctx, const uint8_t* in, size_t W, size_t H, size_t S, const uint32_t* hist, double scale, uint8_t* out, size_t So, uint8_t* lut)
{
	if (!ctx) return COMPVHIP_E_INVALID_PARAMETER;
	if (!out || So < W) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "equalize: null output frame or stride < width");
	return hostStats(ctx, in, W, H, S, [&](const StatsFrames& g, HostCall& hc) -> int {
		HOSTSTEP(ctx, hc, ctx->dStatsU32.reserve(ctx, 256 + 64));          // the caller's histogram, the table behind it
		HOSTSTEP(ctx, hc, ctx->dOut.reserve(ctx, g.S * H));
		uint8_t* const dLut = reinterpret_cast<uint8_t*>(ctx->dStatsU32.ptr + 256);
		if (hist && !hc.upload(ctx->dStatsU32, hist, 256 * sizeof(uint32_t))) return hostStatus(ctx, hc);
		const int rc = equalizeImpl(g, hist ? ctx->dStatsU32.ptr : nullptr, scale, ctx->dOut, dLut);
		if (rc) return rc;
		hc.download2D(out, So, ctx->dOut, g.S, W, H);
		if (lut) hc.download(lut, dLut, 256);
		return COMPVHIP_OK;
	});
}

int compvhip_projections_u8(compvhip_ctx* ctx, const uint8_t* in, size_t W, size_t H, size_t S, int32_t* projX, int32_t* projY)
{
	if (!ctx) return COMPVHIP_E_INVALID_PARAMETER;
	if (!projX && !projY) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "projections: both outputs are NULL");
	return hostStats(ctx, in, W, H, S, [&](const StatsFrames& g, HostCall& hc) -> int {
		HOSTSTEP(ctx, hc, ctx->dStatsU32.reserve(ctx, W + H));
		int32_t* const dX = projX ? reinterpret_cast<int32_t*>(ctx->dStatsU32.ptr) : nullptr;
		int32_t* const dY = projY ? reinterpret_cast<int32_t*>(ctx->dStatsU32.ptr) + W : nullptr;
		const int rc = projectionsImpl(g, dX, dY);
		if (rc) return rc;
		if (projX) hc.download(projX, dX, W * sizeof(int32_t));
		if (projY) hc.download(projY, dY, H * sizeof(int32_t));
		return COMPVHIP_OK;
	});
}

// One frame of any served pair through the context's staging buffers: the planes lie one behind the other, rows 64-byte and planes 256-byte aligned
// (the kernel's word path), in dPacked (source) and dOut (destination).
int compvhip_convert_u8(compvhip_ctx* ctx, size_t W, size_t H, const compvhip_image* in, const compvhip_image* out)
{
	ConvertArgs h; ConvertGeometry g;
	const int rc = convertCheck(ctx, W, H, 1, in, out, &h, &g);
	if (rc) return rc;
	HIPCHK(ctx, hipSetDevice(ctx->device));
	ConvertArgs d = h;
	size_t offIn[3] = {}, offOut[3] = {}, bytesIn = 0, bytesOut = 0;
	for (int p = 0; p < g.planesIn; ++p) { d.inRow[p] = alignUp(g.minIn[p], 64); offIn[p] = bytesIn; bytesIn += alignUp(d.inRow[p] * g.rowsIn[p], 256); }
	for (int p = 0; p < g.planesOut; ++p) { d.outRow[p] = alignUp(g.minOut[p], 64); offOut[p] = bytesOut; bytesOut += alignUp(d.outRow[p] * g.rowsOut[p], 256); }
	HostCall hc(ctx->stream);
	HOSTSTEP(ctx, hc, ctx->dPacked.reserve(ctx, bytesIn));
	HOSTSTEP(ctx, hc, ctx->dOut.reserve(ctx, bytesOut));
	for (int p = 0; p < g.planesIn; ++p) {
		d.in[p] = ctx->dPacked + offIn[p];
		hc.upload2D(ctx->dPacked + offIn[p], d.inRow[p], h.in[p], h.inRow[p], g.minIn[p], g.rowsIn[p]);
	}
	for (int p = 0; p < g.planesOut; ++p) d.out[p] = ctx->dOut + offOut[p];
	HOSTSTEP(ctx, hc, launch_convert(d, in->pixfmt, out->pixfmt, 1, ctx->stream));
	for (int p = 0; p < g.planesOut; ++p) hc.download2D(h.out[p], h.outRow[p], d.out[p], d.outRow[p], g.minOut[p], g.rowsOut[p]);
	return hostWait(ctx, hc);
}

size_t compvhip_api::stagePlane(compvhip_ctx* ctx, HostCall& hc, DevBuf<uint8_t>& buf, const void* in, size_t W, size_t H, size_t S, size_t bpp)
{
	const size_t Sd = alignUp(W, 64);
	if (hc.ok()) hc.step(buf.reserve(ctx, Sd * H * bpp), "plane staging");
	hc.upload2D(buf, Sd * bpp, in, S * bpp, W * bpp, H, "plane upload");
	return Sd;
}
