// api_features.cpp -- plan-level calls of the features built on the Canny / SHT plan: line segments, line fits, connected components,
// thresholding and morphology, FAST corners, ORB keypoints and descriptors, bilinear scale and the ORB pyramid, remap and inverse warp, brute-force matching, HOG, image
// statistics.  (The RANSAC homography and curve fits: api_ransac.cpp.)
#include "api_internal.hpp"

// what the segment and the fit kernels read alike: the edge pixels, the vote's tables, the lines
static void fillLineSet(ShtLineSetArgs& a, const compvhip_plan* p, const uint8_t* d_edges, size_t edgeStride, const compvhip_line* d_lines, const int32_t* d_counts,
                        size_t lineCap, size_t nLines)
{
	a.ebits = p->ebits; a.edges = d_edges; a.bitsFrameStride = p->bitsFrameStride; a.edgeFrameStride = edgeStride * p->H; a.wb = p->wb; a.S = static_cast<int>(edgeStride);
	a.sinQ = p->sinQ; a.cosQ = p->cosQ; a.lines = d_lines; a.lineCounts = d_counts; a.lineCap = lineCap; a.nLines = static_cast<int>(nLines);
	a.W = static_cast<int>(p->W); a.H = static_cast<int>(p->H); a.R = static_cast<int>(p->R); a.T = static_cast<int>(p->T); a.barrier = static_cast<int>(p->W + p->H);
}

// ---- Hough line segments (sht_segments_kernels.hip; definition in include/compv_hip.h) ---------------------------------------
// edges / edgeStride: byte maps [frames][H][edgeStride], or nullptr = the plan's bit masks
int compvhip_api::segmentsImpl(compvhip_plan* p, const uint8_t* d_edges, size_t edgeStride, const compvhip_line* d_lines, const int32_t* d_counts, size_t lineCap,
                               int maxLines, int minLength, int maxGap, compvhip_segment* d_segs, size_t segCap, int32_t* d_segCounts, hipStream_t st)
{
	compvhip_ctx* ctx = p->ctx;
	if (!d_lines || !d_counts || !d_segCounts || !lineCap || (segCap && !d_segs)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "null line / count / segment buffer");
	if (minLength < 1 || maxGap < 0) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "segments need minLength >= 1 and maxGap >= 0");
	if (misaligned(3, d_lines, d_counts, d_segs, d_segCounts)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "lines, segments and counts must be 4-byte aligned");
	HIPCHK(ctx, hipSetDevice(ctx->device));
	int rc = ensureSht(p);
	if (rc) return rc;
	size_t nLines = std::min(lineCap, p->R * p->T);   // a frame has at most R * T lines
	if (maxLines > 0) nLines = std::min(nLines, static_cast<size_t>(maxLines));
	if (nLines > static_cast<size_t>(INT32_MAX)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "line capacity beyond 2^31");
	HIPCHK(ctx, p->segPerLine.reserve(ctx, nLines * p->frames));
	if (p->timing) timelineClear(p);
	ShtSegArgs a;
	fillLineSet(a, p, d_edges, edgeStride, d_lines, d_counts, lineCap, nLines);
	a.minLength = minLength; a.maxGap = maxGap; a.perLine = p->segPerLine; a.segs = d_segs; a.segCap = segCap; a.segCounts = d_segCounts; a.frame0 = 0;
	const int frames = static_cast<int>(p->frames);
	{ Stamp s(p, st, "sht_segments_count_kernel"); HIPCHK(ctx, launch_sht_segments(a, frames, 0, st)); }
	{ Stamp s(p, st, "sht_segments_scan_kernel"); HIPCHK(ctx, launch_sht_segments(a, frames, 1, st)); }
	if (segCap) { Stamp s(p, st, "sht_segments_write_kernel"); HIPCHK(ctx, launch_sht_segments(a, frames, 2, st)); }
	return COMPVHIP_OK;
}

int compvhip_plan_houghsht_segments(compvhip_plan* p, const uint8_t* d_edges, const compvhip_line* d_lines, const int32_t* d_counts, size_t lineCap, int maxLines,
                                    int minLength, int maxGap, compvhip_segment* d_segs, size_t segCap, int32_t* d_segCounts, void* stream)
{
	if (!p) return COMPVHIP_E_INVALID_PARAMETER;
	compvhip_ctx* ctx = p->ctx;
	if (stepsInFlight(p)) return fail(ctx, COMPVHIP_E_INVALID_STATE, "asynchronous steps in flight: call compvhip_plan_wait first (a replayed step rewrites the lines)");
	if (!segCap) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "segCap must be > 0");
	if (!d_edges && !p->bitsValid) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "no edge masks of a Canny run on this plan: pass d_edges");
	return segmentsImpl(p, d_edges, p->S, d_lines, d_counts, lineCap, maxLines, minLength, maxGap, d_segs, segCap, d_segCounts, static_cast<hipStream_t>(stream));
}

// ---- Hough line refinement (sht_fit_kernels.hip; definition in include/compv_hip.h) -------------------------------------------
// edges / edgeStride: byte maps [frames][H][edgeStride], or nullptr = the plan's bit masks
int compvhip_api::fitImpl(compvhip_plan* p, const uint8_t* d_edges, size_t edgeStride, const compvhip_line* d_lines, const int32_t* d_counts, size_t lineCap, int maxLines,
                   int halfWidth, const compvhip_segment* d_segs, const int32_t* d_segCounts, size_t segCap, compvhip_line_fit* d_fits, size_t fitCap,
                   int32_t* d_fitCounts, compvhip_line* d_refined, hipStream_t st)
{
	compvhip_ctx* ctx = p->ctx;
	if (!d_lines || !d_counts || !d_fitCounts || !lineCap || (fitCap && !d_fits)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "null line / count / fit buffer");
	if (d_segs && (!d_segCounts || d_refined)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "per-segment fits need d_segCounts and take no d_refined");
	if (halfWidth < 0 || halfWidth > kFitMaxHalfWidth) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "halfWidth must be 0 .. 8");
	if (misaligned(3, d_lines, d_counts, d_segs, d_segCounts, d_fitCounts, d_refined) || misaligned(alignof(compvhip_line_fit) - 1, d_fits))
		return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "fit records must be 8-byte aligned; lines, segments and counts 4-byte aligned");
	if (std::max(p->W, p->H) > kFitMaxSide) return fail(ctx, COMPVHIP_E_NOT_IMPLEMENTED, "line fits need max(W, H) <= 8192 (int64 central moments)");
	HIPCHK(ctx, hipSetDevice(ctx->device));
	int rc = ensureSht(p);
	if (rc) return rc;
	size_t nLines = std::min(lineCap, p->R * p->T);   // a frame has at most R * T lines
	if (maxLines > 0) nLines = std::min(nLines, static_cast<size_t>(maxLines));
	if (nLines > static_cast<size_t>(INT32_MAX) || (d_segs && segCap > static_cast<size_t>(INT32_MAX)))
		return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "line / segment capacity beyond 2^31");
	if (p->timing) timelineClear(p);
	ShtFitArgs a;
	fillLineSet(a, p, d_edges, edgeStride, d_lines, d_counts, lineCap, nLines);
	a.halfWidth = halfWidth; a.segs = d_segs; a.segCounts = d_segCounts; a.segCap = d_segs ? segCap : 0;
	a.fits = d_fits; a.fitCap = fitCap; a.fitCounts = d_fitCounts; a.refined = d_refined; a.frame0 = 0;
	{ Stamp s(p, st, "sht_fit_kernel"); HIPCHK(ctx, launch_sht_fit(a, static_cast<int>(p->frames), st)); }
	return COMPVHIP_OK;
}

int compvhip_plan_houghsht_fit(compvhip_plan* p, const uint8_t* d_edges, const compvhip_line* d_lines, const int32_t* d_counts, size_t lineCap, int maxLines,
                               int halfWidth, const compvhip_segment* d_segs, const int32_t* d_segCounts, size_t segCap, compvhip_line_fit* d_fits, size_t fitCap,
                               int32_t* d_fitCounts, compvhip_line* d_refined, void* stream)
{
	if (!p) return COMPVHIP_E_INVALID_PARAMETER;
	compvhip_ctx* ctx = p->ctx;
	if (stepsInFlight(p)) return fail(ctx, COMPVHIP_E_INVALID_STATE, "asynchronous steps in flight: call compvhip_plan_wait first (a replayed step rewrites the lines)");
	if (!d_edges && !p->bitsValid) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "no edge masks of a Canny run on this plan: pass d_edges");
	return fitImpl(p, d_edges, p->S, d_lines, d_counts, lineCap, maxLines, halfWidth, d_segs, d_segCounts, segCap, d_fits, fitCap, d_fitCounts, d_refined,
	               static_cast<hipStream_t>(stream));
}

// ---- connected components (components_kernels.hip; definition in include/compv_hip.h) -----------------------------------------
// edges / edgeStride: byte maps [frames][H][edgeStride] (packed into the plan's compBits first), or nullptr = the plan's bit masks
int compvhip_api::componentsImpl(compvhip_plan* p, const uint8_t* d_edges, size_t edgeStride, int connectivity, int minPixels, int32_t* d_labels, size_t labelStride,
                          compvhip_component* d_comps, size_t compCap, int32_t* d_compCounts, hipStream_t st)
{
	compvhip_ctx* ctx = p->ctx;
	if (connectivity != 4 && connectivity != 8) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "connectivity must be 4 or 8");
	if (minPixels < 1) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "minPixels must be >= 1");
	if (!d_compCounts || (compCap && !d_comps)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "null count / record buffer");
	if (d_labels && labelStride < p->W) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "labelStride < W");
	if (misaligned(3, d_labels, d_comps, d_compCounts)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "labels, records and counts must be 4-byte aligned");
	if (p->W * p->H > static_cast<size_t>(INT32_MAX)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "W * H beyond 2^31");
	HIPCHK(ctx, hipSetDevice(ctx->device));
	const size_t frames = p->frames;
	HIPCHK(ctx, p->compRows.reserve(ctx, p->H * frames));
	if (d_edges) HIPCHK(ctx, p->compBits.reserve(ctx, p->bitsFrameStride * frames));
	if (!d_labels) HIPCHK(ctx, p->compParent.reserve(ctx, p->W * p->H * frames));
	if (p->timing) timelineClear(p);
	const int nf = static_cast<int>(frames);
	if (d_edges) {
		Stamp s(p, st, "bytes_to_bits_kernel");
		HIPCHK(ctx, launch_bytes_to_bits(d_edges, static_cast<int>(p->W), static_cast<int>(p->H), static_cast<int>(edgeStride), edgeStride * p->H, p->compBits, p->wb,
		                                 p->bitsFrameStride, nf, st));
	}
	CompArgs a;
	a.bits = d_edges ? p->compBits : p->ebits; a.bitsFrameStride = p->bitsFrameStride; a.wb = p->wb;
	a.W = static_cast<int>(p->W); a.H = static_cast<int>(p->H); a.words = static_cast<int>((p->W + 31) / 32);
	a.lastMask = (p->W & 31) ? (1u << (p->W & 31)) - 1u : ~0u;
	a.conn8 = connectivity == 8; a.minPixels = minPixels;
	a.parent = d_labels ? d_labels : p->compParent; a.ps = static_cast<int>(d_labels ? labelStride : p->W);
	a.parentFrameStride = static_cast<size_t>(a.ps) * p->H; a.wantLabels = d_labels != nullptr;
	a.comps = d_comps; a.compCap = compCap; a.compCounts = d_compCounts; a.rowCounts = p->compRows; a.frame0 = 0;
	static const char* const names[9] = { "comp_tile_kernel", "comp_border_kernel", "comp_flatten_kernel", "comp_count_kernel", "comp_rows_kernel<false>",
	                                      "comp_scan_kernel", "comp_rows_kernel<true>", "comp_boxes_kernel", "comp_finish_kernel" };
	for (int phase = 0; phase < 9; ++phase) {
		if (phase == 7 && !a.wantLabels && !compCap) continue;   // nothing to label, no box to grow
		if (phase == 8 && !a.wantLabels) continue;
		Stamp s(p, st, names[phase]);
		HIPCHK(ctx, launch_components(a, nf, phase, st));
	}
	return COMPVHIP_OK;
}

int compvhip_plan_components(compvhip_plan* p, const uint8_t* d_edges, int connectivity, int minPixels, int32_t* d_labels, size_t labelStride,
                             compvhip_component* d_comps, size_t compCap, int32_t* d_compCounts, void* stream)
{
	if (!p) return COMPVHIP_E_INVALID_PARAMETER;
	compvhip_ctx* ctx = p->ctx;
	if (stepsInFlight(p)) return fail(ctx, COMPVHIP_E_INVALID_STATE, "asynchronous steps in flight: call compvhip_plan_wait first (a replayed step rewrites the masks)");
	if (!d_edges && !p->bitsValid) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "no edge masks of a Canny run on this plan: pass d_edges");
	if (labelStride > static_cast<size_t>(INT32_MAX)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "labelStride beyond 2^31");
	return componentsImpl(p, d_edges, p->S, connectivity, minPixels, d_labels, labelStride, d_comps, compCap, d_compCounts, static_cast<hipStream_t>(stream));
}

// ---- thresholding and morphology (morph_kernels.hip; definitions in include/compv_hip.h) ---------------------------------------------------
static bool planeOverlap(const compvhip_plan* p, const uint8_t* a, const uint8_t* b)
{
	const size_t span = p->S * p->H * p->frames;
	return overlaps(a, span, b, span);
}

// COMPV_MATH_ROUNDFU_2_NEAREST_INT(COMPV_MATH_CLIP3(0x00, 0xff, v), int) (compv_image_threshold.cxx:133-136,213-220)
static int roundClipU8(double v) { return static_cast<int>((v > 255.0 ? 255.0 : (v < 0.0 ? 0.0 : v)) + 0.5); }

int compvhip_plan_threshold(compvhip_plan* p, const uint8_t* d_in, double threshold, const int32_t* d_levels, uint8_t* d_out, void* stream)
{
	if (!p) return COMPVHIP_E_INVALID_PARAMETER;
	compvhip_ctx* ctx = p->ctx;
	if (!d_in || !d_out) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "null frame pointer");
	if (!d_levels && !(threshold >= 0.0)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "threshold < 0"); // compv_image_threshold.cxx:120
	if (misaligned(3, d_levels)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "levels must be 4-byte aligned");
	HIPCHK(ctx, hipSetDevice(ctx->device));
	hipStream_t st = static_cast<hipStream_t>(stream);
	if (p->timing) timelineClear(p);
	ThreshArgs a;
	a.in = d_in; a.out = d_out; a.levels = d_levels; a.frameStride = p->S * p->H;
	a.W = static_cast<int>(p->W); a.H = static_cast<int>(p->H); a.S = static_cast<int>(p->S);
	a.t8 = d_levels ? 0 : roundClipU8(threshold);
	Stamp s(p, st, "threshold_kernel");
	HIPCHK(ctx, launch_threshold(a, static_cast<int>(p->frames), st));
	return COMPVHIP_OK;
}

int compvhip_api::checkAdaptive(compvhip_ctx* ctx, size_t W, size_t H, size_t blockSize, double delta, double maxVal)
{
	if (!(blockSize & 1) || blockSize < 3) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "blockSize must be odd and >= 3"); // compv_image_threshold.cxx:185
	if (blockSize > 31) return fail(ctx, COMPVHIP_E_NOT_IMPLEMENTED, "adaptive threshold supports block sizes 3..31");
	if (W < blockSize || H < blockSize) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "image smaller than the block"); // compv_math_convlt.h:100
	if (!(maxVal >= 0.0) || delta != delta) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "maxVal < 0"); // compv_image_threshold.cxx:202
	return COMPVHIP_OK;
}

int compvhip_plan_threshold_adaptive(compvhip_plan* p, const uint8_t* d_in, size_t blockSize, double delta, double maxVal, int invert, uint8_t* d_out, void* stream)
{
	if (!p) return COMPVHIP_E_INVALID_PARAMETER;
	compvhip_ctx* ctx = p->ctx;
	if (!d_in || !d_out) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "null frame pointer");
	int rc = checkAdaptive(ctx, p->W, p->H, blockSize, delta, maxVal);
	if (rc) return rc;
	HIPCHK(ctx, hipSetDevice(ctx->device));
	const size_t span = p->S * p->H * p->frames;
	const bool alias = planeOverlap(p, d_in, d_out);
	if (alias && d_in != d_out) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "input and output overlap without being the same buffer");
	if (alias) HIPCHK(ctx, p->morphTmp.reserve(ctx, span)); // a tile reads the halo its neighbours write: in place goes through the plan's plane
	hipStream_t st = static_cast<hipStream_t>(stream);
	if (p->timing) timelineClear(p);
	AdaptArgs a;
	a.in = d_in; a.out = alias ? p->morphTmp : d_out; a.frameStride = p->S * p->H;
	a.W = static_cast<int>(p->W); a.H = static_cast<int>(p->H); a.S = static_cast<int>(p->S);
	a.r = static_cast<int>(blockSize >> 1);
	a.k = static_cast<uint16_t>((1.f / static_cast<float>(blockSize)) * 0xffff);   // CompVKernel::mean (compv_kernel.cxx:16) through fixedPointKernel (compv_math_convlt.h:88)
	a.delta = roundClipU8(delta); a.maxVal = roundClipU8(maxVal); a.invert = invert != 0;
	{
		Stamp s(p, st, "threshold_adaptive_kernel");
		HIPCHK(ctx, launch_threshold_adaptive(a, static_cast<int>(p->frames), st));
	}
	if (alias) {   // rows only up to W: the padding columns of the caller's buffer stay as they are
		for (size_t f = 0; f < p->frames; ++f)
			HIPCHK(ctx, hipMemcpy2DAsync(d_out + f * p->S * p->H, p->S, p->morphTmp + f * p->S * p->H, p->S, p->W, p->H, hipMemcpyDeviceToDevice, st));
	}
	return COMPVHIP_OK;
}

// buildStructuringElementGeneric (compv_math_morph.cxx:476-540)
int compvhip_morph_strel(int type, size_t w, size_t h, uint8_t* strel)
{
	if (!strel || !w || !h) return COMPVHIP_E_INVALID_PARAMETER; // :478
	if (type != COMPVHIP_MORPH_STREL_RECT && type != COMPVHIP_MORPH_STREL_DIAMOND && type != COMPVHIP_MORPH_STREL_CROSS) return COMPVHIP_E_NOT_IMPLEMENTED; // :534
	if (type == COMPVHIP_MORPH_STREL_DIAMOND && w != h) return COMPVHIP_E_INVALID_PARAMETER;
	if (type == COMPVHIP_MORPH_STREL_RECT) { memset(strel, 0xff, w * h); return COMPVHIP_OK; }
	memset(strel, 0, w * h);
	if (type == COMPVHIP_MORPH_STREL_CROSS) {
		memset(strel + (h >> 1) * w, 0xff, w);
		for (size_t j = 0; j < h; ++j) strel[j * w + (w >> 1)] = 0xff;
		return COMPVHIP_OK;
	}
	const size_t c = w >> 1;
	for (size_t j = 0; j < h; ++j) {   // 1, 3, 5, ... members centred on column w / 2 down to the middle row, then back
		const size_t half = j <= (h >> 1) ? j : h - 1 - j;
		memset(strel + j * w + c - half, 0xff, 2 * half + 1);
	}
	return COMPVHIP_OK;
}

// strel -> member masks + the kernel that serves it
int compvhip_api::morphPrepare(compvhip_ctx* ctx, size_t W, size_t H, const uint8_t* strel, size_t sw, size_t sh, int op, int border, int kernel, MorphArgs* a)
{
	if (!strel || !sw || !sh) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "null / empty structuring element");
	if (!(sw & 1) || !(sh & 1) || sw > static_cast<size_t>(kMorphMaxStrel) || sh > static_cast<size_t>(kMorphMaxStrel))
		return fail(ctx, COMPVHIP_E_NOT_IMPLEMENTED, "structuring elements are odd-sized, 1..31 a side");
	if (W < sw || H < sh) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "image smaller than the structuring element"); // compv_math_morph.cxx:131
	if (op != COMPVHIP_MORPH_OP_ERODE && op != COMPVHIP_MORPH_OP_DILATE && op != COMPVHIP_MORPH_OP_OPEN && op != COMPVHIP_MORPH_OP_CLOSE)
		return fail(ctx, COMPVHIP_E_NOT_IMPLEMENTED, "morph op (erode, dilate, open, close)"); // :119
	if (border != COMPVHIP_BORDER_REPLICATE && border != COMPVHIP_BORDER_ZERO) return fail(ctx, COMPVHIP_E_NOT_IMPLEMENTED, "border type (replicate, zero)"); // :571
	size_t members = 0, cross = 0;
	for (size_t j = 0; j < sh; ++j) {
		uint32_t m = 0;
		for (size_t i = 0; i < sw; ++i) {
			if (!strel[j * sw + i]) continue;
			m |= 1u << i; ++members;
			if (j == (sh >> 1) || i == (sw >> 1)) ++cross;
		}
		a->rows[j] = m;
	}
	for (size_t j = sh; j < static_cast<size_t>(kMorphMaxStrel); ++j) a->rows[j] = 0;
	if (!members) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "structuring element is full of zeros"); // :460
	const bool isRect = members == sw * sh, isCross = !isRect && members == cross && cross == sw + sh - 1;
	if (kernel == COMPVHIP_MORPH_KERNEL_GENERAL) a->kind = kMorphGeneral;
	else if (kernel == COMPVHIP_MORPH_KERNEL_AUTO || kernel == COMPVHIP_MORPH_KERNEL_SEPARABLE) {
		a->kind = isRect ? kMorphRect : (isCross ? kMorphCross : kMorphGeneral);
		// up to 15 members the member-list kernel is the faster one (3x3: 0.28 ms against 0.35 ms at 4K x 32; docs/kernels/morph.md): the second LDS plane
		// and barrier of the separable kernel cost more than the taps it saves
		if (kernel == COMPVHIP_MORPH_KERNEL_AUTO && members <= kMorphGeneralMaxMembers) a->kind = kMorphGeneral;
		if (kernel == COMPVHIP_MORPH_KERNEL_SEPARABLE && a->kind == kMorphGeneral)
			return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "the separable kernel serves full rectangles and crosses only");
	}
	else return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "kernel selector");
	a->sw = static_cast<int>(sw); a->sh = static_cast<int>(sh); a->replicate = border == COMPVHIP_BORDER_REPLICATE;
	return COMPVHIP_OK;
}

int compvhip_plan_morph_ex(compvhip_plan* p, const uint8_t* d_in, const uint8_t* strel, size_t sw, size_t sh, int op, int border, int kernel, uint8_t* d_out,
                           void* stream)
{
	if (!p) return COMPVHIP_E_INVALID_PARAMETER;
	compvhip_ctx* ctx = p->ctx;
	if (!d_in || !d_out) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "null frame pointer");
	MorphArgs a;
	int rc = morphPrepare(ctx, p->W, p->H, strel, sw, sh, op, border, kernel, &a);
	if (rc) return rc;
	if (planeOverlap(p, d_in, d_out)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "input and output must not overlap"); // compv_math_morph.cxx:140-145 reallocates
	HIPCHK(ctx, hipSetDevice(ctx->device));
	const bool two = op == COMPVHIP_MORPH_OP_OPEN || op == COMPVHIP_MORPH_OP_CLOSE;
	if (two) HIPCHK(ctx, p->morphTmp.reserve(ctx, p->S * p->H * p->frames));
	hipStream_t st = static_cast<hipStream_t>(stream);
	if (p->timing) timelineClear(p);
	a.frameStride = p->S * p->H; a.W = static_cast<int>(p->W); a.H = static_cast<int>(p->H); a.S = static_cast<int>(p->S);
	const int nf = static_cast<int>(p->frames);
	static const char* const names[3] = { "morph_general_kernel", "morph_separable_kernel<rect>", "morph_separable_kernel<cross>" };
	// OPEN = erode then dilate, CLOSE = dilate then erode (compv_math_morph.cxx:104-111): two complete basic operations, borders included
	a.in = d_in; a.out = two ? p->morphTmp : d_out; a.dilate = op == COMPVHIP_MORPH_OP_DILATE || op == COMPVHIP_MORPH_OP_CLOSE;
	{ Stamp s(p, st, names[a.kind]); HIPCHK(ctx, launch_morph(a, nf, st)); }
	if (two) {
		a.in = p->morphTmp; a.out = d_out; a.dilate = !a.dilate;
		Stamp s(p, st, names[a.kind]); HIPCHK(ctx, launch_morph(a, nf, st));
	}
	return COMPVHIP_OK;
}

int compvhip_plan_morph(compvhip_plan* p, const uint8_t* d_in, const uint8_t* strel, size_t sw, size_t sh, int op, int border, uint8_t* d_out, void* stream)
{
	return compvhip_plan_morph_ex(p, d_in, strel, sw, sh, op, border, COMPVHIP_MORPH_KERNEL_AUTO, d_out, stream);
}

// ---- FAST corners (fast_kernels.hip; definition in include/compv_hip.h) ------------------------------------------------------------------
int compvhip_api::checkFast(compvhip_ctx* ctx, size_t W, size_t H, int fastType)
{
	if (W < 7 || H < 7) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "FAST needs W, H >= 7 (one interior pixel)");
	if (fastType != 9 && fastType != 12) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "fastType must be 9 or 12"); // compv_core_feature_fast_dete.cxx:146
	return COMPVHIP_OK;
}

// ints of FAST's scratch for `frames` planes of H rows: [frames][H] corners per row, [frames][256] score histogram, [frames] cut level, [frames][H] row scan
static size_t fastWorkInts(size_t frames, size_t H) { return frames * (2 * H + 257); }

// the arguments of launch_fast for `frames` planes [H][S] on `work` (fastWorkInts(frames, H) ints at least); enqueues the fill of the sums in it
static hipError_t fastArgs(FastArgs& a, const uint8_t* plane, size_t W, size_t H, size_t S, size_t frames, int threshold, int fastType, int nonmax, int maxFeatures,
                           int* work, uint8_t* scores, compvhip_corner* corners, size_t cornerCap, int32_t* counts, hipStream_t st)
{
	a.in = plane; a.scores = scores; a.frameStride = S * H;
	a.W = static_cast<int>(W); a.H = static_cast<int>(H); a.S = static_cast<int>(S);
	a.t = threshold < 0 ? 0 : (threshold > 255 ? 255 : threshold); a.N = fastType; a.nonmax = nonmax != 0; a.maxFeatures = maxFeatures;   // compv_core_feature_fast_dete.cxx:135
	a.rowCounts = work; a.hist = a.rowCounts + frames * H; a.minScore = a.hist + frames * 256; a.rowOffsets = a.minScore + frames;
	a.corners = corners; a.cornerCap = cornerCap; a.counts = counts;
	return hipMemsetAsync(a.rowCounts, 0, frames * (H + 256) * sizeof(int), st);   // the row counts and the histogram are sums
}

int compvhip_plan_fast(compvhip_plan* p, const uint8_t* d_gray, int threshold, int fastType, int nonmax, int maxFeatures, uint8_t* d_scores,
                       compvhip_corner* d_corners, size_t cornerCap, int32_t* d_counts, void* stream)
{
	if (!p) return COMPVHIP_E_INVALID_PARAMETER;
	compvhip_ctx* ctx = p->ctx;
	if (!d_gray || !d_counts || (cornerCap && !d_corners)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "null frame / count / corner pointer");
	int rc = refuseBeyondLaunchLimit(ctx, p->frames, "compvhip_plan_fast");
	if (rc) return rc;
	rc = checkFast(ctx, p->W, p->H, fastType);
	if (rc) return rc;
	if (misaligned(7, d_gray, d_scores)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "frames must be 8-byte aligned");
	if (misaligned(3, d_corners, d_counts)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "records and counts must be 4-byte aligned");
	if (d_scores && planeOverlap(p, d_gray, d_scores)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "frame and score map must not overlap");
	HIPCHK(ctx, hipSetDevice(ctx->device));
	const size_t F = p->frames, H = p->H;
	HIPCHK(ctx, p->fastWork.reserve(ctx, fastWorkInts(F, H)));
	if (!d_scores) HIPCHK(ctx, p->fastScores.reserve(ctx, p->S * H * F));
	hipStream_t st = static_cast<hipStream_t>(stream);
	if (p->timing) timelineClear(p);
	FastArgs a;
	HIPCHK(ctx, fastArgs(a, d_gray, p->W, H, p->S, F, threshold, fastType, nonmax, maxFeatures, p->fastWork, d_scores ? d_scores : p->fastScores, d_corners, cornerCap, d_counts, st));
	{ Stamp s(p, st, "fast_score_kernel"); HIPCHK(ctx, launch_fast(a, static_cast<int>(F), 0, st)); }
	{ Stamp s(p, st, "fast_list_kernels"); HIPCHK(ctx, launch_fast(a, static_cast<int>(F), 1, st)); }   // cut level, row recount, scan, emit
	return COMPVHIP_OK;
}

// ---- ORB keypoints and descriptors (orb_kernels.hip; definition in include/compv_hip.h) -------------------------------------------------------
int compvhip_api::checkOrb(compvhip_ctx* ctx, size_t W, size_t H, float scale)
{
	if (W < 2 * kOrbBorder + 1 || H < 2 * kOrbBorder + 1) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "ORB needs W, H >= 37 (one position 18 pixels from every border)");
	if (!(scale > 0.f)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "scale must be > 0");
	return COMPVHIP_OK;
}

int compvhip_plan_orb_keypoints(compvhip_plan* p, const uint8_t* d_gray, const compvhip_corner* d_corners, size_t cornerCap, const int32_t* d_cornerCounts, int level,
                                float scale, compvhip_keypoint* d_keypoints, size_t keyCap, int32_t* d_keyCounts, int32_t* d_moments, void* stream)
{
	if (!p) return COMPVHIP_E_INVALID_PARAMETER;
	compvhip_ctx* ctx = p->ctx;
	if (!d_gray || !d_corners || !d_cornerCounts || !d_keyCounts || (keyCap && !d_keypoints)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "null frame / corner / count / keypoint pointer");
	int rc = refuseBeyondLaunchLimit(ctx, p->frames, "compvhip_plan_orb_keypoints");
	if (rc) return rc;
	rc = checkOrb(ctx, p->W, p->H, scale);
	if (rc) return rc;
	if (cornerCap > static_cast<size_t>(INT32_MAX) || keyCap > static_cast<size_t>(INT32_MAX)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "capacity beyond 2^31");
	if (misaligned(3, d_corners, d_cornerCounts, d_keypoints, d_keyCounts, d_moments, d_gray))
		return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "frames, records, counts and moments must be 4-byte aligned");
	HIPCHK(ctx, hipSetDevice(ctx->device));
	const int frames = static_cast<int>(p->frames);
	HIPCHK(ctx, p->orbIndex.reserve(ctx, p->frames * keyCap));
	hipStream_t st = static_cast<hipStream_t>(stream);
	if (p->timing) timelineClear(p);
	OrbKeyArgs a;
	a.gray = d_gray; a.frameStride = p->S * p->H; a.W = static_cast<int>(p->W); a.H = static_cast<int>(p->H); a.S = static_cast<int>(p->S);
	a.corners = d_corners; a.cornerCap = cornerCap; a.cornerCounts = d_cornerCounts; a.level = level; a.scale = scale;
	a.index = p->orbIndex; a.keys = d_keypoints; a.keyCap = keyCap; a.keyCounts = d_keyCounts; a.moments = d_moments;
	{ Stamp s(p, st, "orb_select_kernel"); HIPCHK(ctx, launch_orb_select(a, frames, st)); }
	if (keyCap) { Stamp s(p, st, "orb_orient_kernel"); HIPCHK(ctx, launch_orb_orient(a, frames, st)); }
	return COMPVHIP_OK;
}

int compvhip_plan_orb_describe(compvhip_plan* p, const uint8_t* d_gray, const compvhip_keypoint* d_keypoints, size_t keyCap, const int32_t* d_keyCounts, float scale,
                               int blur, uint8_t* d_desc, size_t descStride, void* stream)
{
	if (!p) return COMPVHIP_E_INVALID_PARAMETER;
	compvhip_ctx* ctx = p->ctx;
	if (!d_gray || !d_keypoints || !d_keyCounts || !d_desc || !keyCap) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "null frame / keypoint / count / descriptor pointer or keyCap == 0");
	int rc = refuseBeyondLaunchLimit(ctx, p->frames, "compvhip_plan_orb_describe");
	if (rc) return rc;
	rc = checkOrb(ctx, p->W, p->H, scale);
	if (rc) return rc;
	if (descStride < 32 || (descStride & 3)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "descStride below 32 or no multiple of 4");
	if (keyCap > static_cast<size_t>(INT32_MAX)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "capacity beyond 2^31");
	if (misaligned(3, d_gray, d_keypoints, d_keyCounts, d_desc))
		return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "frames, records, counts and descriptors must be 4-byte aligned");
	HIPCHK(ctx, hipSetDevice(ctx->device));
	const int frames = static_cast<int>(p->frames);
	if (!p->orbKernReady) {
		if (compvhip_gauss_kernel_fixedpoint(5, 2.0f, p->orbKern) != COMPVHIP_OK) return fail(ctx, COMPVHIP_E_INVALID_STATE, "Gaussian kernel");   // compv_core_feature_orb_desc.cxx:119-120
		const char* e = getenv("COMPVHIP_ORB_BRIEF");   // lab knob (tools/orb_bench.py, tests): "lds" / "global" name the byte-read variant of orb_brief_kernel
		p->orbBriefLds = e ? !strcmp(e, "lds") : kOrbBriefLdsDefault;
		p->orbKernReady = true;
	}
	if (blur) HIPCHK(ctx, p->orbBlur.reserve(ctx, p->S * p->H * p->frames));
	hipStream_t st = static_cast<hipStream_t>(stream);
	if (p->timing) timelineClear(p);
	if (blur) {   // out of place: the fused kernel, no intermediate
		Stamp s(p, st, "convlt_fxp_kernels");
		HIPCHK(ctx, launch_convlt_fxp(d_gray, nullptr, p->orbBlur, static_cast<int>(p->W), static_cast<int>(p->H), static_cast<int>(p->S), p->S * p->H, frames, p->orbKern,
		                              p->orbKern, 5, st));
	}
	OrbDescArgs a;
	a.blurred = blur ? p->orbBlur : d_gray; a.frameStride = p->S * p->H; a.W = static_cast<int>(p->W); a.H = static_cast<int>(p->H); a.S = static_cast<int>(p->S);
	a.keys = d_keypoints; a.keyCap = keyCap; a.keyCounts = d_keyCounts; a.scale = scale; a.desc = d_desc; a.descStride = descStride;
	{ Stamp s(p, st, p->orbBriefLds ? "orb_brief_kernel" : "orb_brief_kernel_global"); HIPCHK(ctx, launch_orb_brief(a, frames, p->orbBriefLds, st)); }
	return COMPVHIP_OK;
}

// ---- bilinear scale and the ORB pyramid (scale_kernels.hip, orb_kernels.hip; definition in include/compv_hip.h) ---------------------------------------
int compvhip_api::scaleImpl(compvhip_ctx* ctx, const uint8_t* d_in, size_t W, size_t H, size_t S, size_t frames, uint8_t* d_out, size_t Wout, size_t Hout, size_t Sout,
                            hipStream_t st)
{
	if (!d_in || !d_out) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "null frame pointer");
	if (!Wout || !Hout || Wout > 32767 || Hout > 32767 || W > 32767 || H > 32767 || Sout < Wout || Sout > static_cast<size_t>(INT32_MAX))
		return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "scale: a size of 0 or beyond 32767, or Sout < Wout");
	const size_t inSpan = S * H * frames, outSpan = Sout * Hout * frames;
	if (d_in < d_out + outSpan && d_out < d_in + inSpan) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "input and output must not overlap");
	ScaleArgs a;
	a.in = d_in; a.frameStride = S * H; a.W = static_cast<int>(W); a.H = static_cast<int>(H); a.S = static_cast<int>(S); a.levels = 1;
	ScaleLevel& L = a.lv[0];
	L.out = d_out; L.frameStride = Sout * Hout; L.W = static_cast<int>(Wout); L.H = static_cast<int>(Hout); L.S = static_cast<int>(Sout);
	if (!scale_level_init(L, a.W, a.H)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "scale ratio outside (0, 256)");   // compv_image_scale_bilinear.cxx:175
	HIPCHK(ctx, launch_scale_bilinear(a, static_cast<int>(frames), st));
	return COMPVHIP_OK;
}

int compvhip_plan_scale(compvhip_plan* p, const uint8_t* d_in, uint8_t* d_out, size_t Wout, size_t Hout, size_t Sout, void* stream)
{
	if (!p) return COMPVHIP_E_INVALID_PARAMETER;
	compvhip_ctx* ctx = p->ctx;
	if (int rc = refuseBeyondLaunchLimit(ctx, p->frames, "compvhip_plan_scale")) return rc;   // (scaleImpl's other callers: one frame, or a pyramid's, limited at its creation)
	HIPCHK(ctx, hipSetDevice(ctx->device));
	hipStream_t st = static_cast<hipStream_t>(stream);
	if (p->timing) timelineClear(p);
	Stamp s(p, st, "scale_bilinear_kernel");
	return scaleImpl(ctx, d_in, p->W, p->H, p->S, p->frames, d_out, Wout, Hout, Sout, st);
}

// ---- remap and inverse warp (remap_kernels.hip; definition in include/compv_hip.h) ------------------------------------------------------------------
int compvhip_warp_tables(const float* M, int rows, size_t Wout, size_t Hout, float* ac, float* df, float* gi, float* by, float* ey, float* hy)
{
	if (!M || (rows != 2 && rows != 3) || !Wout || !Hout || !ac || !df || !by || !ey || (rows == 3 && (!gi || !hy))) return COMPVHIP_E_INVALID_PARAMETER;
	// compv_image.cxx:1031-1048,1114-1137: running sums, one float32 addition per entry (this file is built with -ffp-contract=off)
	const float a = M[0], b = M[1], c = M[2], d = M[3], e = M[4], f = M[5];
	ac[0] = c; df[0] = f;
	for (size_t x = 1; x < Wout; ++x) { ac[x] = ac[x - 1] + a; df[x] = df[x - 1] + d; }
	by[0] = 0.f; ey[0] = 0.f;
	for (size_t y = 1; y < Hout; ++y) { by[y] = by[y - 1] + b; ey[y] = ey[y - 1] + e; }
	if (rows == 3) {
		const float g = M[6], h = M[7];
		gi[0] = M[8];
		for (size_t x = 1; x < Wout; ++x) gi[x] = gi[x - 1] + g;
		hy[0] = 0.f;
		for (size_t y = 1; y < Hout; ++y) hy[y] = hy[y - 1] + h;
	}
	return COMPVHIP_OK;
}

int compvhip_api::remapPrepare(compvhip_ctx* ctx, const uint8_t* d_in, size_t W, size_t H, size_t S, size_t frames, int interp, const compvhip_roi* roi, void* d_out,
                               size_t Wout, size_t Hout, size_t Sout, uint8_t defaultValue, RemapArgs* a)
{
	if (!d_in || !d_out) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "null frame pointer");
	const size_t elem = interpElemBytes(interp);
	if (!elem) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "unknown interpolation");
	if (!W || !H || !Wout || !Hout || Wout > 32767 || Hout > 32767 || W > 32767 || H > 32767 || S < W || Sout < Wout || Sout > static_cast<size_t>(INT32_MAX) || !frames ||
	    frames > static_cast<size_t>(INT32_MAX) || S * H > static_cast<size_t>(INT32_MAX))
		return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "remap: a size of 0 or beyond 32767, Sout < Wout, or a frame beyond 2^31 bytes");
	if (elem > 1 && misaligned(3, d_out)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "float32 destination not 4-byte aligned");
	const uint8_t* const o = static_cast<const uint8_t*>(d_out);
	if (d_in < o + Sout * Hout * frames * elem && o < d_in + S * H * frames) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "input and output must not overlap");
	*a = RemapArgs{};
	a->in = d_in; a->inFrameStride = S * H; a->W = static_cast<int>(W); a->H = static_cast<int>(H); a->S = static_cast<int>(S);
	a->out = d_out; a->outFrameStride = Sout * Hout; a->Wout = static_cast<int>(Wout); a->Hout = static_cast<int>(Hout); a->Sout = static_cast<int>(Sout);
	a->defaultValue = defaultValue; a->frames = static_cast<int>(frames);
	// compv_image_remap.cxx:346-360 (COMPV_MATH_CLIP3(lo, hi, v) = v < lo ? lo : (v > hi ? hi : v))
	const float w1 = static_cast<float>(W - 1), h1 = static_cast<float>(H - 1);
	auto clip3 = [](float lo, float hi, float v) { return v < lo ? lo : (v > hi ? hi : v); };
	a->left = 0.f; a->right = w1; a->top = 0.f; a->bottom = h1;
	if (roi) {
		a->left = clip3(0.f, w1, roi->left); a->right = clip3(a->left, w1, roi->right);
		a->top = clip3(0.f, h1, roi->top); a->bottom = clip3(a->top, h1, roi->bottom);
		// a NaN passes the clip and fails every compare of the inside test: nothing is inside, which the empty ROI says as well
		if (!(a->left <= a->right && a->top <= a->bottom)) { a->left = a->top = 1.f; a->right = a->bottom = 0.f; }
	}
	return COMPVHIP_OK;
}

int compvhip_api::warpUpload(compvhip_ctx* ctx, WarpTables* t, const float* M, int rows, size_t count, RemapArgs* a, hipStream_t st)
{
	const size_t Wout = static_cast<size_t>(a->Wout), Hout = static_cast<size_t>(a->Hout), per = static_cast<size_t>(rows) * (Wout + Hout), total = per * count;
	float* host = nullptr;
	WarpTables::Slot* s = nullptr;
	int rc = tablesSlot(ctx, t, total, &host, &s);
	if (rc) return rc;
	for (size_t m = 0; m < count; ++m) {
		float* cols = host + m * per;
		float* rws = cols + static_cast<size_t>(rows) * Wout;
		rc = compvhip_warp_tables(M + m * static_cast<size_t>(rows) * 3, rows, Wout, Hout, cols, cols + Wout, rows == 3 ? cols + 2 * Wout : nullptr, rws, rws + Hout,
		                          rows == 3 ? rws + 2 * Hout : nullptr);
		if (rc) return fail(ctx, rc, "warp tables");
	}
	rc = tablesSend(ctx, t, s, total, st);
	a->tables = t->dev; a->coordFrameStride = per;
	return rc;
}

int compvhip_plan_remap(compvhip_plan* p, const uint8_t* d_in, const float* d_mapX, const float* d_mapY, size_t mapCount, int interp, const compvhip_roi* roi,
                        uint8_t defaultValue, void* d_out, size_t Wout, size_t Hout, size_t Sout, void* stream)
{
	if (!p) return COMPVHIP_E_INVALID_PARAMETER;
	compvhip_ctx* ctx = p->ctx;
	HIPCHK(ctx, hipSetDevice(ctx->device));
	hipStream_t st = static_cast<hipStream_t>(stream);
	if (!d_mapX || !d_mapY || misaligned(3, d_mapX, d_mapY)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "null or misaligned map");
	if (mapCount != 1 && mapCount != p->frames) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "mapCount must be 1 or the plan's frames");
	RemapArgs a;
	int rc = remapPrepare(ctx, d_in, p->W, p->H, p->S, p->frames, interp, roi, d_out, Wout, Hout, Sout, defaultValue, &a);
	if (rc) return rc;
	a.mapX = d_mapX; a.mapY = d_mapY; a.coordFrameStride = Wout * Hout;
	if (p->timing) timelineClear(p);
	Stamp s(p, st, "remap_kernel");
	HIPCHK(ctx, launch_remap(a, kRemapMap, interp, mapCount != 1, st));
	return COMPVHIP_OK;
}

int compvhip_plan_warp_inverse(compvhip_plan* p, const uint8_t* d_in, const float* M, int rows, size_t matrixCount, int interp, uint8_t defaultValue, void* d_out,
                               size_t Wout, size_t Hout, size_t Sout, void* stream)
{
	if (!p) return COMPVHIP_E_INVALID_PARAMETER;
	compvhip_ctx* ctx = p->ctx;
	HIPCHK(ctx, hipSetDevice(ctx->device));
	hipStream_t st = static_cast<hipStream_t>(stream);
	if (!M || (rows != 2 && rows != 3)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "M must be a 2 x 3 or 3 x 3 float32 matrix");
	if (matrixCount != 1 && matrixCount != p->frames) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "matrixCount must be 1 or the plan's frames");
	RemapArgs a;
	int rc = remapPrepare(ctx, d_in, p->W, p->H, p->S, p->frames, interp, nullptr, d_out, Wout, Hout, Sout, defaultValue, &a);
	if (rc) return rc;
	rc = warpUpload(ctx, &p->warp, M, rows, matrixCount, &a, st);
	if (rc) return rc;
	if (p->timing) timelineClear(p);
	Stamp s(p, st, "warp_inverse_kernel");
	HIPCHK(ctx, launch_remap(a, rows == 3 ? kRemapWarp3 : kRemapWarp2, interp, matrixCount != 1, st));
	return COMPVHIP_OK;
}

int compvhip_orbpyr_create(compvhip_ctx* ctx, size_t W, size_t H, size_t S, size_t frames, const compvhip_orbpyr_opts* opts, size_t cornerCap, compvhip_orbpyr** out)
{
	if (!ctx || !out) return COMPVHIP_E_INVALID_PARAMETER;
	*out = nullptr;
	if (!opts) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "null options");
	if (opts->levels < 1 || opts->levels > kPyrMaxLevels || !(opts->scaleFactor > 0.f && opts->scaleFactor < 1.f))
		return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "levels must be 1 .. 16 and 0 < scaleFactor < 1");
	int rc = checkOrb(ctx, W, H, 1.f);
	if (!rc) rc = checkFast(ctx, W, H, opts->fastType);
	if (rc) return rc;
	rc = refuseBeyondLaunchLimit(ctx, frames, "compvhip_orbpyr_create");   // every kernel of the pyramid has the frame index in blockIdx.y / .z
	if (rc) return rc;
	if (W > 32767 || H > 32767 || S < W || (S & 7) || !frames || !cornerCap || cornerCap > static_cast<size_t>(INT32_MAX))
		return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "pyramid: size beyond 32767, S < W or no multiple of 8, no frames, or cornerCap outside 1 .. 2^31");
	HIPCHK(ctx, hipSetDevice(ctx->device));
	compvhip_orbpyr* y = new (std::nothrow) compvhip_orbpyr();
	if (!y) return fail(ctx, COMPVHIP_E_OUT_OF_MEMORY, "pyramid");
	y->ctx = ctx; y->W = W; y->H = H; y->S = S; y->frames = frames; y->cornerCap = cornerCap; y->opts = *opts;
	// compv_image_scale_pyramid.cxx:39-44,166 and compv_core_feature_orb_dete.cxx:319-321, operation by operation in float32
	float sf = 1.f, sfs = 1.f, f = opts->scaleFactor;
	for (int l = 1; l < opts->levels; ++l, f *= opts->scaleFactor) sfs += f;
	f = opts->scaleFactor;
	size_t planeBytes = 0;
	for (int l = 0; l < opts->levels; ++l) {
		compvhip_orbpyr::Level& L = y->lv[l];
		if (l) { sf = f; f *= opts->scaleFactor; }
		L.sf = sf;
		L.W = l ? static_cast<size_t>(static_cast<float>(W) * sf) : W; L.H = l ? static_cast<size_t>(static_cast<float>(H) * sf) : H;
		if (opts->maxFeatures > 0) {
			const float nf = (static_cast<float>(opts->maxFeatures) / sfs) * sf;
			L.quota = std::max(10, static_cast<int32_t>(static_cast<double>(nf) + 0.5));
		}
		if (L.W < 2 * kOrbBorder + 1 || L.H < 2 * kOrbBorder + 1) continue;          // empty: S stays 0
		L.S = l ? alignUp(L.W, 8) : S;
		y->active = l + 1;
		if (l) planeBytes += alignUp(L.S * L.H * frames, 256);
	}
	if (compvhip_gauss_kernel_fixedpoint(5, 2.0f, y->kern) != COMPVHIP_OK) { compvhip_orbpyr_destroy(y); return fail(ctx, COMPVHIP_E_INVALID_STATE, "Gaussian kernel"); }   // compv_core_feature_orb_desc.cxx:119-120
	const char* e = getenv("COMPVHIP_ORB_BRIEF");   // the lab knob of compvhip_plan_orb_describe
	if (e) y->briefLds = !strcmp(e, "lds");
	const size_t L = static_cast<size_t>(opts->levels);
	if (y->planes.reserve(ctx, planeBytes) != hipSuccess || y->corners.reserve(ctx, frames * cornerCap) != hipSuccess ||
	    y->fastWork.reserve(ctx, fastWorkInts(frames, H)) != hipSuccess || y->fastScores.reserve(ctx, S * H * frames) != hipSuccess ||
	    y->counts.reserve(ctx, (3 * L + 1) * frames) != hipSuccess) {
		compvhip_orbpyr_destroy(y);
		return fail(ctx, COMPVHIP_E_OUT_OF_MEMORY, "pyramid planes / scratch");
	}
	size_t off = 0;
	for (int l = 1; l < y->active; ++l) { y->lv[l].plane = y->planes + off; off += alignUp(y->lv[l].S * y->lv[l].H * frames, 256); }
	*out = y;
	return COMPVHIP_OK;
}

void compvhip_orbpyr_destroy(compvhip_orbpyr* y) { handleDestroy(y); }
int compvhip_orbpyr_set_timing(compvhip_orbpyr* y, int enabled) { return handleSetTiming(y, enabled); }
int compvhip_orbpyr_get_timing(compvhip_orbpyr* y, const char** names, float* ms, int cap) { return handleGetTiming(y, names, ms, cap); }

int compvhip_orbpyr_geometry(const compvhip_orbpyr* y, int level, size_t* W, size_t* H, size_t* S, float* scale, int* quota)
{
	if (!y) return COMPVHIP_E_INVALID_PARAMETER;
	if (level < 0 || level >= y->opts.levels) return fail(y->ctx, COMPVHIP_E_INVALID_PARAMETER, "level outside 0 .. levels - 1");
	const compvhip_orbpyr::Level& L = y->lv[level];
	if (W) *W = L.W;
	if (H) *H = L.H;
	if (S) *S = L.S;
	if (scale) *scale = L.sf;
	if (quota) *quota = L.quota;
	return COMPVHIP_OK;
}

int compvhip_orbpyr_plane(compvhip_orbpyr* y, int level, int blurred, const uint8_t** d_plane)
{
	if (!y || !d_plane) return COMPVHIP_E_INVALID_PARAMETER;
	compvhip_ctx* ctx = y->ctx;
	if (level < 0 || level >= y->opts.levels || level >= y->active) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "level outside 0 .. levels - 1, or an empty level");
	if (blurred ? !y->blurredOf : !y->planesOf) return fail(ctx, COMPVHIP_E_INVALID_STATE, "no call has built this plane yet");
	*d_plane = blurred ? y->lv[level].blurred : (level ? y->lv[level].plane : y->planesOf);
	return COMPVHIP_OK;
}

namespace {
int checkPyrFrame(compvhip_orbpyr* y, const uint8_t* d_gray)
{
	if (!d_gray) return fail(y->ctx, COMPVHIP_E_INVALID_PARAMETER, "null frame pointer");
	if (misaligned(7, d_gray)) return fail(y->ctx, COMPVHIP_E_INVALID_PARAMETER, "frames must be 8-byte aligned");
	return COMPVHIP_OK;
}

// levels 1 .. active - 1 of every frame from d_gray: one launch
int pyrScale(compvhip_orbpyr* y, const uint8_t* d_gray, hipStream_t st)
{
	compvhip_ctx* ctx = y->ctx;
	y->planesOf = d_gray;
	if (y->active < 2) return COMPVHIP_OK;
	ScaleArgs a;
	a.in = d_gray; a.frameStride = y->S * y->H; a.W = static_cast<int>(y->W); a.H = static_cast<int>(y->H); a.S = static_cast<int>(y->S); a.levels = y->active - 1;
	for (int l = 1; l < y->active; ++l) {
		const compvhip_orbpyr::Level& src = y->lv[l];
		ScaleLevel& L = a.lv[l - 1];
		L.out = src.plane; L.frameStride = src.S * src.H; L.W = static_cast<int>(src.W); L.H = static_cast<int>(src.H); L.S = static_cast<int>(src.S);
		if (!scale_level_init(L, a.W, a.H)) return fail(ctx, COMPVHIP_E_INVALID_STATE, "pyramid level ratio");   // 37 <= W_l <= W <= 32767: cannot happen
	}
	Stamp s(y, st, "scale_bilinear_kernel");
	HIPCHK(ctx, launch_scale_bilinear(a, static_cast<int>(y->frames), st));
	return COMPVHIP_OK;
}
} // namespace

int compvhip_orbpyr_detect(compvhip_orbpyr* y, const uint8_t* d_gray, compvhip_keypoint* d_keypoints, size_t keyCap, int32_t* d_keyCounts, int32_t* d_levelCounts,
                           int32_t* d_levelCorners, void* stream)
{
	if (!y) return COMPVHIP_E_INVALID_PARAMETER;
	compvhip_ctx* ctx = y->ctx;
	int rc = checkPyrFrame(y, d_gray);
	if (rc) return rc;
	if (!d_keyCounts || (keyCap && !d_keypoints) || keyCap > static_cast<size_t>(INT32_MAX)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "null count / keypoint pointer or keyCap beyond 2^31");
	if (misaligned(3, d_keypoints, d_keyCounts, d_levelCounts, d_levelCorners))
		return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "records and counts must be 4-byte aligned");
	HIPCHK(ctx, hipSetDevice(ctx->device));
	HIPCHK(ctx, y->index.reserve(ctx, y->frames * keyCap));
	hipStream_t st = static_cast<hipStream_t>(stream);
	if (y->timing) timelineClear(y);
	const size_t F = y->frames, NL = static_cast<size_t>(y->opts.levels);
	const int frames = static_cast<int>(F);
	int32_t* lvCorners = y->counts; int32_t* lvKeys = lvCorners + NL * F; int32_t* totals = lvKeys + NL * F;
	HIPCHK(ctx, hipMemsetAsync(totals, 0, F * sizeof(int32_t), st));          // nothing in front of level 0
	rc = pyrScale(y, d_gray, st);
	if (rc) return rc;
	for (int l = 0; l < y->active; ++l) {
		const compvhip_orbpyr::Level& L = y->lv[l];
		const uint8_t* plane = l ? L.plane : d_gray;
		FastArgs a;
		HIPCHK(ctx, fastArgs(a, plane, L.W, L.H, L.S, F, y->opts.threshold, y->opts.fastType, y->opts.nonmax, y->opts.maxFeatures > 0 ? L.quota : -1, y->fastWork, y->fastScores,
		                     y->corners, y->cornerCap, lvCorners + l * F, st));
		{ Stamp s(y, st, "fast_score_kernel"); HIPCHK(ctx, launch_fast(a, frames, 0, st)); }
		{ Stamp s(y, st, "fast_list_kernels"); HIPCHK(ctx, launch_fast(a, frames, 1, st)); }
		OrbKeyArgs k;
		k.gray = plane; k.frameStride = L.S * L.H; k.W = a.W; k.H = a.H; k.S = a.S;
		k.corners = y->corners; k.cornerCap = y->cornerCap; k.cornerCounts = a.counts; k.level = l; k.scale = L.sf;
		k.index = y->index; k.keys = d_keypoints; k.keyCap = keyCap; k.keyCounts = lvKeys + l * F; k.moments = nullptr;
		k.keyBase = totals + l * F; k.keyTotal = totals + (l + 1) * F;
		{ Stamp s(y, st, "orb_select_kernel"); HIPCHK(ctx, launch_orb_select(k, frames, st)); }
		if (keyCap) { Stamp s(y, st, "orb_orient_kernel"); HIPCHK(ctx, launch_orb_orient(k, frames, st)); }
	}
	OrbPyrCountArgs c;
	c.totals = totals + static_cast<size_t>(y->active) * F; c.lvKeys = lvKeys; c.lvCorners = lvCorners; c.active = y->active; c.levels = y->opts.levels; c.frames = frames;
	c.keyCounts = d_keyCounts; c.levelCounts = d_levelCounts; c.levelCorners = d_levelCorners;
	{ Stamp s(y, st, "orb_pyramid_counts_kernel"); HIPCHK(ctx, launch_orb_pyramid_counts(c, st)); }
	return COMPVHIP_OK;
}

int compvhip_orbpyr_describe(compvhip_orbpyr* y, const uint8_t* d_gray, int reusePlanes, const compvhip_keypoint* d_keypoints, size_t keyCap, const int32_t* d_keyCounts,
                             uint8_t* d_desc, size_t descStride, void* stream)
{
	if (!y) return COMPVHIP_E_INVALID_PARAMETER;
	compvhip_ctx* ctx = y->ctx;
	int rc = checkPyrFrame(y, d_gray);
	if (rc) return rc;
	if (!d_keypoints || !d_keyCounts || !d_desc || !keyCap || keyCap > static_cast<size_t>(INT32_MAX)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "null keypoint / count / descriptor pointer, keyCap == 0 or beyond 2^31");
	if (descStride < 32 || (descStride & 3)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "descStride below 32 or no multiple of 4");
	if (misaligned(3, d_keypoints, d_keyCounts, d_desc))
		return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "records, counts and descriptors must be 4-byte aligned");
	if (reusePlanes && y->planesOf != d_gray) return fail(ctx, COMPVHIP_E_INVALID_STATE, "reusePlanes: no planes of a compvhip_orbpyr_detect call on this d_gray");
	HIPCHK(ctx, hipSetDevice(ctx->device));
	const size_t F = y->frames;
	const int frames = static_cast<int>(F);
	if (!y->blurredAll) {
		size_t bytes = 0;
		for (int l = 0; l < y->active; ++l) bytes += alignUp(y->lv[l].S * y->lv[l].H * F, 256);
		HIPCHK(ctx, y->blurredAll.reserve(ctx, bytes));
		size_t off = 0;
		for (int l = 0; l < y->active; ++l) { y->lv[l].blurred = y->blurredAll + off; off += alignUp(y->lv[l].S * y->lv[l].H * F, 256); }
	}
	hipStream_t st = static_cast<hipStream_t>(stream);
	if (y->timing) timelineClear(y);
	if (!reusePlanes) { rc = pyrScale(y, d_gray, st); if (rc) return rc; }
	OrbPyrDescArgs a;
	a.levels = y->opts.levels;
	for (int l = 0; l < kPyrMaxLevels; ++l) {
		const compvhip_orbpyr::Level& L = y->lv[l];
		OrbLevelPlane& P = a.lv[l];
		P.blurred = l < y->active ? L.blurred : nullptr; P.frameStride = L.S * L.H; P.W = static_cast<int>(L.W); P.H = static_cast<int>(L.H); P.S = static_cast<int>(L.S);
		P.scale = L.sf;
		if (l >= y->active) continue;
		Stamp s(y, st, "convlt_fxp_kernels");          // out of place: the fused kernel, no intermediate
		HIPCHK(ctx, launch_convlt_fxp(l ? L.plane : d_gray, nullptr, L.blurred, P.W, P.H, P.S, P.frameStride, frames, y->kern, y->kern, 5, st));
	}
	y->blurredOf = d_gray;
	a.keys = d_keypoints; a.keyCap = keyCap; a.keyCounts = d_keyCounts; a.desc = d_desc; a.descStride = descStride;
	{ Stamp s(y, st, y->briefLds ? "orb_brief_pyramid_kernel" : "orb_brief_pyramid_kernel_global"); HIPCHK(ctx, launch_orb_brief_pyramid(a, frames, y->briefLds, st)); }
	return COMPVHIP_OK;
}

// ---- brute-force Hamming matching (match_kernels.hip; definition in include/compv_hip.h) ---------------------------------------------------
namespace {
constexpr size_t kMatchMaxCap = size_t(1) << 22;   // rows per side: keeps every grid dimension and 32-bit row index in range

int checkMatchBuffers(compvhip_matcher* m, const uint8_t* d_query, size_t queryStride, const uint8_t* d_train, size_t trainStride)
{
	compvhip_ctx* ctx = m->ctx;
	const size_t bytes = static_cast<size_t>(m->descDwords) * 4;
	if (!d_query || !d_train) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "null descriptor pointer");
	if (queryStride < bytes || trainStride < bytes || (queryStride & 3) || (trainStride & 3) || queryStride > 65536 || trainStride > 65536)
		return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "descriptor stride below descBytes, above 65536 or no multiple of 4");
	if (misaligned(3, d_query, d_train)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "descriptors must be 4-byte aligned");
	return COMPVHIP_OK;
}
} // namespace

MatchSliceArgs compvhip_api::matchForward(const compvhip_matcher* m, const uint8_t* d_query, size_t queryStride, const int32_t* d_queryCounts, const uint8_t* d_train, size_t trainStride,
                            const int32_t* d_trainCounts, int trainShared, compvhip_match* d_matches)
{
	MatchSliceArgs a;
	a.query = d_query; a.train = d_train; a.queryCounts = d_queryCounts; a.trainCounts = d_trainCounts;
	a.queryCap = m->queryCap; a.trainCap = m->trainCap; a.queryStride = static_cast<int>(queryStride); a.trainStride = static_cast<int>(trainStride);
	a.queryShared = 0; a.trainShared = trainShared != 0;
	a.descDwords = m->descDwords; a.knn = m->knn; a.slices = (m->trainCap + kMatchTrainSlice - 1) / kMatchTrainSlice;
	a.partial = m->partial; a.matches = d_matches;
	return a;
}

int compvhip_matcher_create(compvhip_ctx* ctx, size_t descBytes, size_t queryCap, size_t trainCap, size_t pairs, int knn, compvhip_matcher** out)
{
	if (!ctx || !out) return COMPVHIP_E_INVALID_PARAMETER;
	*out = nullptr;
	if (descBytes < 4 || descBytes > 4 * static_cast<size_t>(kMatchMaxDwords) || (descBytes & 3)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "descBytes must be a multiple of 4 in 4..128");
	if (knn < 1 || knn > kMatchMaxKnn) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "knn must be in 1..8");
	if (int rc = refuseBeyondLaunchLimit(ctx, pairs, "compvhip_matcher_create (pairs)")) return rc;   // a pair is the matcher's frame: blockIdx.y / .z
	if (!queryCap || !trainCap || !pairs || queryCap > kMatchMaxCap || trainCap > kMatchMaxCap) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "capacity out of range");
	HIPCHK(ctx, hipSetDevice(ctx->device));
	compvhip_matcher* m = new (std::nothrow) compvhip_matcher();
	if (!m) return fail(ctx, COMPVHIP_E_OUT_OF_MEMORY, "matcher");
	m->ctx = ctx; m->descDwords = static_cast<int>(descBytes / 4); m->queryCap = static_cast<int>(queryCap); m->trainCap = static_cast<int>(trainCap);
	m->pairs = static_cast<int>(pairs); m->knn = knn;
	const size_t tSlices = (trainCap + kMatchTrainSlice - 1) / kMatchTrainSlice, qSlices = (queryCap + kMatchTrainSlice - 1) / kMatchTrainSlice;
	const size_t words = pairs * std::max(tSlices * static_cast<size_t>(knn) * queryCap, qSlices * trainCap);
	if (m->partial.reserve(ctx, words) != hipSuccess || m->reverse.reserve(ctx, pairs * trainCap) != hipSuccess) {
		compvhip_matcher_destroy(m);
		return fail(ctx, COMPVHIP_E_OUT_OF_MEMORY, "matcher scratch");
	}
	*out = m;
	return COMPVHIP_OK;
}

void compvhip_matcher_destroy(compvhip_matcher* m) { handleDestroy(m); }
int compvhip_matcher_set_timing(compvhip_matcher* m, int enabled) { return handleSetTiming(m, enabled); }
int compvhip_matcher_get_timing(compvhip_matcher* m, const char** names, float* ms, int cap) { return handleGetTiming(m, names, ms, cap); }

int compvhip_matcher_knn(compvhip_matcher* m, const uint8_t* d_query, size_t queryStride, const int32_t* d_queryCounts, const uint8_t* d_train, size_t trainStride,
                         const int32_t* d_trainCounts, int trainShared, compvhip_match* d_matches, void* stream)
{
	if (!m) return COMPVHIP_E_INVALID_PARAMETER;
	compvhip_ctx* ctx = m->ctx;
	int rc = checkMatchBuffers(m, d_query, queryStride, d_train, trainStride);
	if (rc) return rc;
	if (!d_matches || misaligned(15, d_matches)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "match records: null or not 16-byte aligned");
	if (misaligned(3, d_queryCounts, d_trainCounts)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "counts must be 4-byte aligned");
	HIPCHK(ctx, hipSetDevice(ctx->device));
	hipStream_t st = static_cast<hipStream_t>(stream);
	if (m->timing) timelineClear(m);
	const MatchSliceArgs a = matchForward(m, d_query, queryStride, d_queryCounts, d_train, trainStride, d_trainCounts, trainShared, d_matches);
	{ Stamp s(m, st, "match_slice_kernel"); HIPCHK(ctx, launch_match_slices(a, m->pairs, st)); }
	{ Stamp s(m, st, "match_merge_kernel"); HIPCHK(ctx, launch_match_merge(a, m->pairs, st)); }
	return COMPVHIP_OK;
}

int compvhip_matcher_good(compvhip_matcher* m, const compvhip_match* d_matches, const uint8_t* d_query, size_t queryStride, const int32_t* d_queryCounts,
                          const uint8_t* d_train, size_t trainStride, const int32_t* d_trainCounts, int trainShared, const compvhip_match_opts* opts,
                          compvhip_match* d_good, size_t goodCap, int32_t* d_goodCounts, void* stream)
{
	if (!m) return COMPVHIP_E_INVALID_PARAMETER;
	compvhip_ctx* ctx = m->ctx;
	if (!opts || !d_matches || !d_goodCounts || (goodCap && !d_good)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "null options / match / count / good pointer");
	if (opts->ratio > 0.0 && m->knn < 2) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "the ratio test needs knn >= 2");
	if (misaligned(15, d_matches, d_good)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "match records must be 16-byte aligned");
	if (misaligned(3, d_queryCounts, d_trainCounts, d_goodCounts))
		return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "counts must be 4-byte aligned");
	if (misaligned(3, d_query, d_train)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "descriptors must be 4-byte aligned");   // with or without the cross check, which alone reads them
	if (opts->crossCheck) {
		int rc = checkMatchBuffers(m, d_query, queryStride, d_train, trainStride);
		if (rc) return rc;
	}
	HIPCHK(ctx, hipSetDevice(ctx->device));
	hipStream_t st = static_cast<hipStream_t>(stream);
	if (m->timing) timelineClear(m);
	if (opts->crossCheck) {          // the same kernels with the roles swapped and knn = 1: reverse[pair][t] = the best query of train row t
		MatchSliceArgs r;
		r.query = d_train; r.train = d_query; r.queryCounts = d_trainCounts; r.trainCounts = d_queryCounts;
		r.queryCap = m->trainCap; r.trainCap = m->queryCap; r.queryStride = static_cast<int>(trainStride); r.trainStride = static_cast<int>(queryStride);
		r.queryShared = trainShared != 0; r.trainShared = 0;
		r.descDwords = m->descDwords; r.knn = 1; r.slices = (m->queryCap + kMatchTrainSlice - 1) / kMatchTrainSlice;
		r.partial = m->partial; r.matches = m->reverse;
		{ Stamp s(m, st, "match_reverse_slice_kernel"); HIPCHK(ctx, launch_match_slices(r, m->pairs, st)); }
		{ Stamp s(m, st, "match_reverse_merge_kernel"); HIPCHK(ctx, launch_match_merge(r, m->pairs, st)); }
	}
	MatchGoodArgs g;
	g.matches = d_matches; g.reverse = opts->crossCheck ? m->reverse : nullptr; g.queryCounts = d_queryCounts; g.trainCounts = d_trainCounts;
	g.queryCap = m->queryCap; g.trainCap = m->trainCap; g.trainShared = trainShared != 0; g.knn = m->knn;
	g.ratio = opts->ratio; g.maxDistance = opts->maxDistance; g.crossCheck = opts->crossCheck != 0;
	g.good = d_good; g.goodCap = goodCap; g.counts = d_goodCounts;
	{ Stamp s(m, st, "match_good_kernel"); HIPCHK(ctx, launch_match_good(g, m->pairs, st)); }
	return COMPVHIP_OK;
}

// ---- HOG descriptors (hog_kernels.hip; definition in include/compv_hip.h) -----------------------------------------------------------------------------
// Items 5, 6 and 8 of the definition: resolves the defaults, refuses what the definition refuses and fills the geometry fields of `a` (no pointer, no launch field)
int compvhip_api::hogGeometry(compvhip_ctx* ctx, size_t W, size_t H, const compvhip_hog_opts* opts, HogArgs* a)
{
	if (!opts || opts->size != sizeof(compvhip_hog_opts)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "HOG: null options, or their size field is not sizeof(compvhip_hog_opts)");
	const int32_t given[10] = { opts->blockW, opts->blockH, opts->strideW, opts->strideH, opts->cellW, opts->cellH, opts->nbins, opts->blockNorm, opts->gradientSigned, opts->interp };
	static const int32_t defaults[10] = { 16, 16, 8, 8, 8, 8, 9, COMPVHIP_HOG_NORM_L2HYS, COMPVHIP_HOG_GRADIENT_SIGNED, COMPVHIP_HOG_INTERP_BILINEAR };   // hog_std.cxx:459-467
	int32_t o[10];
	for (int i = 0; i < 10; ++i) {
		if (given[i] < 0) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "HOG: a negative option");
		o[i] = given[i] ? given[i] : defaults[i];
	}
	const int32_t nbins = o[6], norm = o[7], gradient = o[8], interp = o[9];
	if (norm > COMPVHIP_HOG_NORM_L2HYS || gradient > COMPVHIP_HOG_GRADIENT_UNSIGNED) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "HOG: unknown block norm or gradient kind");
	if (interp != COMPVHIP_HOG_INTERP_NEAREST && interp != COMPVHIP_HOG_INTERP_BILINEAR)
		return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "HOG: interpolation must be NEAREST or BILINEAR (BILINEAR_LUT is not supported)");
	const int thetaMax = gradient == COMPVHIP_HOG_GRADIENT_SIGNED ? 360 : 180;
	if (nbins < 2 || nbins > 360 || thetaMax % nbins) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "HOG: nbins must lie in 2..360 and divide 360 (signed) or 180 (unsigned)");
	if (W > 32767 || H > 32767) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "HOG: frame beyond 32767");
	int cells[2], valid[2], blocks[2], cpb[2], step[2];
	for (int ax = 0; ax < 2; ++ax) {
		const long long size = static_cast<long long>(ax ? H : W), block = o[ax], stride = o[2 + ax], cell = o[4 + ax];
		if (block % cell) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "HOG: the block size must be a multiple of the cell size");
		if (!(stride == cell || (2 * stride == cell && block == cell)))
			return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "HOG: per axis stride == cell, or 2 * stride == cell with block == cell");
		if (size < block) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "HOG: the frame is smaller than a block");
		const float ratio = static_cast<float>(stride) / static_cast<float>(cell);                                        // szStrideInCellsCount, hog_std.cxx:219
		cells[ax] = static_cast<int>(static_cast<float>(size / cell) / ratio);                                            // :238-239
		valid[ax] = cells[ax] - (static_cast<long long>(cells[ax] - 1) * stride + cell > size ? 1 : 0);                  // xGuard / yGuard, :249,255
		blocks[ax] = static_cast<int>((size - block) / stride + 1);                                                       // :320-321
		cpb[ax] = static_cast<int>(block / cell);
		step[ax] = static_cast<int>(static_cast<double>(ratio) + 0.5);                                                    // COMPV_MATH_ROUNDFU_2_NEAREST_INT, :355,357
		// what the reference asserts (:358): the last block's cells lie in the map
		if (cells[ax] < 1 || static_cast<long long>(blocks[ax] - 1) * step[ax] + cpb[ax] > cells[ax]) return fail(ctx, COMPVHIP_E_INVALID_STATE, "HOG: a block leaves the cell map");
	}
	const long long count = static_cast<long long>(cpb[0]) * cpb[1] * nbins, mapFloats = static_cast<long long>(cells[0]) * cells[1] * nbins;
	if (count > INT32_MAX || mapFloats > INT32_MAX || count * blocks[0] > INT32_MAX || count * blocks[0] * blocks[1] > INT32_MAX)
		return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "HOG: a block, the cell map or the descriptor of a frame has 2^31 floats or more");
	a->W = static_cast<int>(W); a->H = static_cast<int>(H);
	a->cellW = o[4]; a->cellH = o[5]; a->strideW = o[2]; a->strideH = o[3]; a->nbins = nbins;
	a->interp = interp; a->gradientSigned = gradient == COMPVHIP_HOG_GRADIENT_SIGNED; a->norm = norm;
	a->cellsX = cells[0]; a->cellsY = cells[1]; a->validX = valid[0]; a->validY = valid[1];
	a->blocksX = blocks[0]; a->blocksY = blocks[1]; a->cpbX = cpb[0]; a->cpbY = cpb[1]; a->stepX = step[0]; a->stepY = step[1]; a->count = static_cast<int>(count);
	a->cellsFrameStride = static_cast<size_t>(mapFloats);
	a->gray = nullptr; a->frameStride = 0; a->S = 0; a->cells = nullptr; a->desc = nullptr; a->descStride = 0;
	if (!hog_plan_launch(*a)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "HOG: three rows of one cell and the histogram exceed the LDS of a compute unit");
	return COMPVHIP_OK;
}

int compvhip_hog_geometry(size_t W, size_t H, const compvhip_hog_opts* opts, size_t* cellsX, size_t* cellsY, size_t* blocksX, size_t* blocksY, size_t* descLen)
{
	HogArgs a;
	const int rc = hogGeometry(nullptr, W, H, opts, &a);
	if (rc) return rc;
	if (cellsX) *cellsX = static_cast<size_t>(a.cellsX);
	if (cellsY) *cellsY = static_cast<size_t>(a.cellsY);
	if (blocksX) *blocksX = static_cast<size_t>(a.blocksX);
	if (blocksY) *blocksY = static_cast<size_t>(a.blocksY);
	if (descLen) *descLen = static_cast<size_t>(a.blocksX) * a.blocksY * a.count;
	return COMPVHIP_OK;
}

int compvhip_plan_hog(compvhip_plan* p, const uint8_t* d_gray, const compvhip_hog_opts* opts, float* d_cells, float* d_desc, size_t descStride, void* stream)
{
	if (!p) return COMPVHIP_E_INVALID_PARAMETER;
	compvhip_ctx* ctx = p->ctx;
	if (!d_gray || !d_desc) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "null frame / descriptor pointer");
	HogArgs a;
	const int rc = hogGeometry(ctx, p->W, p->H, opts, &a);
	if (rc) return rc;
	const size_t descLen = static_cast<size_t>(a.blocksX) * a.blocksY * a.count;
	if (descStride < descLen) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "descStride below the descriptor's length");
	if (p->frames > static_cast<size_t>(INT32_MAX)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "frames beyond 2^31");
	if (misaligned(3, d_cells, d_desc)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "cell map and descriptors must be 4-byte aligned");
	HIPCHK(ctx, hipSetDevice(ctx->device));
	if (!d_cells) HIPCHK(ctx, p->hogCells.reserve(ctx, a.cellsFrameStride * p->frames));
	hipStream_t st = static_cast<hipStream_t>(stream);
	if (p->timing) timelineClear(p);
	a.gray = d_gray; a.frameStride = p->S * p->H; a.S = static_cast<int>(p->S);
	a.cells = d_cells ? d_cells : p->hogCells.ptr; a.desc = d_desc; a.descStride = descStride;
	hog_plan_launch(a);          // again with the frames' pointer and stride: whole dwords are loaded where they are 4-byte aligned
	const int frames = static_cast<int>(p->frames);
	{ Stamp s(p, st, "hog_cells_kernel"); HIPCHK(ctx, launch_hog_cells(a, frames, st)); }
	{ Stamp s(p, st, "hog_blocks_kernel"); HIPCHK(ctx, launch_hog_blocks(a, frames, st)); }
	return COMPVHIP_OK;
}

// ---- image statistics (stats_kernels.hip; definition in include/compv_hip.h) ----------------------------------------------------------------------------
int compvhip_api::integralDims(compvhip_ctx* ctx, size_t W, size_t H)
{
	if (!W || !H) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "integral: an empty frame");
	if (W > 32767 || H > 32767) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "integral: frame beyond 32767");
	if (W * H >= (static_cast<size_t>(1) << 31)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "integral: 2^31 pixels or more");
	return COMPVHIP_OK;
}

int compvhip_integral_dims(size_t W, size_t H, size_t* rows, size_t* cols)
{
	const int rc = integralDims(nullptr, W, H);
	if (rc) return rc;
	if (rows) *rows = H + 1;
	if (cols) *cols = W + 1;
	return COMPVHIP_OK;
}

namespace {
// what every statistics call checks first: the frames and their geometry (a plan's holds by construction; the host calls come with any size)
int statsCheck(const StatsFrames& g, const char* what)
{
	if (!g.d_gray) return fail(g.ctx, COMPVHIP_E_INVALID_PARAMETER, "null frame pointer");
	if (!g.W || !g.H || g.W > 32767 || g.H > 32767 || g.S < g.W) return fail(g.ctx, COMPVHIP_E_INVALID_PARAMETER, what);
	if (!g.frames || g.frames > static_cast<size_t>(INT32_MAX)) return fail(g.ctx, COMPVHIP_E_INVALID_PARAMETER, "frames beyond 2^31");
	return COMPVHIP_OK;
}
// the entry of a kernel in the plan's timing (every kernel with mode 1; the host calls have no plan and no timing)
struct StatsStamp : Stamp {
	StatsStamp(const StatsFrames& g, const char* name) : Stamp(g.plan, g.st, name, g.plan && g.plan->timing == 1) {}
};
} // namespace

int compvhip_api::integralImpl(const StatsFrames& g, double* d_sum, double* d_sumsq, size_t sumStride)
{
	compvhip_ctx* ctx = g.ctx;
	int rc = statsCheck(g, "integral: frame size out of range (1..32767) or stride below the width");
	if (rc) return rc;
	if ((rc = integralDims(ctx, g.W, g.H))) return rc;
	if (!d_sum && !d_sumsq) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "integral: both outputs are NULL");
	if (sumStride < g.W + 1) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "integral: sumStride below W + 1");
	if (misaligned(7, d_sum, d_sumsq)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "integral: outputs must be 8-byte aligned");
	HIPCHK(ctx, hipSetDevice(ctx->device));
	const int frames = static_cast<int>(g.frames), bands = stats_bands(static_cast<int>(g.H));
	const size_t cols = g.frames * bands * g.W;
	if (d_sum) HIPCHK(ctx, g.scratch->colSum.reserve(ctx, cols));
	if (d_sumsq) HIPCHK(ctx, g.scratch->colSq.reserve(ctx, cols));
	if (g.plan && g.plan->timing) timelineClear(g.plan);
	StatsBandArgs b;
	b.in = g.d_gray; b.frameStride = g.S * g.H; b.W = static_cast<int>(g.W); b.H = static_cast<int>(g.H); b.S = static_cast<int>(g.S); b.bands = bands;
	b.colSum = d_sum ? g.scratch->colSum.ptr : nullptr; b.colSq = d_sumsq ? g.scratch->colSq.ptr : nullptr; b.rowSum = nullptr;
	{ StatsStamp s(g, "stats_band_sums_kernel"); HIPCHK(ctx, launch_stats_band_sums(b, frames, g.st)); }
	{ StatsStamp s(g, "stats_band_scan_kernel"); HIPCHK(ctx, launch_stats_band_scan(b.colSum, b.colSq, bands, b.W, nullptr, frames, g.st)); }
	StatsIntegralArgs a;
	a.in = b.in; a.frameStride = b.frameStride; a.W = b.W; a.H = b.H; a.S = b.S; a.bands = bands;
	a.edgeSum = b.colSum; a.edgeSq = b.colSq; a.sum = d_sum; a.sumsq = d_sumsq; a.sumStride = sumStride;
	{ StatsStamp s(g, "stats_integral_kernel"); HIPCHK(ctx, launch_stats_integral(a, frames, g.st)); }
	return COMPVHIP_OK;
}

int compvhip_api::histogramImpl(const StatsFrames& g, uint32_t* d_hist)
{
	compvhip_ctx* ctx = g.ctx;
	const int rc = statsCheck(g, "histogram: frame size out of range (1..32767) or stride below the width");
	if (rc) return rc;
	if (!d_hist) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "histogram: null output");
	if (misaligned(3, d_hist)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "histogram: the output must be 4-byte aligned");
	HIPCHK(ctx, hipSetDevice(ctx->device));
	const int frames = static_cast<int>(g.frames), chunks = stats_row_chunks(static_cast<int>(g.H), frames);
	HIPCHK(ctx, g.scratch->hist.reserve(ctx, g.frames * chunks * 256));
	if (g.plan && g.plan->timing) timelineClear(g.plan);
	{ StatsStamp s(g, "stats_hist_kernel");
	  HIPCHK(ctx, launch_stats_hist(g.d_gray, static_cast<int>(g.W), static_cast<int>(g.H), static_cast<int>(g.S), g.S * g.H, frames, chunks, g.scratch->hist, g.st)); }
	{ StatsStamp s(g, "stats_hist_finish_kernel"); HIPCHK(ctx, launch_stats_hist_finish(g.scratch->hist, chunks, d_hist, 0.f, nullptr, frames, g.st)); }
	return COMPVHIP_OK;
}

int compvhip_api::equalizeImpl(const StatsFrames& g, const uint32_t* d_hist, double scale, uint8_t* d_out, uint8_t* d_lut)
{
	compvhip_ctx* ctx = g.ctx;
	const int rc = statsCheck(g, "equalize: frame size out of range (1..32767) or stride below the width");
	if (rc) return rc;
	if (!d_out) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "equalize: null output frame");
	if (misaligned(3, d_hist)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "equalize: the histogram must be 4-byte aligned");
	const float scaleF = static_cast<float>(scale > 0.0 ? scale : 255.0 / static_cast<double>(g.W * g.H));
	if (!(scale == scale) || !std::isfinite(scaleF)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "equalize: the scale is not a finite float32");
	HIPCHK(ctx, hipSetDevice(ctx->device));
	const int frames = static_cast<int>(g.frames), chunks = stats_row_chunks(static_cast<int>(g.H), frames);
	if (!d_hist) HIPCHK(ctx, g.scratch->hist.reserve(ctx, g.frames * chunks * 256));
	if (!d_lut) HIPCHK(ctx, g.scratch->lut.reserve(ctx, g.frames * 256));
	if (g.plan && g.plan->timing) timelineClear(g.plan);
	uint8_t* const lut = d_lut ? d_lut : g.scratch->lut.ptr;
	if (!d_hist) {
		StatsStamp s(g, "stats_hist_kernel");
		HIPCHK(ctx, launch_stats_hist(g.d_gray, static_cast<int>(g.W), static_cast<int>(g.H), static_cast<int>(g.S), g.S * g.H, frames, chunks, g.scratch->hist, g.st));
	}
	{ StatsStamp s(g, "stats_hist_finish_kernel");
	  HIPCHK(ctx, launch_stats_hist_finish(d_hist ? d_hist : g.scratch->hist.ptr, d_hist ? 1 : chunks, nullptr, scaleF, lut, frames, g.st)); }
	StatsEqualizeArgs a;
	a.in = g.d_gray; a.out = d_out; a.lut = lut; a.frameStride = g.S * g.H; a.W = static_cast<int>(g.W); a.H = static_cast<int>(g.H); a.S = static_cast<int>(g.S);
	{ StatsStamp s(g, "stats_equalize_kernel"); HIPCHK(ctx, launch_stats_equalize(a, frames, chunks, g.st)); }
	return COMPVHIP_OK;
}

int compvhip_api::projectionsImpl(const StatsFrames& g, int32_t* d_projX, int32_t* d_projY)
{
	compvhip_ctx* ctx = g.ctx;
	const int rc = statsCheck(g, "projections: frame size out of range (1..32767) or stride below the width");
	if (rc) return rc;
	if (!d_projX && !d_projY) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "projections: both outputs are NULL");
	if (misaligned(3, d_projX, d_projY)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "projections: outputs must be 4-byte aligned");
	HIPCHK(ctx, hipSetDevice(ctx->device));
	const int frames = static_cast<int>(g.frames), bands = stats_bands(static_cast<int>(g.H));
	if (d_projX) HIPCHK(ctx, g.scratch->colSum.reserve(ctx, g.frames * bands * g.W));
	if (g.plan && g.plan->timing) timelineClear(g.plan);
	StatsBandArgs b;
	b.in = g.d_gray; b.frameStride = g.S * g.H; b.W = static_cast<int>(g.W); b.H = static_cast<int>(g.H); b.S = static_cast<int>(g.S); b.bands = bands;
	b.colSum = d_projX ? g.scratch->colSum.ptr : nullptr; b.colSq = nullptr; b.rowSum = d_projY;
	{ StatsStamp s(g, "stats_band_sums_kernel"); HIPCHK(ctx, launch_stats_band_sums(b, frames, g.st)); }          // the frames are read once, here
	if (d_projX) { StatsStamp s(g, "stats_band_scan_kernel"); HIPCHK(ctx, launch_stats_band_scan(b.colSum, nullptr, bands, b.W, d_projX, frames, g.st)); }
	return COMPVHIP_OK;
}

static StatsFrames planFrames(compvhip_plan* p, const uint8_t* d_gray, void* stream)
{
	return StatsFrames{ p->ctx, p, &p->stats, d_gray, p->W, p->H, p->S, p->frames, static_cast<hipStream_t>(stream) };
}

int compvhip_plan_integral(compvhip_plan* p, const uint8_t* d_gray, double* d_sum, double* d_sumsq, size_t sumStride, void* stream)
{
	if (!p) return COMPVHIP_E_INVALID_PARAMETER;
	return integralImpl(planFrames(p, d_gray, stream), d_sum, d_sumsq, sumStride);
}

int compvhip_plan_histogram(compvhip_plan* p, const uint8_t* d_gray, uint32_t* d_hist, void* stream)
{
	if (!p) return COMPVHIP_E_INVALID_PARAMETER;
	return histogramImpl(planFrames(p, d_gray, stream), d_hist);
}

int compvhip_plan_equalize(compvhip_plan* p, const uint8_t* d_gray, const uint32_t* d_hist, double scale, uint8_t* d_out, uint8_t* d_lut, void* stream)
{
	if (!p) return COMPVHIP_E_INVALID_PARAMETER;
	return equalizeImpl(planFrames(p, d_gray, stream), d_hist, scale, d_out, d_lut);
}

int compvhip_plan_projections(compvhip_plan* p, const uint8_t* d_gray, int32_t* d_projX, int32_t* d_projY, void* stream)
{
	if (!p) return COMPVHIP_E_INVALID_PARAMETER;
	return projectionsImpl(planFrames(p, d_gray, stream), d_projX, d_projY);
}

// ---- colour conversion (include/compv_hip.h, "colour conversion") ---------------------------------------------------------------------------------
static_assert(conv::kNV12 == COMPVHIP_FMT_NV12 && conv::kHSV == COMPVHIP_FMT_HSV && conv::kY == COMPVHIP_FMT_Y && conv::kRGBA32 == COMPVHIP_FMT_RGBA32, "convert_math.hpp restates compvhip_pixfmt");

int compvhip_convert_layout(int pixfmt, size_t W, size_t H, int* planes, size_t minRowBytes[3], size_t rows[3])
{
	return conv::layout(pixfmt, W, H, planes, minRowBytes, rows) ? COMPVHIP_OK : COMPVHIP_E_INVALID_PARAMETER;
}

int compvhip_api::convertCheck(compvhip_ctx* ctx, size_t W, size_t H, size_t frames, const compvhip_image* in, const compvhip_image* out, ConvertArgs* a, ConvertGeometry* g)
{
	if (!ctx) return COMPVHIP_E_INVALID_PARAMETER;
	if (!in || !out) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "convert: null image description");
	if (!W || !H || !frames) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "convert: W, H or frames is 0");
	if (W > 32767 || H > 32767 || frames > 0x7fffffffu) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "convert: W or H beyond 32767, or frames beyond 2^31 - 1");
	if (!conv::layout(in->pixfmt, W, H, &g->planesIn, g->minIn, g->rowsIn) || !conv::layout(out->pixfmt, W, H, &g->planesOut, g->minOut, g->rowsOut))
		return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "convert: unknown pixel format");
	if (!conv::served(in->pixfmt, out->pixfmt)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "convert: this pair of formats is not served");
	// a plane's byte range: from its first byte to the last byte of its last row in the last frame
	struct Span { const uint8_t* p; size_t bytes, row, frame; };
	Span si[3] = {}, so[3] = {};
	auto spans = [&](const compvhip_image* im, int planes, const size_t* minRow, const size_t* rows, Span* s) -> const char* {
		for (int p = 0; p < planes; ++p) {
			if (!im->plane[p]) return "convert: a plane of the format is NULL";
			if (im->rowBytes[p] < minRow[p]) return "convert: rowBytes below the plane's row";
			const size_t one = (rows[p] - 1) * im->rowBytes[p] + minRow[p];
			if (frames > 1 && im->frameBytes[p] < one) return "convert: frameBytes makes frames overlap";
			s[p] = Span{ static_cast<const uint8_t*>(im->plane[p]), (frames - 1) * (frames > 1 ? im->frameBytes[p] : 0) + one, im->rowBytes[p], frames > 1 ? im->frameBytes[p] : 0 };
		}
		return nullptr;
	};
	if (const char* why = spans(in, g->planesIn, g->minIn, g->rowsIn, si)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, why);
	if (const char* why = spans(out, g->planesOut, g->minOut, g->rowsOut, so)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, why);
	for (int p = 0; p < g->planesOut; ++p)
		for (int q = p + 1; q < g->planesOut; ++q)
			if (overlaps(so[p].p, so[p].bytes, so[q].p, so[q].bytes)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "convert: two output planes overlap");
	const bool threeToThree = (in->pixfmt == COMPVHIP_FMT_RGB24 || in->pixfmt == COMPVHIP_FMT_BGR24) && g->minOut[0] == g->minIn[0] && g->planesOut == 1;
	for (int p = 0; p < g->planesIn; ++p)
		for (int q = 0; q < g->planesOut; ++q) {
			if (!overlaps(si[p].p, si[p].bytes, so[q].p, so[q].bytes)) continue;
			if (threeToThree && si[p].p == so[q].p && si[p].row == so[q].row && si[p].frame == so[q].frame) continue;   // in place
			return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, threeToThree ? "convert: in place needs the same pointer, rowBytes and frameBytes" : "convert: an output plane overlaps an input plane");
		}
	*a = ConvertArgs{};
	for (int p = 0; p < g->planesIn; ++p) { a->in[p] = si[p].p; a->inRow[p] = si[p].row; a->inFrame[p] = si[p].frame; }
	for (int p = 0; p < g->planesOut; ++p) { a->out[p] = const_cast<uint8_t*>(so[p].p); a->outRow[p] = so[p].row; a->outFrame[p] = so[p].frame; }
	a->W = static_cast<int>(W); a->H = static_cast<int>(H);
	return COMPVHIP_OK;
}

int compvhip_convert_frames(compvhip_ctx* ctx, size_t W, size_t H, size_t frames, const compvhip_image* in, const compvhip_image* out, void* stream)
{
	ConvertArgs a; ConvertGeometry g;
	const int rc = convertCheck(ctx, W, H, frames, in, out, &a, &g);
	if (rc) return rc;
	HIPCHK(ctx, hipSetDevice(ctx->device));
	HIPCHK(ctx, launch_convert(a, in->pixfmt, out->pixfmt, static_cast<int>(frames), static_cast<hipStream_t>(stream)));
	return COMPVHIP_OK;
}
