// api_curvefit.cpp -- the host side of the RANSAC line and parabola fits (curvefit_kernels.hip; definition in include/compv_hip.h, "RANSAC curve
// fitting").  A handle carries its stream: every device call of the family runs on it.
#include "api_internal.hpp"
#include "curvefit_math.hpp"

namespace {
constexpr size_t kCurvefitMaxCap = size_t(1) << 22;     // points per set and tries: keeps every index and grid dimension in 32 bits

bool knownModel(int model) { return model >= 0 && model < cf::kModels; }

CurvefitFindArgs curvefitArgs(const compvhip_curvefit* h)
{
	CurvefitFindArgs a = {};
	a.points = h->points; a.counts = h->counts; a.pointCap = h->pointCap; a.maxTries = h->maxTries;
	a.sel = h->points + static_cast<size_t>(h->sets) * h->pointCap;
	a.scoreCount = h->scoreCount;
	return a;
}
} // namespace

int compvhip_curvefit_create(compvhip_ctx* ctx, const compvhip_curvefit_desc* desc, compvhip_curvefit** out)
{
	if (!ctx || !out) return COMPVHIP_E_INVALID_PARAMETER;
	*out = nullptr;
	if (!desc || desc->size != sizeof(compvhip_curvefit_desc)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "curvefit: null descriptor, or its size field is not sizeof(compvhip_curvefit_desc)");
	const size_t sets = desc->sets, pointCap = desc->pointCap, maxTries = desc->maxTries;
	if (int rc = refuseBeyondLaunchLimit(ctx, sets, "compvhip_curvefit_create (sets)")) return rc;   // a set is blockIdx.x / .y
	if (!sets || pointCap < 3 || !maxTries || pointCap > kCurvefitMaxCap || maxTries > kCurvefitMaxCap)
		return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "sets and maxTries must be >= 1, pointCap >= 3");
	HIPCHK(ctx, hipSetDevice(ctx->device));
	compvhip_curvefit* h = new (std::nothrow) compvhip_curvefit();
	if (!h) return fail(ctx, COMPVHIP_E_OUT_OF_MEMORY, "curvefit");
	h->ctx = ctx; h->stream = static_cast<hipStream_t>(desc->stream);
	h->sets = static_cast<int>(sets); h->pointCap = static_cast<int>(pointCap); h->maxTries = static_cast<int>(maxTries);
	if (h->points.reserve(ctx, 2 * sets * pointCap) != hipSuccess || h->counts.reserve(ctx, sets) != hipSuccess || h->scoreCount.reserve(ctx, sets * maxTries) != hipSuccess) {
		compvhip_curvefit_destroy(h);
		return fail(ctx, COMPVHIP_E_OUT_OF_MEMORY, "curvefit scratch");
	}
	*out = h;
	return COMPVHIP_OK;
}

void compvhip_curvefit_destroy(compvhip_curvefit* h)
{
	if (!h) return;
	(void)hipSetDevice(h->ctx->device);
	timingTeardown(h);
	delete h;
}

int compvhip_curvefit_set_timing(compvhip_curvefit* h, int enabled)
{
	if (!h) return COMPVHIP_E_INVALID_PARAMETER;
	h->timing = enabled != 0;
	return COMPVHIP_OK;
}

int compvhip_curvefit_get_timing(compvhip_curvefit* h, const char** names, float* ms, int cap)
{
	if (!h) return COMPVHIP_E_INVALID_PARAMETER;
	return timingRead(h, h->ctx->device, names, ms, cap);
}

int compvhip_curvefit_points_from_labels(compvhip_curvefit* h, const int32_t* d_labels, size_t W, size_t H, size_t labelStride, const compvhip_component* d_comps,
                                         size_t compCap, const int32_t* d_compCounts, size_t frames)
{
	if (!h) return COMPVHIP_E_INVALID_PARAMETER;
	compvhip_ctx* ctx = h->ctx;
	if (!d_labels || !d_comps || !d_compCounts) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "null label map / record / count pointer");
	if (!W || !H || W > 32767 || H > 32767 || labelStride < W || labelStride > 0x7fffffffull) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "frame size out of range (1..32767), or labelStride < W");
	if (!compCap || !frames || compCap > static_cast<size_t>(h->sets) || frames > static_cast<size_t>(h->sets) || frames * compCap != static_cast<size_t>(h->sets))
		return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "frames * compCap must equal the handle's sets");
	if (misaligned(3, d_labels, d_comps, d_compCounts)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "labels, records and counts must be 4-byte aligned");
	HIPCHK(ctx, hipSetDevice(ctx->device));
	if (h->timing) timelineClear(h);
	CurvefitGatherArgs a = {};
	a.labels = d_labels; a.W = static_cast<int>(W); a.H = static_cast<int>(H); a.labelStride = static_cast<int>(labelStride);
	a.comps = d_comps; a.compCap = static_cast<int>(compCap); a.compCounts = d_compCounts;
	a.points = h->points; a.pointCap = h->pointCap; a.counts = h->counts;
	{ Stamp s(h, h->stream, "curvefit_gather_kernel"); HIPCHK(ctx, launch_curvefit_gather(a, h->sets, h->stream)); }
	h->gathered = true;
	return COMPVHIP_OK;
}

int compvhip_curvefit_find(compvhip_curvefit* h, const double* d_points, const int32_t* d_counts, const compvhip_curvefit_opts* opts, const int32_t* d_samples,
                           compvhip_curvefit_result* d_results, uint8_t* d_mask)
{
	if (!h) return COMPVHIP_E_INVALID_PARAMETER;
	compvhip_ctx* ctx = h->ctx;
	if (!opts || !d_results) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "null options / result pointer");
	if (opts->size != sizeof(compvhip_curvefit_opts)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "curvefit: the options' size field is not sizeof(compvhip_curvefit_opts)");
	if (!knownModel(opts->model)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "unknown model");
	if (opts->tries < 1 || opts->tries > h->maxTries) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "tries must be in 1..maxTries");
	if (!(opts->threshold > 0.0)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "threshold must be > 0");
	if (!d_points && !h->gathered) return fail(ctx, COMPVHIP_E_INVALID_STATE, "no points: compvhip_curvefit_points_from_labels has not run on this handle");
	if (misaligned(15, d_points, d_samples)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "points and samples must be 16-byte aligned");
	if (misaligned(7, d_results) || misaligned(3, d_counts)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "results must be 8-byte, counts 4-byte aligned");
	HIPCHK(ctx, hipSetDevice(ctx->device));
	if (h->timing) timelineClear(h);
	CurvefitFindArgs a = curvefitArgs(h);
	if (d_points) { a.points = reinterpret_cast<const double2*>(d_points); a.counts = d_counts; }
	a.model = opts->model; a.tries = opts->tries; a.seed = opts->seed; a.threshold = opts->threshold; a.samples = d_samples; a.results = d_results; a.mask = d_mask;
	{ Stamp s(h, h->stream, "curvefit_score_kernel"); HIPCHK(ctx, launch_curvefit_score(a, h->sets, h->stream)); }
	{ Stamp s(h, h->stream, "curvefit_refit_kernel"); HIPCHK(ctx, launch_curvefit_refit(a, h->sets, h->stream)); }
	return COMPVHIP_OK;
}

int compvhip_curvefit_distances(compvhip_curvefit* h, const double* d_points, const int32_t* d_counts, int model, const double* d_params, double* d_out)
{
	if (!h) return COMPVHIP_E_INVALID_PARAMETER;
	compvhip_ctx* ctx = h->ctx;
	if (!d_params || !d_out) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "null params / output pointer");
	if (!knownModel(model)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "unknown model");
	if (!d_points && !h->gathered) return fail(ctx, COMPVHIP_E_INVALID_STATE, "no points: compvhip_curvefit_points_from_labels has not run on this handle");
	if (misaligned(15, d_points)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "points must be 16-byte aligned");
	if (misaligned(7, d_params, d_out) || misaligned(3, d_counts)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "params and distances must be 8-byte, counts 4-byte aligned");
	HIPCHK(ctx, hipSetDevice(ctx->device));
	if (h->timing) timelineClear(h);
	CurvefitDistanceArgs a = {};
	a.points = h->points; a.counts = h->counts; a.pointCap = h->pointCap; a.model = model; a.params = d_params; a.out = d_out;
	if (d_points) { a.points = reinterpret_cast<const double2*>(d_points); a.counts = d_counts; }
	{ Stamp s(h, h->stream, "curvefit_distance_kernel"); HIPCHK(ctx, launch_curvefit_distances(a, h->sets, h->stream)); }
	return COMPVHIP_OK;
}

int compvhip_curvefit_scores(compvhip_curvefit* h, size_t tries, int32_t* counts, int32_t* gathered)
{
	if (!h) return COMPVHIP_E_INVALID_PARAMETER;
	compvhip_ctx* ctx = h->ctx;
	if (!tries || tries > static_cast<size_t>(h->maxTries)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "tries must be in 1..maxTries");
	HIPCHK(ctx, hipSetDevice(ctx->device));
	const size_t S = static_cast<size_t>(h->sets), T = static_cast<size_t>(h->maxTries);
	if (counts) HIPCHK(ctx, hipMemcpy2DAsync(counts, tries * 4, h->scoreCount, T * 4, tries * 4, S, hipMemcpyDeviceToHost, h->stream));
	if (gathered) HIPCHK(ctx, hipMemcpyAsync(gathered, h->counts, S * 4, hipMemcpyDeviceToHost, h->stream));
	HIPCHK(ctx, hipStreamSynchronize(h->stream));
	return COMPVHIP_OK;
}

int compvhip_curvefit_gathered(compvhip_curvefit* h, const double** d_points, const int32_t** d_counts)
{
	if (!h) return COMPVHIP_E_INVALID_PARAMETER;
	if (d_points) *d_points = reinterpret_cast<const double*>(h->points.ptr);
	if (d_counts) *d_counts = h->counts.ptr;
	return COMPVHIP_OK;
}

// ---- the host forms -----------------------------------------------------------------------------------------------------------------------------
int compvhip_curvefit_samples(int model, uint32_t seed, size_t set, size_t k, size_t tries, int32_t* samples)
{
	if (!samples || !knownModel(model)) return COMPVHIP_E_INVALID_PARAMETER;
	const size_t m = static_cast<size_t>(cf::modelPoints(model));
	if (k <= m || k > 0xffffffffull || set > 0xffffffffull || tries > 0xffffffffull) return COMPVHIP_E_INVALID_PARAMETER;
	for (size_t t = 0; t < tries; ++t) {
		int32_t q[3];
		cf::sample(model, seed, static_cast<uint32_t>(set), static_cast<uint32_t>(t), static_cast<uint32_t>(k), q);
		for (size_t j = 0; j < m; ++j) samples[m * t + j] = q[j];
	}
	return COMPVHIP_OK;
}

int compvhip_curvefit_find_f64(compvhip_ctx* ctx, const double* points, size_t n, const compvhip_curvefit_opts* opts, const int32_t* samples,
                               compvhip_curvefit_result* result, uint8_t* mask)
{
	if (!ctx) return COMPVHIP_E_INVALID_PARAMETER;
	if (!opts || !result || (n && !points)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "null argument");
	if (opts->size != sizeof(compvhip_curvefit_opts) || !knownModel(opts->model) || opts->tries < 1 || n > kCurvefitMaxCap)
		return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "curvefit: wrong size field, unknown model, tries < 1 or too many points");
	HIPCHK(ctx, hipSetDevice(ctx->device));
	const size_t cap = std::max<size_t>(n, 3), T = static_cast<size_t>(opts->tries), m = static_cast<size_t>(cf::modelPoints(opts->model));
	compvhip_curvefit_desc desc = {};
	desc.size = sizeof(desc); desc.sets = 1; desc.pointCap = static_cast<uint32_t>(cap); desc.maxTries = static_cast<uint32_t>(T); desc.stream = ctx->stream;
	compvhip_curvefit* h = nullptr;
	int rc = compvhip_curvefit_create(ctx, &desc, &h);
	if (rc) return rc;
	DevBuf<double> dPts; DevBuf<int32_t> dInts; DevBuf<compvhip_curvefit_result> dRes; DevBuf<uint8_t> dMask;   // freed on the way out, behind the drain of the stream below
	do {
		if (dPts.reserve(ctx, 2 * cap) != hipSuccess || dInts.reserve(ctx, 4 + m * T) != hipSuccess || dRes.reserve(ctx, 1) != hipSuccess || dMask.reserve(ctx, cap) != hipSuccess) {
			rc = fail(ctx, COMPVHIP_E_OUT_OF_MEMORY, "curvefit staging"); break;
		}
		const int32_t count = static_cast<int32_t>(n);
		hipError_t e = hipMemcpyAsync(dInts, &count, 4, hipMemcpyHostToDevice, ctx->stream);
		if (e == hipSuccess && n) e = hipMemcpyAsync(dPts, points, n * 16, hipMemcpyHostToDevice, ctx->stream);
		if (e == hipSuccess && samples) e = hipMemcpyAsync(dInts + 4, samples, m * T * 4, hipMemcpyHostToDevice, ctx->stream);
		if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);          // `count` is the host's stack
		if (e != hipSuccess) { rc = fail(ctx, COMPVHIP_E_HIP, "point upload", e); break; }
		rc = compvhip_curvefit_find(h, dPts, dInts, opts, samples ? dInts + 4 : nullptr, dRes, mask ? dMask.ptr : nullptr);
		if (rc) break;
		compvhip_curvefit_result r;
		e = hipMemcpyAsync(&r, dRes, sizeof(r), hipMemcpyDeviceToHost, ctx->stream);
		if (e == hipSuccess && mask && n) e = hipMemcpyAsync(mask, dMask, n, hipMemcpyDeviceToHost, ctx->stream);
		if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
		if (e != hipSuccess) { rc = fail(ctx, COMPVHIP_E_HIP, "result download", e); break; }
		*result = r;
	} while (0);
	(void)hipStreamSynchronize(ctx->stream);
	compvhip_curvefit_destroy(h);
	return rc;
}
