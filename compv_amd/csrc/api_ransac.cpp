// api_ransac.cpp -- the host side of the two RANSAC families: the homography (homography_kernels.hip; definition in include/compv_hip.h, "RANSAC
// homography") and the line and parabola fits (curvefit_kernels.hip; "RANSAC curve fitting").  The handles share a base (RansacHandle), one create
// path, one check of the find options, one download of the scores and one body of the host forms; a family adds its buffers, its gather call and its
// launches.  The homography takes its stream per call, a curve-fit handle carries its stream: that difference is ABI.
#include "api_internal.hpp"
#include "curvefit_math.hpp"

namespace {
constexpr size_t kRansacMaxCap = size_t(1) << 22;     // points per set and tries: keeps every index and grid dimension in 32 bits

// what the shared paths need to know about a family: its words in the messages, the least pointCap (the points of a model, at least 3), the point
// arrays of a set and the reservation of its own buffers
struct HomographyFamily {
	static constexpr const char* name = "homography"; static constexpr const char* sets = "pairs"; static constexpr const char* gather = "compvhip_homography_points";
	static constexpr size_t minCap = 4, arrays = 2;
	static bool reserve(compvhip_homography* h, size_t sets, size_t maxTries)
	{
		return h->tryF64.reserve(h->ctx, sets * maxTries * 19) == hipSuccess && h->tryI32.reserve(h->ctx, sets * maxTries * 3) == hipSuccess;
	}
};
struct CurvefitFamily {
	static constexpr const char* name = "curvefit"; static constexpr const char* sets = "sets"; static constexpr const char* gather = "compvhip_curvefit_points_from_labels";
	static constexpr size_t minCap = 3, arrays = 1;
	static bool reserve(compvhip_curvefit* h, size_t sets, size_t maxTries) { return h->scoreCount.reserve(h->ctx, sets * maxTries) == hipSuccess; }
};

// the limit checks, the handle and its buffers; a reservation that fails destroys the handle and reports
template <typename F, typename H>
int ransacCreate(compvhip_ctx* ctx, size_t sets, size_t pointCap, size_t maxTries, H** out)
{
	if (!ctx || !out) return COMPVHIP_E_INVALID_PARAMETER;
	*out = nullptr;
	const std::string name = F::name;
	if (int rc = refuseBeyondLaunchLimit(ctx, sets, ("compvhip_" + name + "_create (" + F::sets + ")").c_str())) return rc;   // a set is blockIdx.x / .y
	if (!sets || pointCap < F::minCap || !maxTries || pointCap > kRansacMaxCap || maxTries > kRansacMaxCap)
		return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, (std::string(F::sets) + " and maxTries must be >= 1, pointCap >= " + std::to_string(F::minCap)).c_str());
	HIPCHK(ctx, hipSetDevice(ctx->device));
	H* h = new (std::nothrow) H();
	if (!h) return fail(ctx, COMPVHIP_E_OUT_OF_MEMORY, F::name);
	h->ctx = ctx; h->sets = static_cast<int>(sets); h->pointCap = static_cast<int>(pointCap); h->maxTries = static_cast<int>(maxTries);
	if (h->points.reserve(ctx, 2 * F::arrays * sets * pointCap) != hipSuccess || h->counts.reserve(ctx, sets) != hipSuccess || !F::reserve(h, sets, maxTries)) {
		handleDestroy(h);
		return fail(ctx, COMPVHIP_E_OUT_OF_MEMORY, (name + " scratch").c_str());
	}
	*out = h;
	return COMPVHIP_OK;
}

// the find options both families have; callerPoints: the call brings its own points
template <typename F>
int ransacCheckFind(const RansacHandle* h, int tries, double threshold, bool callerPoints)
{
	if (tries < 1 || tries > h->maxTries) return fail(h->ctx, COMPVHIP_E_INVALID_PARAMETER, "tries must be in 1..maxTries");
	if (!(threshold > 0.0)) return fail(h->ctx, COMPVHIP_E_INVALID_PARAMETER, "threshold must be > 0");
	if (!callerPoints && !h->gathered) return fail(h->ctx, COMPVHIP_E_INVALID_STATE, (std::string("no points: ") + F::gather + " has not run on this handle").c_str());
	return COMPVHIP_OK;
}

// the first `tries` entries of per-try rows [sets][maxTries] to the host, packed; then the gathered counts; synchronous
struct ScoreRows { void* host; const void* dev; size_t elem; };
int ransacScores(RansacHandle* h, size_t tries, hipStream_t st, std::initializer_list<ScoreRows> rows, int32_t* gathered)
{
	compvhip_ctx* ctx = h->ctx;
	if (!tries || tries > static_cast<size_t>(h->maxTries)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "tries must be in 1..maxTries");
	HIPCHK(ctx, hipSetDevice(ctx->device));
	const size_t S = static_cast<size_t>(h->sets), T = static_cast<size_t>(h->maxTries);
	HostCall hc(st);
	for (const ScoreRows& r : rows)
		if (r.host) hc.download2D(r.host, tries * r.elem, r.dev, T * r.elem, tries * r.elem, S, "score download");
	if (gathered) hc.download(gathered, h->counts, S * 4, "count download");
	return hostWait(ctx, hc);
}

// The body of the *_find_f64 host forms, behind their argument checks: a handle of one set of max(n, minCap) points and T tries (create), the points'
// F::arrays arrays, the count and the optional samples (m indices per try) staged on the context's stream, find(h, points, cap, counts, samples,
// result, mask) on device pointers, the record and the mask back.
template <typename F, typename H, typename Result, typename Create, typename Find>
int ransacFindF64(compvhip_ctx* ctx, const double* const* pts, size_t n, size_t T, size_t m, const int32_t* samples, Result* result, uint8_t* mask, Create create, Find find)
{
	HIPCHK(ctx, hipSetDevice(ctx->device));
	const size_t cap = std::max<size_t>(n, F::minCap);
	H* h = nullptr;
	int rc = create(cap, T, &h);
	if (rc) return rc;
	const TempHandle<H> handle{ ctx, h, handleDestroy<H> };          // it, the buffers and the stack variables of the copies go behind the drain of the frame
	DevBuf<double> dPts; DevBuf<int32_t> dInts; DevBuf<Result> dRes; DevBuf<uint8_t> dMask;
	const int32_t count = static_cast<int32_t>(n);
	Result r;
	HostCall hc(ctx->stream);
	HOSTSTEP(ctx, hc, dPts.reserve(ctx, 2 * F::arrays * cap));
	HOSTSTEP(ctx, hc, dInts.reserve(ctx, 4 + m * T));
	HOSTSTEP(ctx, hc, dRes.reserve(ctx, 1));
	HOSTSTEP(ctx, hc, dMask.reserve(ctx, cap));
	hc.upload(dInts, &count, 4, "point upload");
	for (size_t a = 0; a < F::arrays; ++a)
		if (n) hc.upload(dPts + 2 * cap * a, pts[a], n * 16, "point upload");
	if (samples) hc.upload(dInts + 4, samples, m * T * 4, "point upload");
	if (!hc.wait()) return hostStatus(ctx, hc);
	rc = find(h, dPts.ptr, cap, dInts.ptr, samples ? dInts + 4 : nullptr, dRes.ptr, mask ? dMask.ptr : nullptr);
	if (rc) return rc;
	hc.download(&r, dRes, sizeof(r), "result download");
	if (mask && n) hc.download(mask, dMask, n, "result download");
	if (!hc.wait()) return hostStatus(ctx, hc);
	*result = r;
	return COMPVHIP_OK;
}

HomographyFindArgs homographyArgs(const compvhip_homography* h)
{
	const size_t P = static_cast<size_t>(h->sets), cap = static_cast<size_t>(h->pointCap), T = static_cast<size_t>(h->maxTries);
	HomographyFindArgs a = {};
	a.src = h->points; a.dst = h->points + P * cap; a.counts = h->counts; a.pointCap = h->pointCap;
	a.selSrc = h->points + 2 * P * cap; a.selDst = h->points + 3 * P * cap;
	a.maxTries = h->maxTries;
	a.hyp = h->tryF64; a.scoreVar = h->tryF64 + P * T * 18;
	a.state = h->tryI32; a.rotations = h->tryI32 + P * T; a.scoreCount = h->tryI32 + 2 * P * T;
	return a;
}

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

// ---- RANSAC homography ----------------------------------------------------------------------------------------------------------------------------
int compvhip_homography_create(compvhip_ctx* ctx, size_t pairs, size_t pointCap, size_t maxTries, compvhip_homography** out)
{
	return ransacCreate<HomographyFamily>(ctx, pairs, pointCap, maxTries, out);
}
void compvhip_homography_destroy(compvhip_homography* h) { handleDestroy(h); }
int compvhip_homography_set_timing(compvhip_homography* h, int enabled) { return handleSetTiming(h, enabled); }
int compvhip_homography_get_timing(compvhip_homography* h, const char** names, float* ms, int cap) { return handleGetTiming(h, names, ms, cap); }

int compvhip_homography_points(compvhip_homography* h, const compvhip_match* d_good, size_t goodCap, const int32_t* d_goodCounts, const compvhip_keypoint* d_query,
                               size_t queryCap, const compvhip_keypoint* d_train, size_t trainCap, int trainShared, void* stream)
{
	if (!h) return COMPVHIP_E_INVALID_PARAMETER;
	compvhip_ctx* ctx = h->ctx;
	if (!d_query || !d_train || (goodCap && !d_good)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "null good / keypoint pointer");
	if (!queryCap || !trainCap || goodCap > kRansacMaxCap || queryCap > kRansacMaxCap || trainCap > kRansacMaxCap)
		return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "capacity out of range");
	if (misaligned(15, d_good)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "match records must be 16-byte aligned");
	if (misaligned(3, d_goodCounts, d_query, d_train)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "counts and keypoints must be 4-byte aligned");
	HIPCHK(ctx, hipSetDevice(ctx->device));
	hipStream_t st = static_cast<hipStream_t>(stream);
	if (h->timing) timelineClear(h);
	const HomographyFindArgs f = homographyArgs(h);
	HomographyPointsArgs a = {};
	a.good = d_good; a.goodCap = static_cast<int>(goodCap); a.goodCounts = d_goodCounts;
	a.query = d_query; a.queryCap = static_cast<int>(queryCap); a.train = d_train; a.trainCap = static_cast<int>(trainCap); a.trainShared = trainShared != 0;
	a.src = const_cast<double2*>(f.src); a.dst = const_cast<double2*>(f.dst); a.pointCap = h->pointCap; a.counts = h->counts;
	{ Stamp s(h, st, "homography_points_kernel"); HIPCHK(ctx, launch_homography_points(a, h->sets, st)); }
	h->gathered = true;
	return COMPVHIP_OK;
}

int compvhip_homography_find(compvhip_homography* h, const double* d_src, const double* d_dst, const int32_t* d_counts, const compvhip_homography_opts* opts,
                             const int32_t* d_quads, compvhip_homography_result* d_results, uint8_t* d_mask, void* stream)
{
	if (!h) return COMPVHIP_E_INVALID_PARAMETER;
	compvhip_ctx* ctx = h->ctx;
	if (!opts || !d_results) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "null options / result pointer");
	if (int rc = ransacCheckFind<HomographyFamily>(h, opts->tries, opts->threshold, d_src != nullptr)) return rc;
	if (d_src && !d_dst) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "d_src without d_dst");
	if (misaligned(15, d_src, d_dst, d_quads)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "points and quads must be 16-byte aligned");
	if (misaligned(7, d_results) || misaligned(3, d_counts)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "results must be 8-byte, counts 4-byte aligned");
	HIPCHK(ctx, hipSetDevice(ctx->device));
	hipStream_t st = static_cast<hipStream_t>(stream);
	if (h->timing) timelineClear(h);
	HomographyFindArgs a = homographyArgs(h);
	if (d_src) { a.src = reinterpret_cast<const double2*>(d_src); a.dst = reinterpret_cast<const double2*>(d_dst); a.counts = d_counts; }
	a.tries = opts->tries; a.seed = opts->seed; a.threshold = opts->threshold; a.quads = d_quads; a.results = d_results; a.mask = d_mask;
	{ Stamp s(h, st, "homography_solve_kernel"); HIPCHK(ctx, launch_homography_solve(a, h->sets, st)); }
	{ Stamp s(h, st, "homography_score_kernel"); HIPCHK(ctx, launch_homography_score(a, h->sets, st)); }
	{ Stamp s(h, st, "homography_refit_kernel"); HIPCHK(ctx, launch_homography_refit(a, h->sets, st)); }
	return COMPVHIP_OK;
}

int compvhip_homography_project(compvhip_homography* h, const compvhip_homography_result* d_results, const double* d_points, size_t n, int shared, double* d_out,
                                void* stream)
{
	if (!h) return COMPVHIP_E_INVALID_PARAMETER;
	compvhip_ctx* ctx = h->ctx;
	if (!d_results || (n && (!d_points || !d_out)) || n > kRansacMaxCap) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "null result / point pointer, or n out of range");
	if (misaligned(15, d_points, d_out) || misaligned(7, d_results)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "points must be 16-byte, results 8-byte aligned");
	HIPCHK(ctx, hipSetDevice(ctx->device));
	hipStream_t st = static_cast<hipStream_t>(stream);
	if (h->timing) timelineClear(h);
	HomographyProjectArgs a = {};
	a.results = d_results; a.points = reinterpret_cast<const double2*>(d_points); a.n = static_cast<int>(n); a.shared = shared != 0;
	a.out = reinterpret_cast<double2*>(d_out);
	{ Stamp s(h, st, "homography_project_kernel"); HIPCHK(ctx, launch_homography_project(a, h->sets, st)); }
	return COMPVHIP_OK;
}

int compvhip_homography_scores(compvhip_homography* h, size_t tries, int32_t* counts, double* variances, int32_t* rotations, void* stream)
{
	if (!h) return COMPVHIP_E_INVALID_PARAMETER;
	const HomographyFindArgs a = homographyArgs(h);
	return ransacScores(h, tries, static_cast<hipStream_t>(stream), { { counts, a.scoreCount, 4 }, { rotations, a.rotations, 4 }, { variances, a.scoreVar, 8 } }, nullptr);
}

int compvhip_homography_quads(uint32_t seed, size_t pair, size_t k, size_t tries, int32_t* quads)
{
	if (!quads || k < 4 || k > 0xffffffffull || pair > 0xffffffffull || tries > 0xffffffffull) return COMPVHIP_E_INVALID_PARAMETER;
	for (size_t t = 0; t < tries; ++t) hg::quad(seed, static_cast<uint32_t>(pair), static_cast<uint32_t>(t), static_cast<uint32_t>(k), quads + 4 * t);
	return COMPVHIP_OK;
}

int compvhip_homography_find_f64(compvhip_ctx* ctx, const double* src, const double* dst, size_t n, const compvhip_homography_opts* opts, const int32_t* quads,
                                 compvhip_homography_result* result, uint8_t* mask)
{
	if (!ctx) return COMPVHIP_E_INVALID_PARAMETER;
	if (!opts || !result || (n && (!src || !dst))) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "null argument");
	if (opts->tries < 1) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "tries must be >= 1");
	const double* const pts[2] = { src, dst };
	return ransacFindF64<HomographyFamily, compvhip_homography>(ctx, pts, n, static_cast<size_t>(opts->tries), 4, quads, result, mask,
		[&](size_t cap, size_t T, compvhip_homography** h) { return compvhip_homography_create(ctx, 1, cap, T, h); },
		[&](compvhip_homography* h, const double* d_pts, size_t cap, const int32_t* d_counts, const int32_t* d_quads, compvhip_homography_result* d_res, uint8_t* d_mask) {
			return compvhip_homography_find(h, d_pts, d_pts + 2 * cap, d_counts, opts, d_quads, d_res, d_mask, ctx->stream);
		});
}

// ---- RANSAC curve fitting -------------------------------------------------------------------------------------------------------------------------
int compvhip_curvefit_create(compvhip_ctx* ctx, const compvhip_curvefit_desc* desc, compvhip_curvefit** out)
{
	if (!ctx || !out) return COMPVHIP_E_INVALID_PARAMETER;
	*out = nullptr;
	if (!desc || desc->size != sizeof(compvhip_curvefit_desc)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "curvefit: null descriptor, or its size field is not sizeof(compvhip_curvefit_desc)");
	const int rc = ransacCreate<CurvefitFamily>(ctx, desc->sets, desc->pointCap, desc->maxTries, out);
	if (!rc) (*out)->stream = static_cast<hipStream_t>(desc->stream);
	return rc;
}
void compvhip_curvefit_destroy(compvhip_curvefit* h) { handleDestroy(h); }
int compvhip_curvefit_set_timing(compvhip_curvefit* h, int enabled) { return handleSetTiming(h, enabled); }
int compvhip_curvefit_get_timing(compvhip_curvefit* h, const char** names, float* ms, int cap) { return handleGetTiming(h, names, ms, cap); }

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
	if (int rc = ransacCheckFind<CurvefitFamily>(h, opts->tries, opts->threshold, d_points != nullptr)) return rc;
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
	return ransacScores(h, tries, h->stream, { { counts, h->scoreCount.ptr, 4 } }, gathered);
}

int compvhip_curvefit_gathered(compvhip_curvefit* h, const double** d_points, const int32_t** d_counts)
{
	if (!h) return COMPVHIP_E_INVALID_PARAMETER;
	if (d_points) *d_points = reinterpret_cast<const double*>(h->points.ptr);
	if (d_counts) *d_counts = h->counts.ptr;
	return COMPVHIP_OK;
}

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
	if (opts->size != sizeof(compvhip_curvefit_opts) || !knownModel(opts->model) || opts->tries < 1 || n > kRansacMaxCap)
		return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "curvefit: wrong size field, unknown model, tries < 1 or too many points");
	return ransacFindF64<CurvefitFamily, compvhip_curvefit>(ctx, &points, n, static_cast<size_t>(opts->tries), static_cast<size_t>(cf::modelPoints(opts->model)), samples, result, mask,
		[&](size_t cap, size_t T, compvhip_curvefit** h) {
			compvhip_curvefit_desc desc = {};
			desc.size = sizeof(desc); desc.sets = 1; desc.pointCap = static_cast<uint32_t>(cap); desc.maxTries = static_cast<uint32_t>(T); desc.stream = ctx->stream;
			return compvhip_curvefit_create(ctx, &desc, h);
		},
		[&](compvhip_curvefit* h, const double* d_pts, size_t, const int32_t* d_counts, const int32_t* d_samples, compvhip_curvefit_result* d_res, uint8_t* d_mask) {
			return compvhip_curvefit_find(h, d_pts, d_counts, opts, d_samples, d_res, d_mask);
		});
}
