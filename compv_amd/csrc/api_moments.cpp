// api_moments.cpp -- the host side of the image moments (definition in include/compv_hip.h, "image moments"; arithmetic in moments_math.hpp; kernels in
// moments_kernels.hip).  The device calls are stateless on a context: every refusal comes before anything is enqueued, the sums land in the caller's
// records, and the stream travels in the descriptor.  The host form stages one plane in the context's buffers and runs on the context's stream.
#include "api_internal.hpp"
#include "moments_math.hpp"

namespace {
constexpr size_t kMaxCount = static_cast<size_t>(INT32_MAX);

bool knownWeights(int w) { return w == COMPVHIP_MOMENTS_VALUE || w == COMPVHIP_MOMENTS_UNIT; }

// what every call with a descriptor checks first
int checkDesc(compvhip_ctx* ctx, const compvhip_moments_desc* desc)
{
	if (!desc || desc->size != sizeof(compvhip_moments_desc)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "moments: null descriptor, or its size field is not sizeof(compvhip_moments_desc)");
	return COMPVHIP_OK;
}

// the refusals of a frames call that need no pointer
int checkFrames(compvhip_ctx* ctx, const compvhip_moments_desc* desc, size_t W, size_t H, size_t S, size_t frames)
{
	if (!knownWeights(desc->weights)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "moments: unknown weights");
	if (desc->origin != COMPVHIP_MOMENTS_ORIGIN_FRAME) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "moments: a frames call takes COMPVHIP_MOMENTS_ORIGIN_FRAME only");
	if (!moments::fits(W, H, desc->weights))
		return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "moments: W or H of 0 or beyond 32767, W * H >= 2^31, or wmax * W * H * max(W - 1, H - 1)^2 >= 2^64");
	if (S < W) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "moments: S < W");
	if (!frames || frames > kMaxCount) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "moments: frames outside 1 .. 2^31 - 1");
	return COMPVHIP_OK;
}

int enqueueFrames(compvhip_ctx* ctx, int weights, const uint8_t* d_gray, size_t W, size_t H, size_t S, size_t frames, compvhip_moments* d_raw, compvhip_moments_shape* d_shape,
                  hipStream_t st)
{
	MomentsFramesArgs a = {};
	a.gray = d_gray; a.W = static_cast<int>(W); a.H = static_cast<int>(H); a.S = S; a.frames = static_cast<int>(frames);
	a.unit = weights == COMPVHIP_MOMENTS_UNIT; a.raw = d_raw;
	HIPCHK(ctx, launch_moments_frames(a, st));
	if (d_shape) HIPCHK(ctx, launch_moments_shapes(MomentsShapeArgs{ d_raw, d_shape, frames, 1, nullptr }, st));
	return COMPVHIP_OK;
}
} // namespace

int compvhip_moments_fits(size_t W, size_t H, int weights) { return moments::fits(W, H, weights) ? 1 : 0; }

int compvhip_moments_shape_host(const compvhip_moments* raw, size_t n, compvhip_moments_shape* shape)
{
	if (n && (!raw || !shape)) return COMPVHIP_E_INVALID_PARAMETER;
	for (size_t k = 0; k < n; ++k) moments::shape(raw[k], shape + k);
	return COMPVHIP_OK;
}

int compvhip_moments_frames(compvhip_ctx* ctx, const compvhip_moments_desc* desc, const uint8_t* d_gray, size_t W, size_t H, size_t S, size_t frames, compvhip_moments* d_raw,
                            compvhip_moments_shape* d_shape)
{
	if (!ctx) return COMPVHIP_E_INVALID_PARAMETER;
	int rc = checkDesc(ctx, desc);
	if (!rc) rc = checkFrames(ctx, desc, W, H, S, frames);
	if (rc) return rc;
	if (!d_gray || !d_raw) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "moments: null frames or records");
	if (misaligned(7, d_raw, d_shape)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "moments: raw and shape records must be 8-byte aligned");
	HIPCHK(ctx, hipSetDevice(ctx->device));
	return enqueueFrames(ctx, desc->weights, d_gray, W, H, S, frames, d_raw, d_shape, static_cast<hipStream_t>(desc->hipStream));
}

int compvhip_moments_components(compvhip_ctx* ctx, const compvhip_moments_desc* desc, const int32_t* d_labels, size_t W, size_t H, size_t labelStride, const uint8_t* d_gray,
                                size_t S, const compvhip_component* d_comps, size_t compCap, const int32_t* d_compCounts, size_t frames, compvhip_moments* d_raw,
                                compvhip_moments_shape* d_shape)
{
	if (!ctx) return COMPVHIP_E_INVALID_PARAMETER;
	const int rc = checkDesc(ctx, desc);
	if (rc) return rc;
	if (!knownWeights(desc->weights)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "moments: unknown weights");
	if (desc->origin != COMPVHIP_MOMENTS_ORIGIN_FRAME && desc->origin != COMPVHIP_MOMENTS_ORIGIN_BOX) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "moments: unknown origin");
	// without gray planes every pixel of a component weighs 1
	if (!moments::fits(W, H, d_gray ? desc->weights : COMPVHIP_MOMENTS_UNIT))
		return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "moments: W or H of 0 or beyond 32767, W * H >= 2^31, or wmax * W * H * max(W - 1, H - 1)^2 >= 2^64");
	if (labelStride < W || (d_gray && S < W)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "moments: labelStride < W or S < W");
	if (!frames || frames > kMaxCount || !compCap || compCap > kMaxCount) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "moments: frames or compCap outside 1 .. 2^31 - 1");
	if (!d_labels || !d_comps || !d_compCounts || !d_raw) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "moments: null labels, component records, counts or records");
	if (misaligned(3, d_labels, d_compCounts) || misaligned(3, d_comps) || misaligned(7, d_raw, d_shape))
		return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "moments: labels, component records and counts must be 4-byte, raw and shape records 8-byte aligned");
	HIPCHK(ctx, hipSetDevice(ctx->device));
	hipStream_t st = static_cast<hipStream_t>(desc->hipStream);
	MomentsCompArgs a = {};
	a.labels = d_labels; a.W = static_cast<int>(W); a.H = static_cast<int>(H); a.labelStride = labelStride; a.gray = d_gray; a.S = S;
	a.comps = d_comps; a.compCap = static_cast<int>(compCap); a.counts = d_compCounts; a.frames = static_cast<int>(frames);
	a.unit = desc->weights == COMPVHIP_MOMENTS_UNIT; a.box = desc->origin == COMPVHIP_MOMENTS_ORIGIN_BOX; a.raw = d_raw;
	HIPCHK(ctx, launch_moments_components(a, st));
	if (d_shape) HIPCHK(ctx, launch_moments_shapes(MomentsShapeArgs{ d_raw, d_shape, frames, a.compCap, d_compCounts }, st));
	return COMPVHIP_OK;
}

int compvhip_moments_shapes(compvhip_ctx* ctx, const compvhip_moments_desc* desc, const compvhip_moments* d_raw, size_t n, compvhip_moments_shape* d_shape)
{
	if (!ctx) return COMPVHIP_E_INVALID_PARAMETER;
	const int rc = checkDesc(ctx, desc);
	if (rc) return rc;
	if (n > kMaxCount) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "moments: n beyond 2^31 - 1");
	if (!n) return COMPVHIP_OK;
	if (!d_raw || !d_shape) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "moments: null records");
	if (misaligned(7, d_raw) || misaligned(7, d_shape)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "moments: raw and shape records must be 8-byte aligned");
	HIPCHK(ctx, hipSetDevice(ctx->device));
	HIPCHK(ctx, launch_moments_shapes(MomentsShapeArgs{ d_raw, d_shape, n, 1, nullptr }, static_cast<hipStream_t>(desc->hipStream)));
	return COMPVHIP_OK;
}

int compvhip_moments_host(compvhip_ctx* ctx, const compvhip_moments_desc* desc, const uint8_t* in, size_t W, size_t H, size_t S, compvhip_moments* raw,
                          compvhip_moments_shape* shape)
{
	if (!ctx) return COMPVHIP_E_INVALID_PARAMETER;
	int rc = checkDesc(ctx, desc);
	if (!rc) rc = checkFrames(ctx, desc, W, H, S, 1);
	if (rc) return rc;
	if (!in || !raw) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "moments: null image or record");
	HIPCHK(ctx, hipSetDevice(ctx->device));
	static_assert(sizeof(compvhip_moments) == 48 && sizeof(compvhip_moments_shape) == 72, "the records of include/compv_hip.h");
	// staging of the call's own (in front of the frame, which drains before it goes): the caller's records are written only by a call that succeeded as a whole
	compvhip_moments r; compvhip_moments_shape s;
	HostCall hc(ctx->stream);
	const size_t Sd = stagePlane(ctx, hc, ctx->dIn, in, W, H, S);
	HOSTSTEP(ctx, hc, ctx->dMoments.reserve(ctx, (sizeof(compvhip_moments) + sizeof(compvhip_moments_shape)) / 8));
	compvhip_moments* dRaw = reinterpret_cast<compvhip_moments*>(ctx->dMoments.ptr);
	compvhip_moments_shape* dShape = shape ? reinterpret_cast<compvhip_moments_shape*>(dRaw + 1) : nullptr;
	rc = enqueueFrames(ctx, desc->weights, ctx->dIn, W, H, Sd, 1, dRaw, dShape, ctx->stream);
	if (rc) return rc;
	hc.download(&r, dRaw, sizeof(r), "moments: record download");
	if (shape) hc.download(&s, dShape, sizeof(s), "moments: record download");
	if (!hc.wait()) return hostStatus(ctx, hc);
	*raw = r; if (shape) *shape = s;
	return COMPVHIP_OK;
}
