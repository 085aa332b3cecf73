// api_pca.cpp -- the host side of the PCA projection (definition in include/compv_hip.h, "PCA projection"; arithmetic in pca_math.hpp; kernels in
// pca_kernels.hip).  The device calls are stateless on a context: every refusal comes before anything is enqueued, the model lives in arrays the
// caller owns, and the stream travels in the descriptor.  The host form stages the model and slices of rows in the context's buffers and runs on the
// context's stream.  The parser and the dot product need no GPU.
#include "api_internal.hpp"
#include "pca_math.hpp"

namespace {
constexpr size_t kPcaHostSlice = 512;

// what every call with a descriptor checks first
int checkDesc(compvhip_ctx* ctx, const compvhip_pca_desc* desc)
{
	if (!desc || desc->size != sizeof(compvhip_pca_desc)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "pca: null descriptor, or its size field is not sizeof(compvhip_pca_desc)");
	return COMPVHIP_OK;
}

// the refusals of R[aRows][bRows] = A[aRows][cols] * B[bRows][cols]^T that need no pointer
int checkShape(compvhip_ctx* ctx, size_t aRows, size_t aMax, size_t aStride, size_t bRows, size_t bMax, size_t bStride, size_t cols, size_t rStride)
{
	if (!cols || cols > pca::kMaxDim) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "pca: dim / cols outside 1 .. 2^20");
	if (!bRows || bRows > bMax) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "pca: components outside 1 .. 65535 (bRows: 1 .. 2^20)");
	if (aRows > aMax) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "pca: n beyond 2^31 - 1 (aRows: beyond 2^20)");
	if (!pca::strideFits(aRows, aStride, cols) || !pca::strideFits(bRows, bStride, cols) || !pca::strideFits(aRows, rStride, bRows))
		return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "pca: a stride below its row length, or rows * stride reaches 2^40");
	return COMPVHIP_OK;
}

int enqueueProject(compvhip_ctx* ctx, const float* d_mean, const float* d_vectors, size_t vecStride, size_t dim, size_t components, const float* d_in, size_t n, size_t inStride,
                   float* d_out, size_t outStride, hipStream_t st)
{
	PcaProjectArgs a = {};
	a.in = d_in; a.n = static_cast<int>(n); a.inStride = inStride; a.mean = d_mean;
	a.vectors = d_vectors; a.comps = static_cast<int>(components); a.vecStride = vecStride; a.dim = static_cast<int>(dim);
	a.out = d_out; a.outStride = outStride;
	HIPCHK(ctx, launch_pca_project(a, st));
	return COMPVHIP_OK;
}

int scratchShape(size_t n, size_t dim, size_t* nPad)
{
	if (!n || n > pca::kMaxRows || !dim || dim > pca::kMaxDim) return COMPVHIP_E_INVALID_PARAMETER;
	*nPad = (n + 15) / 16 * 16;
	return pca::strideFits(dim, *nPad, n) ? COMPVHIP_OK : COMPVHIP_E_INVALID_PARAMETER;
}
} // namespace

int compvhip_pca_project(compvhip_ctx* ctx, const compvhip_pca_desc* desc, const float* d_mean, const float* d_vectors, size_t vecStride, size_t dim, size_t components,
                         const float* d_in, size_t n, size_t inStride, float* d_out, size_t outStride)
{
	if (!ctx) return COMPVHIP_E_INVALID_PARAMETER;
	int rc = checkDesc(ctx, desc);
	if (!rc) rc = checkShape(ctx, n, pca::kMaxRows, inStride, components, pca::kMaxComponents, vecStride, dim, outStride);
	if (rc) return rc;
	if (!n) return COMPVHIP_OK;
	if (!d_vectors || !d_in || !d_out) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "pca: null vectors, input or output");
	if (misaligned(3, d_mean, d_vectors, d_in) || misaligned(3, d_out)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "pca: pointers must be 4-byte aligned");
	HIPCHK(ctx, hipSetDevice(ctx->device));
	return enqueueProject(ctx, d_mean, d_vectors, vecStride, dim, components, d_in, n, inStride, d_out, outStride, static_cast<hipStream_t>(desc->hipStream));
}

int compvhip_mulabt_f32(compvhip_ctx* ctx, const compvhip_pca_desc* desc, const float* d_A, size_t aRows, size_t aStride, const float* d_B, size_t bRows, size_t bStride,
                        size_t cols, float* d_R, size_t rStride)
{
	if (!ctx) return COMPVHIP_E_INVALID_PARAMETER;
	int rc = checkDesc(ctx, desc);
	if (!rc) rc = checkShape(ctx, aRows, pca::kMaxDim, aStride, bRows, pca::kMaxDim, bStride, cols, rStride);
	if (rc) return rc;
	if (!aRows) return COMPVHIP_OK;
	if (!d_A || !d_B || !d_R) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "mulabt: null A, B or R");
	if (misaligned(3, d_A, d_B) || misaligned(3, d_R)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "mulabt: pointers must be 4-byte aligned");
	HIPCHK(ctx, hipSetDevice(ctx->device));
	return enqueueProject(ctx, nullptr, d_B, bStride, cols, bRows, d_A, aRows, aStride, d_R, rStride, static_cast<hipStream_t>(desc->hipStream));
}

int compvhip_pca_covariance_scratch(size_t n, size_t dim, size_t* bytes)
{
	size_t nPad = 0;
	if (!bytes || scratchShape(n, dim, &nPad)) return COMPVHIP_E_INVALID_PARAMETER;
	*bytes = dim * nPad * sizeof(float);
	return COMPVHIP_OK;
}

int compvhip_pca_covariance(compvhip_ctx* ctx, const compvhip_pca_desc* desc, const float* d_obs, size_t n, size_t obsStride, size_t dim, float* d_mean, float* d_covar,
                            size_t covStride, void* d_scratch)
{
	if (!ctx) return COMPVHIP_E_INVALID_PARAMETER;
	const int rc = checkDesc(ctx, desc);
	if (rc) return rc;
	size_t nPad = 0;
	if (scratchShape(n, dim, &nPad)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "pca covariance: n outside 1 .. 2^31 - 1, dim outside 1 .. 2^20, or dim * nPad reaches 2^40");
	if (!pca::strideFits(n, obsStride, dim) || !pca::strideFits(dim, covStride, dim))
		return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "pca covariance: a stride below its row length, or rows * stride reaches 2^40");
	if (!d_obs || !d_mean || !d_covar || !d_scratch) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "pca covariance: null observations, mean, covariance or scratch");
	if (misaligned(3, d_obs, d_mean, d_covar) || misaligned(15, static_cast<const uint8_t*>(d_scratch)))
		return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "pca covariance: pointers must be 4-byte, the scratch 16-byte aligned");
	HIPCHK(ctx, hipSetDevice(ctx->device));
	hipStream_t st = static_cast<hipStream_t>(desc->hipStream);
	float* centred = static_cast<float*>(d_scratch);
	HIPCHK(ctx, launch_pca_mean(PcaMeanArgs{ d_obs, static_cast<int>(n), obsStride, static_cast<int>(dim), d_mean }, st));
	HIPCHK(ctx, launch_pca_centre_transpose(PcaCentreArgs{ d_obs, static_cast<int>(n), obsStride, static_cast<int>(dim), d_mean, centred, nPad }, st));
	PcaProjectArgs a = {};
	a.in = centred; a.n = static_cast<int>(dim); a.inStride = nPad; a.mean = nullptr;
	a.vectors = centred; a.comps = static_cast<int>(dim); a.vecStride = nPad; a.dim = static_cast<int>(n);
	a.out = d_covar; a.outStride = covStride;
	if (n > 1) { a.scaled = 1; a.scale = pca::covarScale(n); }
	HIPCHK(ctx, launch_pca_project(a, st));
	return COMPVHIP_OK;
}

int compvhip_pca_project_host(compvhip_ctx* ctx, const compvhip_pca_desc* desc, const float* mean, const float* vectors, size_t vecStride, size_t dim, size_t components,
                              const float* in, size_t n, size_t inStride, float* out, size_t outStride)
{
	if (!ctx) return COMPVHIP_E_INVALID_PARAMETER;
	int rc = checkDesc(ctx, desc);
	if (!rc) rc = checkShape(ctx, n, pca::kMaxRows, inStride, components, pca::kMaxComponents, vecStride, dim, outStride);
	if (rc) return rc;
	if (!n) return COMPVHIP_OK;
	if (!vectors || !in || !out) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "pca: null vectors, input or output");
	HIPCHK(ctx, hipSetDevice(ctx->device));
	const size_t slice = std::min(n, kPcaHostSlice);
	HostCall hc(ctx->stream);
	HOSTSTEP(ctx, hc, ctx->dPcaModel.reserve(ctx, dim + components * dim));
	HOSTSTEP(ctx, hc, ctx->dPcaIn.reserve(ctx, slice * dim));
	HOSTSTEP(ctx, hc, ctx->dPcaOut.reserve(ctx, slice * components));
	float* dMean = mean ? ctx->dPcaModel.ptr : nullptr;
	float* dVectors = ctx->dPcaModel.ptr + dim;
	if (mean) hc.upload(dMean, mean, dim * 4, "pca: model upload");
	hc.upload2D(dVectors, dim * 4, vectors, vecStride * 4, dim * 4, components, "pca: model upload");
	for (size_t at = 0; at < n; at += slice) {
		const size_t cnt = std::min(slice, n - at);
		if (!hc.upload2D(ctx->dPcaIn.ptr, dim * 4, in + at * inStride, inStride * 4, dim * 4, cnt, "pca: row upload")) break;
		rc = enqueueProject(ctx, dMean, dVectors, dim, dim, components, ctx->dPcaIn.ptr, cnt, dim, ctx->dPcaOut.ptr, components, ctx->stream);
		if (rc) return rc;
		hc.download2D(out + at * outStride, outStride * 4, ctx->dPcaOut.ptr, components * 4, components * 4, cnt, "pca: row download");
		if (!hc.wait()) break;          // the staging is used again by the next slice
	}
	return hostStatus(ctx, hc);
}

int compvhip_pca_model_parse(const char* path, int32_t* dim, int32_t* components, float* mean, float* vectors, float* values)
{
	if (!path || !dim || !components) return COMPVHIP_E_INVALID_PARAMETER;
	pca::Model m;
	if (!pca::parse_model(path, m, nullptr)) return COMPVHIP_E_INVALID_PARAMETER;
	*dim = m.dim; *components = m.components;
	if (mean) memcpy(mean, m.mean.data(), m.mean.size() * 4);
	if (vectors) memcpy(vectors, m.vectors.data(), m.vectors.size() * 4);
	if (values) memcpy(values, m.values.data(), m.values.size() * 4);
	return COMPVHIP_OK;
}

int compvhip_pca_dot_host(const float* a, const float* b, size_t n, float* out)
{
	if (!out || (n && (!a || !b))) return COMPVHIP_E_INVALID_PARAMETER;
	*out = pca::dot16(a, b, n);
	return COMPVHIP_OK;
}
