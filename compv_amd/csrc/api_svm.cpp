// api_svm.cpp -- the host side of SVM prediction (svm_kernels.hip; definition in include/compv_hip.h, "SVM prediction"): the handle that owns a model on
// the device and the scratch of maxVectors queries, the two create paths (host arrays, libsvm model file), the device and host predict calls, and the
// host-only helpers (exp_ref, the parser) that need no GPU.  Built like the curve-fit handle: the stream travels in the descriptor.
#include "api_internal.hpp"
#include "svm_math.hpp"

namespace {
constexpr size_t kSvmMaxVectors = size_t(1) << 22;
constexpr size_t kSvmHostSlice = 512;

const uint64_t* expTable()
{
	static const std::vector<uint64_t> table = [] { std::vector<uint64_t> t(svm::kExpTable); svm::exp_table(t.data()); return t; }();
	return table.data();
}

// the checks of item F and of the descriptor, the handle, the model's upload and every scratch buffer
int svmCreate(compvhip_ctx* ctx, int kernel, int nrClass, int l, int dim, double gamma, const double* sv, const double* svCoef, const double* rho, const int32_t* nSV,
              const int32_t* label, const compvhip_svm_desc* desc, compvhip_svm** out)
{
	if (!desc || desc->size != sizeof(compvhip_svm_desc)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "svm: null descriptor, or its size field is not sizeof(compvhip_svm_desc)");
	if (!sv || !svCoef || !rho || !nSV || !label) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "svm: null model array");
	if (nrClass < 2 || nrClass > svm::kMaxClasses) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "svm: nrClass outside 2 .. 32");
	if (const char* bad = svm::refuse_shape(kernel, nrClass, l, dim, nSV)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, (std::string("svm: ") + bad).c_str());
	const size_t maxVectors = desc->maxVectors;
	if (!maxVectors || maxVectors > kSvmMaxVectors || maxVectors * static_cast<size_t>(l) >= (size_t(1) << 31))
		return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "svm: maxVectors outside 1 .. 2^22, or maxVectors * totalSV reaches 2^31");
	HIPCHK(ctx, hipSetDevice(ctx->device));
	compvhip_svm* h = new (std::nothrow) compvhip_svm();
	if (!h) return fail(ctx, COMPVHIP_E_OUT_OF_MEMORY, "svm");
	TempHandle<compvhip_svm> handle{ ctx, h, handleDestroy<compvhip_svm> };   // a failed create destroys it
	h->ctx = ctx; h->stream = static_cast<hipStream_t>(desc->stream);
	h->kernel = kernel; h->nrClass = nrClass; h->l = l; h->dim = dim; h->pairs = nrClass * (nrClass - 1) / 2; h->gamma = gamma;
	h->maxVectors = maxVectors; h->hostSlice = std::min(maxVectors, kSvmHostSlice);
	const size_t L = static_cast<size_t>(l), D = static_cast<size_t>(dim), P = static_cast<size_t>(h->pairs);
	HostCall hc(h->stream);
	stageArray(ctx, hc, h->sv, sv, L * D);
	stageArray(ctx, hc, h->svCoef, svCoef, static_cast<size_t>(nrClass - 1) * L);
	stageArray(ctx, hc, h->rho, rho, P);
	stageArray(ctx, hc, h->nSV, nSV, static_cast<size_t>(nrClass));
	stageArray(ctx, hc, h->label, label, static_cast<size_t>(nrClass));
	stageArray(ctx, hc, h->expTable, expTable(), static_cast<size_t>(svm::kExpTable));
	HOSTSTEP(ctx, hc, h->kvalues.reserve(ctx, maxVectors * L));
	HOSTSTEP(ctx, hc, h->hostVectors.reserve(ctx, h->hostSlice * D));
	HOSTSTEP(ctx, hc, h->hostDec.reserve(ctx, h->hostSlice * P));
	HOSTSTEP(ctx, hc, h->hostLabels.reserve(ctx, h->hostSlice));
	if (!hc.wait()) return hostStatus(ctx, hc);          // the uploads read the caller's arrays
	*out = h; handle.h = nullptr;
	return COMPVHIP_OK;
}

bool knownType(int type) { return type == COMPVHIP_SVM_F32 || type == COMPVHIP_SVM_F64; }

void fillShape(compvhip_svm_shape* s, int kernel, int nrClass, int l, int dim, size_t maxVectors, double gamma)
{
	s->kernel = kernel; s->nrClass = nrClass; s->totalSV = l; s->dim = dim; s->pairs = nrClass * (nrClass - 1) / 2;
	s->maxVectors = static_cast<uint32_t>(maxVectors); s->reserved = 0; s->gamma = gamma;
}
} // namespace

int compvhip_svm_create(compvhip_ctx* ctx, const compvhip_svm_model* model, const compvhip_svm_desc* desc, compvhip_svm** out)
{
	if (!ctx || !out) return COMPVHIP_E_INVALID_PARAMETER;
	*out = nullptr;
	if (!model || model->size != sizeof(compvhip_svm_model)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "svm: null model, or its size field is not sizeof(compvhip_svm_model)");
	return svmCreate(ctx, model->kernel, model->nrClass, model->totalSV, model->dim, model->gamma, model->sv, model->svCoef, model->rho, model->nSV, model->label, desc, out);
}

int compvhip_svm_create_from_file(compvhip_ctx* ctx, const char* path, const compvhip_svm_desc* desc, compvhip_svm** out)
{
	if (!ctx || !out) return COMPVHIP_E_INVALID_PARAMETER;
	*out = nullptr;
	svm::Model m;
	std::string why;
	if (!svm::parse_model(path, m, &why)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, ("svm model file: " + why).c_str());
	return svmCreate(ctx, m.kernel, m.nrClass, m.l, m.dim, m.gamma, m.sv.data(), m.svCoef.data(), m.rho.data(), m.nSV.data(), m.label.data(), desc, out);
}

void compvhip_svm_destroy(compvhip_svm* h) { handleDestroy(h); }
int compvhip_svm_set_timing(compvhip_svm* h, int enabled) { return handleSetTiming(h, enabled); }
int compvhip_svm_get_timing(compvhip_svm* h, const char** names, float* ms, int cap) { return handleGetTiming(h, names, ms, cap); }

int compvhip_svm_info(compvhip_svm* h, compvhip_svm_shape* shape)
{
	if (!h) return COMPVHIP_E_INVALID_PARAMETER;
	if (!shape || shape->size != sizeof(compvhip_svm_shape)) return fail(h->ctx, COMPVHIP_E_INVALID_PARAMETER, "svm: null shape, or its size field is not sizeof(compvhip_svm_shape)");
	fillShape(shape, h->kernel, h->nrClass, h->l, h->dim, h->maxVectors, h->gamma);
	return COMPVHIP_OK;
}

int compvhip_svm_predict(compvhip_svm* h, const void* d_vectors, int type, size_t n, size_t strideElems, int32_t* d_labels, double* d_dec, double* d_kvalues)
{
	if (!h) return COMPVHIP_E_INVALID_PARAMETER;
	compvhip_ctx* ctx = h->ctx;
	if (!d_vectors || !d_labels) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "svm: null vector / label pointer");
	if (!knownType(type)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "svm: unknown vector type");
	if (!n || n > h->maxVectors) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "svm: n must be in 1..maxVectors");
	if (strideElems < static_cast<size_t>(h->dim) || strideElems >= (size_t(1) << 40) || n * strideElems >= (size_t(1) << 40))
		return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "svm: strideElems below dim, or n * strideElems reaches 2^40");
	if (misaligned(type == COMPVHIP_SVM_F32 ? 3 : 7, static_cast<const uint8_t*>(d_vectors))) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "svm: vectors must be aligned to their element size");
	if (misaligned(7, d_dec, d_kvalues) || misaligned(3, d_labels)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "svm: decision and kernel values must be 8-byte, labels 4-byte aligned");
	HIPCHK(ctx, hipSetDevice(ctx->device));
	if (h->timing) timelineClear(h);
	SvmKvaluesArgs k = {};
	k.vectors = d_vectors; k.f32 = type == COMPVHIP_SVM_F32; k.n = static_cast<int>(n); k.stride = strideElems;
	k.sv = h->sv; k.l = h->l; k.dim = h->dim; k.rbf = h->kernel == COMPVHIP_SVM_KERNEL_RBF; k.gamma = h->gamma; k.expTable = h->expTable;
	k.K = d_kvalues ? d_kvalues : h->kvalues.ptr;
	SvmDecideArgs d = {};
	d.K = k.K; d.n = k.n; d.l = h->l; d.nrClass = h->nrClass; d.nSV = h->nSV; d.svCoef = h->svCoef; d.rho = h->rho; d.label = h->label;
	d.labels = d_labels; d.dec = d_dec;
	{ Stamp s(h, h->stream, "svm_kvalues_kernel"); HIPCHK(ctx, launch_svm_kvalues(k, h->stream)); }
	{ Stamp s(h, h->stream, "svm_decide_kernel"); HIPCHK(ctx, launch_svm_decide(d, h->stream)); }
	return COMPVHIP_OK;
}

int compvhip_svm_predict_host(compvhip_svm* h, const void* vectors, int type, size_t n, size_t strideElems, int32_t* labels, double* dec)
{
	if (!h) return COMPVHIP_E_INVALID_PARAMETER;
	compvhip_ctx* ctx = h->ctx;
	if (!vectors || !labels) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "svm: null vector / label pointer");
	if (!knownType(type)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "svm: unknown vector type");
	const size_t D = static_cast<size_t>(h->dim), P = static_cast<size_t>(h->pairs), elem = type == COMPVHIP_SVM_F32 ? 4 : 8;
	if (!n || strideElems < D || strideElems >= (size_t(1) << 40) || n >= (size_t(1) << 40) / strideElems)
		return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "svm: n of 0, strideElems below dim, or n * strideElems reaches 2^40");
	HIPCHK(ctx, hipSetDevice(ctx->device));
	const uint8_t* src = static_cast<const uint8_t*>(vectors);
	HostCall hc(h->stream);
	for (size_t at = 0; at < n; at += h->hostSlice) {
		const size_t cnt = std::min(h->hostSlice, n - at);
		if (!hc.upload2D(h->hostVectors.ptr, D * elem, src + at * strideElems * elem, strideElems * elem, D * elem, cnt, "svm: vector upload")) break;
		if (int rc = compvhip_svm_predict(h, h->hostVectors.ptr, type, cnt, D, h->hostLabels, dec ? h->hostDec.ptr : nullptr, nullptr)) return rc;
		hc.download(labels + at, h->hostLabels, cnt * 4, "svm: label download");
		if (dec) hc.download(dec + at * P, h->hostDec, cnt * P * 8, "svm: decision download");
		if (!hc.wait()) break;          // the staging is used again by the next slice
	}
	return hostStatus(ctx, hc);
}

int compvhip_svm_exp_f64(const double* in, double* out, size_t n)
{
	if (n && (!in || !out)) return COMPVHIP_E_INVALID_PARAMETER;
	const uint64_t* T = expTable();
	for (size_t i = 0; i < n; ++i) out[i] = svm::exp_ref(in[i], T);
	return COMPVHIP_OK;
}

int compvhip_svm_model_parse(const char* path, compvhip_svm_shape* shape, double* sv, double* svCoef, double* rho, int32_t* nSV, int32_t* label)
{
	if (!path || !shape || shape->size != sizeof(compvhip_svm_shape)) return COMPVHIP_E_INVALID_PARAMETER;
	svm::Model m;
	if (!svm::parse_model(path, m, nullptr)) return COMPVHIP_E_INVALID_PARAMETER;
	fillShape(shape, m.kernel, m.nrClass, m.l, m.dim, 0, m.gamma);
	if (sv) memcpy(sv, m.sv.data(), m.sv.size() * 8);
	if (svCoef) memcpy(svCoef, m.svCoef.data(), m.svCoef.size() * 8);
	if (rho) memcpy(rho, m.rho.data(), m.rho.size() * 8);
	if (nSV) memcpy(nSV, m.nSV.data(), m.nSV.size() * 4);
	if (label) memcpy(label, m.label.data(), m.label.size() * 4);
	return COMPVHIP_OK;
}
