// api_undistort.cpp -- the host side of lens undistortion (definition in include/compv_hip.h, "lens undistortion"; arithmetic in undistort_math.hpp): the
// host-only coefficient and map calls, the handle that owns the staging of the cameras, and its device calls -- the fused image form (remap_kernels.hip,
// kRemapUndist), maps, points and projection (undistort_kernels.hip).  Built like the SVM handle: the stream travels in the descriptor.  Cameras and poses
// are host arrays per call: their coefficient records are worked out on the host into a ring of pinned slots (WarpTables, as the inverse warp's tables)
// and uploaded in stream order, so the caller's arrays are free when the call returns.
#include "api_internal.hpp"
#include "undistort_math.hpp"

namespace {
constexpr size_t kMaxSide = 32767;
constexpr size_t kRec = undist::kCoeffs, kPose = undist::kPose;

template <typename T>
int hostCoeffs(const T* K, const T* d, int nd, T* coeffs)
{
	if (!K || !d || !coeffs) return COMPVHIP_E_INVALID_PARAMETER;
	return undist::coeffs(K, d, nd, coeffs) ? COMPVHIP_OK : COMPVHIP_E_INVALID_PARAMETER;
}

bool windowOk(size_t x0, size_t y0, size_t Wout, size_t Hout)
{
	return Wout && Hout && Wout <= kMaxSide && Hout <= kMaxSide && x0 <= kMaxSide && y0 <= kMaxSide && x0 + Wout <= kMaxSide && y0 + Hout <= kMaxSide;
}

template <typename T>
int hostMap(const T* K, const T* d, int nd, size_t x0, size_t y0, size_t Wout, size_t Hout, T* mapX, T* mapY)
{
	if (!K || !d || !mapX || !mapY || !windowOk(x0, y0, Wout, Hout)) return COMPVHIP_E_INVALID_PARAMETER;
	T c[kRec];
	if (!undist::coeffs(K, d, nd, c)) return COMPVHIP_E_INVALID_PARAMETER;
	for (size_t j = 0, k = 0; j < Hout; ++j)
		for (size_t i = 0; i < Wout; ++i, ++k) undist::map_entry(c, static_cast<T>(x0 + i), static_cast<T>(y0 + j), mapX[k], mapY[k]);
	return COMPVHIP_OK;
}

// `count` records of T from K [count][9] and d [count][nd] into rec; false: a singular camera (nd was checked)
template <typename T>
bool buildRecords(const void* K, const void* d, int nd, size_t count, void* rec)
{
	for (size_t m = 0; m < count; ++m)
		if (!undist::coeffs(static_cast<const T*>(K) + 9 * m, static_cast<const T*>(d) + static_cast<size_t>(nd) * m, nd, static_cast<T*>(rec) + kRec * m)) return false;
	return true;
}

bool knownType(int type) { return type == COMPVHIP_UNDISTORT_F32 || type == COMPVHIP_UNDISTORT_F64; }

// what every device call checks about its cameras; `units`: the frames or sets a camera count may equal
int checkCameras(compvhip_ctx* ctx, const void* K, const void* d, int nd, size_t cameraCount, size_t units)
{
	if (!K || !d) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "undistort: null K or d");
	if (nd < 2 || nd > 4) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "undistort: nd outside 2 .. 4");
	if (cameraCount != 1 && cameraCount != units) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "undistort: cameraCount must be 1 or the frames / sets of the call");
	return COMPVHIP_OK;
}

// the records of the call's cameras (float64: f64), then `extraBytes` of `extra` (the poses), through the next slot; *dev: where they lie on the device
int stageCameras(compvhip_ctx* ctx, WarpTables* t, const void* K, const void* d, int nd, size_t count, bool f64, const void* extra, size_t extraBytes, hipStream_t st,
                 const uint8_t** dev)
{
	const size_t recBytes = count * kRec * (f64 ? 8 : 4), floats = (recBytes + extraBytes + 3) / 4;
	float* host = nullptr;
	WarpTables::Slot* s = nullptr;
	int rc = tablesSlot(ctx, t, floats, &host, &s);
	if (rc) return rc;
	if (!(f64 ? buildRecords<double>(K, d, nd, count, host) : buildRecords<float>(K, d, nd, count, host)))
		return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "undistort: fx * fy == 0, the camera matrix is singular");          // nothing was enqueued
	if (extraBytes) memcpy(reinterpret_cast<uint8_t*>(host) + recBytes, extra, extraBytes);
	rc = tablesSend(ctx, t, s, floats, st);
	*dev = reinterpret_cast<const uint8_t*>(t->dev.ptr);
	return rc;
}

// the shape of a point call against the handle's caps
int checkPoints(compvhip_undistort* u, size_t sets, size_t n)
{
	if (!sets || sets > u->maxSets || !n || n > u->maxPoints) return fail(u->ctx, COMPVHIP_E_INVALID_PARAMETER, "undistort: sets must be in 1 .. maxSets and n in 1 .. maxPoints");
	return COMPVHIP_OK;
}
} // namespace

int compvhip_api::tablesSlot(compvhip_ctx* ctx, WarpTables* t, size_t floats, float** host, WarpTables::Slot** slot)
{
	WarpTables::Slot& s = t->slot[t->next];
	t->next = (t->next + 1) % kAsyncDepth;
	if (s.copied) HIPCHK(ctx, hipEventSynchronize(s.copied));          // the copy that last read this slot (kAsyncDepth calls ago)
	else HIPCHK(ctx, hipEventCreateWithFlags(&s.copied, hipEventDisableTiming));
	HIPCHK(ctx, s.host.reserve(floats));
	HIPCHK(ctx, t->dev.reserve(ctx, floats));          // grows only: a reallocation frees with hipFree, which waits for the kernels that still read the old one
	*host = s.host; *slot = &s;
	return COMPVHIP_OK;
}

int compvhip_api::tablesSend(compvhip_ctx* ctx, WarpTables* t, WarpTables::Slot* s, size_t floats, hipStream_t st)
{
	HIPCHK(ctx, hipMemcpyAsync(t->dev, s->host, floats * sizeof(float), hipMemcpyHostToDevice, st));
	HIPCHK(ctx, hipEventRecord(s->copied, st));
	return COMPVHIP_OK;
}

int compvhip_api::undistCoords(compvhip_ctx* ctx, WarpTables* t, const float* K, const float* d, int nd, size_t count, size_t x0, size_t y0, RemapArgs* a, hipStream_t st)
{
	const uint8_t* dev = nullptr;
	const int rc = stageCameras(ctx, t, K, d, nd, count, false, nullptr, 0, st, &dev);
	if (rc) return rc;
	a->tables = reinterpret_cast<const float*>(dev); a->coordFrameStride = kRec;
	a->originX = static_cast<int>(x0); a->originY = static_cast<int>(y0);
	return COMPVHIP_OK;
}

bool compvhip_api::undistWindowOk(size_t x0, size_t y0, size_t Wout, size_t Hout) { return windowOk(x0, y0, Wout, Hout); }

int compvhip_undistort_coeffs_f32(const float* K, const float* d, int nd, float* coeffs) { return hostCoeffs(K, d, nd, coeffs); }
int compvhip_undistort_coeffs_f64(const double* K, const double* d, int nd, double* coeffs) { return hostCoeffs(K, d, nd, coeffs); }
int compvhip_undistort_map_f32(const float* K, const float* d, int nd, size_t x0, size_t y0, size_t Wout, size_t Hout, float* mapX, float* mapY)
{
	return hostMap(K, d, nd, x0, y0, Wout, Hout, mapX, mapY);
}
int compvhip_undistort_map_f64(const double* K, const double* d, int nd, size_t x0, size_t y0, size_t Wout, size_t Hout, double* mapX, double* mapY)
{
	return hostMap(K, d, nd, x0, y0, Wout, Hout, mapX, mapY);
}

int compvhip_undistort_create(compvhip_ctx* ctx, const compvhip_undistort_desc* desc, compvhip_undistort** out)
{
	if (!ctx || !out) return COMPVHIP_E_INVALID_PARAMETER;
	*out = nullptr;
	if (!desc || desc->size != sizeof(compvhip_undistort_desc)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "undistort: null descriptor, or its size field is not sizeof(compvhip_undistort_desc)");
	const size_t W = desc->W, H = desc->H, S = desc->S, frames = desc->frames;
	if (!W || !H || W > kMaxSide || H > kMaxSide || S < W || S < 4 || S * H > static_cast<size_t>(INT32_MAX) || !frames || frames > static_cast<size_t>(INT32_MAX))
		return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "undistort: a source size of 0 or beyond 32767, S < W, S < 4, a frame beyond 2^31 bytes, or frames outside 1 .. 2^31 - 1");
	if (!windowOk(desc->x0, desc->y0, desc->Wout, desc->Hout))
		return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "undistort: an output size of 0 or beyond 32767, or x0 + Wout / y0 + Hout beyond 32767");
	if (desc->maxSets > static_cast<uint32_t>(INT32_MAX) || desc->maxPoints > static_cast<uint32_t>(INT32_MAX) ||
	    static_cast<size_t>(desc->maxSets) * desc->maxPoints >= (size_t(1) << 40))
		return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "undistort: maxSets or maxPoints beyond 2^31 - 1, or maxSets * maxPoints reaches 2^40");
	HIPCHK(ctx, hipSetDevice(ctx->device));
	compvhip_undistort* u = new (std::nothrow) compvhip_undistort();
	if (!u) return fail(ctx, COMPVHIP_E_OUT_OF_MEMORY, "undistort");
	u->ctx = ctx; u->stream = static_cast<hipStream_t>(desc->stream);
	u->W = W; u->H = H; u->S = S; u->frames = frames; u->Wout = desc->Wout; u->Hout = desc->Hout; u->x0 = desc->x0; u->y0 = desc->y0;
	u->maxSets = desc->maxSets; u->maxPoints = desc->maxPoints;
	// the largest staging a call can ask for, in floats: float64 records of every frame (maps), or float64 records and poses of every set (projection)
	const size_t floats = std::max(frames * kRec * 2, u->maxSets * (kRec + kPose) * 2);
	hipError_t e = u->stage.dev.reserve(ctx, floats);
	for (auto& s : u->stage.slot) {
		if (e == hipSuccess) e = s.host.reserve(floats);
		if (e == hipSuccess) e = hipEventCreateWithFlags(&s.copied, hipEventDisableTiming);
	}
	if (e != hipSuccess) {
		handleDestroy(u);
		return fail(ctx, e == hipErrorOutOfMemory ? COMPVHIP_E_OUT_OF_MEMORY : COMPVHIP_E_HIP, "undistort: staging", e);
	}
	*out = u;
	return COMPVHIP_OK;
}

void compvhip_undistort_destroy(compvhip_undistort* u) { handleDestroy(u); }
int compvhip_undistort_set_timing(compvhip_undistort* u, int enabled) { return handleSetTiming(u, enabled); }
int compvhip_undistort_get_timing(compvhip_undistort* u, const char** names, float* ms, int cap) { return handleGetTiming(u, names, ms, cap); }

int compvhip_undistort_frames(compvhip_undistort* u, const uint8_t* d_in, const float* K, const float* d, int nd, size_t cameraCount, int interp, const compvhip_roi* roi,
                              uint8_t defaultValue, void* d_out, size_t Sout)
{
	if (!u) return COMPVHIP_E_INVALID_PARAMETER;
	compvhip_ctx* ctx = u->ctx;
	int rc = checkCameras(ctx, K, d, nd, cameraCount, u->frames);
	if (rc) return rc;
	HIPCHK(ctx, hipSetDevice(ctx->device));
	RemapArgs a;
	rc = remapPrepare(ctx, d_in, u->W, u->H, u->S, u->frames, interp, roi, d_out, u->Wout, u->Hout, Sout, defaultValue, &a);
	if (rc) return rc;
	rc = undistCoords(ctx, &u->stage, K, d, nd, cameraCount, u->x0, u->y0, &a, u->stream);
	if (rc) return rc;
	if (u->timing) timelineClear(u);
	Stamp s(u, u->stream, "undistort_kernel");
	HIPCHK(ctx, launch_remap(a, kRemapUndist, interp, cameraCount != 1, u->stream));
	return COMPVHIP_OK;
}

int compvhip_undistort_maps(compvhip_undistort* u, const void* K, const void* d, int nd, size_t cameraCount, int type, void* d_mapX, void* d_mapY)
{
	if (!u) return COMPVHIP_E_INVALID_PARAMETER;
	compvhip_ctx* ctx = u->ctx;
	int rc = checkCameras(ctx, K, d, nd, cameraCount, u->frames);
	if (rc) return rc;
	if (!knownType(type)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "undistort: unknown type");
	const bool f64 = type == COMPVHIP_UNDISTORT_F64;
	const size_t elem = f64 ? 8 : 4, planeBytes = cameraCount * u->Wout * u->Hout * elem;
	if (!d_mapX || !d_mapY) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "undistort: null map");
	if (misaligned(elem - 1, static_cast<const uint8_t*>(d_mapX), static_cast<const uint8_t*>(d_mapY)))
		return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "undistort: maps must be aligned to their element size");
	if (overlaps(static_cast<const uint8_t*>(d_mapX), planeBytes, static_cast<const uint8_t*>(d_mapY), planeBytes))
		return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "undistort: mapX and mapY must not overlap");
	HIPCHK(ctx, hipSetDevice(ctx->device));
	const uint8_t* dev = nullptr;
	rc = stageCameras(ctx, &u->stage, K, d, nd, cameraCount, f64, nullptr, 0, u->stream, &dev);
	if (rc) return rc;
	UndistMapArgs m = {};
	m.coeffs = dev; m.coeffStride = cameraCount != 1 ? static_cast<int>(kRec) : 0; m.mapX = d_mapX; m.mapY = d_mapY;
	m.Wout = static_cast<int>(u->Wout); m.Hout = static_cast<int>(u->Hout); m.originX = static_cast<int>(u->x0); m.originY = static_cast<int>(u->y0);
	m.cameras = static_cast<int>(cameraCount); m.f64 = f64;
	if (u->timing) timelineClear(u);
	Stamp s(u, u->stream, "undist_map_kernel");
	HIPCHK(ctx, launch_undist_map(m, u->stream));
	return COMPVHIP_OK;
}

int compvhip_undistort_points(compvhip_undistort* u, const void* K, const void* d, int nd, size_t cameraCount, int type, const void* d_in, size_t sets, size_t n,
                              const int32_t* d_counts, void* d_out)
{
	if (!u) return COMPVHIP_E_INVALID_PARAMETER;
	compvhip_ctx* ctx = u->ctx;
	int rc = checkPoints(u, sets, n);
	if (!rc) rc = checkCameras(ctx, K, d, nd, cameraCount, sets);
	if (rc) return rc;
	if (!knownType(type)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "undistort: unknown type");
	const bool f64 = type == COMPVHIP_UNDISTORT_F64;
	const size_t elem = f64 ? 8 : 4, bytes = sets * n * 2 * elem;
	if (!d_in || !d_out) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "undistort: null point array");
	if (misaligned(elem - 1, static_cast<const uint8_t*>(d_in), static_cast<const uint8_t*>(d_out)) || misaligned(3, d_counts))
		return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "undistort: points must be aligned to their element size, counts to 4 bytes");
	if (d_in != d_out && overlaps(static_cast<const uint8_t*>(d_in), bytes, static_cast<const uint8_t*>(d_out), bytes))
		return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "undistort: input and output points must be the same array or must not overlap");
	HIPCHK(ctx, hipSetDevice(ctx->device));
	const uint8_t* dev = nullptr;
	rc = stageCameras(ctx, &u->stage, K, d, nd, cameraCount, f64, nullptr, 0, u->stream, &dev);
	if (rc) return rc;
	UndistPointsArgs p = {};
	p.coeffs = dev; p.coeffStride = cameraCount != 1 ? static_cast<int>(kRec) : 0; p.in = d_in; p.out = d_out; p.counts = d_counts;
	p.n = static_cast<int>(n); p.sets = static_cast<int>(sets); p.f64 = f64;
	if (u->timing) timelineClear(u);
	Stamp s(u, u->stream, "undist_points_kernel");
	HIPCHK(ctx, launch_undist_points(p, u->stream));
	return COMPVHIP_OK;
}

int compvhip_undistort_project(compvhip_undistort* u, const double* K, const double* d, int nd, size_t cameraCount, const double* Rt, const double* d_in, size_t sets,
                               size_t n, const int32_t* d_counts, double* d_out)
{
	if (!u) return COMPVHIP_E_INVALID_PARAMETER;
	compvhip_ctx* ctx = u->ctx;
	int rc = checkPoints(u, sets, n);
	if (!rc) rc = checkCameras(ctx, K, d, nd, cameraCount, sets);
	if (rc) return rc;
	if (!Rt || !d_in || !d_out) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "undistort: null pose or point array");
	if (misaligned(7, d_in, d_out) || misaligned(3, d_counts)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "undistort: points must be 8-byte, counts 4-byte aligned");
	if (overlaps(reinterpret_cast<const uint8_t*>(d_in), sets * n * 24, reinterpret_cast<const uint8_t*>(d_out), sets * n * 16))
		return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "undistort: input and output points must not overlap");
	HIPCHK(ctx, hipSetDevice(ctx->device));
	const uint8_t* dev = nullptr;
	rc = stageCameras(ctx, &u->stage, K, d, nd, cameraCount, true, Rt, sets * kPose * 8, u->stream, &dev);
	if (rc) return rc;
	UndistProjectArgs p = {};
	p.coeffs = reinterpret_cast<const double*>(dev); p.coeffStride = cameraCount != 1 ? static_cast<int>(kRec) : 0;
	p.poses = p.coeffs + cameraCount * kRec; p.in = d_in; p.out = d_out; p.counts = d_counts; p.n = static_cast<int>(n); p.sets = static_cast<int>(sets);
	if (u->timing) timelineClear(u);
	Stamp s(u, u->stream, "undist_project_kernel");
	HIPCHK(ctx, launch_undist_project(p, u->stream));
	return COMPVHIP_OK;
}
