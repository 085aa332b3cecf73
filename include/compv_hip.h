/* compv_hip.h -- C ABI of the MI355X (gfx950) implementation of CompV's Sobel -> Canny -> Hough hot path.
 *
 * This is the drop-in boundary: plain pointers and sizes, no C++ types, no ownership transfer.  It is what a
 * CompV maintainer binds from the replacement factories registered with CompVFeature::addFactory()
 * (reference: base/include/compv/base/compv_features.h:36-44 registry, base/compv_features.cxx:30-40 replace-by-id);
 * the reference-side binding is shown in INTEGRATION.md and implemented in integration/compv_hip_plugin.cxx.
 * Precedent for a function-pointer GPU hook in the reference: gpu/include/compv/gpu/base/math/compv_gpu_math_convlt.h.
 *
 * All file:line citations are relative to the CompV source tree.
 *
 * Conventions
 *   - return value: 0 = success (COMPV_ERROR_CODE_S_OK), negative = COMPVHIP_E_* (mapping to COMPV_ERROR_CODE in
 *     INTEGRATION.md).  No exceptions cross this boundary.
 *   - W,H = columns/rows, S = row stride in elements (bytes for u8).  Images are single-plane uint8.
 *   - "host" entry points take HOST pointers, are synchronous and leave results valid in host memory on return
 *     (what CompVEdgeDete::process / CompVHough::process promise their callers).
 *   - "dev" entry points take DEVICE pointers to frames resident in HBM and enqueue work on a HIP stream.
 *   - an instance (ctx / plan) is not re-entrant, exactly like a CompVEdgeDeteCanny / CompVHoughSht object
 *     (persistent scratch sized on first use: core/features/edges/compv_core_feature_canny_dete.cxx:133-147).
 */
#ifndef COMPV_HIP_H
#define COMPV_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#	define COMPVHIP_API __attribute__((visibility("default")))
#else
#	define COMPVHIP_API
#endif

/* ---- error codes (negative) ------------------------------------------------------------------------------- */
enum {
	COMPVHIP_OK = 0,
	COMPVHIP_E_NOT_IMPLEMENTED = -1,    /* COMPV_ERROR_CODE_E_NOT_IMPLEMENTED */
	COMPVHIP_E_NOT_INITIALIZED = -2,    /* COMPV_ERROR_CODE_E_NOT_INITIALIZED */
	COMPVHIP_E_INVALID_STATE = -3,      /* COMPV_ERROR_CODE_E_INVALID_STATE   (tLow >= tHigh, canny_dete.cxx:126) */
	COMPVHIP_E_INVALID_PARAMETER = -4,  /* COMPV_ERROR_CODE_E_INVALID_PARAMETER */
	COMPVHIP_E_OUT_OF_MEMORY = -5,      /* COMPV_ERROR_CODE_E_OUT_OF_MEMORY */
	COMPVHIP_E_OUT_OF_BOUND = -6,       /* COMPV_ERROR_CODE_E_OUT_OF_BOUND    (caller's line buffer too small) */
	COMPVHIP_E_HIP = -7                 /* a hipError_t; class of COMPV_ERROR_CODE_E_CUDA / _E_OPENCL (compv_common.h:265-266) */
};

/* ---- operator / mode ids ---------------------------------------------------------------------------------- */
enum { /* gradient operator of the edge detector; ids mirror COMPV_SOBEL_ID / _SCHARR_ID / _PREWITT_ID
          (compv_features.h:84-90), kernels compv_features.h:124-133 */
	COMPVHIP_OP_SOBEL = 0,
	COMPVHIP_OP_SCHARR = 2,
	COMPVHIP_OP_PREWITT = 3
};
enum { /* COMPV_CANNY_THRESHOLD_TYPE_* (compv_features.h:80-81) */
	COMPVHIP_CANNY_THRESHOLD_COMPARE_TO_GRADIENT = 0,
	COMPVHIP_CANNY_THRESHOLD_PERCENT_OF_MEAN = 1,
	/* plan API only -- the sample's per-frame sequence fused on the device (samples/hough_lines/main.cxx:103-105):
	 * t = thresholdOtsu(frame); LOW = (float)(t * tLow); HIGH = (float)(t * tHigh); then COMPARE_TO_GRADIENT.
	 * The sample uses the factors tLow = 0.5, tHigh = 1.0. */
	COMPVHIP_CANNY_THRESHOLD_OTSU = 2
};
typedef enum compvhip_pixfmt { /* packed input formats of CompVImage::convertGrayscale (COMPV_SUBTYPE_PIXELS_*, compv_common.h:347-367) */
	COMPVHIP_FMT_RGBA32 = 0, COMPVHIP_FMT_ARGB32 = 1, COMPVHIP_FMT_BGRA32 = 2, COMPVHIP_FMT_RGB24 = 3, COMPVHIP_FMT_BGR24 = 4,
	COMPVHIP_FMT_RGB565LE = 5, COMPVHIP_FMT_RGB565BE = 6, COMPVHIP_FMT_BGR565LE = 7, COMPVHIP_FMT_BGR565BE = 8,
	COMPVHIP_FMT_YUYV422 = 9, COMPVHIP_FMT_UYVY422 = 10,
	COMPVHIP_FMT_Y = 11, /* the Y plane of Y / NV12 / NV21 / YUV420P / YVU420P / YUV422P / YUV444P: a copy */
	/* formats of the colour conversion calls only (compvhip_convert_frames): every other call that takes a pixfmt refuses them with
	 * COMPVHIP_E_INVALID_PARAMETER */
	COMPVHIP_FMT_NV12 = 12, COMPVHIP_FMT_NV21 = 13, COMPVHIP_FMT_YUV420P = 14, COMPVHIP_FMT_YUV422P = 15, COMPVHIP_FMT_YUV444P = 16, COMPVHIP_FMT_HSV = 17
} compvhip_pixfmt;

/* One Hough line.  rho/theta/strength are CompVHoughLine's fields (compv_common.h:686-693); row/col are the
 * accumulator cell (rho = barrier - row, theta = col * thetaStepRad) and define the canonical tie order of the plan API. */
typedef struct compvhip_line {
	float rho;
	float theta;
	int32_t strength;
	int32_t row;
	int32_t col;
} compvhip_line;

typedef struct compvhip_ctx compvhip_ctx;     /* one GPU + its scratch; one per host thread / CompV object */
typedef struct compvhip_plan compvhip_plan;   /* batched device-resident pipeline for a fixed geometry */

/* ---- life cycle -------------------------------------------------------------------------------------------- */
COMPVHIP_API int compvhip_device_count(void);
/* device < 0: use the current HIP device. Replaces nothing in CompV: it is what CompVGpu::init() would call
 * (gpu/compv_gpu.cxx:53-58). */
COMPVHIP_API int compvhip_ctx_create(compvhip_ctx** ctx, int device);
COMPVHIP_API void compvhip_ctx_destroy(compvhip_ctx* ctx);
/* text of the last failure on this ctx (HIP error string included); never NULL */
COMPVHIP_API const char* compvhip_last_error(const compvhip_ctx* ctx);
/* hipMalloc/hipFree balance of this ctx -- the analogue of COMPV_DEBUG_CHECK_FOR_MEMORY_LEAKS (compv_api.h:148-155) */
COMPVHIP_API long compvhip_live_allocations(const compvhip_ctx* ctx);
/* Test hook, PROCESS-WIDE (every context, plan and handle of this library in the process; not for production use).  byte = 0 .. 255: from now on every
 * block of device or pinned host memory the library allocates is filled with that byte before it is used -- hipMalloc and hipHostMalloc promise nothing
 * about what a fresh block holds, and tests/test_gpu_fresh_memory.py shows with it that no call depends on it.  A buffer the library already has and reuses is
 * not touched.  -1 switches the fill off (the default).  Returns the previous value (-1 .. 255); any other byte returns COMPVHIP_E_INVALID_PARAMETER and
 * changes nothing.  While it is on, an allocation waits for the device; no launch path reads it. */
COMPVHIP_API int compvhip_debug_alloc_fill(int byte);

/* ---- host entry points (drop-in for process()) ------------------------------------------------------------- */

/* CompVCornerDeteEdgeBase::process (core/features/edges/compv_core_feature_edge_dete.cxx:55-206):
 * out = sat_u8(trunc(float(|gx|+|gy|) * (255.f / gmax))).  in and out may alias. */
COMPVHIP_API int compvhip_edge_dete_u8(compvhip_ctx* ctx, const uint8_t* in, size_t W, size_t H, size_t S, int op,
                                       uint8_t* out, size_t So);

/* CompVEdgeDeteCanny::process (core/features/edges/compv_core_feature_canny_dete.cxx:123-331).
 * tLow/tHigh are the detector's float thresholds (resolved to uint16 exactly as :251-266), ksize 3 or 5,
 * thresholdType COMPVHIP_CANNY_THRESHOLD_*.  out = {0,0xff}; in and out may alias (samples/edges_canny/main.cxx:72). */
COMPVHIP_API int compvhip_canny_u8(compvhip_ctx* ctx, const uint8_t* in, size_t W, size_t H, size_t S,
                                   float tLow, float tHigh, int ksize, int thresholdType, uint8_t* out, size_t So);

/* CompVImage::convertGrayscale (base/image/compv_image_conv_to_grayscale.cxx:35-90, called at samples/hough_lines/main.cxx:102):
 * packed RGB-family / YUV 4:2:2 frame -> luma plane, Y = ((33 R + 65 G + 13 B) >> 7) + 16 (compv_image_conv_rgbfamily.cxx:108).
 * in: H rows of S samples (S * bytes-per-sample bytes per row, S >= W as in CompVMat); out: H rows of W bytes at stride So. */
COMPVHIP_API int compvhip_grayscale_u8(compvhip_ctx* ctx, const uint8_t* in, int pixfmt, size_t W, size_t H, size_t S,
                                       uint8_t* out, size_t So);

/* CompVImage::thresholdOtsu (base/image/compv_image_threshold.cxx:52-114, called at samples/hough_lines/main.cxx:103):
 * 256-bin histogram of the W x H plane + the reference's f32 scan; *threshold = the integer level as a double. */
COMPVHIP_API int compvhip_otsu_u8(compvhip_ctx* ctx, const uint8_t* in, size_t W, size_t H, size_t S, double* threshold);

/* CompVMathGauss::kernelDim1FixedPoint (base/math/compv_math_gauss.cxx:11-17: kernelDim1<float> of compv_math_gauss.h:24-55, then
 * CompVMathConvlt::fixedPointKernel, compv_math_convlt.h:77-92): `size` (odd) Q16 weights of a normalised 1-D Gaussian.  Host
 * arithmetic only (libm exp/sqrt in the reference's float/double mix); no GPU involved. */
COMPVHIP_API int compvhip_gauss_kernel_fixedpoint(size_t size, float sigma, uint16_t* kernel);

/* CompVMathConvlt::convlt1FixedPoint (base/include/compv/base/math/compv_math_convlt.h:31-33,98-173,386-405): separable Q16
 * convolution u8 -> u8, horizontal pass with hzKern then vertical pass with vtKern through a u8 temporary, each
 * out = min(255, sum_k ((in[k] * kern[k]) >> 16)), zero OUTPUT border of kernSize/2.  kernSize odd, 3..15 (larger:
 * COMPVHIP_E_NOT_IMPLEMENTED), W,H >= kernSize.  The optional Gaussian pre-blur in front of Canny.  in and out may alias. */
COMPVHIP_API int compvhip_convlt1_fixedpoint_u8(compvhip_ctx* ctx, const uint8_t* in, size_t W, size_t H, size_t S,
                                                const uint16_t* vtKern, const uint16_t* hzKern, size_t kernSize, uint8_t* out, size_t So);

/* CompVMathConvlt::convlt1<uint8_t, int16_t, int16_t> and <int16_t, int16_t, int16_t> (base/include/compv/base/math/compv_math_convlt.h:26-28,
 * 37-39; driver :98-173, passes :176-292): separable integer CORRELATION (no kernel flip), horizontal pass with hzKern then vertical pass
 * with vtKern through an int16 temporary, int32 sums saturated to int16 after each pass, zero OUTPUT border of kernSize/2 columns and
 * rows.  The operator the Sobel / Scharr / Prewitt gradients are made of (gx: vt = smoothing, hz = derivative; canny_dete.cxx:237-241);
 * on the hot path it is fused into the tile kernels, this is its stand-alone form (reference known-answer vectors:
 * unittests/math_convlt.cxx:24-25).  kernSize odd, 1..15 (larger: COMPVHIP_E_NOT_IMPLEMENTED), W,H >= kernSize; S, So in ELEMENTS. */
COMPVHIP_API int compvhip_convlt1_8u16s16s(compvhip_ctx* ctx, const uint8_t* in, size_t W, size_t H, size_t S,
                                           const int16_t* vtKern, const int16_t* hzKern, size_t kernSize, int16_t* out, size_t So);
COMPVHIP_API int compvhip_convlt1_16s16s16s(compvhip_ctx* ctx, const int16_t* in, size_t W, size_t H, size_t S,
                                            const int16_t* vtKern, const int16_t* hzKern, size_t kernSize, int16_t* out, size_t So);

/* CompVHoughSht::process (core/features/hough/compv_core_feature_houghsht.cxx:96-262).  rho must be 1 (:306-316),
 * thetaDeg in degrees, threshold > 0 is the NMS/line threshold, maxLines <= 0 keeps every line.
 * lines: caller-allocated, capacity cap; *n receives the number of lines found (after the maxLines cut); if *n > cap
 * only cap lines are written and COMPVHIP_E_OUT_OF_BOUND is returned.  Lines come back in the REFERENCE's order: sorted by strength
 * descending, and inside equal-strength groups -- also at the maxLines cut -- exactly as the reference's unstable std::sort (:241-249)
 * leaves them when it is built with this C++ runtime (the whole list is brought to the host in the (row, col) emission order of
 * nms_apply and put through the same std::sort; callers such as CompVCalibCamera's line grouping depend on that order).  The
 * device-resident plan API keeps the canonical order instead (strength, then (row, col) ascending), see compvhip_plan_houghsht.
 * acc (optional): int32 accumulator in the reference layout, R rows of accStride elements, R = 2(W+H)+1. */
COMPVHIP_API int compvhip_houghsht_u8(compvhip_ctx* ctx, const uint8_t* edges, size_t W, size_t H, size_t S,
                                      float rho, float thetaDeg, int threshold, int maxLines,
                                      compvhip_line* lines, size_t cap, size_t* n,
                                      int32_t* acc, size_t accStride);

/* CompVHoughKht::process (core/features/hough/compv_core_feature_houghkht.cxx:208-447): kernel-based Hough transform.
 * rho in (0,1], thetaDeg in degrees, threshold on the 3x3-smoothed vote count, maxLines <= 0 keeps every line;
 * clusterMinDeviation / clusterMinSize (> 0) / kernelMinHeight (>= 0) are the COMPV_HOUGHKHT_SET_* knobs (defaults 2.0, 10, 0.002,
 * houghkht.cxx:38-40; ranges as CompVHoughKht::set checks them, :169-186).  Lines come back in the reference's order (descending smoothed count, the reference's own
 * std::sort tie order); rho is measured from the image centre (toCartesian, :1249-1280); row/col of compvhip_line hold
 * the rho/theta indices.  *gs receives COMPV_HOUGHKHT_GET_FLT64_GS when kernels survive (left untouched otherwise, like
 * the reference's m_dGS).  Hybrid: edge linking (Appendix A follows chains pixel by pixel in raster order and erases what it visits)
 * and the final sweep are order dependent and run on the host inside this library; cluster subdivision (one thread per string), the
 * per-cluster statistics (Algorithm 2), Gaussian voting (Algorithm 4) and vote-map smoothing run on the GPU. */
COMPVHIP_API int compvhip_houghkht_u8(compvhip_ctx* ctx, const uint8_t* edges, size_t W, size_t H, size_t S,
                                      float rho, float thetaDeg, int threshold, int maxLines,
                                      double clusterMinDeviation, size_t clusterMinSize, double kernelMinHeight,
                                      compvhip_line* lines, size_t cap, size_t* n, double* gs);

/* Stage inspection (tests, profiling): the elliptical kernels of voting_Algorithm2_Kernels (houghkht.cxx:885-1026) BEFORE the height
 * pruning, in cluster order, 7 doubles each in the field order of CompVHoughKhtKernel (houghkht.h:52-62): rho, theta (degrees), h,
 * sigma_theta_square, sigma_rho_square, m2, sigma_rho_times_theta; *hmax = the largest height.  COMPVHIP_E_OUT_OF_BOUND (with *n = the
 * number of kernels) when cap is too small.  compvhip_houghkht_stage_ms: wall-clock milliseconds of the six stages of this context's
 * last compvhip_houghkht_u8 call -- linking, subdivision (upload + GPU), statistics (GPU + download), pruning + Gmin, voting + peaks (GPU),
 * sort + sweep. */
COMPVHIP_API int compvhip_houghkht_kernels_u8(compvhip_ctx* ctx, const uint8_t* edges, size_t W, size_t H, size_t S,
                                              double clusterMinDeviation, size_t clusterMinSize,
                                              double* kernels7, size_t cap, size_t* n, double* hmax);
COMPVHIP_API int compvhip_houghkht_stage_ms(compvhip_ctx* ctx, double* ms6);
/* The host stage of KHT on its own -- linking_AppendixA (houghkht.cxx:544-760) on the bit-plane linker, no device involved (ctx is not needed):
 * xy receives the (x, y) pairs of the points of all strings, string after string (2 * *nPoints int32; cap = capacity in POINTS), stringEnds[i] the
 * index one past the last point of string i (string i = points [stringEnds[i-1], stringEnds[i])).  COMPVHIP_E_OUT_OF_BOUND when a capacity is too
 * small (*nPoints / *nStrings hold what is needed).  What CPU-only hosts test the linker with. */
COMPVHIP_API int compvhip_houghkht_link_u8(const uint8_t* edges, size_t W, size_t H, size_t S, size_t clusterMinSize, int32_t* xy, size_t cap, size_t* nPoints,
                                           uint32_t* stringEnds, size_t stringCap, size_t* nStrings);

/* CompVHoughSht::toCartesian (core/features/hough/compv_core_feature_houghsht.cxx:264-304,566-589) and
 * CompVHoughKht::toCartesian (core/features/hough/compv_core_feature_houghkht.cxx:449-489,1249-1280) for caller-held polar lines:
 * out[4 i ..] = {a.x, a.y, b.x, b.y} of line i (a.z = b.z = 1 in CompVLineFloat32).  SHT: rho from the image origin, endpoints at
 * x = 0 and x = W; KHT: rho from the image centre.  theta == 0 is the perfect vertical line (x = rho, y = +-sqrt(W^2 + H^2)).
 * Host float32 arithmetic in the reference's operation order (libm cosf / sinf called separately); no GPU involved.  Only the
 * rho / theta fields of `lines` are read. */
COMPVHIP_API int compvhip_houghsht_to_cartesian(size_t W, size_t H, const compvhip_line* lines, size_t n, float* out);
COMPVHIP_API int compvhip_houghkht_to_cartesian(size_t W, size_t H, const compvhip_line* lines, size_t n, float* out);

/* Geometry helper: R (rho rows), T (theta bins) and the float32 theta step for a W x H image
 * (initCoords, houghsht.cxx:318-348). */
COMPVHIP_API int compvhip_houghsht_dims(size_t W, size_t H, float thetaDeg, size_t* R, size_t* T, float* thetaStepRad);
/* Geometry helper of the KHT: rho bins and theta bins of its vote map for a W x H image (initCoords,
 * core/features/hough/compv_core_feature_houghkht.cxx:501-541); the map holds (T + 2) x (rhoN + 2) int32 cells. */
COMPVHIP_API int compvhip_houghkht_dims(size_t W, size_t H, float rho, float thetaDeg, size_t* rhoN, size_t* T);
/* Geometry helper: the grid of image tiles (nx x ny) and the rho-window rows per tile a plan of `frames` W x H frames votes with
 * (acc_gather, houghsht.cxx:350-481, runs as one workgroup per frame, tile and 64 theta bins).  Host arithmetic only: what
 * compvhip_plan_create would choose, for tests and capacity planning.  COMPVHIP_E_NOT_IMPLEMENTED when no grid fits. */
COMPVHIP_API int compvhip_houghsht_vote_grid(size_t W, size_t H, float thetaDeg, size_t frames, int* nx, int* ny, int* windowRows);
/* The CPUs this process may really use at once: min(hardware threads, affinity mask, cgroup CPU quota) -- what compvhip_plan_houghkht sizes its default
 * worker pool by (hostThreads = 0), and what the reference's CompVBase::init(-1) (base/compv_base.cxx:62: one thread per logical CPU) does not look at: a
 * container may show 256 logical CPUs and own 16.  Host arithmetic only; always >= 1. */
COMPVHIP_API int compvhip_host_cpu_budget(void);

/* ---- device-resident batched pipeline (frames already in HBM) ---------------------------------------------- */

/* A plan owns every scratch buffer for `frames` frames of W x H (stride S, S % 8 == 0, frame stride S*H) and the
 * Q16 sin/cos tables for thetaDeg.  Frames are independent units: one plan per GPU, shard frames across GPUs. */
COMPVHIP_API int compvhip_plan_create(compvhip_ctx* ctx, size_t W, size_t H, size_t S, size_t frames, float thetaDeg,
                                      compvhip_plan** plan);
/* Batches beyond 65 535 frames.  A plan may hold any number of frames, but most kernels carry the frame index in a grid dimension that holds at most
 * 65 535 (blockIdx.y / .z).  Every plan-form call therefore belongs to one of three classes, named beside it below, and the host decides which before
 * the call allocates or enqueues anything (never by what the runtime makes of an oversized grid):
 *   SLICED          the call launches its kernels in slices of at most 65 535 frames; any frame count gives what the same frames give in smaller batches.
 *   FRAMES IN X     the frame index rides in the x extent (up to 2^31 - 1 workgroups): no limit of its own.
 *   REFUSED         beyond 65 535 frames the call returns COMPVHIP_E_INVALID_PARAMETER, compvhip_last_error names the limit, nothing is allocated, enqueued
 *                   or written.  Split the batch across plans of at most 65 535 frames.
 * The text-detection chain (grayscale, otsu, threshold, threshold_adaptive, morph, components on the caller's bytes), the segment and fit calls on the
 * caller's bytes, remap / warp_inverse, hog, the image statistics (integral, histogram, equalize, projections) and the colour conversion (compvhip_convert_frames) are SLICED; edge_dete has its FRAMES IN X; Canny and everything that needs its masks, the SHT, the batched KHT, the
 * fixed-point blur, FAST, ORB and the bilinear scale are REFUSED, as are a compvhip_orbpyr of more than 65 535 frames and a compvhip_matcher or a
 * compvhip_homography of more than 65 535 pairs at their creation. */
/* Alignment of device pointers.  Every d_* pointer of the plan, pyramid, matcher and homography calls belongs to one of two classes, stated beside its call
 * (tests/alignment_cases.py is the same list, and tests/test_alignment_cases.py fails when a pointer has no entry):
 *   ANY BYTE        uint8 frames, edge maps and planes only: the pointer may start at any byte (a sub-buffer, a region of interest, frames behind a header).
 *                   The call gives the bits it gives at an aligned pointer and writes nothing it does not write there.  Frame f starts S * H bytes after
 *                   frame f - 1, whatever that does to its alignment.
 *   N-BYTE ALIGNED  N = 4, 8 or 16: anything else is refused with COMPVHIP_E_INVALID_PARAMETER before the call allocates, enqueues or writes anything,
 *                   and compvhip_last_error says so.  Every typed array is in this class at the alignment of its element: int32 / uint32 / float32 arrays
 *                   and the records made of them (compvhip_line, _segment, _component, _corner, _keypoint) 4 bytes, float64 arrays, compvhip_line_fit and
 *                   compvhip_homography_result 8 bytes, compvhip_match records and {x, y} float64 points 16 bytes.
 * A null pointer where a call allows one counts as aligned.  A d_* parameter with two stars (compvhip_plan_acc, _edge_counts, compvhip_orbpyr_plane) is a HOST
 * pointer that receives a device address.  The host entry points copy into buffers of their own and take any host pointer. */
/* Stream order.  Every export that takes a `void* stream` (a hipStream_t; NULL = the default stream) belongs to one of two classes, and the two batched KHT
 * calls, which take none, to a third.  The class stands beside each call as "Stream order: CLASS" (tests/stream_cases.py is the same list,
 * tests/test_stream_cases.py fails when a call has no entry, tests/test_gpu_stream_order.py runs every call behind pending work on a non-blocking stream):
 *   ASYNC           Everything the call does on the device -- kernels, clears, copies, the upload of what it derives from host arrays -- is ordered on `stream`:
 *                   after what was enqueued there before the call, before what is enqueued there after it; nothing runs on another stream.  On a warm handle
 *                   (the same call was made before and no scratch has to grow) it returns without waiting for the stream.  Host arrays and option structs
 *                   passed to it (vtKern / hzKern, strel, M, roi, opts, compvhip_image) may be changed as soon as it has returned.
 *   WAITS           The same ordering and the same rule for host arrays, but the call may wait for the stream before it returns.
 *   DRAINS          compvhip_plan_houghkht and compvhip_plan_houghkht_ex take no stream: they drain the whole device first (hipDeviceSynchronize), so edge maps
 *                   still being produced on ANY stream are complete when the workers read them, and they return with their results in host memory.
 * Growing scratch: a later call with a larger capacity (lineCap beyond the plan's key slots, keyCap, a HOG layout with more cells on the plan's own map, a
 * larger warp destination, ...) may have to reallocate plan-owned scratch.  Such a call may wait for the device, whatever its class, and it never disturbs a
 * call that is still pending: the old buffer is released with hipFree, which returns only when the work that reads it has finished.
 * Timing mode (compvhip_plan_set_timing and its siblings) records HIP events around the kernels and changes no class: compvhip_*_get_timing is what waits.
 * The host entry points (*_u8, *_f64) are synchronous on the context's own stream. */
/* A plan must be destroyed BEFORE its context (it keeps a pointer to it); compvhip_ctx_destroy only releases the private
 * single-frame plan of the host entry points. */
COMPVHIP_API void compvhip_plan_destroy(compvhip_plan* plan);

/* Canny on `frames` device frames: d_in -> d_edges (both frames*S*H bytes, may alias).  Asynchronous on `stream`
 * (a hipStream_t; NULL = default stream) except for the hysteresis convergence check, which polls a device flag.
 * Beyond 65 535 frames: REFUSED (the resolve rounds index their change flags by the launch's frame extent).  d_in and d_edges: ANY BYTE.  Stream order: WAITS: the hysteresis convergence poll synchronises the stream at least once per call. */
COMPVHIP_API int compvhip_plan_canny(compvhip_plan* plan, const uint8_t* d_in, float tLow, float tHigh, int ksize,
                                     int thresholdType, uint8_t* d_edges, void* stream);

/* compvhip_grayscale_u8 on `frames` device frames: d_in = [frames][H][S samples], d_gray = [frames][H][S].  Asynchronous.
 * Beyond 65 535 frames: SLICED.  d_in and d_gray: ANY BYTE (the packed samples as well).  Stream order: ASYNC. */
COMPVHIP_API int compvhip_plan_grayscale(compvhip_plan* plan, const uint8_t* d_in, int pixfmt, uint8_t* d_gray, void* stream);

/* compvhip_otsu_u8 on `frames` device frames: d_thresholds[f] = Otsu level of frame f (device array).  Asynchronous.
 * Beyond 65 535 frames: SLICED (histograms and levels slice by slice).  d_gray: ANY BYTE; d_thresholds: 4-byte aligned.  Stream order: ASYNC. */
COMPVHIP_API int compvhip_plan_otsu(compvhip_plan* plan, const uint8_t* d_gray, int32_t* d_thresholds, void* stream);

/* compvhip_convlt1_fixedpoint_u8 on `frames` device frames (vtKern/hzKern are HOST arrays of kernSize weights); d_in and
 * d_out may alias.  Asynchronous.  Beyond 65 535 frames: REFUSED.  d_in and d_out: ANY BYTE.  Stream order: ASYNC. */
COMPVHIP_API int compvhip_plan_convlt1_fixedpoint(compvhip_plan* plan, const uint8_t* d_in, const uint16_t* vtKern, const uint16_t* hzKern,
                                                  size_t kernSize, uint8_t* d_out, void* stream);

/* CompVHoughSht::toCartesian (core/features/hough/compv_core_feature_houghsht.cxx:264-304,566-589) on the device line arrays a
 * compvhip_plan_houghsht / _pipeline call produced: d_cart[f][i] = {a.x, a.y, b.x, b.y} of line i of frame f (a.z = b.z = 1), for
 * i < min(d_counts[f], lineCap).  Asynchronous.  Beyond 65 535 frames: REFUSED (like the calls that produce such line arrays).  d_lines, d_counts and
 * d_cart: 4-byte aligned.  Stream order: ASYNC. */
COMPVHIP_API int compvhip_plan_to_cartesian(compvhip_plan* plan, const compvhip_line* d_lines, const int32_t* d_counts, size_t lineCap,
                                            float* d_cart, void* stream);

/* Sobel / Scharr / Prewitt detector (compvhip_edge_dete_u8 semantics) on `frames` device frames; d_in and d_out must
 * not alias.  Fully asynchronous on `stream`.  Beyond 65 535 frames: FRAMES IN X.  d_in and d_out: ANY BYTE.  Stream order: ASYNC. */
COMPVHIP_API int compvhip_plan_edge_dete(compvhip_plan* plan, const uint8_t* d_in, int op, uint8_t* d_out, void* stream);

/* SHT on the edge maps produced by the last compvhip_plan_canny() of this plan (uses its 1-bit edge masks, no byte
 * re-read) or, when d_edges != NULL, on arbitrary device edge maps.  Results stay on the device:
 * d_lines: frames * lineCap compvhip_line (strength descending, ties by accumulator (row, col) ascending -- the canonical order, not the
 * reference's unstable-sort tie order the host entry point reproduces), d_counts: frames int32 (lines found,
 * before clipping to lineCap).  The call is asynchronous and cannot grow its buffers after the fact: the device key buffer holds
 * min(R*T, max(lineCap, 65536)) candidates per frame, so whatever lineCap is, the lineCap STRONGEST lines are returned as long as
 * d_counts[f] <= max(lineCap, 65536); beyond that the key buffer overflowed and frame f's lines are an arbitrary subset -- call
 * again with lineCap >= d_counts[f] (the host entry point compvhip_houghsht_u8 does that by itself).
 * Beyond 65 535 frames: REFUSED (the whole SHT stage; its key buffers alone would run to gigabytes).  d_edges: ANY BYTE; d_lines and d_counts: 4-byte
 * aligned.  Stream order: ASYNC. */
COMPVHIP_API int compvhip_plan_houghsht(compvhip_plan* plan, const uint8_t* d_edges, int threshold, int maxLines,
                                        compvhip_line* d_lines, size_t lineCap, int32_t* d_counts, void* stream);

/* Sobel -> Canny -> HoughSHT in one call (the benchmark's "step").  Beyond 65 535 frames: REFUSED, like compvhip_plan_pipeline_async and
 * compvhip_plan_pipeline_ex (Canny and the SHT are).  In all three, d_in and d_edges: ANY BYTE; d_lines and d_counts: 4-byte aligned.  Stream order: WAITS (the convergence poll of its Canny). */
COMPVHIP_API int compvhip_plan_pipeline(compvhip_plan* plan, const uint8_t* d_in, float tLow, float tHigh,
                                        int threshold, int maxLines, uint8_t* d_edges,
                                        compvhip_line* d_lines, size_t lineCap, int32_t* d_counts, void* stream);

/* compvhip_plan_pipeline without its host round trip.  The synchronous call reads the hysteresis convergence flag before it
 * returns (one stream synchronisation per step); this one enqueues the step, lets the flag travel to pinned host memory behind
 * the kernels and returns a ticket.  compvhip_plan_wait(plan, ticket) blocks until that step has finished and, in the rare case
 * its hysteresis needed more resolve rounds than were enqueued speculatively, drains the stream and runs the step again
 * synchronously -- so d_in must stay unmodified, and distinct from d_edges, until the step was waited for.  Up to 4 steps may be
 * in flight (further calls return COMPVHIP_E_INVALID_STATE); steps of one plan must use one stream.  Typical use:
 * t1 = async(batch k+1); wait(t0) -- the GPU never idles between steps.
 * Output buffers and the replay: a replayed step writes its d_edges / d_lines / d_counts again, AFTER later steps of the plan have run.  Steps in
 * flight may share output buffers (a caller that only consumes the newest result): every step enqueued after a replayed one is then replayed too
 * when it is waited for, in enqueue order, so after compvhip_plan_wait(t) the buffers of step t always hold step t's results.  Wait for the tickets
 * of a plan in the order they were issued.  Results of step t are only guaranteed to still be there until the next step that shares its buffers
 * starts -- give steps their own buffers to read them later.
 * Speculative rounds: a step enqueues as many hysteresis rounds as the plan's last 8 asynchronous steps needed (the first round that changed nothing,
 * inclusive): 3 for a new plan, 2 once four steps have needed no more (the benchmark's frames: round 0 does the work, round 1 confirms), never more than 3; a
 * step that needs more is the replay described above, and the plan enqueues 3 again for the steps after it.
 * A second replay cause exists only on the library-sort fallback (max(W, H) > 4095, or more than 16 chunks of 8192 lines per frame): there the step
 * sorts a PREDICTED range of the line keys -- the largest line total of the plan's last 8 steps + 1/16 + 4096 -- and compvhip_plan_wait replays the
 * step when its real total exceeded the prediction.  Content whose line count jumps from step to step therefore replays often on such plans, and each
 * replay drains the stream and cascades to the later tickets that share output buffers; plans on the device-sized sort (every size up to 4095 x 4095
 * with at most 131 072 lines per frame, i.e. all BASELINE configurations) never replay for this reason.  Stream order: ASYNC: compvhip_plan_wait is where the host waits. */
COMPVHIP_API int compvhip_plan_pipeline_async(compvhip_plan* plan, const uint8_t* d_in, float tLow, float tHigh,
                                              int threshold, int maxLines, uint8_t* d_edges,
                                              compvhip_line* d_lines, size_t lineCap, int32_t* d_counts, void* stream, int* ticket);
COMPVHIP_API int compvhip_plan_wait(compvhip_plan* plan, int ticket);

/* The general step: what samples/hough_lines/main.cxx:102-109 does per camera frame -- convertGrayscale -> thresholdOtsu ->
 * Canny(Otsu * tLow, Otsu * tHigh) -> HoughSHT -> toCartesian -- as ONE enqueue over the plan's frames.  Zero-initialise the struct and set what
 * is needed; compvhip_plan_pipeline(_async) is this call with ksize 3, COMPARE_TO_GRADIENT, FMT_Y and no optional outputs. */
typedef struct compvhip_pipeline_opts {
	float tLow, tHigh;      /* Canny thresholds (threshold factors in the PERCENT_OF_MEAN / OTSU modes) */
	int threshold, maxLines;/* SHT threshold (> 0) / line cut (<= 0: every line) */
	int ksize;              /* Sobel kernel size of the gradient: 3 or 5 (0 = 3) */
	int thresholdType;      /* COMPVHIP_CANNY_THRESHOLD_* */
	int pixfmt;             /* compvhip_pixfmt of d_in; COMPVHIP_FMT_Y (luma plane, stride S) or a packed format ([frames][H][S samples]): converted first */
	uint8_t* d_gray;        /* packed input: receives the luma planes [frames][H][S] (NULL: plan-owned scratch); ANY BYTE */
	int32_t* d_otsu;        /* OTSU mode: receives the per-frame Otsu levels (NULL: not wanted); 4-byte aligned */
	float* d_cart;          /* receives toCartesian's endpoints [frames][lineCap][4] (NULL: not wanted); 4-byte aligned */
} compvhip_pipeline_opts;
/* ticket == NULL: synchronous like compvhip_plan_pipeline; otherwise asynchronous like compvhip_plan_pipeline_async (same rules: wait with
 * compvhip_plan_wait, d_in unmodified and distinct from d_edges until then).  Stream order: WAITS without a ticket; with a ticket it is ASYNC like compvhip_plan_pipeline_async.  opts may be changed as soon as the call has returned. */
COMPVHIP_API int compvhip_plan_pipeline_ex(compvhip_plan* plan, const uint8_t* d_in, const compvhip_pipeline_opts* opts, uint8_t* d_edges,
                                           compvhip_line* d_lines, size_t lineCap, int32_t* d_counts, void* stream, int* ticket);

/* CompVHoughKht::process (compvhip_houghkht_u8 semantics, same knobs) on the plan's `frames` DEVICE edge maps d_edges = [frames][H][S]
 * ({0, non-zero} bytes, e.g. the edge maps a compvhip_plan_canny / _pipeline call produced); results in HOST memory: lines[f * cap ..] /
 * counts[f] / gs[f] (gs optional; gs[f] is left untouched for a frame without surviving kernels, like the reference's m_dGS).  Synchronous,
 * and it drains the device first (hipDeviceSynchronize): whatever stream produced d_edges has finished before a worker reads them.
 * The edge-linking stage is a sequential chain walk per frame and runs on the host (on a bit plane: the edge maps leave the device as bit masks);
 * frames are independent, so they go through the stages in groups of 8: inside a group the host stages (linking, prune / Gmin, sort + sweep) are
 * parallel loops over its frames and every GPU stage is ONE launch over the strings / clusters / kernels / vote maps of all its frames; up to eight
 * groups are in flight, each with its own stream and a controller thread that only enqueues, SLEEPS on its GPU stages (blocking-sync events) and
 * posts its group's host stages to the hostThreads workers all groups share (it works along on the short prune items only) -- so while one group is on the
 * GPU the workers link / sweep the frames of the others.  hostThreads = 0: min(32, hardware threads / 2, the CPUs this process may really use: affinity mask and cgroup CPU quota).  COMPVHIP_E_OUT_OF_BOUND when a frame has more
 * than cap lines (counts[f] tells); on any other failure the error text names the frame.  clusterMinSize must be >= 2 (for 1 the reference's
 * cluster subdivision does not terminate: a defined deviation, also of compvhip_houghkht_u8 / compvhip_houghkht_kernels_u8).
 * compvhip_plan_houghkht_stage_ms: the six stage clocks of the last call summed over its frames (compvhip_houghkht_stage_ms order), the wall
 * time of the call and the number of workers.
 * Beyond 65 535 frames: REFUSED (compvhip_plan_houghkht_ex as well).  d_edges: ANY BYTE (in both calls; every other array is the host's).  Stream order: DRAINS. */
COMPVHIP_API int compvhip_plan_houghkht(compvhip_plan* plan, const uint8_t* d_edges, float rho, float thetaDeg, int threshold, int maxLines,
                                        double clusterMinDeviation, size_t clusterMinSize, double kernelMinHeight,
                                        compvhip_line* lines, size_t cap, size_t* counts, double* gs, int hostThreads);
COMPVHIP_API int compvhip_plan_houghkht_stage_ms(compvhip_plan* plan, double* ms6, double* wallMs, int* threads);

/* KHT line order.  REFERENCE (0): what compvhip_houghkht_u8 / compvhip_plan_houghkht return -- descending smoothed count, ties as the reference's unstable
 * std::sort leaves them; the visited-map sweep runs on the host.  CANONICAL (1): the order a STABLE sort of the reference's emission list gives, with the
 * peak stage on the GPU:
 *  - Records: exactly the vote cells the reference's peak scan emits (same coverage, threshold and quirk Q6).  Record r has a position p = (thetaIndex,
 *    rhoIndex), a smoothed count s and an emission key e = thetaIndex * 2 (rhoN + 2) + rhoIndex; a record of the scalar remainder (Q6, rhoN % 4 == 3:
 *    position (theta, 1), counts of column rhoN - 1) has e = thetaIndex * 2 (rhoN + 2) + (rhoN + 2) + rhoIndex.  e is unique and below 2^32.
 *  - Order: s descending, then e ascending (the KHT twin of the plan SHT's canonical order).
 *  - Lines: r is a line iff no record r' at a position q != p of p's 8-neighbourhood has s' > s, or s' == s and e' < e.  (The reference marks every swept
 *    cell as visited and never tests a cell's own position: a Q6 record and a main-scan record at the same position do not block each other.)
 *  - Output: the lines in that order, cut at maxLines when maxLines > 0; fields as in the reference order (rho = (float)rho[rhoIndex], theta =
 *    (float)((theta[thetaIndex] * pi) / 180), strength = s, row = rhoIndex, col = thetaIndex); GS unchanged.
 * Lines whose position has no equal-count record among its 8 neighbours are the same in both orders; only the tie groups differ. */
#define COMPVHIP_KHT_ORDER_REFERENCE 0
#define COMPVHIP_KHT_ORDER_CANONICAL 1
/* The knobs of a KHT call.  Zero-initialise and set what is needed: a zero field takes the default -- rho 1, thetaDeg 1, threshold 1, maxLines 0 (every
 * line), clusterMinDeviation 2.0, clusterMinSize 10, kernelMinHeight 0.002 (so a height of exactly 0 is asked for with a tiny positive value), hostThreads 0
 * (compvhip_plan_houghkht's default pool; ignored by compvhip_houghkht_ex_u8), order COMPVHIP_KHT_ORDER_REFERENCE. */
typedef struct compvhip_kht_opts {
	float rho, thetaDeg;
	int threshold, maxLines;
	double clusterMinDeviation;
	size_t clusterMinSize;
	double kernelMinHeight;
	int hostThreads;
	int order;              /* COMPVHIP_KHT_ORDER_* */
} compvhip_kht_opts;
/* compvhip_plan_houghkht / compvhip_houghkht_u8 with the knobs in opts (same buffers, capacity and error contract: COMPVHIP_E_OUT_OF_BOUND when a frame has
 * more than cap lines, counts[f] / *n tell how many).  opts == NULL or an unknown order: COMPVHIP_E_INVALID_PARAMETER.  In CANONICAL order the vote map
 * never leaves the device: the peaks of every frame are found and sorted on the GPU and only the lines and their counts are downloaded; the sixth stage
 * clock (sort + sweep on the host) reads 0 and the GPU peak and sort time is part of the fifth (vote + peaks).  Stream order: DRAINS. */
COMPVHIP_API int compvhip_plan_houghkht_ex(compvhip_plan* plan, const uint8_t* d_edges, const compvhip_kht_opts* opts,
                                           compvhip_line* lines, size_t cap, size_t* counts, double* gs);
COMPVHIP_API int compvhip_houghkht_ex_u8(compvhip_ctx* ctx, const uint8_t* edges, size_t W, size_t H, size_t S, const compvhip_kht_opts* opts,
                                         compvhip_line* lines, size_t cap, size_t* n, double* gs);

/* Device accumulator of frame f after compvhip_plan_houghsht: uint16 (a cell never exceeds the pixels of a 1-px band),
 * theta-major [T][accPitch] (pitch >= R).  compvhip_plan_acc_export gives the reference's int32 rho-major layout.  d_acc: a HOST pointer that receives the
 * device address. */
COMPVHIP_API int compvhip_plan_acc(compvhip_plan* plan, size_t frame, const uint16_t** d_acc, size_t* R, size_t* T, size_t* accPitch);
/* Copies the accumulator of frame f into a caller DEVICE buffer in the reference layout: int32 [R][outStride]
 * (outStride >= T), i.e. acc[(barrier - rho) * outStride + t] (houghsht.cxx:430-431).  Beyond 65 535 frames: REFUSED (one frame per call, but no
 * call that fills the accumulators accepts such a plan).  d_out: 4-byte aligned.  Stream order: ASYNC. */
COMPVHIP_API int compvhip_plan_acc_export(compvhip_plan* plan, size_t frame, int32_t* d_out, size_t outStride, void* stream);
/* Number of edge pixels per frame voted by the last houghsht / pipeline step of this plan (device int32[frames]).  The SHT's voting
 * kernel counts them: a compvhip_plan_canny call alone resets them to zero, and before the plan's first SHT the call is refused.  d_edge_counts: a HOST
 * pointer that receives the device address. */
COMPVHIP_API int compvhip_plan_edge_counts(compvhip_plan* plan, const int32_t** d_edge_counts);

/* ---- Hough line SEGMENTS: where along an SHT line its edge pixels are ----------------------------------------
 * The reference stops at infinite lines (toCartesian: two points at x = 0 and x = W).  The pixels of an SHT line are exactly the edge pixels
 * that voted for its accumulator cell, which gives an integer-only definition (docs/kernels/sht_segments.md):
 *  1. Support: pixel (x, y) belongs to line (row, col) iff (x * cosQ[col] + y * sinQ[col]) >> 16 == (W + H) - row -- the vote's own expression
 *     on the plan's Q16 tables, exact for every geometry.  Only row / col of a compvhip_line are read.
 *  2. Major axis: sinQ[col] >= |cosQ[col]|: x-major (position p = x, N = W, minor coordinate y); otherwise y-major (p = y, N = H, minor x).
 *     A position holds at most 2 support pixels.
 *  3. Occupancy: cnt[p] = support pixels at p that are inside the image and edges (non-zero); the sum over p is the line's strength.
 *  4. Segments: maximal groups of positions with cnt > 0 in which consecutive ones differ by at most maxGap + 1; a group [p0, p1] is a
 *     segment iff p1 - p0 + 1 >= minLength.
 *  5. Record: the line's index in the frame's line array, the pixels at p0 and p1 (of two edges at a position: the smaller minor
 *     coordinate), support = sum of cnt over p0..p1.
 *  6. Order: by line index, then p0, ascending.  Lines considered per frame: min(d_counts[f], lineCap, maxLines if > 0). */
typedef struct compvhip_segment {
	int32_t line;
	int32_t x0, y0, x1, y1;
	int32_t support;
} compvhip_segment;

/* Segments of the lines a compvhip_plan_houghsht / _pipeline call left on the device, for all frames of the plan.  d_edges: the byte edge maps
 * [frames][H][S] the lines were found on, or NULL = the 1-bit masks of the plan's last Canny / pipeline step (no byte re-read;
 * COMPVHIP_E_INVALID_PARAMETER when the plan holds none: before its first Canny, or after a compvhip_plan_houghsht on foreign edge maps replaced
 * them).  d_segs: frames * segCap records; d_segCounts[f]: segments found in frame f BEFORE clipping -- the first min(count, segCap) in the order
 * above are written, so a clipped result is a prefix of the full one.  Asynchronous on `stream` (the plan's SHT tables and a scratch array of
 * frames * min(lineCap, maxLines) counters are allocated on first use).  COMPVHIP_E_INVALID_STATE while the plan has asynchronous steps that
 * were not waited for (a replayed step rewrites d_lines later); COMPVHIP_E_INVALID_PARAMETER for minLength < 1, maxGap < 0, lineCap == 0 or
 * segCap == 0.  Beyond 65 535 frames: SLICED with the caller's d_edges; the plan's own masks exist only behind a Canny run, which is REFUSED there.
 * d_edges: ANY BYTE; d_lines, d_counts, d_segs and d_segCounts: 4-byte aligned.  Stream order: ASYNC. */
COMPVHIP_API int compvhip_plan_houghsht_segments(compvhip_plan* plan, const uint8_t* d_edges, const compvhip_line* d_lines, const int32_t* d_counts,
                                                 size_t lineCap, int maxLines, int minLength, int maxGap,
                                                 compvhip_segment* d_segs, size_t segCap, int32_t* d_segCounts, void* stream);

/* The same for caller-held lines of one HOST edge map (lines of compvhip_houghsht_u8 in either order, or of a plan: only row / col are read;
 * segs[i].line indexes `lines`).  Synchronous.  *nSegs receives the number of segments found; when it exceeds cap only the first cap are written
 * and COMPVHIP_E_OUT_OF_BOUND is returned (cap == 0 with segs == NULL asks for the number).  A line whose (row, col) is outside the R x T
 * accumulator of (W, H, thetaDeg): COMPVHIP_E_INVALID_PARAMETER. */
COMPVHIP_API int compvhip_houghsht_segments_u8(compvhip_ctx* ctx, const uint8_t* edges, size_t W, size_t H, size_t S, float thetaDeg,
                                               const compvhip_line* lines, size_t n, int minLength, int maxGap,
                                               compvhip_segment* segs, size_t cap, size_t* nSegs);

/* ---- Hough line REFINEMENT: where the line really is -------------------------------------------------------------
 * An SHT line is an accumulator cell: rho is an integer and theta a multiple of the theta step.  The fit below is the total-least-squares
 * line through the edge pixels of a band of rho cells around the cell (docs/kernels/sht_fit.md).  Its integer part has no tolerance; its
 * binary64 part uses + - * / sqrt only, each rounded once, in the order given, so it is reproducible bit for bit as well.
 *  Inputs: the edge map (non-zero byte, or set bit of the plan's masks; columns >= W are never edges), the plan's Q16 tables, the line's cell
 *     (row, col) -- rho_i = (W + H) - row, t = col; the float fields of compvhip_line are not read --, halfWidth b in 0 .. 8, and optionally a
 *     range [p0, p1] of positions on the line's major axis (rule 2 of the segment definition: x-major iff sinQ[t] >= |cosQ[t]|).
 *  1. Band: edge pixel (x, y) belongs to the fit iff | ((x * cosQ[t] + y * sinQ[t]) >> 16) - rho_i | <= b (arithmetic shift of the exact sum:
 *     the vote's own expression) and, with a range, its major coordinate lies in [p0, p1].  b = 0 without a range is the line's support
 *     (pixels == strength); in general pixels is the sum of the accumulator cells (row - b .. row + b, col), rows clipped to [0, R).
 *  2. Moments (int64, exact): n, sx = sum x, sy = sum y, sxx = sum x^2, sxy = sum x y, syy = sum y^2.
 *  3. Central moments (int64, exact): A = n sxx - sx^2, B = n sxy - sx sy, C = n syy - sy^2.  A position holds at most 25 band pixels, so
 *     for max(W, H) <= 8192 n <= 204 800 and |A|, |B|, |C| <= n^2 * 8191^2 < 2^63.  Larger geometries: COMPVHIP_E_NOT_IMPLEMENTED.
 *  4. Fit (binary64, no FMA, in this order): a = (double)A, bb = (double)B, c = (double)C; d = a - c; s = sqrt(d * d + 4 * (bb * bb)).
 *     n < 2 or s == 0: the fit is INVALID and nx = ny = rho = rms2 = 0.  Otherwise: d >= 0: u = -(2 * bb), v = d + s; else u = s - d,
 *     v = -(2 * bb).  h = sqrt(u * u + v * v); nx = u / h; ny = v / h; when ny < 0, or ny == 0 and nx < 0, both are negated (the Hough
 *     convention: the normal is (cos theta, sin theta), theta in [0, pi]).  rho = (nx * (double)sx + ny * (double)sy) / (double)n (signed,
 *     from the image origin, as in toCartesian); rms2 = max(0, (a + c) - s) / (2 * (double)n * (double)n), the mean squared distance.
 *  5. Record: compvhip_line_fit, 80 bytes without padding.
 *  6. Per line (d_segs == NULL): record i belongs to line i of the frame's line array; lines considered: min(d_counts[f], lineCap, maxLines
 *     if > 0).  Per segment (d_segs != NULL): record j belongs to segment j of the first min(d_segCounts[f], segCap) segments, line =
 *     segs[j].line, range = [x0, x1] on an x-major line and [y0, y1] otherwise (clipped to the image).  A segment whose line is not one of
 *     the lines considered, or a line whose cell is outside the accumulator, has an empty band (pixels = 0, invalid fit).
 *     d_fitCounts[f] = records BEFORE clipping; the first min(count, fitCap) are written and nothing behind them.
 *  7. Refined lines (optional, per-line mode): a copy of the lines considered in which a valid fit replaces rho by (float)rho, theta by
 *     (float)atan2(ny, nx) and strength by pixels; row / col stay.  theta is the only value of the feature that goes through a libm function. */
typedef struct compvhip_line_fit {
	int32_t line, pixels;
	int64_t sx, sy, sxx, sxy, syy;
	double  nx, ny, rho, rms2;
} compvhip_line_fit;

/* Fits of the lines (or of the segments of the lines) a compvhip_plan_houghsht / _pipeline call left on the device, for all frames of the plan.
 * d_edges: as for compvhip_plan_houghsht_segments (NULL = the plan's masks, with the same state rules and error codes, COMPVHIP_E_INVALID_STATE
 * while asynchronous steps were not waited for included).  d_segs == NULL: per line; otherwise d_segs / d_segCounts / segCap are what
 * compvhip_plan_houghsht_segments wrote for the same lines.  d_fits: frames * fitCap records (NULL with fitCap == 0: counts, and refined lines,
 * only).  d_refined: NULL, or frames * lineCap lines, of which the lines considered are written -- it feeds compvhip_plan_to_cartesian with the
 * same d_counts and lineCap; COMPVHIP_E_INVALID_PARAMETER in per-segment mode.  halfWidth outside 0 .. 8, lineCap == 0 or a null line / count
 * buffer: COMPVHIP_E_INVALID_PARAMETER; max(W, H) > 8192: COMPVHIP_E_NOT_IMPLEMENTED.  Asynchronous on `stream`; no scratch beyond the
 * plan's SHT tables.  Beyond 65 535 frames: SLICED with the caller's d_edges; the plan's own masks exist only behind a Canny run, which is REFUSED there.
 * d_edges: ANY BYTE; d_fits: 8-byte aligned; d_lines, d_counts, d_segs, d_segCounts, d_fitCounts and d_refined: 4-byte aligned.  Stream order: ASYNC. */
COMPVHIP_API int compvhip_plan_houghsht_fit(compvhip_plan* plan, const uint8_t* d_edges, const compvhip_line* d_lines, const int32_t* d_counts,
                                            size_t lineCap, int maxLines, int halfWidth,
                                            const compvhip_segment* d_segs, const int32_t* d_segCounts, size_t segCap,
                                            compvhip_line_fit* d_fits, size_t fitCap, int32_t* d_fitCounts, compvhip_line* d_refined, void* stream);

/* The same for caller-held lines (and, with segs != NULL, nSegs segments of them) of one HOST edge map; lines in either order, only row / col
 * are read.  Synchronous.  *nFits receives the number of records (n, or nSegs); when it exceeds cap only the first cap are written and
 * COMPVHIP_E_OUT_OF_BOUND is returned (cap == 0 with fits == NULL asks for the number).  refined: NULL, or n lines (segs must be NULL).  A line
 * whose (row, col) is outside the R x T accumulator of (W, H, thetaDeg), or a segment whose line is not below n: COMPVHIP_E_INVALID_PARAMETER. */
COMPVHIP_API int compvhip_houghsht_fit_u8(compvhip_ctx* ctx, const uint8_t* edges, size_t W, size_t H, size_t S, float thetaDeg,
                                          const compvhip_line* lines, size_t n, int halfWidth, const compvhip_segment* segs, size_t nSegs,
                                          compvhip_line_fit* fits, size_t cap, size_t* nFits, compvhip_line* refined);

/* ---- connected components of an edge map: which pixels belong together, how many, how big, where ---------------
 * The reference's labeller (core/ccl, PLSL) has a result type of its own; this call has a canonical, integer-only definition instead
 * (docs/kernels/components.md), so that two correct implementations agree on every byte:
 *  Inputs: an edge map of W x H pixels (foreground = non-zero byte, or set bit of the plan's masks; bytes or bits at columns >= W are never
 *     foreground, whatever they hold), connectivity 4 or 8, minPixels >= 1.
 *  1. Components: the maximal sets of foreground pixels connected through foreground pixels by 8- (or 4-) neighbour steps.
 *  2. Root of a component: its pixel with the smallest raster index y * W + x (W, not the stride).
 *  3. Survivors: components with at least minPixels pixels.  The others are dropped: no record, label 0.
 *  4. Id: survivors are numbered 1, 2, ... in ascending order of their root's raster index.
 *  5. Label map (optional): int32 [frames][H][labelStride], labelStride >= W; 0 for background and dropped components, otherwise the id.
 *     Elements at columns >= W are not written.  The label map does not depend on compCap.
 *  6. Record of component id, stored at index id - 1: the root, the inclusive bounding box, the pixel count.
 *  7. Counts and capacity: d_compCounts[f] = survivors of frame f BEFORE clipping; the first min(count, compCap) records are written and
 *     nothing behind them, so a clipped result is a prefix of the full one.  Frames are independent. */
typedef struct compvhip_component {
	int32_t x, y;               /* the root */
	int32_t x0, y0, x1, y1;     /* bounding box, inclusive */
	int32_t pixels;
} compvhip_component;

/* Components of all frames of the plan.  d_edges: byte edge maps [frames][H][S], or NULL = the 1-bit masks of the plan's last Canny / pipeline
 * step (COMPVHIP_E_INVALID_PARAMETER when the plan holds none, COMPVHIP_E_INVALID_STATE while asynchronous steps were not waited for; a byte
 * map is packed into a mask copy of the call's own and leaves the plan's masks alone).  d_labels == NULL: no label map wanted; d_comps == NULL
 * with compCap == 0: counts only.  Bad connectivity, minPixels < 1, labelStride < W (with a label map): COMPVHIP_E_INVALID_PARAMETER.
 * Asynchronous on `stream`.  Scratch is owned by the plan and allocated on first use: frames * H int32, for byte maps a mask copy
 * (frames * H * wb words, 1/8 of the bytes), and -- only when d_labels == NULL -- one int32 parent word per pixel (frames * W * H * 4 bytes:
 * 33 MB per 4K frame); with a label map the parent words live in it (labelled in place).  Beyond 65 535 frames: SLICED with the caller's d_edges; the plan's own masks exist only behind a Canny run, which is REFUSED there.
 * d_edges: ANY BYTE; d_labels, d_comps and d_compCounts: 4-byte aligned (the kernels run atomics on the label words and on the boxes).  Stream order: ASYNC. */
COMPVHIP_API int compvhip_plan_components(compvhip_plan* plan, const uint8_t* d_edges, int connectivity, int minPixels,
                                          int32_t* d_labels, size_t labelStride, compvhip_component* d_comps, size_t compCap,
                                          int32_t* d_compCounts, void* stream);

/* The same for one HOST edge map (3 <= W, H <= 32767 like every host entry point).  Synchronous.  labels: optional, H rows of labelStride
 * int32.  *nComps receives the number of survivors; when it exceeds cap only the first cap records are written and COMPVHIP_E_OUT_OF_BOUND
 * is returned (cap == 0 with comps == NULL asks for the number; the label map is complete either way). */
COMPVHIP_API int compvhip_components_u8(compvhip_ctx* ctx, const uint8_t* edges, size_t W, size_t H, size_t S, int connectivity, int minPixels,
                                        int32_t* labels, size_t labelStride, compvhip_component* comps, size_t cap, size_t* nComps);

/* ---- thresholding and morphology: from a gray frame to text blobs (docs/kernels/morph.md) --------------------------------------
 * The step between the pre-processing (grayscale, Otsu, blur) and compvhip_plan_components: binarise, close the gaps between glyph strokes,
 * label.  All arithmetic is integer; every result is defined bit for bit.  The plan forms are asynchronous on `stream` and work on
 * [frames][H][S] device planes; the host forms are synchronous (3 <= W, H <= 32767 like every host entry point). */
enum { /* COMPV_MATH_MORPH_OP_TYPE_* (compv_common.h:410-419); the reference compiles its gradient out (compv_math_morph.cxx:112-117) */
	COMPVHIP_MORPH_OP_ERODE = 0,
	COMPVHIP_MORPH_OP_DILATE = 1,
	COMPVHIP_MORPH_OP_OPEN = 2,     /* erode, then dilate */
	COMPVHIP_MORPH_OP_CLOSE = 3     /* dilate, then erode */
};
enum { /* COMPV_MATH_MORPH_STREL_TYPE_* (compv_common.h:402-406) */
	COMPVHIP_MORPH_STREL_RECT = 0,
	COMPVHIP_MORPH_STREL_DIAMOND = 1,
	COMPVHIP_MORPH_STREL_CROSS = 2
};
enum { /* COMPV_BORDER_TYPE_* (compv_common.h:306-310); _IGNORE (1) is internal to the reference's threading */
	COMPVHIP_BORDER_ZERO = 0,
	COMPVHIP_BORDER_REPLICATE = 2   /* CompVMathMorph::process's default */
};
enum { /* kernel of compvhip_plan_morph_ex */
	COMPVHIP_MORPH_KERNEL_AUTO = 0,      /* what compvhip_plan_morph takes: separable for a full rectangle or a cross of more than 15 members, general otherwise */
	COMPVHIP_MORPH_KERNEL_GENERAL = 1,   /* the member-list kernel, whatever the shape */
	COMPVHIP_MORPH_KERNEL_SEPARABLE = 2  /* full rectangles and crosses only (anything else: COMPVHIP_E_INVALID_PARAMETER) */
};

/* CompVImageThreshold::global (base/image/compv_image_threshold.cxx:118-180, leaf :320-347): out = in > t8 ? 0xff : 0 with
 * t8 = (uint8_t)(clip(threshold, 0, 255) + 0.5).  threshold < 0: COMPVHIP_E_INVALID_PARAMETER (:120).  in and out may alias. */
COMPVHIP_API int compvhip_threshold_u8(compvhip_ctx* ctx, const uint8_t* in, size_t W, size_t H, size_t S, double threshold,
                                       uint8_t* out, size_t So);
/* The same on `frames` device frames.  d_levels != NULL: frame f is cut at d_levels[f] clipped to 0..255 and `threshold` is ignored --
 * the array compvhip_plan_otsu writes, so Otsu + binarise is CompVImage::thresholdOtsu(input, t, &output) (compv_image_threshold.cxx:110-113)
 * without a host round trip.  d_in and d_out may be the same buffer.  Columns >= W of d_out are never written.  Beyond 65 535 frames: SLICED.
 * d_in and d_out: ANY BYTE; d_levels: 4-byte aligned.  Stream order: ASYNC. */
COMPVHIP_API int compvhip_plan_threshold(compvhip_plan* plan, const uint8_t* d_in, double threshold, const int32_t* d_levels,
                                         uint8_t* d_out, void* stream);

/* CompVImageThreshold::adaptive (base/image/compv_image_threshold.cxx:183-317) as its single-threaded path computes it:
 *   k    = (uint16_t)((1.f / (float)blockSize) * 0xffff)                         CompVKernel::mean, base/compv_kernel.cxx:12-25
 *   mean = compvhip_convlt1_fixedpoint_u8 with blockSize taps k, vertical and horizontal (zero border of blockSize / 2 included)
 *   d = (int)(clip(delta, 0, 255) + 0.5), m = (uint8_t)(clip(maxVal, 0, 255) + 0.5)
 *   hit = (in - mean + 255) >= (256 - d)                                         the 768-entry LUT of :222-226,287
 *   out = (hit != invert) ? m : 0
 * On the border mean is 0 and the formula decides there as everywhere else.  blockSize even or < 3, W or H < blockSize, maxVal < 0:
 * COMPVHIP_E_INVALID_PARAMETER; odd blockSize > 31: COMPVHIP_E_NOT_IMPLEMENTED.  in and out may alias. */
COMPVHIP_API int compvhip_threshold_adaptive_u8(compvhip_ctx* ctx, const uint8_t* in, size_t W, size_t H, size_t S, size_t blockSize,
                                                double delta, double maxVal, int invert, uint8_t* out, size_t So);
/* The same on `frames` device frames, one fused kernel: the mean never reaches memory.  d_in == d_out is served through a plane the plan owns
 * (allocated on first use) and a device copy; any other overlap: COMPVHIP_E_INVALID_PARAMETER.  Columns >= W of d_out are never written.
 * Beyond 65 535 frames: SLICED (in place, the device copy is one enqueue per frame).  d_in and d_out: ANY BYTE.  Stream order: ASYNC. */
COMPVHIP_API int compvhip_plan_threshold_adaptive(compvhip_plan* plan, const uint8_t* d_in, size_t blockSize, double delta, double maxVal,
                                                  int invert, uint8_t* d_out, void* stream);

/* CompVMathMorph::buildStructuringElement (base/math/compv_math_morph.cxx:89-93,476-540): strel = h rows of w bytes, 0xff marks a member.
 * RECT: all; CROSS: row h / 2 and column w / 2; DIAMOND (w == h, else COMPVHIP_E_INVALID_PARAMETER): 1, 3, 5, ... members centred on column
 * w / 2 down to the middle row, then back.  w or h == 0: COMPVHIP_E_INVALID_PARAMETER; unknown type: COMPVHIP_E_NOT_IMPLEMENTED.  Host
 * arithmetic only; no GPU involved. */
COMPVHIP_API int compvhip_morph_strel(int type, size_t w, size_t h, uint8_t* strel);

/* CompVMathMorph::process (base/math/compv_math_morph.cxx:95-123; basicOper :125-247, borders :542-674, leaf :676-692).
 * strel: sh rows of sw bytes, non-zero = member; sw, sh odd, 1..31 (even or larger: COMPVHIP_E_NOT_IMPLEMENTED); all zero, W < sw or
 * H < sh: COMPVHIP_E_INVALID_PARAMETER.  One basic operation, with wd = sw >> 1, hd = sh >> 1, hb = (sh + 1) >> 1:
 *   interior   wd <= x < W - wd, hd <= y < H - hd:  out(y, x) = OP over the members (j, i) of in(y - hd + j, x - wd + i), OP = min (erode) or
 *              max (dilate) -- the same offsets for both: dilation does NOT reflect the strel
 *   borders    afterwards, rows y < hb and y >= H - hb, then columns x < wd and x >= W - wd, take in(y, x) (REPLICATE) or 0 (ZERO).  The
 *              row border is hb rows, one more than the interior leaves open (addBordersVt, :552): with sh = 3 rows 1 and H - 2 are
 *              overwritten although they were computed, with sh = 1 the first and last rows are copied.
 * OPEN / CLOSE are two complete basic operations, borders included.  in and out must not overlap (COMPVHIP_E_INVALID_PARAMETER; the
 * reference reallocates, :140-145).  Other op / border values: COMPVHIP_E_NOT_IMPLEMENTED. */
COMPVHIP_API int compvhip_morph_u8(compvhip_ctx* ctx, const uint8_t* in, size_t W, size_t H, size_t S, const uint8_t* strel, size_t sw,
                                   size_t sh, int op, int border, uint8_t* out, size_t So);
/* The same on `frames` device frames (strel is a HOST array).  An OPEN / CLOSE is two launches through a u8 plane [frames][H][S] the plan owns
 * (allocated on first use).  Columns >= W of d_out are never written.  Beyond 65 535 frames: SLICED (compvhip_plan_morph_ex as well).  d_in and d_out: ANY
 * BYTE (compvhip_plan_morph_ex as well).  Stream order: ASYNC. */
COMPVHIP_API int compvhip_plan_morph(compvhip_plan* plan, const uint8_t* d_in, const uint8_t* strel, size_t sw, size_t sh, int op,
                                     int border, uint8_t* d_out, void* stream);
/* compvhip_plan_morph with the kernel named (COMPVHIP_MORPH_KERNEL_*): for measuring one kernel against the other and for testing both on
 * the same structuring element.  The result does not depend on it.  Stream order: ASYNC. */
COMPVHIP_API int compvhip_plan_morph_ex(compvhip_plan* plan, const uint8_t* d_in, const uint8_t* strel, size_t sw, size_t sh, int op,
                                        int border, int kernel, uint8_t* d_out, void* stream);

/* ---- FAST corner detection (docs/kernels/fast.md) -------------------------------------------------------------------------------------
 * CompVCornerDeteFAST (core/features/fast/compv_core_feature_fast_dete.cxx; COMPV_FAST_ID) on device frames: scores, non-maximum
 * suppression and the corner list, every output defined bit for bit.  For a gray frame I of W x H, threshold t (clipped to 0..255 as the
 * reference's set() does, :135) and N = 9 or 12 (fastType; anything else: COMPVHIP_E_INVALID_PARAMETER, :146):
 *  1. Ring: 16 offsets (dx, dy) clockwise from the top (:221-238):
 *     (0,-3) (1,-3) (2,-2) (3,-1) (3,0) (3,1) (2,2) (1,3) (0,3) (-1,3) (-2,2) (-3,1) (-3,0) (-3,-1) (-2,-2) (-1,-3); p_k = I(x + dx_k, y + dy_k).
 *  2. Limits b = min(255, I + t), d = max(0, I - t); differences D_k = max(0, d - p_k), B_k = max(0, p_k - b).
 *  3. Score of an interior pixel (3 <= x < W - 3, 3 <= y < H - 3): the max over the 16 arcs of N consecutive ring positions of the min over the
 *     arc of D_k, and the same for B_k; the larger of the two.  0 when no arc is entirely darker or entirely brighter.  Every other pixel
 *     scores 0.  (The early exits of CompVFastDataRow_C, :679-688, :729, :748, are necessary conditions and do not change the value.)
 *  4. NMS (nonmax != 0; :773-831): a pixel with score s > 0 is dropped when any of its 8 neighbours has a score >= s.  All comparisons use the
 *     scores before suppression; two equal neighbours both go.
 *  5. Record {x, y, strength}: strength = score + t - 1 as an exact integer (<= 254; :498,:521).  At t == 0 the reference's own code paths
 *     disagree (one wraps a byte); the integer formula holds here.
 *  6. Order: raster (y, then x), the reference's single-threaded order.
 *  7. maxFeatures > 1 and more corners than that: with s* the maxFeatures-th largest strength of the frame, every corner with strength >= s*
 *     stays, in raster order -- ties at the cut all stay, so the count may exceed maxFeatures.  (The reference's selectBest,
 *     compv_common.h:641-656, reads an nth_element pivot the standard leaves unspecified; its result lies between the corners above s* and
 *     this set.)  maxFeatures <= 1: no cut.
 *  8. Counts and capacity, as compvhip_plan_components: d_counts[f] = corners of frame f BEFORE clipping to cornerCap; the first
 *     min(count, cornerCap) records of frame f are written at d_corners + f * cornerCap and nothing behind them, so a clipped result is a
 *     prefix of the full one.  Frames are independent.
 *  9. Score map (optional): uint8 [frames][H][S]; the scores after NMS when NMS is on, untouched by the maxFeatures cut; border pixels
 *     hold 0; columns >= W are never written.
 * W or H < 7 (no interior pixel): COMPVHIP_E_INVALID_PARAMETER (the reference accepts 4..6, where its row length underflows). */
typedef struct compvhip_corner {
	int32_t x, y;
	int32_t strength;           /* score + t - 1 */
} compvhip_corner;

/* Corners of all frames of the plan.  d_gray: [frames][H][S], 8-byte aligned; d_scores: NULL or a score map of the same geometry (8-byte aligned, must not
 * overlap d_gray); d_corners and d_counts: 4-byte aligned (anything else: COMPVHIP_E_INVALID_PARAMETER); d_corners == NULL with cornerCap == 0: counts only.  Asynchronous on `stream`; results are deterministic run to run.  Scratch
 * is owned by the plan, allocated on first use and released with it: frames * (2 * H + 257) int32, and -- only when d_scores == NULL -- a score
 * map of the plan's own.  Beyond 65 535 frames: REFUSED.  Stream order: ASYNC. */
COMPVHIP_API int compvhip_plan_fast(compvhip_plan* plan, const uint8_t* d_gray, int threshold, int fastType, int nonmax, int maxFeatures,
                                    uint8_t* d_scores, compvhip_corner* d_corners, size_t cornerCap, int32_t* d_counts, void* stream);

/* The same for one HOST frame (7 <= W, H <= 32767).  Synchronous, on the context's cached single-frame plan.  scores: optional, H rows of So
 * bytes (So >= W).  *n receives the number of corners; when it exceeds cap only the first cap records are written and COMPVHIP_E_OUT_OF_BOUND
 * is returned (cap == 0 with corners == NULL asks for the number; the score map is complete either way). */
COMPVHIP_API int compvhip_fast_u8(compvhip_ctx* ctx, const uint8_t* gray, size_t W, size_t H, size_t S, int threshold, int fastType, int nonmax,
                                  int maxFeatures, uint8_t* scores, size_t So, compvhip_corner* corners, size_t cap, size_t* n);

/* ---- brute-force Hamming matching (docs/kernels/match.md) --------------------------------------------------------------------------
 * CompVMatcherBruteForce (core/matchers/compv_core_matcher_bruteforce.cxx:81-228; COMPV_BRUTEFORCE_ID) on device descriptors, every output
 * defined bit for bit.  One pair has Q query rows and T train rows of descBytes bytes:
 *  1. Distance: d(q, t) = popcount of the XOR of the two rows over their descBytes bytes.  Stride padding is never read.
 *  2. Neighbours, as compvhip_matcher_knn returns them: the train rows sorted ascending by (d(q, t), t); neighbour r is the r-th of them.
 *     This is NOT the reference's order among equal distances: its loops (:181-191 for KNN == 2, :215-222) let a displaced entry pass the
 *     equally distant entries behind it, so its order depends on the arrival sequence (docs/kernels/match.md).  The distances of every
 *     column agree; only the host form, compvhip_match_hamming_u8, reproduces the reference's train indices on ties.
 *  3. Record: matches[r][q] = {q, t_r, 0, d(q, t_r)} -- CompVDMatch (compv_common.h:674) -- for r < min(knn, T).  The device form has the fixed
 *     shape [pairs][knn][queryCap]: rows r >= T hold {q, -1, 0, INT32_MAX}; columns q >= the pair's query count are never written.
 *  4. Counts: d_queryCounts[p] / d_trainCounts[p] are int32 in device memory and may exceed the capacity (as compvhip_plan_fast's d_counts
 *     can): min(count, cap) rows are used, a negative count is 0, a NULL pointer means every pair is full.
 *  5. Good list (samples/object_recognition/main.cxx:183-200): matches[0][q] of the queries that pass every enabled test, in ascending q --
 *     ratio: (double)d0 < ratio * (double)d1 (one binary64 multiply, one compare; needs knn >= 2; a pair with T < 2 passes none);
 *     distance: d0 <= maxDistance; cross check: among the pair's queries, q has the smallest (d(q', t0), q') for its best train row t0.
 *     d_goodCounts[p] = their number BEFORE clipping to goodCap; the first min(count, goodCap) are written and nothing behind them.
 *     (The sample's loop bound min(rows - 1, cols) drops the last query: its quirk, not reproduced.) */
typedef struct compvhip_match {
	int32_t queryIdx, trainIdx, imageIdx, distance;
} compvhip_match;
typedef struct compvhip_match_opts {
	double ratio;               /* <= 0: no ratio test */
	int maxDistance;            /* < 0: no distance test */
	int crossCheck;             /* != 0: cross check */
} compvhip_match_opts;
typedef struct compvhip_matcher compvhip_matcher;   /* scratch for `pairs` pairs of at most queryCap x trainCap rows; not tied to an image geometry */

/* descBytes: a multiple of 4 in 4..128; knn 1..8; queryCap, trainCap, pairs >= 1 (anything else: COMPVHIP_E_INVALID_PARAMETER).  All scratch
 * is allocated here -- pairs * max(ceil(trainCap / 128) * knn * queryCap, ceil(queryCap / 128) * trainCap) key words (the forward and the
 * reverse run share them) and pairs * trainCap records --
 * and released by compvhip_matcher_destroy: no later call allocates or synchronises.  Destroy a matcher BEFORE its context.  Like a plan, a
 * matcher is not re-entrant: its calls share the scratch and must be ordered on one stream.  More than 65 535 pairs: REFUSED (a pair is the
 * matcher's frame). */
COMPVHIP_API int compvhip_matcher_create(compvhip_ctx* ctx, size_t descBytes, size_t queryCap, size_t trainCap, size_t pairs, int knn,
                                         compvhip_matcher** matcher);
COMPVHIP_API void compvhip_matcher_destroy(compvhip_matcher* matcher);

/* d_query: [pairs][queryCap] rows of queryStride bytes (descBytes <= queryStride <= 65536, queryStride % 4 == 0, 4-byte aligned); d_train: the same with
 * trainCap / trainStride, or, with trainShared != 0, ONE train set [trainCap] and ONE train count that serve every pair (one trained object
 * against many frames).  d_matches: [pairs][knn][queryCap] records, 16-byte aligned; d_queryCounts and d_trainCounts 4-byte aligned.  Asynchronous on `stream`;
 * deterministic run to run.  Stream order: ASYNC. */
COMPVHIP_API int compvhip_matcher_knn(compvhip_matcher* matcher, const uint8_t* d_query, size_t queryStride, const int32_t* d_queryCounts,
                                      const uint8_t* d_train, size_t trainStride, const int32_t* d_trainCounts, int trainShared,
                                      compvhip_match* d_matches, void* stream);

/* The good list of the d_matches a compvhip_matcher_knn call of this matcher wrote for the same descriptors and counts.  The descriptors are
 * read by the cross check only (it runs the distance kernel with the roles swapped and knn = 1 into the matcher's scratch).  d_good:
 * [pairs][goodCap] records, 16-byte aligned (NULL with goodCap == 0: counts only); d_goodCounts: [pairs] int32; d_matches 16-byte aligned, the descriptors and
 * the three count arrays 4-byte aligned.  opts == NULL, or
 * ratio > 0 on a matcher with knn < 2: COMPVHIP_E_INVALID_PARAMETER.  Asynchronous on `stream`.  Stream order: ASYNC. */
COMPVHIP_API int compvhip_matcher_good(compvhip_matcher* matcher, const compvhip_match* d_matches,
                                       const uint8_t* d_query, size_t queryStride, const int32_t* d_queryCounts,
                                       const uint8_t* d_train, size_t trainStride, const int32_t* d_trainCounts, int trainShared,
                                       const compvhip_match_opts* opts, compvhip_match* d_good, size_t goodCap, int32_t* d_goodCounts, void* stream);

/* CompVMatcherBruteForce::process for one HOST pair: Q query rows and T train rows of `cols` bytes (1..128; rows are padded to a dword multiple
 * with zero bytes on the way to the device, which cannot change a distance), knn 1..8.  matches: min(knn, T) rows of matchStride records
 * (matchStride >= Q), the reference's shape (:102); *rows receives min(knn, T).  Among equal distances the records follow the REFERENCE's
 * insertion order (tests/match_model.py: knn_reference; docs/kernels/match.md), not the (d, t) order of item 2: on ties the train indices of
 * this call and of compvhip_matcher_knn differ, the distances never do.  Synchronous; one lane per query walks every train row, so this is
 * the parity path, not the fast one. */
COMPVHIP_API int compvhip_match_hamming_u8(compvhip_ctx* ctx, const uint8_t* query, size_t Q, size_t queryStride, const uint8_t* train, size_t T,
                                           size_t trainStride, size_t cols, int knn, compvhip_match* matches, size_t matchStride, size_t* rows);

/* Per-kernel timing of the matcher's last call (HIP events on the call's stream), as compvhip_plan_set_timing / _get_timing: entries
 * match_slice_kernel, match_merge_kernel [, match_reverse_slice_kernel, match_reverse_merge_kernel], match_good_kernel.  Reading the
 * timing waits for the events. */
COMPVHIP_API int compvhip_matcher_set_timing(compvhip_matcher* matcher, int enabled);
COMPVHIP_API int compvhip_matcher_get_timing(compvhip_matcher* matcher, const char** names, float* ms, int cap);

/* ---- ORB: keypoint orientation and rotated-BRIEF descriptors (docs/kernels/orb.md) ------------------------------------------------------
 * The intensity-centroid orientation of CompVCornerDeteORB::processLevelAt (core/features/orb/compv_core_feature_orb_dete.cxx:281-358) and the
 * BRIEF-256/31 of CompVCornerDescORB (compv_core_feature_orb_desc.cxx:206-319) for ONE pyramid level: a plan is the level's geometry, the calls
 * take the level's number and scale factor.  (The pyramid over them: compvhip_orbpyr below.)  Every output is defined bit for bit.
 * Keypoints, from a corner list {x, y, strength} of a gray frame I of W x H:
 *  1. Border erase (eraseTooCloseToBorder, compv_common.h:657): with b = 18 = (31 + 5) >> 1, a corner with x < b, x + b >= W, y < b or
 *     y + b >= H is dropped; the survivors keep their order.
 *  2. Moments (CompVPatch::moments0110, base/compv_patch.cxx:106-165, radius 15): m10 = sum i * I(x + i, y + j), m01 = sum j * I(x + i, y + j) over
 *     j = -15 .. 15, i = -dX[|j|] .. dX[|j|], dX[k] = (int)sqrt(225 - k * k) (row |j| = 15: the centre column only); exact int32, on the
 *     UNBLURRED plane.
 *  3. Orientation: rad = (float)atan2((double)m01, (double)m10); orient = rad * k180OverPi, a float32 product with
 *     k180OverPi = 180.f / 3.1415926535897932384626433f evaluated in float32 (base/math/compv_math.cxx:27,31); orient += 360.f when orient < 0.
 *     The reference calls std::atan2(float, float), whose last bit depends on the libm; the binary64 call rounded once is the canonical value.
 *  4. Record: x, y = (float) of the corner's integers, multiplied by sfi = 1.f / scale when level != 0 (:351-354); strength = (float) of the
 *     corner's; level = the argument; size = 31 / scale (float32).
 *  5. Counts and capacity, as compvhip_plan_fast: d_keyCounts[f] = survivors of frame f BEFORE clipping to keyCap; the first min(count, keyCap)
 *     records are written at d_keypoints + f * keyCap and nothing behind them.  d_cornerCounts[f] may exceed cornerCap (min is used); a
 *     negative count is 0.
 * Descriptors, 32 bytes per keypoint, row q of frame f at d_desc + (f * keyCap + q) * descStride:
 *  1. Blur: CompVMathConvlt::convlt1FixedPoint with CompVMathGauss::kernelDim1FixedPoint(5, 2.0f) on both axes (zero output border of 2), into a
 *     plane of the plan's own: d_gray is never modified (the reference blurs its pyramid in place).  blur == 0: d_gray IS the blurred plane.
 *  2. Centre: fx = x * scale (float32), xi = (int)((double)fx + 0.5); the same for y (:279-288).
 *  3. Angle: a = orient * kPiOver180 (float32, kPiOver180 = 3.1415926535897932384626433f / 180.f); fcos = (float)cos((double)a),
 *     fsin = (float)sin((double)a) -- canonical as in 3. above (the reference: std::cos / std::sin of a float).
 *  4. Test i of the 256, pattern points (AX, AY), (BX, BY) -- the published rBRIEF pattern of the ORB method, coordinates in -13 .. 12 -- as the
 *     reference's AVX2 leaf computes it: xf = AX * fcos - AY * fsin, yf = AX * fsin + AY * fcos (two float32 products, one float32 sum, no
 *     FMA); x = rint(xf), y = rint(yf), ties to even; a = blurred(xi + x, yi + y), b likewise from (BX, BY); bit i % 8 of byte i / 8 is a < b.
 *  5. A keypoint with xi < 18, xi + 18 >= W, yi < 18 or yi + 18 >= H gets 32 zero bytes IN ITS OWN ROW.  (The reference tests radius 15 and does
 *     not advance its output pointer for such a point, which shifts every later row.  18 is what the detector guarantees and what a rotated
 *     (+-13, +-13) reaches: 13 * sqrt(2) = 18.38 rounds to 18.)
 *  6. Rows q >= min(d_keyCounts[f], keyCap) are never written.
 * W or H < 37: COMPVHIP_E_INVALID_PARAMETER (no admissible position). */
typedef struct compvhip_keypoint {   /* CompVInterestPoint (compv_common.h:629), 24 bytes */
	float x, y;
	float strength;
	float orient;               /* degrees, [0, 360] */
	int32_t level;
	float size;
} compvhip_keypoint;

/* Keypoints of all frames of the plan from the corner lists compvhip_plan_fast wrote (d_corners: [frames][cornerCap], d_cornerCounts: [frames],
 * device).  d_gray: [frames][H][S], 4-byte aligned; d_keypoints: [frames][keyCap] (NULL with keyCap == 0: counts only); d_moments: NULL or
 * [frames][keyCap][2] int32 = {m01, m10}; records, counts and moments 4-byte aligned; scale > 0 (anything else: COMPVHIP_E_INVALID_PARAMETER).
 * Asynchronous on `stream`, no atomic, deterministic.  Scratch is owned by the plan, allocated on first use (and again for a larger keyCap) and
 * released with it: frames * keyCap int32.  Beyond 65 535 frames: REFUSED.  Stream order: ASYNC. */
COMPVHIP_API int compvhip_plan_orb_keypoints(compvhip_plan* plan, const uint8_t* d_gray, const compvhip_corner* d_corners, size_t cornerCap,
                                             const int32_t* d_cornerCounts, int level, float scale, compvhip_keypoint* d_keypoints, size_t keyCap,
                                             int32_t* d_keyCounts, int32_t* d_moments, void* stream);

/* Descriptors of the keypoints (compvhip_plan_orb_keypoints' or the caller's own) with the level's `scale`.  descStride >= 32 and a multiple of 4,
 * d_gray, d_keypoints, d_keyCounts and d_desc 4-byte aligned, keyCap > 0 (anything else: COMPVHIP_E_INVALID_PARAMETER).  With descStride == 32, d_desc / d_keyCounts are what
 * compvhip_matcher_knn takes as d_query / d_queryCounts.  Asynchronous on `stream`.  Scratch, allocated on first use with blur != 0: one blurred
 * batch [frames][H][S].  Beyond 65 535 frames: REFUSED.  Stream order: ASYNC. */
COMPVHIP_API int compvhip_plan_orb_describe(compvhip_plan* plan, const uint8_t* d_gray, const compvhip_keypoint* d_keypoints, size_t keyCap,
                                            const int32_t* d_keyCounts, float scale, int blur, uint8_t* d_desc, size_t descStride, void* stream);

/* Both for one HOST frame (37 <= W, H <= 32767) and n host corners: keypoints and desc have room for n records / n rows of descStride bytes;
 * *kept receives the number of keypoints (<= n).  Synchronous, on the context's cached single-frame plan. */
COMPVHIP_API int compvhip_orb_u8(compvhip_ctx* ctx, const uint8_t* gray, size_t W, size_t H, size_t S, const compvhip_corner* corners, size_t n,
                                 int level, float scale, compvhip_keypoint* keypoints, uint8_t* desc, size_t descStride, size_t* kept);

/* ---- bilinear scale and the ORB scale pyramid (docs/kernels/scale.md, docs/kernels/orb.md) ------------------------------------------------
 * CompVCornerDeteORB::process (core/features/orb/compv_core_feature_orb_dete.cxx:148-358) is defined over a pyramid: every level scaled from the
 * original frame, a feature quota per level, the levels' lists concatenated in level order.  Every output is defined bit for bit.
 * A. Bilinear scale (CompVImageScaleBilinear, base/image/compv_image_scale_bilinear.cxx:48-88,149-192, through CompVImage::scale,
 *    compv_image.cxx:852-905).  Source Win x Hin, destination Wout x Hout, uint8, one plane:
 *  1. sx = (int)(((float)Win / (float)Wout) * 256.f), every operation in float32, truncated; sy likewise.
 *  2. Both ratios (float)Win / (float)Wout and (float)Hin / (float)Hout must lie in (0, 256): anything else, or a size of 0, is
 *     COMPVHIP_E_INVALID_PARAMETER (the reference only warns and distorts).
 *  3. Output pixel (i, j): x = i * sx, y = j * sy; nx = x >> 8, ny = y >> 8; x0 = x & 255, x1 = 255 - x0, y0 = y & 255, y1 = 255 - y0;
 *     A = n0 * x1 + n1 * x0, B = n2 * x1 + n3 * x0 with n0 = I(nx, ny), n1 = I(nx + 1, ny), n2 = I(nx, ny + 1), n3 = I(nx + 1, ny + 1);
 *     out = (uint8)(((y1 * A) >> 16) + ((y0 * B) >> 16)) -- two separate shifts, as the reference's live branch and its AVX2 leaf's two mulhi.
 *     The weights sum to 255, not 256: the reference's arithmetic, kept.  Everything fits in uint32.
 *  4. Wout == Win and Hout == Hin is a copy (the clone branch of CompVImage::scale), not the arithmetic of 3.
 *  5. Neighbour indices are clamped to Win - 1 and Hin - 1.  A strict downscale never reaches past them; for an upscale the reference reads its
 *     stride padding and one row past the plane, so the clamp is this library's rule there.
 *  6. Columns >= Wout of the destination stride are never written (the AVX2 leaf scribbles there).
 * B. Pyramid geometry (CompVImageScalePyramid, base/image/compv_image_scale_pyramid.cxx:16-46,163-168):
 *  1. sf[0] = 1.f, sf[l] = sf[l - 1] * scaleFactor in float32 (sf[1] = scaleFactor); sfs = 1.f + sf[1] + ... accumulated in float32 in level
 *     order (0.83, 8 levels: 4.5574746).
 *  2. W_l = (size_t)((float)W * sf[l]), H_l likewise; every level is scaled FROM THE ORIGINAL frame by A.  Level 0 is the caller's frame
 *     itself and is not copied.
 *  3. levels in 1 .. 16, 0 < scaleFactor < 1, level 0 at least 37 x 37: anything else is COMPVHIP_E_INVALID_PARAMETER.
 *  4. A level with W_l < 37 or H_l < 37 is EMPTY: it owns no plane and contributes no keypoint (the border erase would remove every corner
 *     of it anyway; the reference runs FAST on it for nothing and fails at size 0).
 * C. Detection per level (processLevelAt, :281-358):
 *  1. FAST on the level plane by the FAST section above, with the pyramid's threshold, fastType and nonmax.
 *  2. Quota: with maxFeatures > 0, nf = ((float)maxFeatures / sfs) * sf[l] in float32, quota = max(10, (int32)((double)nf + 0.5)); a level with
 *     more corners is cut by rule 7 of the FAST section with maxFeatures = quota (ties at the cut stay, raster order).  maxFeatures <= 0: no cut.
 *  3. Border erase, moments, orientation and record as compvhip_plan_orb_keypoints with level = l and scale = sf[l].
 *  4. Frame f's keypoints are the levels' lists in level order, each level in its own (raster) order.  d_keyCounts[f] is the total BEFORE
 *     clipping to keyCap; the first min(total, keyCap) records are written and nothing behind them (a clip may fall inside a level).
 *  5. d_levelCounts (optional, [frames][levels] int32): the survivors of each level before clipping; 0 for an empty level.
 *  6. d_levelCorners (optional, [frames][levels] int32): the FAST count of the level after the cut and BEFORE clipping to the object's
 *     cornerCap -- a value above cornerCap says that the level's list was truncated to its raster prefix.
 * D. Description (CompVCornerDescORB::describe, compv_core_feature_orb_desc.cxx:206-319):
 *  1. Each non-empty level plane is blurred out of place (5 taps, sigma 2.0, Q16), as the single-level path does.
 *  2. Each keypoint is described on the plane of ITS OWN `level` field with sf[level], by the descriptor rules of the ORB section.
 *  3. A keypoint whose level is outside 0 .. levels - 1, whose level is empty, or that sits inside the 18-pixel margin gets a zero row in place.
 *  4. The caller's keypoints may mix levels in any order (what CompVCornerDescORB::process accepts). */
typedef struct compvhip_orbpyr compvhip_orbpyr;
typedef struct compvhip_orbpyr_opts {
	int levels; float scaleFactor;           /* 8, 0.83f */
	int threshold, fastType, nonmax;         /* 20, 9, 1 */
	int maxFeatures;                         /* 2000; <= 0: no cut */
} compvhip_orbpyr_opts;

/* A pyramid for `frames` frames of W x H with stride S (S % 8 == 0; frames [frames][H][S]).  It owns lighter state than per-level plans (no
 * Canny / Hough scratch), all allocated here except the index list and the blurred planes, which come with the first call that needs them:
 * level planes, levels 1 .. of the non-empty ones, [frames][H_l][S_l] with S_l = W_l rounded up to 8; the same again, level 0 included, blurred
 * (first describe); ONE corner list [frames][cornerCap] and ONE FAST score map [frames][H][S] that the levels use in turn, with FAST's
 * frames * (2 * H + 257) int32; frames * keyCap int32 source indices (first detect, again for a larger keyCap); (3 * levels + 1) * frames int32
 * counts.  cornerCap >= 1.  Destroy a pyramid BEFORE its context; compvhip_live_allocations then returns to its earlier value.  Like a plan,
 * a pyramid is not re-entrant: its calls share the scratch and must be ordered on one stream.  More than 65 535 frames: REFUSED. */
COMPVHIP_API int compvhip_orbpyr_create(compvhip_ctx* ctx, size_t W, size_t H, size_t S, size_t frames, const compvhip_orbpyr_opts* opts, size_t cornerCap,
                                        compvhip_orbpyr** pyramid);
COMPVHIP_API void compvhip_orbpyr_destroy(compvhip_orbpyr* pyramid);
/* Host arithmetic only: size, stride, sf[level] and quota (0 without a cut) of a level; an empty level has S == 0.  Any output may be NULL. */
COMPVHIP_API int compvhip_orbpyr_geometry(const compvhip_orbpyr* pyramid, int level, size_t* W, size_t* H, size_t* S, float* scale, int* quota);
/* The device plane [frames][H_l][S_l] of a level as the last call built it: blurred == 0 the scaled plane (level 0: the caller's d_gray of that
 * call), else the blurred one.  COMPVHIP_E_INVALID_STATE before a call built it, COMPVHIP_E_INVALID_PARAMETER for an empty level.  d_plane: a HOST
 * pointer that receives the device address. */
COMPVHIP_API int compvhip_orbpyr_plane(compvhip_orbpyr* pyramid, int level, int blurred, const uint8_t** d_plane);
/* C. for every frame.  d_gray 8-byte aligned; d_keypoints: [frames][keyCap] (NULL with keyCap == 0: counts only); keypoints and counts (d_keyCounts,
 * d_levelCounts, d_levelCorners) 4-byte aligned.
 * Asynchronous on `stream`, never synchronises the host, deterministic run to run.  Stream order: ASYNC. */
COMPVHIP_API int compvhip_orbpyr_detect(compvhip_orbpyr* pyramid, const uint8_t* d_gray, compvhip_keypoint* d_keypoints, size_t keyCap, int32_t* d_keyCounts,
                                        int32_t* d_levelCounts, int32_t* d_levelCorners, void* stream);
/* D. for every frame; rows as compvhip_plan_orb_describe writes them (rows q >= min(count, keyCap) are never written).  reusePlanes != 0:
 * describe on the planes the preceding compvhip_orbpyr_detect built from the same d_gray (COMPVHIP_E_INVALID_STATE when there was none);
 * reusePlanes == 0 rebuilds them.  d_gray 8-byte aligned; d_keypoints, d_keyCounts and d_desc 4-byte aligned.  Asynchronous on `stream`, never synchronises
 * the host.  Stream order: ASYNC. */
COMPVHIP_API int compvhip_orbpyr_describe(compvhip_orbpyr* pyramid, const uint8_t* d_gray, int reusePlanes, const compvhip_keypoint* d_keypoints, size_t keyCap,
                                          const int32_t* d_keyCounts, uint8_t* d_desc, size_t descStride, void* stream);
/* A. for every frame of a plan: d_in [frames][H][S] of the plan's geometry -> d_out [frames][Hout][Sout] (Sout >= Wout; sizes up to 32767; the
 * buffers must not overlap).  A destination that is dword-aligned in pointer and stride is written with dword stores.  Asynchronous on `stream`.
 * Beyond 65 535 frames: REFUSED.  d_in and d_out: ANY BYTE (a destination that is not dword-aligned is written byte by byte).  Stream order: ASYNC. */
COMPVHIP_API int compvhip_plan_scale(compvhip_plan* src, const uint8_t* d_in, uint8_t* d_out, size_t Wout, size_t Hout, size_t Sout, void* stream);
/* A. for one HOST plane (sizes 1 .. 32767).  Synchronous. */
COMPVHIP_API int compvhip_scale_u8(compvhip_ctx* ctx, const uint8_t* in, size_t W, size_t H, size_t S, uint8_t* out, size_t Wout, size_t Hout, size_t Sout);
/* C. and D. for one HOST frame (37 <= W, H <= 32767; opts == NULL: the defaults).  *n receives the number of keypoints; when it exceeds cap only
 * the first cap records and rows are written and COMPVHIP_E_OUT_OF_BOUND is returned, as compvhip_fast_u8 does.  Synchronous. */
COMPVHIP_API int compvhip_orb_pyramid_u8(compvhip_ctx* ctx, const uint8_t* gray, size_t W, size_t H, size_t S, const compvhip_orbpyr_opts* opts,
                                         compvhip_keypoint* keypoints, uint8_t* desc, size_t descStride, size_t cap, size_t* n);
/* Per-kernel timing of the pyramid's last call, as compvhip_matcher_set_timing / _get_timing: entries scale_bilinear_kernel, then per level
 * fast_score_kernel, fast_list_kernels, orb_select_kernel, orb_orient_kernel, then orb_pyramid_counts_kernel (detect); scale_bilinear_kernel,
 * convlt_fxp_kernels per level, orb_brief_pyramid_kernel (describe). */
COMPVHIP_API int compvhip_orbpyr_set_timing(compvhip_orbpyr* pyramid, int enabled);
COMPVHIP_API int compvhip_orbpyr_get_timing(compvhip_orbpyr* pyramid, const char** names, float* ms, int cap);

/* ---- remap and inverse warp (docs/kernels/remap.md) -------------------------------------------------------------------------------------------
 * CompVImageRemap::process (base/image/compv_image_remap.cxx) and CompVImage::warpInverse (base/image/compv_image.cxx:997-1195), float32 maps and
 * matrices, one uint8 plane.  Every output is defined bit for bit.  Source Win x Hin, destination Wout x Hout; all floating point is float32, one
 * rounding per operation, unless a step says otherwise.
 * A. Coordinates (x, y) in the source of output pixel (i, j):
 *  1. Remap: two float32 planes of Wout * Hout values, row-major without stride: x = mapX[j * Wout + i], y = mapY[j * Wout + i].
 *  2. Inverse warp: a matrix M = {a b c; d e f[; g h M22]} of 2 x 3 or 3 x 3 float32, row-major, mapping destination to source.  Six tables of
 *     sequential running sums (compvhip_warp_tables): ac[0] = c, ac[i] = ac[i - 1] + a; df[0] = f, df[i] = df[i - 1] + d; gi[0] = M22,
 *     gi[i] = gi[i - 1] + g; by[0] = 0, by[j] = by[j - 1] + b; ey and hy likewise with e and h.  X = ac[i] + by[j], Y = df[i] + ey[j].
 *     2 x 3: x = X, y = Y.  3 x 3: Z = gi[i] + hy[j], s = 1.f / Z (correctly rounded IEEE division), x = X * s, y = Y * s: two multiplications
 *     by the reciprocal, not two divisions.  The running sums are the definition: a * i + c is a different number.
 * B. ROI {left, right, top, bottom}.  Remap: the caller's, clipped as compv_image_remap.cxx:348-354 does -- left to [0, Win - 1], right to
 *    [left, Win - 1], top to [0, Hin - 1], bottom to [top, Hin - 1] -- or, without one, the whole frame.  Inverse warp: always the whole frame.
 *    A pixel is INSIDE iff x >= left && x <= right && y >= top && y <= bottom (ordered compares: a NaN is outside).  An outside pixel gets
 *    defaultValue: the byte for uint8 output, (float)defaultValue for float32 output.
 * C. COMPVHIP_INTERP_NEAREST, inside: out = I[(int)((double)y + 0.5)][(int)((double)x + 0.5)].
 * D. COMPVHIP_INTERP_BILINEAR and _BILINEAR_FLOAT32, inside: x1 = (int)x, x2 = min((int)(x + 1.f), Win - 1), y1 = (int)y,
 *    y2 = min((int)(y + 1.f), Hin - 1) -- the neighbours clamp to the frame, not to the ROI; xf = x - (float)x1, yf = y - (float)y1, xy = xf * yf;
 *    A = ((1.f - xf) - yf) + xy, B = xf - xy, C = yf - xy, each operation rounded on its own;
 *    p = fma(I[y2][x2], xy, fma(I[y2][x1], C, fma(I[y1][x2], B, I[y1][x1] * A))) -- one product and three FUSED multiply-adds, which is what the
 *    reference's AVX2 leaf computes as its build contracts it.  uint8 output is (uint8)p by truncation (p lies in [0, 256)); float32 output is p.
 * E. Where this library differs from the reference:
 *  1. float32 output is the value of D for every pixel.  The reference's rows overwrite the last (j * Wout) % 8 values of the row before with
 *     values of other map entries when Wout % 8 != 0; that is not reproduced.
 *  2. Elements >= Wout of a destination row are never written.
 *  3. The reference picks a leaf without fused operations when the caller's map is not 32-byte aligned; this library always computes D.
 *  4. float64 maps and matrices and the forward CompVImage::warp are not provided: a caller inverts on the host.
 *  5. The reference's bicubic leaf tests `x < left || x > right || ...` and so takes a NaN coordinate for inside; this library keeps B for every
 *     interpolation: a NaN is outside.
 * F. Bicubic interpolation: COMPVHIP_INTERP_BICUBIC and _BICUBIC_FLOAT32, inside (compv_image_remap.cxx:293-310, compv_image_scale_bicubic.cxx:34-101).
 *    Every operation below is rounded on its own and nothing is fused.
 *  1. xi = (int)x, xf = x - floorf(x), xf2 = xf * xf, xf3 = xf2 * xf; yi, yf, yf2, yf3 likewise from y.  Taps x_k = clamp(xi - 1 + k, 0, Win - 1)
 *     and y_k = clamp(yi - 1 + k, 0, Hin - 1) for k = 0..3: they clamp to the frame, not to the ROI.
 *  2. Row r = 0..3, with A, B, C, D = (float)I[y_r][x_0], .. [x_3] (HERMITE4_32F_C): a = ((D - A) * 0.5f) + ((B - C) * 1.5f);
 *     b = ((A + (B * -2.5f)) + (C * 2.0f)) + (D * -0.5f); c = (C - A) * 0.5f; c_r = ((a * xf3) + (c * xf)) + ((b * xf2) + B).
 *  3. Column, with A, B, C, D = c_0 .. c_3 (HERMITE1_32F_C, a different association of the same polynomial):
 *     a = ((A * -0.5f) + (B * 1.5f)) + ((C * -1.5f) + (D * 0.5f)); b = (A + (B * -2.5f)) + ((C * 2.0f) + (D * -0.5f));
 *     c = (A * -0.5f) + (C * 0.5f); v = ((a * yf3) + (c * yf)) + ((b * yf2) + B).
 *  4. w = v < 0 ? 0 : (v > 255 ? 255 : v), by compares (COMPV_MATH_CLIP3): a zero keeps its sign.  uint8 output is (uint8)w by truncation
 *     (compv_math_cast.cxx:215); float32 output is w (CompVMathClip::clip3).
 *  5. The parity target is the reference with every SIMD CPU flag switched off, its plain leaves, which tests/golden/make_golden_bicubic.py holds
 *     tests/bicubic_model.py against on every element; how far the reference's SIMD build departs from them is recorded in the fixture
 *     (docs/kernels/remap.md) and asserted nowhere.
 * Refused with COMPVHIP_E_INVALID_PARAMETER, the destination untouched: a null pointer; a size of 0 or beyond 32767; Sout < Wout (for float32
 * output Sout counts ELEMENTS); rows other than 2 or 3; a count other than 1 or the plan's frames; an unknown interpolation; a float32
 * destination that is not 4-byte aligned; source and destination that overlap. */
#define COMPVHIP_INTERP_NEAREST 0
#define COMPVHIP_INTERP_BILINEAR 1
#define COMPVHIP_INTERP_BILINEAR_FLOAT32 2          /* bilinear, float32 destination */
#define COMPVHIP_INTERP_BICUBIC 4                   /* bicubic, uint8 destination (3 is unassigned and refused) */
#define COMPVHIP_INTERP_BICUBIC_FLOAT32 5           /* bicubic, float32 destination */
typedef struct compvhip_roi { float left, right, top, bottom; } compvhip_roi;
/* A.2 on the host, no context: the tables of one matrix (rows = 2: gi and hy may be NULL and are not written).  ac, df, gi: Wout values; by, ey,
 * hy: Hout values. */
COMPVHIP_API int compvhip_warp_tables(const float* M, int rows, size_t Wout, size_t Hout, float* ac, float* df, float* gi, float* by, float* ey, float* hy);
/* Remap for every frame of a plan: d_in [frames][H][S] of the plan's geometry -> d_out [frames][Hout][Sout], uint8 or (the two _FLOAT32
 * interpolations) float32.  d_mapX, d_mapY: device, [mapCount][Hout * Wout] float32 each; mapCount == 1: all frames share the map (a workgroup then reads its part of
 * the map once for 8 frames); mapCount == frames: one map per frame.  roi == NULL: the whole frame.  A destination that is aligned in pointer, stride
 * and frame size (4 bytes for uint8, 16 for float32) is written with vector stores.  Asynchronous on `stream`, never synchronises the host.
 * Beyond 65 535 frames (shared map: beyond 65 535 groups of 8): SLICED.  d_in: ANY BYTE; d_mapX and d_mapY: 4-byte aligned; d_out: ANY BYTE for uint8, 4-byte
 * aligned for float32.  Stream order: ASYNC. */
COMPVHIP_API int compvhip_plan_remap(compvhip_plan* plan, const uint8_t* d_in, const float* d_mapX, const float* d_mapY, size_t mapCount, int interp,
                                     const compvhip_roi* roi, uint8_t defaultValue, void* d_out, size_t Wout, size_t Hout, size_t Sout, void* stream);
/* Inverse warp for every frame of a plan.  M: HOST, [matrixCount][rows][3] float32, rows 2 or 3; matrixCount 1 or frames.  The tables of A.2 are
 * built on the host into pinned staging owned by the plan and uploaded in stream order; M may be reused as soon as the call returns.  Asynchronous
 * on `stream`: the host waits only when 4 earlier uploads of the plan are all still pending.  Timing entries (compvhip_plan_set_timing):
 * remap_kernel, warp_inverse_kernel.  Beyond 65 535 frames: SLICED, like compvhip_plan_remap.  d_in: ANY BYTE; d_out: ANY BYTE for uint8, 4-byte aligned for
 * float32.  Stream order: ASYNC, with one exception: M is staged in a ring of 4 pinned slots, so a call may wait for the copy of the call four before it (never for more).  M may be changed as soon as the call has returned. */
COMPVHIP_API int compvhip_plan_warp_inverse(compvhip_plan* plan, const uint8_t* d_in, const float* M, int rows, size_t matrixCount, int interp,
                                            uint8_t defaultValue, void* d_out, size_t Wout, size_t Hout, size_t Sout, void* stream);
/* Both for one HOST plane (sizes 1 .. 32767) with host maps / a host matrix; S and Sout in elements.  Synchronous. */
COMPVHIP_API int compvhip_remap_u8(compvhip_ctx* ctx, const uint8_t* in, size_t W, size_t H, size_t S, const float* mapX, const float* mapY, int interp,
                                   const compvhip_roi* roi, uint8_t defaultValue, void* out, size_t Wout, size_t Hout, size_t Sout);
COMPVHIP_API int compvhip_warp_inverse_u8(compvhip_ctx* ctx, const uint8_t* in, size_t W, size_t H, size_t S, const float* M, int rows, int interp,
                                          uint8_t defaultValue, void* out, size_t Wout, size_t Hout, size_t Sout);

/* ---- RANSAC homography (docs/kernels/homography.md) -----------------------------------------------------------------------------------------
 * CompVHomography<double>::find (core/calib/compv_core_calib_homography.cxx:60-551) followed by CompVMathTransform::perspective2D, for `pairs`
 * point sets at once, on the device: the step between compvhip_matcher_good and the 3 x 3 matrix compvhip_plan_warp_inverse consumes.  All
 * arithmetic is IEEE binary64, one rounding per operation (no fused multiply-add), divisions and square roots correctly rounded, no transcendental
 * function: tests/homography_model.py is the same definition in numpy and equals the device bit for bit.  Two departures from the reference, both
 * deliberate: its random quads (std::random_device) are replaced by a counter hash, so a result is a function of the inputs; and its adaptive early
 * exit (:318-331, a CPU time saver) is NOT reproduced -- all `tries` tries run.
 * A pair has k correspondences src[i] -> dst[i] (src = the train side, dst = the query side, as samples/object_recognition passes them), either
 *  - gathered by compvhip_homography_points from a good list: n = min(max(goodCount, 0), goodCap, pointCap) records are read; record r gives
 *    src = (double)train[trainIdx].xy, dst = (double)query[queryIdx].xy; a record with queryIdx outside [0, queryCap) or trainIdx outside
 *    [0, trainCap) is dropped, the others keep their order; k = the number kept; or
 *  - given directly: two [pairs][pointCap] arrays of {x, y} float64 and d_counts, k = min(max(count, 0), pointCap) (d_counts == NULL: pointCap).
 * A. Quads.  The four indices of pair p, try t, in uint32 wrap-around arithmetic: lowbias32(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15;
 *    x *= 0x846ca68b; x ^= x >> 16.  u(c) = lowbias32(lowbias32(lowbias32(seed ^ p) + t) + c), c = 0, 1, 2, ...; idx = ((uint64)u * k) >> 32.  Slots
 *    0..3 fill in order; a draw equal to an earlier slot of the try is discarded; when c reaches 64 with slots open they take the smallest unused
 *    indices in ascending order.  d_quads ([pairs][tries][4] int32) replaces the generator; a quad with an index outside [0, k) scores 0.
 *    compvhip_homography_quads is the same function on the host.
 * B. Collinearity of the quad's src points (:284-298): x0 == x1 ? (x0 == x2 && x0 == x3) : with slope = (y1 - y0) / (x1 - x0) and
 *    intercept = y0 - slope * x0, y2 == slope * x2 + intercept && y3 == slope * x3 + intercept.  A collinear try scores 0.
 * C. computeH(N points) (:346-495).  Per side the Hartley normalisation: t = (sum x, sum y) * (1 / N); mean = (sum sqrt(a * a + b * b)) * (1 / N) with
 *    a = x - tx, b = y - ty; s = sqrt(2) / mean, or sqrt(2) when mean == 0; xn = s * x + (-(tx * s)).  Per point two rows of M
 *    (compv_math_matrix.cxx:828-850): {-x, -y, -1, 0, 0, 0, X * x, X * y, X} and {0, 0, 0, -x, -y, -1, Y * x, Y * y, Y} with (x, y) = src, (X, Y) = dst
 *    normalised.  S = MtM: entry (a, b) is the sum, over the points, of row0[a] * row0[b] and then row1[a] * row1[b], two additions per point.
 *    Sums over N == 4 points run in index order from 0.0.  Sums over N > 4 points are sum64: point i adds to partial i mod 64 in ascending i, and
 *    the partials fold with p[l] += p[l + stride] for stride 32, 16, ..., 1.
 * D. Jacobi on D = S with Qt = I (compv_math_eigen.cxx).  Pivot: the largest |D[r][c]| over r > c, scanned in ascending r then c, the first
 *    maximum wins.  Rotate while it is > 2^-52, at most 2430 times.  The angle theta = atan2(2 D[r][c], D[c][c] - D[r][r]) / 2 of :377-393, taken
 *    algebraically: D[r][r] == D[c][c]: cos = sin = 0.70710678118654757; else y = 2 D[r][c], x = D[c][c] - D[r][r], rho = sqrt(x * x + y * y),
 *    c2 = x / rho, s2 = y / rho; c2 >= 0: cos = sqrt((1 + c2) * 0.5), sin = s2 / (2 cos); else sin = copysign(sqrt((1 - c2) * 0.5), s2) (a zero s2
 *    counts as positive), cos = s2 / (2 sin).  mulGA(A, r, c, cos, -sin) (compv_math_matrix.cxx:339-345: ai = ri * cos + (-sin) * rj,
 *    aj = ri * sin + cos * rj) on the rows r, c of Qt, then of D, then -- the same formula on the elements -- on the columns r, c of D.  h = the row
 *    of Qt at the smallest diagonal entry of D, scanning from index 8 downwards with strict <.  De-normalisation (:446-469): M = T1 * Hn^t,
 *    H = T2 * M^t with T1 = {s, 0, 0; 0, s, 0; -tx s, -ty s, 1} of src, T2 = {1 / s, 0, tx; 0, 1 / s, ty; 0, 0, 1} of dst, every entry a three-term dot
 *    product (a0 b0 + a1 b1) + a2 b2.  With promotion, |h| <= 2^-52 becomes 0 on the first eight entries.  H *= 1 / h22 when h22 != 0.
 * E. Score of a try: H = computeH(the quad, no promotion); the inverse by the C formula of compv_math_matrix.cxx:520-544, a determinant of
 *    exactly 0 scoring 0; d_i = mse(H src_i, dst_i) + mse(H^-1 dst_i, src_i) with mse of compv_math_stats.cxx:200-203 (X, Y, Z three-term dot
 *    products with z = 1; scale = 1 / Z; ex = X * scale - bx; ey likewise; ex * ex + ey * ey); inlier iff d_i < threshold; count = the inliers;
 *    mean = sum / count and variance = sum (d - mean)^2 / (count - 1), both sums over the inliers in index order; variance = DBL_MAX when
 *    count < 2.  A try that scores 0 has count 0 and variance DBL_MAX.
 * F. Selection over all tries: count >= 4, then the largest count, then the smallest variance, then the smallest t.
 * G. Result: a best exists: status 0, H = computeH(the inliers of the best try in index order, promotion on), inliers = its count, variance and
 *    bestTry its; none and k >= 4: status 1, H = computeH(all k points, promotion on) (:141-145), inliers 0; k < 4: status 2, H zeros, inliers 0.
 *    status != 0: variance = DBL_MAX, bestTry = -1.  rotations = the Jacobi rotations of that last computeH.  The mask, [pairs][pointCap] bytes:
 *    1 for an inlier of the best try, else 0, for i < k; bytes at and after k are never written.
 * H. Projection (compv_math_transform.cxx:99-104): X, Y, Z three-term dot products, s = 1 / Z, (X * s, Y * s). */
typedef struct compvhip_homography_opts {
	int32_t tries;              /* 1 .. maxTries */
	uint32_t seed;
	double threshold;           /* > 0; the reference's is 30 */
} compvhip_homography_opts;
typedef struct compvhip_homography_result {
	double H[9];
	double variance;
	int32_t inliers, bestTry, status, rotations;
} compvhip_homography_result;
typedef struct compvhip_homography compvhip_homography;   /* scratch for `pairs` pairs of at most pointCap points and maxTries tries; not tied to an image geometry */

/* pairs, maxTries >= 1, pointCap >= 4 (anything else: COMPVHIP_E_INVALID_PARAMETER).  All scratch is allocated here -- per pair 4 * pointCap {x, y}
 * float64 (gathered and selected points) and a count, per pair and try 19 float64 and 3 int32 -- and released by compvhip_homography_destroy: no
 * later call allocates or synchronises (the two host forms excepted).  Destroy it BEFORE its context.  Not re-entrant: its calls share the scratch
 * and must be ordered on one stream.  More than 65 535 pairs: REFUSED. */
COMPVHIP_API int compvhip_homography_create(compvhip_ctx* ctx, size_t pairs, size_t pointCap, size_t maxTries, compvhip_homography** homography);
COMPVHIP_API void compvhip_homography_destroy(compvhip_homography* homography);
/* Gathers the pairs' points into the handle.  d_good: [pairs][goodCap] records, 16-byte aligned; d_goodCounts: [pairs] int32 or NULL (every pair
 * full); d_query: [pairs][queryCap] keypoints; d_train: [pairs][trainCap], or ONE set [trainCap] with trainShared != 0; 4-byte aligned.
 * Asynchronous on `stream`.  Stream order: ASYNC. */
COMPVHIP_API int compvhip_homography_points(compvhip_homography* homography, const compvhip_match* d_good, size_t goodCap, const int32_t* d_goodCounts,
                                            const compvhip_keypoint* d_query, size_t queryCap, const compvhip_keypoint* d_train, size_t trainCap,
                                            int trainShared, void* stream);
/* d_src, d_dst: [pairs][pointCap] {x, y} float64, 16-byte aligned, with d_counts; d_src == NULL: the points compvhip_homography_points gathered
 * (d_dst and d_counts are then ignored).  d_quads: NULL or [pairs][opts->tries][4] int32, 16-byte aligned.  d_results: [pairs] records, 8-byte
 * aligned; d_counts 4-byte aligned.  d_mask: NULL or [pairs][pointCap] bytes, ANY BYTE.  A null handle, opts or d_results, tries < 1 or > maxTries, a threshold that is not > 0, a
 * misaligned pointer: COMPVHIP_E_INVALID_PARAMETER, nothing written.  Asynchronous on `stream`; deterministic run to run.  Stream order: ASYNC. */
COMPVHIP_API int compvhip_homography_find(compvhip_homography* homography, const double* d_src, const double* d_dst, const int32_t* d_counts,
                                          const compvhip_homography_opts* opts, const int32_t* d_quads, compvhip_homography_result* d_results,
                                          uint8_t* d_mask, void* stream);
/* Sends n points through each pair's H.  d_points: [pairs][n] {x, y} float64, or ONE set [n] with shared != 0 (the train rectangle of the sample);
 * d_out: [pairs][n]; both 16-byte aligned.  A pair of status 2 (H zeros) yields NaN.  Asynchronous on `stream`.  Stream order: ASYNC. */
COMPVHIP_API int compvhip_homography_project(compvhip_homography* homography, const compvhip_homography_result* d_results, const double* d_points,
                                             size_t n, int shared, double* d_out, void* stream);
/* Item A on the host (standard library only, no GPU): quads[tries][4] of pair `pair` among k >= 4 points. */
COMPVHIP_API int compvhip_homography_quads(uint32_t seed, size_t pair, size_t k, size_t tries, int32_t* quads);
/* The whole call for one HOST pair of n points ({x, y} float64 each; n may be below 4: status 2).  quads: NULL or [opts->tries][4]; mask: NULL or n
 * bytes.  Synchronous; allocates and frees its own scratch. */
COMPVHIP_API int compvhip_homography_find_f64(compvhip_ctx* ctx, const double* src, const double* dst, size_t n, const compvhip_homography_opts* opts,
                                              const int32_t* quads, compvhip_homography_result* result, uint8_t* mask);
/* Test hook: what the last compvhip_homography_find left in the score scratch, copied to HOST arrays of [pairs][tries] (NULL: not wanted) --
 * per try the inlier count, the variance and the Jacobi rotations of its computeH.  Entries of a pair with k < 4 are not defined.  Synchronises
 * `stream`.  Stream order: WAITS: the arrays are the host's, the call returns when they are filled. */
COMPVHIP_API int compvhip_homography_scores(compvhip_homography* homography, size_t tries, int32_t* counts, double* variances, int32_t* rotations,
                                            void* stream);
/* Per-kernel timing of the handle's last call, as compvhip_matcher_set_timing / _get_timing: entries homography_points_kernel;
 * homography_solve_kernel, homography_score_kernel, homography_refit_kernel; homography_project_kernel. */
COMPVHIP_API int compvhip_homography_set_timing(compvhip_homography* homography, int enabled);
COMPVHIP_API int compvhip_homography_get_timing(compvhip_homography* homography, const char** names, float* ms, int cap);

/* ---- RANSAC curve fitting: lines and parabolas (docs/kernels/curvefit.md) -------------------------------------------------------------------
 * CompVMathStatsFit::line and ::parabola (base/math/compv_math_stats_fit.cxx) on CompVMathStatsRansac and CompVMathDistance::line / ::parabola, for
 * `sets` point sets at once, on the device: the step behind compvhip_plan_components that turns a component's pixels into a curve without downloading
 * them.  The sibling of the RANSAC homography above, with the same two departures from the reference: the random samples are a counter hash, so a
 * result is a function of the inputs, and the adaptive early exit (compv_math_stats_ransac.cxx:240-254, a CPU time saver) is NOT reproduced -- all
 * `tries` tries run.  All arithmetic is IEEE binary64, one rounding per operation (no fused multiply-add), divisions and square roots correctly
 * rounded, no transcendental function: compv_amd/csrc/curvefit_math.hpp is the arithmetic, tests/curvefit_model.py the same definition in numpy, and
 * the device equals both bit for bit.
 * A set has k points {x, y} float64, either given as [sets][pointCap] with d_counts (k = min(max(count, 0), pointCap); d_counts == NULL: pointCap) or
 * gathered by compvhip_curvefit_points_from_labels (item G).  Models: LINE, m = 2, Ax + By + C = 0; PARABOLA, m = 3, y = Ax^2 + Bx + C;
 * PARABOLA_SIDEWAYS, the same with the roles of x and y exchanged everywhere (compv_math_stats_fit.cxx:246-248, compv_math_distance.cxx:360-362).
 * A. Samples.  The generator of homography item A with m slots instead of four (one function, hg::drawDistinct, serves both): u(c) =
 *    lowbias32(lowbias32(lowbias32(seed ^ set) + t) + c), idx = ((uint64)u * k) >> 32, duplicates discarded, the smallest unused indices from c = 64.
 *    d_samples ([sets][tries][m] int32) replaces the generator; a sample with an index outside [0, k) scores 0.  compvhip_curvefit_samples is the
 *    same function on the host.
 * B. Model of a sample (:156-168, :252-266), every expression evaluated left to right as the reference writes it.  Line: rejected when x0 == x1 &&
 *    y0 == y1; A = y1 - y0, B = x0 - x1, C = (x1 * y0) - (x0 * y1).  Parabola: rejected when two of the three x are equal;
 *    scale = 1 / ((x1 - x2) * (x1 - x3) * (x2 - x3)); A = (x3 * (y2 - y1) + x2 * (y1 - y3) + x1 * (y3 - y2)) * scale;
 *    B = (x3 * x3 * (y1 - y2) + x2 * x2 * (y3 - y1) + x1 * x1 * (y2 - y3)) * scale;
 *    C = (x2 * x3 * (x2 - x3) * y1 + x3 * x1 * (x3 - x1) * y2 + x1 * x2 * (x1 - x2) * y3) * scale, in C's precedence.  A rejected try scores 0.
 * C. Residual (compv_math_distance.cxx:263-268, :242, :343).  Line: s = 1 / sqrt(A * A + B * B); d = |((A * s) * x + (C * s)) + (B * s) * y| (A = B = 0,
 *    which the reference refuses, gives NaN).  Parabola: d = |(((A * (x * x)) + C) + (B * x)) - y|.  Inlier iff d < threshold, strict
 *    (ransac.cxx:233); a NaN is never an inlier.
 * D. The score of a try is its inlier count.  The best try has the largest count, then the smallest t (ransac.cxx:235); a best exists only when
 *    its count is >= m.
 * E. Refit on the inliers of the best try, n of them, in index order (ransac.cxx:117-142).  n == m: the formula of B on them.  Sums over n > m points
 *    are sum64 as in homography item C; mean = sum * (1 / n).  Line, total least squares (:176-209): a = x - mean_x, b = y - mean_y;
 *    num = (sum a * b) * -2; den = sum (b * b - a * a); num == 0 && den == 0: (cos, sin) = (1, 0); else phi = atan2(num, den) / 2 by the half-angle
 *    formulas of homography item D with y = num, x = den (within 2.3e-16 of libm over 20 000 random (num, den)); A = cos, B = sin,
 *    C = -((mean_x * cos) + (mean_y * sin)).  Parabola: the reference runs Levenberg-Marquardt (lmmin) on this LINEAR problem; the definition is the
 *    least-squares solution itself: u = x - mean; S1..S4 = sum u, u * u, (u * u) * u, (u * u) * (u * u); T0..T2 = sum y, u * y, (u * u) * y; the
 *    symmetric system {S4, S3, S2; S3, S2, S1; S2, S1, n} (a, b, c) = (T2, T1, T0) by cofactors, one division by the determinant per unknown
 *    (parabolaFromSums of curvefit_math.hpp is the expression order); A = a, B = b - (2 * a) * mean, C = (c - b * mean) + a * (mean * mean).  A
 *    determinant that is 0 or not finite, or a rejected m-point formula: the refit fails.
 * F. Record.  status 0: a best exists and the refit succeeded: the refit's A, B, C, the best try's inliers and bestTry.  status 3: a best exists,
 *    the refit failed: the best try's own model (item B, unscaled).  status 1: k >= m but no best: zeros, as the reference returns (:79-85),
 *    bestTry -1.  status 2: k < m: zeros, bestTry -1.  k == m: the sample is the points 0 .. m - 1, no generator, no refit (:53-65, :101-114):
 *    status 0 with inliers = m and bestTry 0, or status 1 when rejected.  Mask, [sets][pointCap] bytes: 1 for an inlier of the best try, else 0, for
 *    i < k (k == m: all 1, or all 0 when rejected); bytes at and behind k are never written.
 * G. Gather from a label map: the inputs are what compvhip_plan_components wrote.  Component id of frame f becomes set f * compCap + id - 1 for
 *    id <= min(max(count, 0), compCap); the other sets get k = 0.  The pixels carrying the id inside the record's box (clipped to the frame) get ranks
 *    0, 1, ... in raster order; step = ceil(pixels / pointCap) with the record's pixel count; a pixel is taken iff rank % step == 0 and becomes point
 *    rank / step = ((double)x, (double)y); k = ceil(ranked pixels / step), at most pointCap.
 * Streams.  A handle takes its stream at creation (the descriptor), not as a `void* stream` parameter of every call: its calls share the scratch and
 *    must be ordered on one stream anyway (as the homography handle demands), and the table of per-call stream classes above
 *    (tests/stream_cases.py) lists the exports that take such a parameter.  Every device call of the family is ASYNC in that table's sense on the
 *    handle's stream; compvhip_curvefit_scores and compvhip_curvefit_find_f64 WAIT.
 * Alignment.  Points and samples: 16 bytes.  Results, params and distances: 8 bytes.  Counts, labels and component records: 4 bytes.  Mask: any byte.
 *    A misaligned pointer is refused with COMPVHIP_E_INVALID_PARAMETER and nothing is written. */
enum {
	COMPVHIP_CURVEFIT_LINE = 0,
	COMPVHIP_CURVEFIT_PARABOLA = 1,            /* COMPV_MATH_PARABOLA_TYPE_REGULAR */
	COMPVHIP_CURVEFIT_PARABOLA_SIDEWAYS = 2    /* COMPV_MATH_PARABOLA_TYPE_SIDEWAYS */
};
typedef struct compvhip_curvefit_desc {
	uint32_t size;              /* sizeof(compvhip_curvefit_desc) */
	uint32_t sets;              /* 1 .. 65 535 */
	uint32_t pointCap;          /* >= 3 */
	uint32_t maxTries;          /* >= 1 */
	void* stream;               /* a hipStream_t; NULL = the default stream */
} compvhip_curvefit_desc;
typedef struct compvhip_curvefit_opts {
	uint32_t size;              /* sizeof(compvhip_curvefit_opts) */
	int32_t model;              /* COMPVHIP_CURVEFIT_* */
	int32_t tries;              /* 1 .. maxTries */
	uint32_t seed;
	double threshold;           /* > 0 */
} compvhip_curvefit_opts;
typedef struct compvhip_curvefit_result {
	double A, B, C;
	int32_t inliers, bestTry, status, k;
} compvhip_curvefit_result;
typedef struct compvhip_curvefit compvhip_curvefit;   /* scratch for `sets` sets of at most pointCap points and maxTries tries */

/* All scratch is allocated here -- per set 2 * pointCap {x, y} float64 (gathered and selected points), a count and maxTries int32 -- and released by
 * compvhip_curvefit_destroy: no later call allocates (the host form excepted).  Destroy it BEFORE its context.  Not re-entrant.  A null pointer, a wrong
 * size field, sets outside 1 .. 65 535, pointCap < 3 or maxTries < 1 (either beyond 2^22): COMPVHIP_E_INVALID_PARAMETER. */
COMPVHIP_API int compvhip_curvefit_create(compvhip_ctx* ctx, const compvhip_curvefit_desc* desc, compvhip_curvefit** fit);
COMPVHIP_API void compvhip_curvefit_destroy(compvhip_curvefit* fit);
/* Item G.  d_labels: int32 [frames][H][labelStride], labelStride >= W; d_comps: [frames][compCap]; d_compCounts: [frames]; all 4-byte aligned.
 * frames * compCap must equal the handle's sets; 1 <= W, H <= 32767.  Asynchronous on the handle's stream. */
COMPVHIP_API int compvhip_curvefit_points_from_labels(compvhip_curvefit* fit, const int32_t* d_labels, size_t W, size_t H, size_t labelStride,
                                                      const compvhip_component* d_comps, size_t compCap, const int32_t* d_compCounts, size_t frames);
/* d_points: [sets][pointCap] {x, y} float64, 16-byte aligned, with d_counts ([sets] int32, 4-byte aligned, or NULL); d_points == NULL: the gathered
 * points (d_counts is then ignored; COMPVHIP_E_INVALID_STATE when nothing was gathered).  d_samples: NULL or [sets][opts->tries][m] int32, 16-byte
 * aligned.  d_results: [sets] records, 8-byte aligned.  d_mask: NULL or [sets][pointCap] bytes, ANY BYTE.  A null handle, opts or d_results, a wrong
 * size field, an unknown model, tries < 1 or > maxTries, a threshold that is not > 0, a misaligned pointer: COMPVHIP_E_INVALID_PARAMETER, nothing
 * written.  Asynchronous on the handle's stream; deterministic run to run. */
COMPVHIP_API int compvhip_curvefit_find(compvhip_curvefit* fit, const double* d_points, const int32_t* d_counts, const compvhip_curvefit_opts* opts,
                                        const int32_t* d_samples, compvhip_curvefit_result* d_results, uint8_t* d_mask);
/* Item C alone -- CompVMathDistance::line / ::parabola: d_out[set][i] = the residual of point i under d_params[set] = {A, B, C}, for i < k; elements
 * at and behind k are not written.  d_points as in find (NULL: the gathered points); d_params [sets][3] and d_out [sets][pointCap] float64, 8-byte
 * aligned.  Asynchronous on the handle's stream. */
COMPVHIP_API int compvhip_curvefit_distances(compvhip_curvefit* fit, const double* d_points, const int32_t* d_counts, int model, const double* d_params,
                                             double* d_out);
/* Test hook: the inlier count of every try the last compvhip_curvefit_find left in the scratch, copied to the HOST array counts[sets][tries], and the
 * gathered sets' point counts to the HOST array gathered[sets] (either may be NULL).  Entries of a set with k <= m are not defined.  Waits for the
 * handle's stream. */
COMPVHIP_API int compvhip_curvefit_scores(compvhip_curvefit* fit, size_t tries, int32_t* counts, int32_t* gathered);
/* The gathered points as the device sees them: *d_points receives the device address of [sets][pointCap] {x, y} float64, *d_counts that of [sets]
 * int32 (HOST pointers that receive device addresses; either may be NULL). */
COMPVHIP_API int compvhip_curvefit_gathered(compvhip_curvefit* fit, const double** d_points, const int32_t** d_counts);
/* Per-kernel timing of the handle's last call, as compvhip_matcher_set_timing / _get_timing: entries curvefit_gather_kernel; curvefit_score_kernel,
 * curvefit_refit_kernel; curvefit_distance_kernel. */
COMPVHIP_API int compvhip_curvefit_set_timing(compvhip_curvefit* fit, int enabled);
COMPVHIP_API int compvhip_curvefit_get_timing(compvhip_curvefit* fit, const char** names, float* ms, int cap);
/* Item A on the host (standard library only, no GPU): samples[tries][m] of set `set` among k > m points. */
COMPVHIP_API int compvhip_curvefit_samples(int model, uint32_t seed, size_t set, size_t k, size_t tries, int32_t* samples);
/* The whole call for one HOST set of n points ({x, y} float64 each; n may be below m: status 2).  samples: NULL or [opts->tries][m]; mask: NULL or n
 * bytes.  Synchronous on the context's stream; allocates and frees its own scratch. */
COMPVHIP_API int compvhip_curvefit_find_f64(compvhip_ctx* ctx, const double* points, size_t n, const compvhip_curvefit_opts* opts, const int32_t* samples,
                                            compvhip_curvefit_result* result, uint8_t* mask);

/* ---- HOG descriptors (docs/kernels/hog.md) --------------------------------------------------------------------------------------------------
 * CompVHogStd::process (core/features/hog/compv_core_feature_hog_std.cxx; COMPV_HOGS_ID) on gray frames: per-cell orientation histograms, then the
 * blocks' normalised vectors.  Every output is defined bit for bit.  All arithmetic is float32 with one rounding per operation; the divide and the
 * square root are the correctly rounded ones; nothing is flushed to zero.  This is the reference with its AVX2 + FMA3 leaf switched off: compiled with
 * -mfma, that leaf's two sub(mul()) expressions (..._hog_std_intrin_avx2.cxx:54-55) are contracted and the last bits differ (its unit test carries an
 * md5 and an md5_fma column for this; the uncontracted one is canonical here).  For a frame I of W x H:
 *  1. Gradient (base/compv_gradient_fast.cxx:111-162, 266-314): gx = I(x + 1, y) - I(x - 1, y), 0 in columns 0 and W - 1; gy = I(x, y + 1) - I(x, y - 1),
 *     0 in rows 0 and H - 1.  Exact integers as float32.
 *  2. Magnitude (base/math/compv_math_trig.cxx:497-509): m = sqrt(gx * gx + gy * gy).
 *  3. Direction in degrees (:412-447, constants at compv_math.cxx:39-43): ax = |gx|, ay = |gy|; ax >= ay: c = ay / (ax + eps),
 *     a = (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c with c2 = c * c; otherwise c = ax / (ay + eps) and a = 90 - that polynomial.  gx < 0: a = 180 - a;
 *     then gy < 0: a = 360 - a.  eps = (float)2.2204460492503131e-16, p1 = 57.2836266f, p3 = -18.6674461f, p5 = 8.91400051f, p7 = -2.53972459f.
 *  4. Binning (hog_std.cxx:564-632, 715-743): thetaMax = 360 (signed) or 180; theta = a - thetaMax when a > thetaMax, else a; w = thetaMax / nbins,
 *     s = 1.f / w.  The pixels of a cell are walked row-major, each adding to the cell's histogram h:
 *     NEAREST: b = (int)(theta * s); h[b] += m; a vote with b == nbins (theta == thetaMax: every pixel with gy == 0 and gx < 0 of an unsigned
 *     gradient) is DROPPED (the reference writes it behind its histogram, into a float it clears afterwards).
 *     BILINEAR: b = (int)(theta * s - 0.5f); d = (theta - (float)b * w) * s - 0.5f; v = |m * d|; the other bin is b + 1 when d >= 0, else b - 1, wrapped
 *     into 0 .. nbins - 1; FIRST h[other] += v, THEN h[b] += m - v.  The order is part of the result.
 *  5. Cell grid (:238-261): cell origins step by the block stride.  cellsX = (int)((float)(W / cellW) / ((float)strideW / (float)cellW)); the last column is
 *     LEFT OUT when (cellsX - 1) * strideW + cellW > W; the same in y.  A left-out cell of the map holds 0 (the reference leaves it unwritten); no block
 *     reads one.
 *  6. Blocks (:318-376, 429-457): blocksX = (W - blockW) / strideW + 1, likewise in y.  Block (bx, by) takes, for each of its blockH / cellH cell rows,
 *     the blockW / cellW adjacent map cells from index bx * round(strideW / cellW) of map row by * round(strideH / cellH) + row (round(x) = (int)(x + 0.5)).  Blocks
 *     are stored row-major; inside a block: cell row, then cell, then bin.  descLen = blocksX * blocksY * count, count the floats of a block.
 *  7. Norms (intrin/x86/compv_core_feature_hog_common_norm_intrin_sse2.cxx), one summation order for any count: two 4-lane accumulators are fed 8 terms
 *     at a time (lane l of the first takes terms 8k + l, of the second 8k + 4 + l); one more group of 4 goes to the first if it fits; then
 *     acc0 + acc1, then (l0 + l2) + (l1 + l3), then the remaining terms one by one, then + eps (1e-6f for L1 and L1SQRT, 1e-6f * 1e-6f for L2 and
 *     L2HYS).  L1, L1SQRT: terms v, r = 1.f / sum; L2, L2HYS: terms v * v, r = 1.f / sqrt(sum).  Result v * r; sqrt(v * r) for L1SQRT; L2HYS is L2, then
 *     min(., 0.2f), then L2 again.  NONE copies the cells.  (The reference's _9 variants are the same arithmetic.)
 *  8. Accepted parameters.  block % cell == 0; per axis EITHER stride == cell OR 2 * stride == cell together with block == cell (the default shape and the
 *     reference's unit-test shape; for any other mix the reference pairs map cells `stride` apart as if they were `cell` apart); 2 <= nbins <= 360 and
 *     nbins divides thetaMax (otherwise the reference indexes outside its histogram); blockW <= W <= 32767, blockH <= H <= 32767; interpolation NEAREST
 *     or BILINEAR (BILINEAR_LUT is refused: the reference itself calls it "not faster"); count and the floats of a frame's map and descriptor below 2^31.
 *     One resource limit: a cell so wide that three of its rows and the histogram (nbins * 256 bytes) exceed the 160 KB of LDS (cellW beyond 22 000 at
 *     360 bins).  Anything else: COMPVHIP_E_INVALID_PARAMETER, and nothing is written. */
enum { COMPVHIP_HOG_NORM_DEFAULT = 0 /* L2HYS */, COMPVHIP_HOG_NORM_NONE = 1, COMPVHIP_HOG_NORM_L1 = 2, COMPVHIP_HOG_NORM_L1SQRT = 3, COMPVHIP_HOG_NORM_L2 = 4,
       COMPVHIP_HOG_NORM_L2HYS = 5 };                      /* COMPV_HOG_BLOCK_NORM_* (compv_features.h:113-117) */
enum { COMPVHIP_HOG_GRADIENT_DEFAULT = 0 /* signed */, COMPVHIP_HOG_GRADIENT_SIGNED = 1, COMPVHIP_HOG_GRADIENT_UNSIGNED = 2 };
enum { COMPVHIP_HOG_INTERP_DEFAULT = 0 /* BILINEAR */, COMPVHIP_HOG_INTERP_NEAREST = 1, COMPVHIP_HOG_INTERP_BILINEAR = 2,
       COMPVHIP_HOG_INTERP_BILINEAR_LUT = 3 /* refused */ };   /* COMPV_HOG_INTERPOLATION_* (compv_features.h:118-120) */
/* Zero-initialise, set `size` = sizeof(compvhip_hog_opts) and what is needed: a zero field takes the reference's default (hog_std.cxx:459-467) -- block 16 x 16,
 * stride 8 x 8, cell 8 x 8, 9 bins, L2HYS, signed, BILINEAR.  Another `size`, or a negative field: COMPVHIP_E_INVALID_PARAMETER. */
typedef struct compvhip_hog_opts {
	uint32_t size;
	int32_t blockW, blockH, strideW, strideH, cellW, cellH, nbins;
	int32_t blockNorm;          /* COMPVHIP_HOG_NORM_* */
	int32_t gradientSigned;     /* COMPVHIP_HOG_GRADIENT_* */
	int32_t interp;             /* COMPVHIP_HOG_INTERP_* */
} compvhip_hog_opts;

/* Items 5, 6 and 8 on the host (no GPU): the map's cells (left-out ones included), the blocks and the descriptor's length in floats of a W x H frame.  Any
 * of the five outputs may be NULL.  Returns what the device calls return for the same W, H and opts. */
COMPVHIP_API int compvhip_hog_geometry(size_t W, size_t H, const compvhip_hog_opts* opts, size_t* cellsX, size_t* cellsY, size_t* blocksX, size_t* blocksY,
                                       size_t* descLen);

/* Descriptors of all frames of the plan.  d_gray: [frames][H][S], ANY BYTE; d_desc: [frames][descStride] float32, descStride >= descLen counted in floats, the floats
 * behind descLen are never written; d_cells: NULL or the cell map [frames][cellsY][cellsX][nbins] float32; d_desc and d_cells 4-byte aligned.  A batch of
 * crops is a plan of the crop's size with one frame per crop.  Asynchronous on `stream`, no atomic, deterministic.  Scratch is owned by the plan, allocated on
 * first use with d_cells == NULL and released with it: one cell map.  Like every plan call it is not re-entrant.  Beyond 65 535 frames: SLICED.  Stream order: ASYNC. */
COMPVHIP_API int compvhip_plan_hog(compvhip_plan* plan, const uint8_t* d_gray, const compvhip_hog_opts* opts, float* d_cells, float* d_desc, size_t descStride,
                                   void* stream);

/* The same for one HOST frame (3 <= W, H).  Synchronous, on the context's cached single-frame plan.  *n receives descLen; with cap < descLen nothing is
 * computed or written and COMPVHIP_E_OUT_OF_BOUND is returned (cap == 0 with desc == NULL asks for the length). */
COMPVHIP_API int compvhip_hog_u8(compvhip_ctx* ctx, const uint8_t* gray, size_t W, size_t H, size_t S, const compvhip_hog_opts* opts, float* desc, size_t cap,
                                 size_t* n);

/* ---- image statistics: integral images, histogram, equalisation, projections (docs/kernels/stats.md) ------------------------------------------
 * The static CompVImage functions integral (base/image/compv_image_integral.cxx), histogramBuild, histogramEqualiz, histogramBuildProjectionX / Y
 * (base/image/compv_image.cxx:704-757,846, base/math/compv_math_histogram.cxx) on gray frames p of W x H.  Every output is defined bit for bit: all of it is
 * integer arithmetic, the equalisation table two float32 operations on integers.  Common to the four plan calls: the frames are [frames][H][S] bytes in the
 * plan's geometry and are never written (but for an in-place equalisation); bytes at columns >= W never count; no alignment is asked of the frames (d_gray: ANY
 * BYTE); the
 * calls are asynchronous on `stream`, the frames independent, and beyond 65 535 frames the calls are SLICED.  Scratch is owned by the plan, allocated on
 * first use and released with it.  A refusal returns COMPVHIP_E_INVALID_PARAMETER, names its reason in compvhip_last_error and happens before anything is
 * allocated, enqueued or written.  The host forms take one frame of any size from 1 x 1 (they need no plan) and are synchronous.
 *  1. Integral images: sum[y][x] = the sum of p[y'][x'] over y' < y, x' < x; sumsq[y][x] = the same sum of p[y'][x'] * p[y'][x'], for 0 <= y <= H,
 *     0 <= x <= W, as float64.  Row 0 and column 0 are zeros and are written.  With W, H <= 32 767 and W * H < 2^31 every value is an integer below 2^47:
 *     exact in float64 in any summation order (the kernels carry u32 along a row, u64 down a column, and convert once at the store).  The reference's
 *     layout is CompVMat::newObjAligned<double>(H + 1, W + 1); here the stride is the caller's.
 *  2. Histogram: hist[v] = the number of pixels that equal v, uint32, 256 bins.
 *  3. Equalisation (CompVImage::histogramEqualiz, compv_image.cxx:720-757): scaleF = (float)(scale > 0 ? scale : 255.0 / (double)(W * H)), computed on the
 *     host; run = the running sum of the histogram, uint32 modulo 2^32; v = (float)run * scaleF -- the conversion rounds to nearest even, the multiply
 *     rounds once --; lut[i] = min(trunc(v), 255); out[y][x] = lut[p[y][x]].  The reference converts v to uint8_t without saturation, which is undefined
 *     for v >= 256 (only a caller's own scale or histogram gets there): the clamp is this library's definition of that case.  A scale that is NaN, or
 *     not finite as a float32, is refused.
 *  4. Projections: projX[x] = the sum of p[y][x] over y (buildProjectionX), projY[y] = the sum of p[y][x] over x (buildProjectionY), int32; at most
 *     255 * 32 767. */

/* Host arithmetic only: rows = H + 1, cols = W + 1 of the integral images of a W x H frame (either may be NULL); COMPVHIP_E_INVALID_PARAMETER for W = 0,
 * H = 0, W or H beyond 32 767, or W * H >= 2^31 -- what the device calls refuse. */
COMPVHIP_API int compvhip_integral_dims(size_t W, size_t H, size_t* rows, size_t* cols);

/* d_sum, d_sumsq: [frames][H + 1][sumStride] float64, sumStride >= W + 1 counted in elements, 8-byte aligned; elements at columns > W are not written.
 * Either may be NULL, not both.  Three kernels: the bands' column sums, their scan down the frame, the integral (one pass over 16-row bands).  Stream order: ASYNC. */
COMPVHIP_API int compvhip_plan_integral(compvhip_plan* plan, const uint8_t* d_gray, double* d_sum, double* d_sumsq, size_t sumStride, void* stream);
COMPVHIP_API int compvhip_integral_u8(compvhip_ctx* ctx, const uint8_t* in, size_t W, size_t H, size_t S, double* sum, double* sumsq, size_t sumStride);

/* d_hist: [frames][256] uint32, 4-byte aligned.  Stream order: ASYNC. */
COMPVHIP_API int compvhip_plan_histogram(compvhip_plan* plan, const uint8_t* d_gray, uint32_t* d_hist, void* stream);
COMPVHIP_API int compvhip_histogram_u8(compvhip_ctx* ctx, const uint8_t* in, size_t W, size_t H, size_t S, uint32_t* hist);

/* d_hist: [frames][256], or NULL: each frame's own histogram (the reference's first overload; a non-NULL d_hist is its second).  d_out: [frames][H][S],
 * columns >= W are not written; d_out == d_gray is allowed, as in the reference: the histogram of a frame is complete before any of its pixels is
 * rewritten.  Any other overlap of the two is not.  d_lut: NULL or [frames][256] bytes, the tables.  d_hist 4-byte aligned; d_out and d_lut ANY BYTE, like
 * d_gray.  Stream order: ASYNC. */
COMPVHIP_API int compvhip_plan_equalize(compvhip_plan* plan, const uint8_t* d_gray, const uint32_t* d_hist, double scale, uint8_t* d_out, uint8_t* d_lut,
                                        void* stream);
COMPVHIP_API int compvhip_equalize_u8(compvhip_ctx* ctx, const uint8_t* in, size_t W, size_t H, size_t S, const uint32_t* hist, double scale, uint8_t* out,
                                      size_t So, uint8_t* lut);

/* d_projX: [frames][W], d_projY: [frames][H], int32, dense, 4-byte aligned.  Either may be NULL, not both; with both the frames are read once.  Stream order: ASYNC. */
COMPVHIP_API int compvhip_plan_projections(compvhip_plan* plan, const uint8_t* d_gray, int32_t* d_projX, int32_t* d_projY, void* stream);
COMPVHIP_API int compvhip_projections_u8(compvhip_ctx* ctx, const uint8_t* in, size_t W, size_t H, size_t S, int32_t* projX, int32_t* projY);

/* ---- colour conversion (docs/kernels/convert.md) -----------------------------------------------------------------------------------------------
 * The RGBx, HSV and YUV444P arms of CompVImage::convert (base/image/compv_image.cxx:662-685); the grayscale arm is compvhip_grayscale_u8.  Stateless calls
 * on the context: no scratch memory, no handle, one kernel (convert_kernel).  Every output byte is defined bit for bit.
 * Planes and layout (compvhip_convert_layout): with cw = (W + 1) / 2, ch = (H + 1) / 2
 *   RGBA32 ARGB32 BGRA32     1 plane, 4 W bytes per row          RGB24 BGR24 HSV    1 plane, 3 W bytes per row (HSV: packed H, S, V)
 *   RGB565LE/BE BGR565LE/BE  1 plane, 2 W bytes per row          Y                  1 plane, W bytes per row
 *   YUYV422 UYVY422          1 plane, 4 cw bytes per row (pairs of pixels share U and V)
 *   NV12 NV21                Y: W x H; interleaved UV (NV21: VU): 2 cw bytes per row, ch rows
 *   YUV420P                  Y: W x H; U, V: cw x ch             YUV422P   Y: W x H; U, V: cw x H          YUV444P   Y, U, V: W x H
 * Pixel (x, y) reads chroma sample (x >> 1, y >> 1) of a 4:2:0 format and (x >> 1, y) of a 4:2:2 format.
 * Served pairs and their definition:
 *   to RGBA32 / RGB24 from NV12, NV21, YUV420P, YUV422P, YUV444P, YUYV422, UYVY422 (compv_image_conv_to_rgbx.cxx:625-776): with Y' = Y - 16, U' = U - 127,
 *       V' = V - 127 (127 is the reference's constant), >> arithmetic, clamp8 to 0..255:
 *         R = clamp8((37 Y' + 51 V') >> 5)    G = clamp8((37 Y' - 13 U' - 26 V') >> 5)    B = clamp8((37 Y' + 65 U') >> 5)    A = 255
 *       and from COMPVHIP_FMT_Y: R = G = B = Y, A = 255 (:511-542)
 *   RGBA32 -> RGB24; BGRA32 / BGR24 -> RGB24; RGBA32 / RGB24 -> BGR24 (:544-623): the channels, reordered, alpha dropped.  YUV sources are not served to
 *       BGR / BGRA outputs.
 *   to HSV from RGB24 and RGBA32 (compv_image_conv_hsv.cxx:285-310): max, min over r, g, b; minus = max - min; diff = g - b when max == r, else b - r
 *       when max == g, else r - g; t43[i] = 43 * (1 / i) and t255[i] = 255 * (1 / i), a float32 division then a float32 product, entry 0 = 0;
 *         H = (uint8)(int)round(float(diff) * t43[minus]) + (0 | 85 | 171, chosen like diff), modulo 256 (a negative hue wraps)
 *         S = (uint8)(int)round(float(minus) * t255[max])        V = max
 *       one float32 rounding per operation; round(f) = trunc(f + 0.5) for f >= 0, trunc(f - 0.5) below, computed in float64 (compv_math.h:59).
 *       HSV is served from every YUV source above as well, defined as source -> RGB24 -> HSV (computed in registers, one kernel).
 *   to YUV444P from RGBA32, ARGB32, BGRA32, RGB24, BGR24 and the four 5:6:5 formats (compv_image_conv_to_yuv444p.cxx; 5:6:5 channels are widened by bit
 *       replication as in the grayscale call):
 *         Y = ((33 R + 65 G + 13 B) >> 7) + 16    U = clamp8(((-38 R - 74 G + 112 B) >> 8) + 128)    V = clamp8(((112 R - 94 G - 18 B) >> 8) + 128)
 * Pointers: every plane pointer is ANY BYTE; any rowBytes at or above the layout's minimum and any frameBytes that keeps frames apart are served.  When
 * every plane pointer, rowBytes and (for more than one frame) frameBytes is a multiple of 16 the kernel moves whole words; anything else takes its
 * byte loop and gives the same bytes.  Bytes between a row's end and rowBytes, and between frames, are never written.
 * Aliasing: a plane's byte range runs from its first byte to the last byte of its last row in the last frame.  An output plane may share memory with
 * an input plane only in the 3-byte-to-3-byte pairs (RGB24 -> HSV, RGB24 <-> BGR24), and only with the same pointer, rowBytes and frameBytes: in
 * place.  Any other overlap of an input range with an output range, or of two output ranges, is refused.
 * Refused with COMPVHIP_E_INVALID_PARAMETER before anything is allocated, enqueued or written, the reason in compvhip_last_error: a pair outside the
 * list, W, H or frames of 0, W or H beyond 32 767, a missing plane, a rowBytes below the minimum, a frameBytes (frames > 1) below the plane's size, and
 * the overlaps above.  Beyond 65 535 frames: SLICED. */
typedef struct compvhip_image {     /* `frames` images of one format */
	int pixfmt;
	void* plane[3];                  /* unused planes NULL */
	size_t rowBytes[3];              /* bytes from one row of the plane to the next */
	size_t frameBytes[3];            /* bytes from frame f's plane to frame f+1's */
} compvhip_image;

/* Host arithmetic only: plane count, least row bytes and row count of each plane (entries of absent planes: 0); any output may be NULL.
 * COMPVHIP_E_INVALID_PARAMETER for an unknown format or a zero size, nothing written. */
COMPVHIP_API int compvhip_convert_layout(int pixfmt, size_t W, size_t H, int* planes, size_t minRowBytes[3], size_t rows[3]);
/* device memory, asynchronous on `stream`  Stream order: ASYNC. */
COMPVHIP_API int compvhip_convert_frames(compvhip_ctx* ctx, size_t W, size_t H, size_t frames, const compvhip_image* in, const compvhip_image* out, void* stream);
/* host memory, one frame (frameBytes ignored), synchronous; staged through the context's device buffers */
COMPVHIP_API int compvhip_convert_u8(compvhip_ctx* ctx, size_t W, size_t H, const compvhip_image* in, const compvhip_image* out);

/* ---- SVM prediction: RBF and linear C-SVC (docs/kernels/svm.md) ------------------------------------------------------------------------------
 * CompVMachineLearningSVM::load -> svm_makeSVs_SIMD_frienly (RBF only) -> predict -> svm_predict_values (base/ml/libsvm-322/libsvm.cxx:2692-2784) for n
 * query vectors at once, on the device: the consumer of compvhip_plan_hog's descriptors.  Labels, decision values and kernel values are defined bit for
 * bit.  The leaves are the reference's plain C ones, which its SSE2 / AVX non-FMA leaves are written to equal.  All arithmetic is IEEE binary64, one
 * rounding per operation, no fused multiply-add; a float32 query is widened to float64 first, which is exact.  compv_amd/csrc/svm_math.hpp is the
 * arithmetic, tests/svm_model.py the same definition in numpy, and the device equals both bit for bit.
 * A. Model.  C-SVC: nrClass >= 2 classes; totalSV support vectors of dim dense values, sv[totalSV][dim], grouped by class with counts nSV[c];
 *    svCoef[nrClass - 1][totalSV]; rho[nrClass * (nrClass - 1) / 2]; label[nrClass]; gamma.  The model FILE is the truth: libsvm writes gamma and rho
 *    with %g, coefficients with %.16g and SV values with %.8g, and the loaded values are what strtod in the C locale makes of that text.
 * B. RBF kernel value (svm_k_function_rbf, :3503-3534): K[i] = exp_ref(dotSub(x, SV_i) * (-gamma)).  dotSub (CompVMathDotDotSub_C,
 *    base/math/compv_math_dot.cxx:90-143) keeps four accumulators s0 .. s3.  Whole groups of 16 columns: m_k = (a_k - b_k) * (a_k - b_k);
 *    t_j = m_j + m_{j+4} and t_{j+4} = m_{j+8} + m_{j+12} for j = 0 .. 3; s_j += (t_j + t_{j+4}).  Then pairs of columns: s0 += m, s1 += m.  Then one
 *    last column: s0 += m.  Finally s0 += s2; s1 += s3; s0 += s1.
 * C. exp_ref (CompVMathExpExp_minpack1_64f64f_C, base/math/compv_math_exp.cxx:83-123, after herumi/fmath): x clipped to [ExpMin, ExpMax] =
 *    [-708.39641853226408, 709.78271289338397]; d = x * ca + b with b = 3 * 2^51; t = (d - b) * cra - x; u = ((bits(d) + 2095104) >> 11) << 52;
 *    y = (C3 - t) * (t * t) * C2 - t + C1 in C's precedence; the result is y * asdouble(u | T[bits(d) & 2047]).  T[i] holds the 52 mantissa bits of
 *    pow(2.0, i / 2048.0), built on the host with the C library's pow when a handle is made; ca = 2954.6394437405970 (2048 / ln 2),
 *    cra = 0.00033845077175778578, C1 = 1, C2 = 0.16666666685227835, C3 = 3.0000000027955394.
 * D. LINEAR kernel value (Kernel::dot on the indexed path, :410-430): one accumulator, sum += x_j * sv_j for j = 0 .. dim - 1 in order.
 * E. Decision (:2743-2782): start[c] = the prefix sums of nSV.  For each pair i < j in row-major order, index p:
 *    sumi = dot(svCoef[j - 1] + start[i], K + start[i], nSV[i]); sumj = dot(svCoef[i] + start[j], K + start[j], nSV[j]); dot is CompVMathDotDot_C
 *    (:42-87), the 16 / 2 / 1 structure of B on products, the groups counted from the segment's start; dec[p] = (sumi + sumj) - rho[p];
 *    dec[p] > 0 votes for i, anything else for j.  The label is label[c] of the first class with the most votes.
 * F. Accepted: RBF and LINEAR C-SVC; 2 <= nrClass <= 32; totalSV >= 1, dim >= 1, totalSV * dim and totalSV * (nrClass - 1) below 2^31; nSV >= 0
 *    adding up to totalSV; in a file, dense SV lines whose indices are exactly 1 .. dim in order on every line (the reference asserts the count at
 *    :3476).  Refused with COMPVHIP_E_INVALID_PARAMETER: POLY, SIGMOID, PRECOMPUTED, nu-SVC, one-class, the two SVR types, sparse SV lines, and a file
 *    that does not open or parse.  Queries must be finite: a NaN or an infinity gives an unspecified value, never a fault.
 * Out of scope: training and cross-validation; probA / probB and svm_predict_distance (the reference calls it "not fully tested"; a file's probA /
 *    probB lines are read over); the KNN / annoy classifier; sliding windows.
 * Streams.  As the curve-fit handle, an SVM handle takes its stream at creation (the descriptor): compvhip_svm_predict is asynchronous on it,
 *    compvhip_svm_predict_host and the create calls wait.
 * Alignment.  Vectors by their element size (4 or 8 bytes); d_dec and d_kvalues 8 bytes; d_labels 4 bytes.  A misaligned pointer is refused with
 *    COMPVHIP_E_INVALID_PARAMETER and nothing is written. */
enum {
	COMPVHIP_SVM_KERNEL_LINEAR = 0,            /* libsvm's kernel_type numbers */
	COMPVHIP_SVM_KERNEL_RBF = 2
};
enum {
	COMPVHIP_SVM_F32 = 0,
	COMPVHIP_SVM_F64 = 1
};
typedef struct compvhip_svm_model {            /* HOST arrays; compvhip_svm_create copies them */
	uint32_t size;              /* sizeof(compvhip_svm_model) */
	int32_t kernel;             /* COMPVHIP_SVM_KERNEL_* */
	int32_t nrClass;
	int32_t totalSV;
	int32_t dim;
	int32_t reserved;           /* 0 */
	double gamma;               /* RBF */
	const double* sv;           /* [totalSV][dim] */
	const double* svCoef;       /* [nrClass - 1][totalSV] */
	const double* rho;          /* [nrClass * (nrClass - 1) / 2] */
	const int32_t* nSV;         /* [nrClass] */
	const int32_t* label;       /* [nrClass] */
} compvhip_svm_model;
typedef struct compvhip_svm_desc {
	uint32_t size;              /* sizeof(compvhip_svm_desc) */
	uint32_t maxVectors;        /* 1 .. 2^22 queries of one call; maxVectors * totalSV below 2^31 */
	void* stream;               /* a hipStream_t; NULL = the default stream */
} compvhip_svm_desc;
typedef struct compvhip_svm_shape {
	uint32_t size;              /* sizeof(compvhip_svm_shape), set by the caller */
	int32_t kernel, nrClass, totalSV, dim;
	int32_t pairs;              /* nrClass * (nrClass - 1) / 2: decision values of a query */
	uint32_t maxVectors;        /* 0 from compvhip_svm_model_parse */
	uint32_t reserved;
	double gamma;
} compvhip_svm_shape;
typedef struct compvhip_svm compvhip_svm;   /* a model on the device and the scratch for maxVectors queries */

/* All device memory is allocated here -- the model, the table of item C, maxVectors * totalSV float64 kernel values, and the staging of
 * compvhip_svm_predict_host (at most 512 vectors, their labels and decision values) -- and released by compvhip_svm_destroy: no later call allocates.
 * The K scratch is not sliced: a handle whose maxVectors * totalSV reaches 2^31 (16 GiB) is refused; call with fewer vectors at a time instead.
 * Destroy it BEFORE its context.  Not re-entrant.  A null pointer, a wrong size field, a model item F refuses, maxVectors outside 1 .. 2^22:
 * COMPVHIP_E_INVALID_PARAMETER, *svm = NULL.  Waits for the upload on the descriptor's stream. */
COMPVHIP_API int compvhip_svm_create(compvhip_ctx* ctx, const compvhip_svm_model* model, const compvhip_svm_desc* desc, compvhip_svm** svm);
/* The same from a libsvm model file (svm_save_model's text, parsed as svm_load_model does, strtod in the C locale). */
COMPVHIP_API int compvhip_svm_create_from_file(compvhip_ctx* ctx, const char* path, const compvhip_svm_desc* desc, compvhip_svm** svm);
COMPVHIP_API void compvhip_svm_destroy(compvhip_svm* svm);
COMPVHIP_API int compvhip_svm_info(compvhip_svm* svm, compvhip_svm_shape* shape);
/* d_vectors: [n][strideElems] float32 (COMPVHIP_SVM_F32) or float64 (COMPVHIP_SVM_F64), strideElems >= dim; elements at and behind dim are never
 * read.  d_labels: [n] int32.  d_dec: NULL or [n][pairs] float64.  d_kvalues: NULL or [n][totalSV] float64 (NULL: the handle's scratch holds them).
 * 1 <= n <= maxVectors.  A null handle, d_vectors or d_labels, an unknown type, n outside 1 .. maxVectors, strideElems < dim, n * strideElems at or
 * beyond 2^40, a misaligned pointer: COMPVHIP_E_INVALID_PARAMETER, nothing written.  Elements behind n are never written.  Asynchronous on the handle's
 * stream; deterministic run to run. */
COMPVHIP_API int compvhip_svm_predict(compvhip_svm* svm, const void* d_vectors, int type, size_t n, size_t strideElems, int32_t* d_labels, double* d_dec,
                                      double* d_kvalues);
/* The same on HOST arrays, any n >= 1: slices of at most min(maxVectors, 512) vectors through the handle's staging.  labels: [n]; dec: NULL or
 * [n][pairs].  Waits. */
COMPVHIP_API int compvhip_svm_predict_host(compvhip_svm* svm, const void* vectors, int type, size_t n, size_t strideElems, int32_t* labels, double* dec);
/* Per-kernel timing of the handle's last call, as compvhip_matcher_set_timing / _get_timing: entries svm_kvalues_kernel, svm_decide_kernel. */
COMPVHIP_API int compvhip_svm_set_timing(compvhip_svm* svm, int enabled);
COMPVHIP_API int compvhip_svm_get_timing(compvhip_svm* svm, const char** names, float* ms, int cap);
/* Item C on the host (standard library only, no GPU): out[i] = exp_ref of in[i] for i < n. */
COMPVHIP_API int compvhip_svm_exp_f64(const double* in, double* out, size_t n);
/* The file parser on the host (no GPU).  shape (its size field set) receives the model's numbers; every array may be NULL (a first call learns the
 * sizes) or has room for sv[totalSV][dim], svCoef[nrClass - 1][totalSV], rho[pairs], nSV[nrClass], label[nrClass].  A null path or shape, a wrong size
 * field, a file item F refuses: COMPVHIP_E_INVALID_PARAMETER, nothing written. */
COMPVHIP_API int compvhip_svm_model_parse(const char* path, compvhip_svm_shape* shape, double* sv, double* svCoef, double* rho, int32_t* nSV, int32_t* label);

/* ---- lens undistortion: fused remap, maps, points, projection (docs/kernels/undistort.md) -----------------------------------------------------------
 * CompVCalibUtils::initUndistMap, undist2DImage, dist2DPoints and proj2D (core/calib/compv_core_calib_utils.cxx).  Every output is defined bit for
 * bit.  T is float32 or float64; every operation below is rounded on its own in T and nothing is fused; the one division of item A and the
 * per-point division of item E are correctly rounded IEEE divisions.
 * A. Camera.  K is 3 x 3 row-major, of which fx = K[0], skew = K[1], cx = K[2], fy = K[4], cy = K[5] are read; d holds nd in 2 .. 4 values
 *    k1, k2[, p1[, p2]], a missing one being 0.  Coefficients, once per camera on the host (compvhip_undistort_coeffs_*): det = 1 / (fx * fy);
 *    kinv11 = fy * det; kinv21 = -(skew * det); kinv31 = ((skew * cy) - (fy * cx)) * det; kinv22 = fx * det; kinv32 = -((cy * fx) * det).
 *    The record of a camera is 14 values of T: fx, fy, cx, cy, skew, k1, k2, p1, p2, kinv11, kinv21, kinv31, kinv22, kinv32.
 * B. Distort, for normalised (x, y): x2 = x * x; y2 = y * y; r2 = x2 + y2; r4 = r2 * r2; rdist = (1 + k1 * r2) + k2 * r4; x = x * rdist;
 *    y = y * rdist; a1 = 2 * (x * y) with the scaled x, y; a2 = r2 + 2 * x2 and a3 = r2 + 2 * y2 with the unscaled squares;
 *    x = x + ((p1 * a1) + (p2 * a2)); y = y + ((p1 * a3) + (p2 * a1)); result u = ((x * fx) + (skew * y)) + cx, v = (y * fy) + cy.
 * C. Map entry of output pixel (i, j) with origin (x0, y0): X = (T)(x0 + i), Y = (T)(y0 + j); x = ((kinv11 * X) + (kinv21 * Y)) + kinv31;
 *    y = (kinv22 * Y) + kinv32; then B.  Evaluating kinv11 * X + kinv31 in a wider type and rounding once gives another number.  The reference's
 *    third map row (all ones) is not produced; its float ROI rounds to integers (COMPV_MATH_ROUNDFU_2_NEAREST_INT), which stays with the caller:
 *    x0, y0, Wout, Hout are integers here.
 * D. dist2DPoints: C with (X, Y) the input point.
 * E. proj2D (float64 only), point (xp, yp, zp), pose R (3 x 3 row-major) and t: x = ((R0 * xp + R1 * yp) + R2 * zp) + tx, y and z likewise with
 *    rows 1 and 2; s = z != 0 ? 1.0 / z : 1.0; x = x * s; y = y * s; then B (no kinv step).  The reference's third output row (ones) is not produced.
 * F. Undistorted image: paragraphs B - F of "remap and inverse warp" above, unchanged, applied to the float32 map entry of C: the ROI (the caller's,
 *    clipped, in SOURCE coordinates), the inside test with ordered compares (a NaN or infinite coordinate is outside), nearest, fused bilinear,
 *    unfused bicubic, uint8 and float32 output, the default value.  The fused form computes the entry in registers and reads no map; its output
 *    equals compvhip_plan_remap fed with the float32 maps of compvhip_undistort_maps byte for byte.
 * Out of scope: CompVCalibCamera itself; proj2DError (the sum order of its mse2D is another definition); float64 maps into the remap; an inverse
 *    (distorted -> undistorted points), which the reference does not have either.
 * Streams.  As the SVM handle, an undistort handle takes its stream at creation (the descriptor): compvhip_undistort_frames, _maps, _points and
 *    _project are asynchronous on the handle's stream and never synchronise the host, with the exception the inverse warp has: cameras and poses
 *    are staged in a ring of 4 pinned slots, so a call may wait for the copy of the call four before it (never for more).  K, d and Rt may be changed
 *    as soon as the call has returned.  compvhip_undistort_u8 waits.
 * Alignment.  d_in and a uint8 d_out: any byte (an unaligned destination, stride or frame size is served with element stores; stride padding and
 *    bytes behind Wout are never written); a float32 d_out: 4 bytes (16 for vector stores); maps and points: their element size (4 or 8 bytes;
 *    float32 maps of Wout % 4 == 0 at 16 bytes are written with vector stores); d_counts: 4 bytes.  A misaligned pointer is refused.
 * Batches beyond 65 535: SLICED everywhere -- frames (shared camera: beyond 65 535 groups of 8) in compvhip_undistort_frames, cameras in _maps, sets
 *    in _points and _project.
 * Refused with COMPVHIP_E_INVALID_PARAMETER, nothing written and nothing enqueued: a null pointer or a wrong size field; a size of 0 or beyond
 *    32767; x0 + Wout or y0 + Hout beyond 32767; S < W, and S < 4 (the gathers read 4 bytes of a row at once); nd outside 2 .. 4; fx * fy == 0 for
 *    any camera; a cameraCount other than 1 or the frames (_frames, _maps) / the sets (_points, _project) of the call; an unknown interpolation or
 *    type; Sout < Wout (for float32 output Sout counts ELEMENTS); a misaligned float destination, map, point or count array; source and destination
 *    that overlap (mapX and mapY likewise; points may be transformed in place, d_in == d_out, and may not overlap otherwise); n or sets of 0 or
 *    beyond the handle's caps. */
enum {
	COMPVHIP_UNDISTORT_F32 = 0,
	COMPVHIP_UNDISTORT_F64 = 1
};
typedef struct compvhip_undistort_desc {
	uint32_t size;              /* sizeof(compvhip_undistort_desc) */
	uint32_t W, H, S;           /* the source frames [frames][H][S] of compvhip_undistort_frames: 1 .. 32767, S >= max(W, 4), S * H below 2^31 */
	uint32_t frames;            /* 1 .. 2^31 - 1 */
	uint32_t Wout, Hout;        /* the window of the undistorted frame that is produced (fused form and maps): 1 .. 32767 */
	uint32_t x0, y0;            /* its origin: output pixel (i, j) is pixel (x0 + i, y0 + j); x0 + Wout and y0 + Hout at most 32767 */
	uint32_t maxSets;           /* point sets of one compvhip_undistort_points / _project call; 0: no point calls */
	uint32_t maxPoints;         /* points per set */
	uint32_t reserved;          /* 0 */
	void* stream;               /* a hipStream_t; NULL = the default stream */
} compvhip_undistort_desc;
typedef struct compvhip_undistort compvhip_undistort;   /* the geometry of the fused form and the staging of cameras and poses */

/* Items A and C on the host (standard library only, no GPU, no context).  coeffs: the 14 values of item A.  mapX, mapY: Wout * Hout values each,
 * row-major without stride: the reference loop for callers without a device.  A null pointer, nd outside 2 .. 4, fx * fy == 0, a size of 0 or a
 * window beyond 32767: COMPVHIP_E_INVALID_PARAMETER, nothing written. */
COMPVHIP_API int compvhip_undistort_coeffs_f32(const float* K, const float* d, int nd, float* coeffs);
COMPVHIP_API int compvhip_undistort_coeffs_f64(const double* K, const double* d, int nd, double* coeffs);
COMPVHIP_API int compvhip_undistort_map_f32(const float* K, const float* d, int nd, size_t x0, size_t y0, size_t Wout, size_t Hout, float* mapX, float* mapY);
COMPVHIP_API int compvhip_undistort_map_f64(const double* K, const double* d, int nd, size_t x0, size_t y0, size_t Wout, size_t Hout, double* mapX, double* mapY);
/* All device memory and pinned staging is allocated here -- the device copy and 4 pinned slots of max(frames * 28, maxSets * 52) float32 words: the
 * float64 records of every frame, or the float64 records and poses of every set -- and released by compvhip_undistort_destroy: no later call
 * allocates.  Destroy it BEFORE its context.  Not re-entrant.  On a refusal *undistort = NULL. */
COMPVHIP_API int compvhip_undistort_create(compvhip_ctx* ctx, const compvhip_undistort_desc* desc, compvhip_undistort** undistort);
COMPVHIP_API void compvhip_undistort_destroy(compvhip_undistort* undistort);
/* Item F for every frame of the handle: d_in [frames][H][S] uint8 -> d_out [frames][Hout][Sout], uint8 or (the two _FLOAT32 interpolations) float32.
 * K: HOST, [cameraCount][9] float32; d: HOST, [cameraCount][nd] float32.  cameraCount == 1: all frames share the camera, and a workgroup works its
 * coordinates out once for 8 frames; cameraCount == frames: one camera per frame.  roi == NULL: the whole source frame.  Asynchronous on the
 * handle's stream.  Timing entry: undistort_kernel. */
COMPVHIP_API int compvhip_undistort_frames(compvhip_undistort* undistort, const uint8_t* d_in, const float* K, const float* d, int nd, size_t cameraCount,
                                           int interp, const compvhip_roi* roi, uint8_t defaultValue, void* d_out, size_t Sout);
/* Item C on the device: d_mapX, d_mapY [cameraCount][Hout * Wout] of float32 (COMPVHIP_UNDISTORT_F32) or float64 (_F64); K and d: HOST arrays of the
 * same type, as above; cameraCount 1 or frames.  The float32 planes are in exactly the layout compvhip_plan_remap takes (mapCount = cameraCount).
 * Asynchronous on the handle's stream.  Timing entry: undist_map_kernel. */
COMPVHIP_API int compvhip_undistort_maps(compvhip_undistort* undistort, const void* K, const void* d, int nd, size_t cameraCount, int type, void* d_mapX,
                                         void* d_mapY);
/* Item D on the device: d_in, d_out [sets][n] {x, y} of `type`; d_counts: NULL or [sets] int32 -- points of set s at and behind
 * min(max(d_counts[s], 0), n) are neither read nor written.  cameraCount 1 or sets.  Asynchronous on the handle's stream.  Timing entry:
 * undist_points_kernel. */
COMPVHIP_API int compvhip_undistort_points(compvhip_undistort* undistort, const void* K, const void* d, int nd, size_t cameraCount, int type, const void* d_in,
                                           size_t sets, size_t n, const int32_t* d_counts, void* d_out);
/* Item E on the device: d_in [sets][n] {x, y, z} float64 -> d_out [sets][n] {u, v} float64; Rt: HOST, [sets][12] float64, R row-major then t;
 * d_counts as above.  Asynchronous on the handle's stream.  Timing entry: undist_project_kernel. */
COMPVHIP_API int compvhip_undistort_project(compvhip_undistort* undistort, const double* K, const double* d, int nd, size_t cameraCount, const double* Rt,
                                            const double* d_in, size_t sets, size_t n, const int32_t* d_counts, double* d_out);
/* Item F for one HOST plane (sizes 1 .. 32767) with one host camera; S and Sout in elements.  Synchronous, like compvhip_remap_u8. */
COMPVHIP_API int compvhip_undistort_u8(compvhip_ctx* ctx, const uint8_t* in, size_t W, size_t H, size_t S, const float* K, const float* d, int nd, size_t x0,
                                       size_t y0, int interp, const compvhip_roi* roi, uint8_t defaultValue, void* out, size_t Wout, size_t Hout, size_t Sout);
/* Per-kernel timing of the handle's last call, as compvhip_svm_set_timing / _get_timing. */
COMPVHIP_API int compvhip_undistort_set_timing(compvhip_undistort* undistort, int enabled);
COMPVHIP_API int compvhip_undistort_get_timing(compvhip_undistort* undistort, const char** names, float* ms, int cap);

/* ---- image moments: per frame and per component (docs/kernels/moments.md) ------------------------------------------------------------------------
 * CompVMathMoments::rawFirstOrder, rawSecondOrder, skewness and orientation (base/math/compv_math_moments.cxx), batched, and the same applied to
 * every blob of a label map of compvhip_plan_components without a host trip.
 * Inputs: a plane p of W x H bytes; column i is x, row j is y; bytes at columns >= W never count.  `weights` selects how a pixel counts:
 *    COMPVHIP_MOMENTS_VALUE  w = p[j][i]: what the reference does (its `binar` argument is accepted and ignored, :19-39, :43-71);
 *    COMPVHIP_MOMENTS_UNIT   w = (p[j][i] != 0): what `binar` promises; equal to the reference on a 0 / 1 plane.
 * A. Raw record: the six sums m00 = sum w, m01 = sum j w, m10 = sum i w, m11 = sum i j w, m02 = sum j j w, m20 = sum i i w over all pixels, as EXACT
 *    integers, in the order of the reference's moments[0 .. 5].  Integer sums have no order: the record is the same from run to run.
 * B. Range: a call is refused, before anything is enqueued or written, when wmax * W * H * max(W - 1, H - 1)^2 >= 2^64 (wmax = 255 for VALUE, 1 for
 *    UNIT and for components without gray planes): below that no sum can wrap.  4K and 16384 x 16384 pass with VALUE, 32767 x 32767 only with UNIT.
 *    Also refused: W or H of 0 or beyond 32767, W * H >= 2^31.  compvhip_moments_fits answers for a size.
 * C. The reference accumulates in double.  Wherever all six exact sums are below 2^53 each of its partial sums is an exactly representable integer,
 *    and (double)m_k equals its moments[k] on every bit; beyond that the reference rounds and this library does not.
 * D. Shape record of a raw record; Mk = (double)m_k rounded to nearest even, one IEEE binary64 rounding per operation, nothing contracted:
 *    m00 == 0: status 1, cs = 1, every other field 0.  Otherwise status 0 and
 *      scale = 1.0 / M00; ybar = M01 * scale; xbar = M10 * scale;
 *      u20 = (M20 * scale) - (xbar * xbar); u02 = (M02 * scale) - (ybar * ybar); u11 = (M11 * scale) - (xbar * ybar); den = u20 - u02;   (:177-187)
 *      (cs, sn) = |den| > DBL_EPSILON ? (cos, sin) of atan2(2 * u11, den) / 2 by the half-angle formulas of "RANSAC homography" item D : (1, 0);
 *        the reference's theta is the angle of (cs, sn) -- the one value that is not defined bit for bit against it (no libm on the device);
 *      a = M02 - (ybar * M01); b = M11 - (xbar * M01); skew = |a| > DBL_EPSILON ? b / a : 0   (its own unnormalised terms, :141-149).
 * E. Per component.  Inputs are what compvhip_plan_components wrote: the label map int32 [frames][H][labelStride], the records [frames][compCap], the
 *    counts [frames]; optionally gray planes [frames][H][S] (NULL: every pixel of a component weighs 1, whatever `weights` says; with gray planes a
 *    pixel weighs its gray value (VALUE: a gray 0 inside a component weighs 0) or gray != 0 (UNIT)).  Component id of frame f is served for
 *    id <= min(max(count, 0), compCap); its raw (and shape) record goes to [f][id - 1]; records at and behind that bound are not written.  Label
 *    elements <= 0, labels beyond the bound and everything at columns >= W are ignored.  `origin`: COMPVHIP_MOMENTS_ORIGIN_FRAME: i, j are frame
 *    coordinates; COMPVHIP_MOMENTS_ORIGIN_BOX: i - x0, j - y0 of the component's record -- the reference run on the blob's crop with every foreign
 *    pixel zeroed.  Only x0 and y0 of a record are read, and only with ORIGIN_BOX.
 * The device calls are stateless on a context: they own no scratch (the sums land in the caller's records, which each call zeroes itself), run on the
 *    descriptor's stream and never synchronise the host; nothing is carried from call to call.
 * Alignment.  d_gray: any byte; labels, component records and counts: 4 bytes; raw and shape records: 8 bytes.  A misaligned pointer is refused.
 * Batches beyond 65 535 frames: SLICED.
 * Refused with COMPVHIP_E_INVALID_PARAMETER, nothing written and nothing enqueued: a null context, descriptor or required pointer; a wrong size field;
 *    an unknown weights or origin (compvhip_moments_frames and _host: ORIGIN_FRAME only); item B; S < W; labelStride < W; frames of 0 or beyond
 *    2^31 - 1; compCap of 0 or beyond 2^31 - 1; n beyond 2^31 - 1; a misaligned pointer. */
enum {
	COMPVHIP_MOMENTS_VALUE = 0,
	COMPVHIP_MOMENTS_UNIT = 1
};
enum {
	COMPVHIP_MOMENTS_ORIGIN_FRAME = 0,
	COMPVHIP_MOMENTS_ORIGIN_BOX = 1
};
typedef struct compvhip_moments {
	uint64_t m00, m01, m10, m11, m02, m20;
} compvhip_moments;
typedef struct compvhip_moments_shape {
	double xbar, ybar;          /* the centroid */
	double u20, u02, u11;       /* the normalised central moments of the orientation */
	double skew;
	double cs, sn;              /* cos and sin of the orientation theta */
	int32_t status, pad;        /* 0; 1: m00 == 0.  pad: 0 */
} compvhip_moments_shape;
typedef struct compvhip_moments_desc {
	uint32_t size;              /* sizeof(compvhip_moments_desc) */
	int32_t weights;            /* COMPVHIP_MOMENTS_VALUE / _UNIT */
	int32_t origin;             /* COMPVHIP_MOMENTS_ORIGIN_FRAME / _BOX; the frames calls: FRAME only */
	void* hipStream;            /* a hipStream_t; NULL = the default stream */
} compvhip_moments_desc;

/* Items A (d_raw [frames]) and, with d_shape != NULL, D (d_shape [frames]) of every frame of d_gray [frames][H][S].  Asynchronous. */
COMPVHIP_API int compvhip_moments_frames(compvhip_ctx* ctx, const compvhip_moments_desc* desc, const uint8_t* d_gray, size_t W, size_t H, size_t S, size_t frames,
                                         compvhip_moments* d_raw, compvhip_moments_shape* d_shape);
/* Item E: d_raw and (or NULL) d_shape [frames][compCap].  d_gray NULL: S is not looked at.  Asynchronous. */
COMPVHIP_API int compvhip_moments_components(compvhip_ctx* ctx, const compvhip_moments_desc* desc, const int32_t* d_labels, size_t W, size_t H, size_t labelStride,
                                             const uint8_t* d_gray, size_t S, const compvhip_component* d_comps, size_t compCap, const int32_t* d_compCounts,
                                             size_t frames, compvhip_moments* d_raw, compvhip_moments_shape* d_shape);
/* Item D alone on the device: d_shape[k] of d_raw[k], k < n (n == 0: nothing to do).  Only the descriptor's size and stream are looked at.  Asynchronous. */
COMPVHIP_API int compvhip_moments_shapes(compvhip_ctx* ctx, const compvhip_moments_desc* desc, const compvhip_moments* d_raw, size_t n, compvhip_moments_shape* d_shape);
/* Item D on the host (standard library only, no GPU, no context): shape[k] of raw[k], k < n.  A null pointer: COMPVHIP_E_INVALID_PARAMETER. */
COMPVHIP_API int compvhip_moments_shape_host(const compvhip_moments* raw, size_t n, compvhip_moments_shape* shape);
/* Item B on the host: 1 when a frame of W x H may be given with these weights, 0 when the call would be refused (an unknown `weights` included). */
COMPVHIP_API int compvhip_moments_fits(size_t W, size_t H, int weights);
/* Items A and D of one HOST plane from 1 x 1 on: raw and (or NULL) shape receive one record each.  Synchronous, on the context's own stream: the
 * descriptor's stream is not used.  Staging is the context's and allocated on first use. */
COMPVHIP_API int compvhip_moments_host(compvhip_ctx* ctx, const compvhip_moments_desc* desc, const uint8_t* in, size_t W, size_t H, size_t S, compvhip_moments* raw,
                                       compvhip_moments_shape* shape);

/* ---- PCA projection: HOG to PCA to SVM without a host trip (docs/kernels/pca.md) --------------------------------------------------------------------
 * CompVMathPCA::project (base/math/compv_math_pca.cxx:196-254), CompVMath::mulABt (base/math/compv_math_op_mul.cxx) and the row-based front half of
 * CompVMathPCA::compute (mean and covariance, :267-348), in float32, bit for bit the reference's plain C leaf, which its non-FMA SIMD leaves are written
 * to equal.  All arithmetic is IEEE binary32 with one rounding per operation and nothing contracted; denormals are kept.
 * A. Model: dim D >= 1, components M >= 1; mean[D], vectors[M][D] (the eigenvectors as rows), values[M] (informative: no call reads them).
 * B. Centre: c_k = x_k - mean_k, rounded (CompVMathOpSubSub).  With no mean, c = x.
 * C. dot16(a, b, D): sixteen accumulators v0 .. v15 start at +0.  For every whole group of 16 columns v_i += a[k + i] * b[k + i] (the product is
 *    rounded, then the sum); for every whole group of 4 of what remains the same into v0 .. v3.  Then the fold, in this order:
 *      v0 += v4; v1 += v5; v2 += v6; v3 += v7; v8 += v12; v9 += v13; v10 += v14; v11 += v15;
 *      v0 += v8; v1 += v9; v2 += v10; v3 += v11;   v0 += v2; v1 += v3;   v0 += v1;
 *    then the last 0 .. 3 columns in order, v0 += a[k] * b[k].  The value is v0 (compv_math_op_mul.cxx:132-181).
 * D. Projection: out[r][m] = dot16(c_r, vectors_m, D).
 * E. mulABt: R[i][j] = dot16(A_i, B_j, cols).
 * F. Mean and covariance of n >= 1 row-based observations: mean_j = (float)(s * (1.0 / (double)n)), s the binary64 sum of (double)obs[i][j] over
 *    i = 0 .. n - 1 in that order; c[j][i] = obs[i][j] - mean_j; covar[a][b] = dot16(c[a], c[b], n) * scale, scale = 1 / (float)(n - 1), applied (one
 *    more rounded multiply) only when n > 1.  dot16(a, b) = dot16(b, a) on every bit, so covar is symmetric on every bit.
 * G. Model file: what CompVMathPCA::write produces and read accepts -- a JSON object with members "mean", "vectors" and "values", each
 *    {"type":"32f","size":[rows,cols],"data":[...]} with rows * cols numbers in row-major order; any member order, unknown members skipped.  A number
 *    becomes (float)strtod(text) in the C locale.  mean is 1 x D, values 1 x M, vectors M x D.
 * Limits: 1 <= D <= 2^20 (aRows, bRows and cols of mulABt: the same), 1 <= M <= 65535, n <= 2^31 - 1 (n == 0: success, nothing enqueued); every stride
 *    (in elements) >= its row length and rows * stride < 2^40.  Pointers: 4-byte aligned; the scratch of the covariance: 16-byte aligned.
 * The device calls are stateless on a context: they own no scratch, run on the descriptor's stream and never synchronise the host.  Elements at and
 *    behind `dim` (input) or `components` (output) of a row are never read or written; rows behind n are never written.  Input and output may not
 *    overlap (not checked).  A NaN or an infinity in the data gives an unspecified value, never a fault.  No grid dimension can pass 65 535 within
 *    the limits (rows ride in x), so no launch is sliced.
 * Refused with COMPVHIP_E_INVALID_PARAMETER, nothing written and nothing enqueued: a null context, descriptor or required pointer; a wrong size field;
 *    a dimension, count or stride outside the limits; a misaligned pointer; a model file that does not open or parse, holds a type other than 32f, a
 *    size that does not match the data count, a number that is not finite in float32, or D or M outside the limits. */
typedef struct compvhip_pca_desc {
	uint32_t size;              /* sizeof(compvhip_pca_desc) */
	uint32_t reserved;          /* 0 */
	void* hipStream;            /* a hipStream_t; NULL = the default stream */
} compvhip_pca_desc;

/* Items B - D: d_in [n][inStride] -> d_out [n][outStride], with d_mean [dim] (NULL: do not centre) and d_vectors [components][vecStride].
 * Asynchronous. */
COMPVHIP_API int compvhip_pca_project(compvhip_ctx* ctx, const compvhip_pca_desc* desc, const float* d_mean, const float* d_vectors, size_t vecStride, size_t dim,
                                      size_t components, const float* d_in, size_t n, size_t inStride, float* d_out, size_t outStride);
/* Item E: d_A [aRows][aStride], d_B [bRows][bStride], `cols` columns each -> d_R [aRows][rStride].  aRows == 0: nothing to do.  Asynchronous. */
COMPVHIP_API int compvhip_mulabt_f32(compvhip_ctx* ctx, const compvhip_pca_desc* desc, const float* d_A, size_t aRows, size_t aStride, const float* d_B, size_t bRows,
                                     size_t bStride, size_t cols, float* d_R, size_t rStride);
/* Item F: d_obs [n][obsStride], n >= 1 -> d_mean [dim] and d_covar [dim][covStride].  d_scratch: compvhip_pca_covariance_scratch bytes, 16-byte
 * aligned, for the centred, transposed data c [dim][nPad], nPad = n rounded up to 16; the padding is neither written nor read.  Asynchronous. */
COMPVHIP_API int compvhip_pca_covariance(compvhip_ctx* ctx, const compvhip_pca_desc* desc, const float* d_obs, size_t n, size_t obsStride, size_t dim, float* d_mean,
                                         float* d_covar, size_t covStride, void* d_scratch);
/* The bytes of that scratch; refused where n or dim is outside the limits or dim * nPad reaches 2^40. */
COMPVHIP_API int compvhip_pca_covariance_scratch(size_t n, size_t dim, size_t* bytes);
/* compvhip_pca_project on HOST arrays.  Synchronous, on the context's own stream: the descriptor's stream is not used.  Staging is the context's,
 * allocated on first use; the rows go through it in slices of at most 512. */
COMPVHIP_API int compvhip_pca_project_host(compvhip_ctx* ctx, const compvhip_pca_desc* desc, const float* mean, const float* vectors, size_t vecStride, size_t dim,
                                           size_t components, const float* in, size_t n, size_t inStride, float* out, size_t outStride);
/* Item G on the host (standard library only, no GPU, no context): the sizes of the model file into *dim and *components, and -- each may be NULL, so a
 * first call learns the sizes -- mean [dim], vectors [components][dim], values [components].  A refused file writes nothing. */
COMPVHIP_API int compvhip_pca_model_parse(const char* path, int32_t* dim, int32_t* components, float* mean, float* vectors, float* values);
/* Item C on the host: *out = dot16(a, b, n).  n == 0: +0, a and b are not looked at. */
COMPVHIP_API int compvhip_pca_dot_host(const float* a, const float* b, size_t n, float* out);

/* Per-kernel timing of the last plan call, measured with hipEvents on the stream the kernels were launched on.
 * names/ms: caller arrays of capacity cap; returns the number of entries (<= cap). compvhip_plan_set_timing(plan, mode):
 * 0 = off, 1 = every kernel, 2 = only canny_tile_kernel and sht_vote_kernel, 3 = only sht_vote_kernel, 4 = only canny_tile_kernel
 * (an event pair costs ~10-20 us of stream time and lengthens the bracketed kernel: the narrow modes keep that out of a
 * throughput measurement). */
COMPVHIP_API int compvhip_plan_set_timing(compvhip_plan* plan, int enabled);
COMPVHIP_API int compvhip_plan_get_timing(compvhip_plan* plan, const char** names, float* ms, int cap);

#ifdef __cplusplus
}
#endif
#endif /* COMPV_HIP_H */
