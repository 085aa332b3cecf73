// api_internal.hpp -- what the translation units of the C ABI's host side (api*.cpp) share: the structs behind the opaque handles, error and
// allocation helpers, per-kernel timing, and the few functions that are called across files (namespace compvhip_api: not exported).
#pragma once
#include "../../include/compv_hip.h"
#include "kernels.hpp"
#include "kht.hpp"
#include "kht_group.hpp"
#include "device_memory.hpp"
#include "host_call.hpp"
#include "frame_slices.hpp"
#include "convert_math.hpp"
#include "step_policy.hpp"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <memory>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

using namespace compvhip;

using namespace compvhip_api;   // (this header serves the api*.cpp files only)

constexpr int kMaxRounds = 4096;       // hysteresis round flag slots (a multiple of 4); a frame that needs more rounds reuses them (enqueueResolve)
constexpr size_t kMinLineCap = 1u << 16;  // per-frame line-key slots: max(caller's lineCap, 65536), clamped to R*T (include/compv_hip.h, compvhip_plan_houghsht)
constexpr int kAsyncDepth = 4;            // outstanding compvhip_plan_pipeline_async steps per plan
constexpr size_t kMaxTimeline = 4096;     // timing entries kept while nobody reads them (asynchronous steps)
// A ticket's pinned host slot, as sht_lines_kernel writes it through ShtArgs::hostStep (kernels.hpp: this mirrors the kernel side): the step's line total, then
// (one 128-byte line on) its first four round flags
constexpr int kSlotTotal = 0, kSlotFlags = kFrameSlot, kSlotStride = kFrameSlot + 4;

// device tables of the canonical KHT path's line fields (khtCanonTables), built once per geometry
struct KhtCanonTabs {
	DevBuf<float> rho, theta;
	size_t W = 0, H = 0; double dRho = 0.0, dTheta = 0.0;
};

// Host state of one frame of a KHT group; persists from call to call (vectors keep their capacity)
struct KhtFrameState : KhtFrameLayout {
	KhtBitPlane plane; size_t most = 0, nPts = 0;              // the linker's working copy (zero border, destroyed by the walk), its set pixels, the points linked
	std::vector<KhtKernel> kernels; double hmax = 0.0; bool haveGS = false;
	std::vector<KhtCell> cells; size_t cellOff = 0; int cellCount = 0;
	KhtPeaksWork peaks; std::vector<KhtLine> out;
	double ms[6] = {};
	int code = COMPVHIP_OK; std::string err;
};
// Device, pinned and host state of a GROUP of 1 <= G <= kKhtBatch KHT frames going through the stages together (api_kht.cpp).  A plan owns one per group in
// flight, each with a stream and events of its own; the context owns one for its host entry points (G = 1), which borrows the context's stream.
struct KhtGroupState {
	hipStream_t stream = nullptr; bool ownsStream = false;                             // (borrowed: the owner of the stream destroys it)
	DevBuf<uint32_t> dBits; PinBuf<uint32_t> hostBits;                                 // [frames of a group][wpr * H]: device / pinned (plan only: the host entry packs the caller's bytes)
	std::vector<hipEvent_t> ready;                                                     // frame f's bit plane has arrived
	PinBuf<KhtPoint> linked; DevBuf<KhtPoint> pts;                                     // points of every frame's strings: pinned arena (the linkers write it) / device
	DevBuf<KhtStringDesc> strings; DevBuf<uint32_t> counts32; PinBuf<KhtStringDesc> stringsHost;
	DevBuf<uint32_t> totals;                                                           // device [kKhtBatch + 1]: clusters per frame, truncation flag
	DevBuf<KhtSpan> spans, scratch; DevBuf<KhtSubdivFrame> stack; DevBuf<KhtKernel> kernelsDev;   // one slot per possible cluster, all four
	PinBuf<KhtKernel> kernelsHost;
	DevBuf<int32_t> counts;
	DevBuf<KhtVoteParams> params; PinBuf<KhtVoteParams> paramsHost;
	DevBuf<KhtCell> cells; DevBuf<int> cellCount; PinBuf<KhtCell> cellsHost;
	KhtCanonTabs tabs; DevBuf<KhtLine> canonLines; DevBuf<int32_t> canonCounts;        // canonical order: [frames][cap] sorted lines, [kKhtBatch] counts (device)
	PinBuf<KhtLine> canonLinesHost;
	std::vector<KhtFrameState> frames;
	// How a stage waits for the stream.  With this blocking-sync event the waiting thread SLEEPS: a plan's controllers (hipStreamSynchronize spins on a CPU of
	// the quota the workers need).  Without it: hipStreamSynchronize, the host entry points' wait (one frame, nobody else wants the CPU).
	hipEvent_t syncEv = nullptr;
	double stageMs[6] = {};   // link, subdivide (GPU), statistics (GPU), prune + Gmin, vote + peaks (GPU), sort + sweep: of the groups this state handled in the current call
	KhtGroupState() = default;
	KhtGroupState(const KhtGroupState&) = delete;
	hipError_t wait()
	{
		if (!syncEv) return hipStreamSynchronize(stream);
		const hipError_t e = hipEventRecord(syncEv, stream);
		return e != hipSuccess ? e : hipEventSynchronize(syncEv);
	}
	// (the owner's device is current: compvhip_plan_destroy, compvhip_ctx_destroy) the events and the stream it created; the buffers free themselves AFTER this
	// body, so the stream goes before them.  The KHT calls are synchronous: the stream is idle, hipStreamDestroy defers anyway and hipFree synchronises.
	~KhtGroupState()
	{
		for (hipEvent_t e : ready) (void)hipEventDestroy(e);
		if (syncEv) (void)hipEventDestroy(syncEv);
		if (ownsStream && stream) (void)hipStreamDestroy(stream);
	}
};

// The running-sum tables of an inverse warp (compvhip_warp_tables) on their way to the device: built on the host into a ring of pinned staging slots and
// uploaded in stream order into `dev`.  A slot is written again only after the copy that last read it has completed (its event), so kAsyncDepth calls
// can be enqueued without the host waiting for the device.
struct WarpTables {
	DevBuf<float> dev;                 // [1 or frames] x { ac, df[, gi] of Wout values, by, ey[, hy] of Hout values }
	struct Slot { PinBuf<float> host; hipEvent_t copied = nullptr; } slot[kAsyncDepth];
	int next = 0;
	WarpTables() = default;
	WarpTables(const WarpTables&) = delete;
	~WarpTables() { for (auto& s : slot) if (s.copied) (void)hipEventDestroy(s.copied); }   // (the owner's device is current: compvhip_plan_destroy, compvhip_ctx_destroy)
};

// Scratch of the image statistics calls (stats_kernels.hip): the bands' column sums of p and of p * p, [frames][bands][W] each; the partial histograms
// [frames][chunks][256]; the look-up tables [frames][256] of the equalisation calls that do not hand them out.  A plan owns one, the context one for its host calls.
struct StatsScratch {
	DevBuf<uint64_t> colSum, colSq; DevBuf<uint32_t> hist; DevBuf<uint8_t> lut;
};

struct compvhip_ctx {
	int device = 0;
	std::string err;
	LiveCount live{0};           // hipMalloc / hipFree balance; KHT workers of a plan allocate from their own threads
	hipStream_t stream = nullptr;      // stream of the host entry points
	compvhip_plan* hostPlan = nullptr; // single-frame plan cached for the host entry points
	DevBuf<uint8_t> dIn, dOut;         // device staging of the host entry points (bytes)
	DevBuf<uint8_t> dPacked;           // packed-pixel staging of compvhip_grayscale_u8
	DevBuf<uint32_t> dHist;            // [256] histogram + 1 result word of compvhip_otsu_u8
	DevBuf<int32_t> dCounts, dAccOut;
	DevBuf<compvhip_line> dSegLines;   // staging of compvhip_houghsht_segments_u8: the caller's lines ...
	DevBuf<compvhip_segment> dSegs;    // ... and the segments; the count travels through dCounts
	DevBuf<int32_t> dSegCount;
	DevBuf<compvhip_line_fit> dFits;   // staging of compvhip_houghsht_fit_u8: the records, their number ...
	DevBuf<int32_t> dFitCount;
	DevBuf<compvhip_line> dFitRefined; // ... and the refined lines (lines and segments travel through dSegLines / dSegs)
	DevBuf<int32_t> dCompLabels;       // staging of compvhip_components_u8: the label map (W * H) ...
	DevBuf<compvhip_component> dComps; // ... the records ...
	DevBuf<int32_t> dCompCount;        // ... and their number
	DevBuf<compvhip_corner> dFastCorners;   // staging of compvhip_fast_u8: the records (the score map travels through dOut) ...
	DevBuf<int32_t> dFastCount;             // ... and their number
	DevBuf<compvhip_keypoint> dOrbKeys;     // staging of compvhip_orb_u8 (the corners and their number travel through dFastCorners / dFastCount): the records ...
	DevBuf<int32_t> dOrbCount;              // ... their number ...
	DevBuf<uint8_t> dOrbDesc;               // ... and the descriptor rows
	DevBuf<float> dMap;                     // staging of compvhip_remap_u8: mapX, then mapY
	WarpTables warp;                        // tables of compvhip_warp_inverse_u8
	DevBuf<float> dHogDesc;                 // staging of compvhip_hog_u8: the descriptor
	StatsScratch stats;                     // scratch of the host statistics calls (they need no plan: a plan has a minimum size, these calls have none)
	DevBuf<double> dStatsF64;               // staging of compvhip_integral_u8: sum, then sumsq, (H + 1) x (W + 1) each
	DevBuf<uint32_t> dStatsU32;             // staging of the other statistics calls: a histogram (with the table behind it), or projX then projY
	DevBuf<uint64_t> dMoments;              // staging of compvhip_moments_host: the raw record, the shape record behind it
	DevBuf<float> dPcaModel, dPcaIn, dPcaOut;   // staging of compvhip_pca_project_host: the mean with the vectors behind it, a slice of rows, its outputs
	KhtGroupState kht;                 // the host KHT entry points' group of one frame (compvhip_houghkht_u8, _ex_u8, _kernels_u8); borrows `stream`
};

struct TimingEntry { const char* name; hipEvent_t a, b; };
// per-kernel timing of the last call of a plan or a matcher: event pairs around the launches, the events pooled and reused
struct TimingState {
	int timing = 0; // plan: 0 off, 1 every kernel, 2 canny_tile + sht_vote, 3 sht_vote only, 4 canny_tile only; matcher: 0 off, 1 every kernel
	std::vector<hipEvent_t> eventPool;
	std::vector<TimingEntry> timeline;
	std::vector<std::string> timingNames; std::vector<float> timingMs;
};

// one step of the device-resident pipeline: [grayscale ->] Canny -> SHT [-> toCartesian] (compvhip_plan_pipeline{,_async,_ex})
struct StepParams {
	const uint8_t* d_in = nullptr; float tLow = 0.f, tHigh = 0.f; int threshold = 0, maxLines = 0;
	int ksize = 3, thresholdType = COMPVHIP_CANNY_THRESHOLD_COMPARE_TO_GRADIENT, pixfmt = COMPVHIP_FMT_Y;
	uint8_t* d_gray = nullptr; int32_t* d_otsu = nullptr; float* d_cart = nullptr;
	uint8_t* d_edges = nullptr; compvhip_line* d_lines = nullptr; size_t lineCap = 0; int32_t* d_counts = nullptr;
};

struct compvhip_plan : TimingState {
	compvhip_ctx* ctx = nullptr;
	size_t W = 0, H = 0, S = 0, frames = 0;
	float thetaDeg = 1.f;
	// canny
	int tilesX = 0, tilesY = 0, wb = 0;
	size_t bitsFrameStride = 0;
	DevBuf<uint32_t> ebits, ubits;
	DevBuf<int> counters;     // ONE device allocation zeroed by ONE memset per step: [edgeCounts frames][lineCounts frames][tileCounts frames*tiles][blockCounts frames*lineBlocks][frameTotals frames*kFrameSlot][lineTotal kFrameSlot][flags kMaxRounds]
	size_t nCounts = 0;       // ints in front of the flags
	int* flags = nullptr; PinBuf<int> hFlags;    // device (a view into counters) / pinned host, 2 ints: [0] the round flag resolveConverged copies back, [1] hTotals
	int* frameTotals = nullptr; unsigned int* lineTotal = nullptr; // device (views into counters): NMS survivors per frame (one per 128-byte line) / key slots in use
	unsigned int* hTotals = nullptr;             // pinned host (a view into hFlags, behind the flag): lineTotal of a synchronous step, copied back in front of its sort (kSortExact)
	// The line sort covers the key slots that exist.  A synchronous step reads their number before it enqueues the sort; an asynchronous step cannot, so it
	// sorts a range predicted from the totals of the plan's last steps (asyncSortRange; none seen yet: the whole capacity) -- compvhip_plan_wait compares with
	// the step's real total and replays the step when the prediction was too small.
	Recent8 recentTotals;
	// speculative hysteresis rounds of a step: what the plan's last 8 asynchronous steps needed (nextSpecRounds); a step that needs more is replayed by
	// compvhip_plan_wait and teaches the plan
	int specRounds = kSpecRounds; Recent8 recentRounds;
	int* hRoundsDev = nullptr;                   // hRounds as the device sees it (a view)
	PinBuf<int> hRounds;                         // pinned host (hipHostMallocMapped), kSlotStride ints per ticket: sht_lines_kernel writes the step's line total and round flags straight into it, compvhip_plan_wait reads them
	int maxRounds = kMaxRounds; // flag slots in use (COMPVHIP_RESOLVE_WRAP lowers it: tests of the slot reuse)
	bool traceRounds = false;   // COMPVHIP_TRACE_ROUNDS was set when the plan was made: compvhip_plan_wait prints what every ticket saw
	// A fact about DEVICE memory that outlives a call: the edge, line and tile counts are zero because the last kernel enqueued that touches them is a Canny tile kernel,
	// which clears them (enqueueCanny).  compvhip_plan_canny leaves it set, and a later compvhip_plan_houghsht relies on it and skips its own fill; every SHT stage
	// uses the counts and clears the mark (planShtImpl).
	bool countersFresh = false;
	DevBuf<int2> thrDev; DevBuf<unsigned int> sums;
	DevBuf<uint8_t> dirty;     // per-workgroup change flags of the resolve rounds
	DevBuf<uint8_t> grayTmp;    // luma plane of a packed-input step when the caller does not want it (compvhip_plan_pipeline_ex)
	DevBuf<uint8_t> tmpOut;    // aliasing (in == out) scratch: a tile may still read the row halo a neighbour has overwritten
	bool bitsValid = false;
	// sht
	bool shtReady = false;
	size_t R = 0, T = 0; float thetaStep = 0.f; int accPitch = 0;
	DevBuf<uint8_t> blurTmp;                          // u8 intermediate of the fixed-point convolution
	DevBuf<uint32_t> hist; DevBuf<int32_t> otsu;       // pre-processing scratch: partial histograms, [frames] Otsu level
	DevBuf<float> cosT, invSinT;                     // toCartesian tables: cosf(theta_col), 1/sinf(theta_col)
	DevBuf<int32_t> sinQ, cosQ;
	DevBuf<uint32_t> edges; size_t edgeCap = 0; int* edgeCounts = nullptr;   // edgeCounts: a view into counters
	DevBuf<uint16_t> acc; size_t accFrameStride = 0;
	DevBuf<uint32_t> keysA, keysB, valsA, valsB; size_t lineCap = 0; int* lineCounts = nullptr;   // lineCounts: a view into counters
	DevBuf<int2> reach;                          // [T] accumulator rows the windows of a theta cover
	DevBuf<int2> nmsRange;                       // [column groups of the NMS] accumulator rows the windows can reach
	DevBuf<uint8_t> nmsFlags;                    // NMS survivors (flag planes)
	int* blockCounts = nullptr; int lineBlocks = 0;   // NMS survivors per 64 accumulator rows (a view into counters)
	DevBuf<uint8_t> sortTemp; size_t sortTempBytes = 0;
	DevBuf<int32_t> segPerLine;   // line segments (sht_segments_kernels.hip): segments per line, then their prefix sums
	// connected components (components_kernels.hip), allocated on first use: survivors per row [frames][H]; the packed copy of a byte edge map
	// [frames][H][wb]; parent words [frames][H][W] of the calls without a label map (with one, the parent words live in it)
	DevBuf<int32_t> compRows; DevBuf<uint32_t> compBits; DevBuf<int32_t> compParent;
	DevBuf<uint8_t> morphTmp;                    // thresholding / morphology (morph_kernels.hip), allocated on first use: the u8 plane [frames][H][S] between the two basic operations of an OPEN / CLOSE, and the out-of-place target of an in-place adaptive threshold
	// FAST corners (fast_kernels.hip), allocated on first use: [frames][H] corners per row, [frames][H] their scan, [frames][256] score histogram, [frames] cut
	// level -- one allocation; and the score map [frames][H][S] of the calls that do not want one
	DevBuf<int> fastWork; DevBuf<uint8_t> fastScores;
	// ORB (orb_kernels.hip), allocated on first use: [frames][keyCap] source indices of the surviving corners (grows with the largest keyCap seen); the blurred
	// batch [frames][H][S] of the describe calls with blur != 0; the Q16 Gaussian (5, 2.0f), computed once; which byte-read variant of orb_brief_kernel runs
	DevBuf<int32_t> orbIndex; DevBuf<uint8_t> orbBlur; uint16_t orbKern[5] = {}; bool orbKernReady = false; bool orbBriefLds = false;
	WarpTables warp;             // inverse warp (remap_kernels.hip), allocated on first use: the matrices' running-sum tables and their pinned staging
	DevBuf<float> hogCells;      // HOG (hog_kernels.hip), allocated on first use without a caller's map: the cell map [frames][cellsY][cellsX][nbins]
	StatsScratch stats;          // image statistics (stats_kernels.hip), allocated on first use
	int strengthBits = 16, keyBits = 0;
	// the line sort sized on the device (sht_sort_kernels.hip): used when a strength has at most 13 bits and a frame at most 16 chunks of keys
	DevBuf<uint16_t> chunkHist; DevBuf<uint32_t> strengthStart; int sortChunks = 0; bool deviceSort = false;
	// voting over image tiles (planned at plan creation: the per-tile edge counters live in `counters`)
	bool voteTiles = false;                      // the tile grid exists
	ShtTileArgs vt = {};                         // geometry + device tables (views of the five buffers below, of reach and of tileCounts)
	std::vector<int32_t> vtKt, vtRowBase;        // host copies of the [tiles][T] tables
	DevBuf<int32_t> dKt, dRowBase; DevBuf<uint8_t> partLo, partHi, colFlag; int* tileCounts = nullptr;   // tileCounts: a view into counters
	// batched KHT (compvhip_plan_houghkht): the states of the groups in flight, the workers' workspaces, stage clocks of the last call
	std::vector<std::unique_ptr<KhtGroupState>> khtBatch;       // device / pinned buffers, stream and per-frame host state: one per group of frames in flight
	std::vector<std::unique_ptr<KhtPeaksWork>> khtWork;   // sort + sweep workspace (axes, 1.6 MB visited map at 4K) of WORKER w: it stays in that core's cache from frame to frame
	double khtStageMs[6] = {}; double khtWallMs = 0.0; int khtThreads = 0;
	// asynchronous steps (compvhip_plan_pipeline_async / compvhip_plan_wait)
	// seq: enqueue order; replay: an EARLIER step of the plan was replayed after this one ran -- its outputs may have been overwritten
	struct AsyncStep { bool used = false; bool replay = false; uint64_t seq = 0; hipEvent_t done = nullptr; hipStream_t stream = nullptr; StepParams sp; size_t sortN = 0; int rounds = 0; } steps[kAsyncDepth];
	uint64_t stepSeq = 0;
};

// brute-force matcher (match_kernels.hip): every buffer is allocated by compvhip_matcher_create
struct compvhip_matcher : TimingState {
	compvhip_ctx* ctx = nullptr;
	int descDwords = 0, queryCap = 0, trainCap = 0, pairs = 0, knn = 0;
	DevBuf<uint32_t> partial;           // keys of the slice kernel: max of the forward ([pairs][train slices][knn][queryCap]) and the reverse ([pairs][query slices][trainCap]) run
	DevBuf<compvhip_match> reverse;     // [pairs][trainCap]: best query of every train row (cross check)
};
// what the RANSAC handles share (api_ransac.cpp); every buffer is allocated by the family's create call
struct RansacHandle : TimingState {
	compvhip_ctx* ctx = nullptr;
	int sets = 0, pointCap = 0, maxTries = 0;   // sets: the homography's pairs
	DevBuf<double2> points;             // [2 * arrays][sets][pointCap]: the family's point arrays as gathered, then as selected
	DevBuf<int32_t> counts;             // [sets] points gathered
	bool gathered = false;              // the family's gather call (compvhip_homography_points, compvhip_curvefit_points_from_labels) has run
};
// RANSAC homography (homography_kernels.hip); two point arrays: src, dst
struct compvhip_homography : RansacHandle {
	DevBuf<double> tryF64;              // [sets][maxTries][18] H and inverse, then [sets][maxTries] variance
	DevBuf<int32_t> tryI32;             // [3][sets][maxTries]: state, rotations, inlier count
};
// RANSAC line and parabola fits (curvefit_kernels.hip); one point array; every call runs on `stream`
struct compvhip_curvefit : RansacHandle {
	hipStream_t stream = nullptr;       // (the caller's: the descriptor's)
	DevBuf<int32_t> scoreCount;         // [sets][maxTries] inlier count of every try
};
// SVM prediction (svm_kernels.hip; api_svm.cpp): the model on the device and the scratch of maxVectors queries; every call runs on `stream`
struct compvhip_svm : TimingState {
	compvhip_ctx* ctx = nullptr;
	hipStream_t stream = nullptr;       // (the caller's: the descriptor's)
	int kernel = 0, nrClass = 0, l = 0, dim = 0, pairs = 0;
	size_t maxVectors = 0, hostSlice = 0;   // hostSlice: vectors of one round of compvhip_svm_predict_host
	double gamma = 0.0;
	DevBuf<double> sv, svCoef, rho;     // [l][dim], [nrClass - 1][l], [pairs]
	DevBuf<int32_t> nSV, label;         // [nrClass]
	DevBuf<uint64_t> expTable;          // [2048] (RBF)
	DevBuf<double> kvalues;             // [maxVectors][l]
	DevBuf<double> hostVectors, hostDec; DevBuf<int32_t> hostLabels;   // staging of the host form: [hostSlice][dim] (float32 or float64), [hostSlice][pairs], [hostSlice]
};
// lens undistortion (remap_kernels.hip's kRemapUndist, undistort_kernels.hip; api_undistort.cpp): the geometry of the fused form and the staging of the
// cameras' coefficient records and of the poses; every call runs on `stream`
struct compvhip_undistort : TimingState {
	compvhip_ctx* ctx = nullptr;
	hipStream_t stream = nullptr;       // (the caller's: the descriptor's)
	size_t W = 0, H = 0, S = 0, frames = 0, Wout = 0, Hout = 0, x0 = 0, y0 = 0, maxSets = 0, maxPoints = 0;
	WarpTables stage;                   // device copy and pinned ring, sized by compvhip_undistort_create for the largest call: no later call allocates
};
// ORB pyramid (scale_kernels.hip, fast_kernels.hip, orb_kernels.hip): the levels' geometry and the scratch they share.  `active` levels (a prefix: the sizes
// only shrink) are at least 37 x 37; the others are empty.
struct compvhip_orbpyr : TimingState {
	compvhip_ctx* ctx = nullptr;
	size_t W = 0, H = 0, S = 0, frames = 0, cornerCap = 0;
	compvhip_orbpyr_opts opts = {};
	int active = 0;
	struct Level { size_t W = 0, H = 0, S = 0; float sf = 0.f; int quota = 0; uint8_t* plane = nullptr; uint8_t* blurred = nullptr; } lv[kPyrMaxLevels];   // plane / blurred: views into planes / blurredAll
	DevBuf<uint8_t> planes;             // levels 1 .. active - 1, [frames][H_l][S_l] each, one allocation
	DevBuf<uint8_t> blurredAll;         // levels 0 .. active - 1 blurred, one allocation (first describe)
	DevBuf<compvhip_corner> corners;    // [frames][cornerCap], one level at a time
	DevBuf<int> fastWork; DevBuf<uint8_t> fastScores;         // as compvhip_plan's, sized for level 0
	DevBuf<int32_t> index;              // [frames][keyCap] source indices of a level's survivors
	DevBuf<int32_t> counts;             // [levels][frames] FAST counts, [levels][frames] survivors, [levels + 1][frames] running totals (row 0 stays 0)
	const uint8_t* planesOf = nullptr;  // (the caller's) the d_gray the level planes were scaled from (nullptr: none yet)
	const uint8_t* blurredOf = nullptr; // the same for the blurred planes
	uint16_t kern[5] = {}; bool briefLds = kOrbBriefLdsDefault;
};
namespace compvhip_api {

inline int fail(compvhip_ctx* ctx, int code, const char* what, hipError_t e = hipSuccess)
{
	if (ctx) {
		ctx->err = what ? what : "";
		if (e != hipSuccess) { ctx->err += ": "; ctx->err += hipGetErrorString(e); }
	}
	return code;
}

// Batches beyond kMaxFramesPerLaunch frames (frame_slices.hpp; include/compv_hip.h, "Batches beyond 65 535 frames").  A call whose launchers carry the frame
// index in blockIdx.y / .z without slicing refuses such a batch here, BEFORE it allocates or enqueues anything: the answer never depends on what the runtime
// makes of an oversized grid, and a sequence of launches never runs behind a rejected first one.  `what`: the call, for the message.
inline int refuseBeyondLaunchLimit(compvhip_ctx* ctx, size_t frames, const char* what)
{
	if (frames <= static_cast<size_t>(kMaxFramesPerLaunch)) return COMPVHIP_OK;
	return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, (std::string(what) + ": more than " + std::to_string(kMaxFramesPerLaunch) + " frames in one batch").c_str());
}

#define HIPCHK(ctx, call) do { hipError_t e__ = (call); if (e__ != hipSuccess) return fail((ctx), COMPVHIP_E_HIP, #call, e__); } while (0)

// what a host-memory call (host_call.hpp) returns for its frame: COMPVHIP_OK, or the first failure with the step's name; hostWait: after a wait()
inline int hostStatus(compvhip_ctx* ctx, const HostCall& hc) { return hc.ok() ? COMPVHIP_OK : fail(ctx, hc.error() == hipErrorOutOfMemory ? COMPVHIP_E_OUT_OF_MEMORY : COMPVHIP_E_HIP, hc.what(), hc.error()); }
inline int hostWait(compvhip_ctx* ctx, HostCall& hc) { hc.wait(); return hostStatus(ctx, hc); }
// `n` elements of the caller's into `buf`, reserved for them, through the call's frame
template <typename T, typename Owner>
void stageArray(Owner* owner, HostCall& hc, DevBuf<T>& buf, const T* host, size_t n) { if (hc.ok()) hc.step(buf.reserve(owner, n), "staging"); hc.upload(buf.ptr, host, n * sizeof(T)); }
// a temporary handle of such a call: destroyed when the scope ends -- declared in front of the frame, so behind its drain -- and the call's message survives that
template <typename H> struct TempHandle { compvhip_ctx* ctx; H* h; void (*destroy)(H*); ~TempHandle() { if (h) { const std::string err = ctx->err; destroy(h); ctx->err = err; } } };
// HIPCHK for a reserve or a launch of such a call: not made behind a failed copy, and the frame drains on the way out
#define HOSTSTEP(ctx, hc, call) do { if (!(hc).ok() || !(hc).step((call), #call)) return hostStatus((ctx), (hc)); } while (0)

inline size_t alignUp(size_t v, size_t a) { return (v + a - 1) / a * a; }

// timing mode 1 = every kernel; 2 = only the two kernels bench.py prices against the roofline (an event pair costs a few
// microseconds of stream time, ~0.1 ms per step when wrapped around all ~13 launches of the pipeline)
inline bool stampWanted(const compvhip_plan* p, const char* name)
{
	if (p->timing == 1) return true;
	if (p->timing == 2) return !strcmp(name, "canny_tile_kernel") || !strcmp(name, "sht_vote_kernel");
	if (p->timing == 3) return !strcmp(name, "sht_vote_kernel");
	if (p->timing == 4) return !strcmp(name, "canny_tile_kernel");
	return false;
}

inline bool takeEvent(TimingState* p, hipEvent_t* e)
{
	if (!p->eventPool.empty()) { *e = p->eventPool.back(); p->eventPool.pop_back(); return true; }
	return hipEventCreate(e) == hipSuccess;
}

struct Stamp {
	TimingState* p; hipStream_t s; size_t idx; bool on;
	Stamp(compvhip_plan* plan, hipStream_t stream, const char* name) : Stamp(plan, stream, name, stampWanted(plan, name)) {}
	template <typename H, typename = std::enable_if_t<std::is_base_of_v<TimingState, H>>>   // the handles whose timing is on / off
	Stamp(H* handle, hipStream_t stream, const char* name) : Stamp(handle, stream, name, handle->timing != 0) {}
	Stamp(TimingState* state, hipStream_t stream, const char* name, bool wanted) : p(state), s(stream), idx(0), on(wanted)
	{
		if (!on) return;
		TimingEntry t; t.name = name;
		if (!takeEvent(p, &t.a)) { on = false; return; }
		if (!takeEvent(p, &t.b)) { p->eventPool.push_back(t.a); on = false; return; }
		(void)hipEventRecord(t.a, s);
		p->timeline.push_back(t);
		idx = p->timeline.size() - 1;
	}
	~Stamp() { if (on) (void)hipEventRecord(p->timeline[idx].b, s); }
};

inline void timelineClear(TimingState* p)
{
	for (auto& t : p->timeline) { p->eventPool.push_back(t.a); p->eventPool.push_back(t.b); } // events are reused, not re-created
	p->timeline.clear();
}

inline void timelineCollect(TimingState* p)
{
	p->timingNames.clear(); p->timingMs.clear();
	for (auto& t : p->timeline) {
		float ms = 0.f;
		if (hipEventElapsedTime(&ms, t.a, t.b) != hipSuccess) ms = -1.f;
		p->timingNames.push_back(t.name); p->timingMs.push_back(ms);
	}
	timelineClear(p);
}

// the body of the *_get_timing entry points: wait for the entries still pending, collect them, hand out up to cap of the last collection
inline int timingRead(TimingState* p, int device, const char** names, float* ms, int cap)
{
	(void)hipSetDevice(device);
	if (!p->timeline.empty()) {
		for (auto& t : p->timeline) (void)hipEventSynchronize(t.b);
		timelineCollect(p);
	}
	const int n = std::min<int>(cap, static_cast<int>(p->timingMs.size()));
	for (int i = 0; i < n; ++i) { if (names) names[i] = p->timingNames[i].c_str(); if (ms) ms[i] = p->timingMs[i]; }
	return n;
}

// the events of the timeline and of the pool (the destroy functions; the handle's device is current)
inline void timingTeardown(TimingState* p)
{
	timelineClear(p);
	for (hipEvent_t e : p->eventPool) (void)hipEventDestroy(e);
	p->eventPool.clear();
}

// the bodies of the destroy, set_timing and get_timing entry points of the handles whose timing is on / off (matcher, pyramid, homography, curve fit)
template <typename H>
void handleDestroy(H* h)
{
	if (!h) return;
	(void)hipSetDevice(h->ctx->device);
	timingTeardown(h);
	delete h;
}
template <typename H>
int handleSetTiming(H* h, int enabled)
{
	if (!h) return COMPVHIP_E_INVALID_PARAMETER;
	h->timing = enabled != 0;
	return COMPVHIP_OK;
}
template <typename H>
int handleGetTiming(H* h, const char** names, float* ms, int cap)
{
	if (!h) return COMPVHIP_E_INVALID_PARAMETER;
	return timingRead(h, h->ctx->device, names, ms, cap);
}

// an asynchronous step of the plan has not been waited for (its replay would rewrite the plan's masks and the caller's lines)
inline bool stepsInFlight(const compvhip_plan* p)
{
	for (const auto& stp : p->steps) if (stp.used) return true;
	return false;
}

// the byte spans [a, a + bytesA) and [b, b + bytesB) share a byte
inline bool overlaps(const uint8_t* a, size_t bytesA, const uint8_t* b, size_t bytesB) { return (a < b + bytesB) && (b < a + bytesA); }

// one of the pointers has a bit of `mask` set (a null pointer counts as aligned)
template <typename... P>
bool misaligned(uintptr_t mask, const P*... ptrs) { return ((reinterpret_cast<uintptr_t>(ptrs) | ...) & mask) != 0; }

// ---- functions called across files ----
// api.cpp
int shtDims(size_t W, size_t H, float thetaDeg, size_t* R, size_t* T, float* step);
int ensureSht(compvhip_plan* p);
int ensureLineCap(compvhip_plan* p, size_t cap);
int validateCannyParams(compvhip_ctx* ctx, float tLow, float tHigh, int ksize, int type, int* lo, int* hi);
int pixfmtBytes(int fmt);
int checkPixfmt(compvhip_ctx* ctx, int fmt, size_t W);   // a format the grayscale kernel converts, at a width it can have
int checkFxpKernel(compvhip_ctx* ctx, size_t W, size_t H, const uint16_t* vt, const uint16_t* hz, size_t k);
// How many key slots the line sort covers (the reference sorts lines.size() elements, houghsht.cxx:241-249):
//   kSortAll   the whole capacity, unused slots zeroed by sht_lines_kernel -- the stream-ordered entry point, which may not wait for the device;
//   kSortExact the slots in use, read back behind sht_lines_kernel (one stream synchronisation) -- the synchronous step, which ends in one anyway;
//   otherwise  that many slots (a prediction: the asynchronous step; the caller checks it against the real total later).
constexpr size_t kSortAll = ~static_cast<size_t>(0), kSortExact = kSortAll - 1;
struct ShtOpts {
	bool clearTimeline = true;   // the call starts a new timeline (a step's Canny stage has started it already: false)
	bool pairsOnly = false;      // stop at the (key, cell) pairs in emission order: no sort, no decode (the host entry point orders them itself)
	size_t sortN = kSortAll;
	int* hostSlot = nullptr;     // asynchronous steps: the ticket's pinned slot as the device sees it (ShtArgs::hostStep); nullptr: nothing is reported
};
int planShtImpl(compvhip_plan* p, const uint8_t* d_edges, int threshold, int maxLines, compvhip_line* d_lines, size_t lineCap, int32_t* d_counts,
                hipStream_t st, const ShtOpts& o);
// api_features.cpp
constexpr size_t kFitMaxSide = 8192;   // the central moments stay below 2^63 up to here
constexpr int kFitMaxHalfWidth = 8;
int segmentsImpl(compvhip_plan* p, const uint8_t* d_edges, size_t edgeStride, const compvhip_line* d_lines, const int32_t* d_counts, size_t lineCap,
                 int maxLines, int minLength, int maxGap, compvhip_segment* d_segs, size_t segCap, int32_t* d_segCounts, hipStream_t st);
int fitImpl(compvhip_plan* p, const uint8_t* d_edges, size_t edgeStride, const compvhip_line* d_lines, const int32_t* d_counts, size_t lineCap, int maxLines,
            int halfWidth, const compvhip_segment* d_segs, const int32_t* d_segCounts, size_t segCap, compvhip_line_fit* d_fits, size_t fitCap,
            int32_t* d_fitCounts, compvhip_line* d_refined, hipStream_t st);
int componentsImpl(compvhip_plan* p, const uint8_t* d_edges, size_t edgeStride, int connectivity, int minPixels, int32_t* d_labels, size_t labelStride,
                   compvhip_component* d_comps, size_t compCap, int32_t* d_compCounts, hipStream_t st);
int checkAdaptive(compvhip_ctx* ctx, size_t W, size_t H, size_t blockSize, double delta, double maxVal);
int morphPrepare(compvhip_ctx* ctx, size_t W, size_t H, const uint8_t* strel, size_t sw, size_t sh, int op, int border, int kernel, MorphArgs* a);
int checkFast(compvhip_ctx* ctx, size_t W, size_t H, int fastType);
int checkOrb(compvhip_ctx* ctx, size_t W, size_t H, float scale);
int hogGeometry(compvhip_ctx* ctx, size_t W, size_t H, const compvhip_hog_opts* opts, HogArgs* a);   // the definition's items 5, 6, 8: refusals, defaults, geometry
// image statistics on frames [frames][H][S] in device memory: the bodies of the plan calls (plan: whose timing they feed) and of the host calls (plan == nullptr)
int integralDims(compvhip_ctx* ctx, size_t W, size_t H);   // the integral image's limits: 1 <= W, H <= 32 767, W * H < 2^31
struct StatsFrames { compvhip_ctx* ctx; compvhip_plan* plan; StatsScratch* scratch; const uint8_t* d_gray; size_t W, H, S, frames; hipStream_t st; };
int integralImpl(const StatsFrames& g, double* d_sum, double* d_sumsq, size_t sumStride);
int histogramImpl(const StatsFrames& g, uint32_t* d_hist);
int equalizeImpl(const StatsFrames& g, const uint32_t* d_hist, double scale, uint8_t* d_out, uint8_t* d_lut);
int projectionsImpl(const StatsFrames& g, int32_t* d_projX, int32_t* d_projY);
// colour conversion: every refusal of compvhip_convert_frames (host or device pointers alike); fills `a`, the planes' row counts and least row bytes
struct ConvertGeometry { int planesIn, planesOut; size_t minIn[3], rowsIn[3], minOut[3], rowsOut[3]; };
int convertCheck(compvhip_ctx* ctx, size_t W, size_t H, size_t frames, const compvhip_image* in, const compvhip_image* out, ConvertArgs* a, ConvertGeometry* g);
int scaleImpl(compvhip_ctx* ctx, const uint8_t* d_in, size_t W, size_t H, size_t S, size_t frames, uint8_t* d_out, size_t Wout, size_t Hout, size_t Sout, hipStream_t st);
// api_host.cpp: the caller's validated plane (rows S pixels of bpp bytes apart) into `buf` at rows of alignUp(W, 64) pixels, through the frame; returns that row length
size_t stagePlane(compvhip_ctx* ctx, HostCall& hc, DevBuf<uint8_t>& buf, const void* in, size_t W, size_t H, size_t S, size_t bpp = 1);
// the bytes of a destination element of remap, inverse warp and undistortion; 0: not one of their interpolations
inline size_t interpElemBytes(int i)
{
	return i == COMPVHIP_INTERP_NEAREST || i == COMPVHIP_INTERP_BILINEAR || i == COMPVHIP_INTERP_BICUBIC ? 1 : i == COMPVHIP_INTERP_BILINEAR_FLOAT32 || i == COMPVHIP_INTERP_BICUBIC_FLOAT32 ? sizeof(float) : 0;
}
// remap and inverse warp: validates everything but the coordinate source and fills `a` (roi == nullptr: the whole frame)
int remapPrepare(compvhip_ctx* ctx, const uint8_t* d_in, size_t W, size_t H, size_t S, size_t frames, int interp, const compvhip_roi* roi, void* d_out, size_t Wout,
                 size_t Hout, size_t Sout, uint8_t defaultValue, RemapArgs* a);
// builds the tables of `count` matrices in a staging slot of `t`, enqueues their upload and points `a` at the device copy
int warpUpload(compvhip_ctx* ctx, WarpTables* t, const float* M, int rows, size_t count, RemapArgs* a, hipStream_t st);
MatchSliceArgs matchForward(const compvhip_matcher* m, const uint8_t* d_query, size_t queryStride, const int32_t* d_queryCounts, const uint8_t* d_train, size_t trainStride,
                            const int32_t* d_trainCounts, int trainShared, compvhip_match* d_matches);
// api_undistort.cpp.  The ring of `t` for any table: the next slot with room for `floats` floats (waits for the copy that last read it), and its upload
// into t->dev behind the work of `st`
int tablesSlot(compvhip_ctx* ctx, WarpTables* t, size_t floats, float** host, WarpTables::Slot** slot);
int tablesSend(compvhip_ctx* ctx, WarpTables* t, WarpTables::Slot* slot, size_t floats, hipStream_t st);
// the coordinate source kRemapUndist: builds the records of `count` float32 cameras (K [count][9], d [count][nd]; nd in 2 .. 4 was checked) in a staging
// slot of `t`, enqueues their upload and points `a` at the device copy; a singular camera: COMPVHIP_E_INVALID_PARAMETER, nothing enqueued
int undistCoords(compvhip_ctx* ctx, WarpTables* t, const float* K, const float* d, int nd, size_t count, size_t x0, size_t y0, RemapArgs* a, hipStream_t st);
bool undistWindowOk(size_t x0, size_t y0, size_t Wout, size_t Hout);   // sizes 1 .. 32767, x0 + Wout and y0 + Hout at most 32767
// api_kht.cpp
size_t hostCpuBudget();
} // namespace compvhip_api
