// kernels.hpp -- argument blocks and launchers shared between the .hip kernel files and the C-ABI host code (api.cpp).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/compv_hip.h" // compvhip_pixfmt

namespace compvhip {

// ---- Canny ------------------------------------------------------------------------------------------------
#ifndef COMPVHIP_BAND_H
#define COMPVHIP_BAND_H 64
#endif
constexpr int kBandH = COMPVHIP_BAND_H;            // rows per resolve band
#ifndef COMPVHIP_BAND_WORDS
#define COMPVHIP_BAND_WORDS 64
#endif
constexpr int kBandWords = COMPVHIP_BAND_WORDS;        // 32-px words per resolve chunk (2048 columns): 0.056 ms per step at 4K, 0.075 ms with 128
constexpr int kResolveThreads = 512;
// Per-frame counters that many workgroups hit with atomics (Sobel gmax, the pixel sum of the mean thresholds) sit one per 128-byte line: the
// L2 serialises the atomics of a line, and the counters of 32 frames side by side are ONE line.
constexpr int kFrameSlot = 32;
constexpr int kResolveRows = kBandH * kBandWords / kResolveThreads; // rows of one word column a resolve thread owns (8)

struct CannyArgs {
	const uint8_t* in;
	uint8_t* out;
	uint32_t* ebits;
	uint32_t* ubits;
	const int2* thrDev;       // per-frame {tLow,tHigh} (PERCENT_OF_MEAN) or nullptr
	size_t inFrameStride, outFrameStride, bitsFrameStride; // elements
	int W, H, S, So;
	int wb;                   // words per bitmask row (= tilesX*16)
	int tilesX, tilesY;
	int tLow, tHigh;
	int simdEnd, cStart;      // quirk Q3 coverage: [1,simdEnd) U [cStart,W-1)
	int blockRows, groups;    // filled by the launcher: workgroup rows per frame, row groups in the launch (XCD-aware map)
	int ksize;                // Sobel kernel size of the gradient: 3 or 5
	int* zero; int nZero;     // counters the STEP needs cleared before its next kernel (edge / line / tile / block counts, round flags): the first nZero / 64 workgroups
	                          // of the tile kernel clear 64 each -- a hipMemsetAsync per step was one more launch on the lane's chain (nullptr: nothing to clear)
};

struct ResolveArgs {
	uint32_t* ebits;
	uint32_t* ubits;
	uint8_t* out;             // byte map to patch with the promoted pixels (nullptr: masks only)
	int* flags;               // flags[round] = 1 when round changed something
	uint8_t* dirty;           // [4][frames][bands][chunks]: which workgroups changed their band in round (r & 3)
	size_t outFrameStride, bitsFrameStride;
	int H, So, wb;
	int round;
};

hipError_t launch_canny_tiles(const CannyArgs& a, int frames, bool gap, hipStream_t stream);
hipError_t launch_canny_tiles_swar(const CannyArgs& a, int frames, bool gap, hipStream_t stream); // kernel size 3 (canny_swar_kernels.hip)
hipError_t launch_canny_resolve(const ResolveArgs& a, int frames, hipStream_t stream);
size_t canny_resolve_dirty_bytes(int H, int wb, int frames);
hipError_t launch_mean_thresholds(const uint8_t* in, int W, int H, int S, size_t frameStride, int frames, float fLow, float fHigh,
                                  unsigned int* sums, int2* thr, hipStream_t stream);

// ---- Sobel / Scharr / Prewitt detector -------------------------------------------------------------------
struct EdgeDeteArgs {
	const uint8_t* in;
	uint8_t* out;
	unsigned int* gmax;       // per frame, one counter per 128-byte line: gmax[frame * kFrameSlot]
	size_t inFrameStride, outFrameStride;
	int W, H, S, So;
	int tilesX, tilesY;
	int blockRows, groups;    // filled by the launcher (XCD-aware map)
};
hipError_t launch_edge_dete(const EdgeDeteArgs& a, int op, int frames, hipStream_t stream);

// ---- colour conversion (convert_kernels.hip) -----------------------------------------------------------------
struct ConvertArgs {
	const uint8_t* in[3];     // planes of the source (unused: nullptr), any byte address
	uint8_t* out[3];          // planes of the destination
	size_t inRow[3], inFrame[3], outRow[3], outFrame[3];   // bytes from row to row and from frame to frame, per plane
	int W, H;
};
// The (inFmt, outFmt) pair must be one that conv::served() lists (hipErrorInvalidValue otherwise).  Any frame count: sliced.
hipError_t launch_convert(const ConvertArgs& a, int inFmt, int outFmt, int frames, hipStream_t stream);

// ---- pre-processing (grayscale, Otsu) -----------------------------------------------------------------------
struct GrayArgs {
	const uint8_t* in;        // [frames][H][S samples of bpp bytes]
	uint8_t* out;             // [frames][H][So]
	int W, H, S, So;
};
hipError_t launch_gray(const GrayArgs& a, int fmt, int frames, hipStream_t stream);
constexpr int kOtsuMaxChunks = 128; // row chunks (= workgroups) per frame of the histogram kernel
// hist: [frames][kOtsuMaxChunks][256] u32 scratch (partial histograms); otsu: int32 per frame (or null); thr: int2 {tLow,tHigh} per frame (or null)
hipError_t launch_otsu(const uint8_t* in, int W, int H, int S, size_t frameStride, int frames, float fLowFactor, float fHighFactor, uint32_t* hist,
                       int32_t* otsu, void* thr, hipStream_t stream);

// ---- fixed-point separable convolution (Gaussian pre-blur) ---------------------------------------------------
constexpr int kFxpMaxTaps = 15;
struct FxpArgs {
	const uint8_t* in;
	uint8_t* out;
	size_t inFrameStride, outFrameStride;
	int W, H, S, So;
	uint32_t kern[kFxpMaxTaps]; // Q16 weights of this pass
};
hipError_t launch_convlt_fxp(const uint8_t* in, uint8_t* tmp, uint8_t* out, int W, int H, int S, size_t frameStride, int frames, const uint16_t* vtKern,
                             const uint16_t* hzKern, int K, hipStream_t stream);

// integer separable correlation, int16 out (CompVMathConvlt::convlt1<u8|s16, s16, s16>)
struct I16Args {
	const void* in;           // u8 or s16 rows of S elements
	int16_t* out;             // s16 rows of So elements
	int W, H, S, So, K;
	int kern[kFxpMaxTaps];    // taps of this pass
};
hipError_t launch_convlt_i16(const void* in, bool inIsU8, int16_t* tmp, int16_t* out, int W, int H, int S, int So, const int16_t* vtKern, const int16_t* hzKern,
                             int K, hipStream_t stream);

// ---- Hough SHT ---------------------------------------------------------------------------------------------
struct ShtArgs {
	const uint32_t* ebits;    // edge bit masks [frames][H][wb]
	uint32_t* edges;          // per-tile edge lists of every frame: (ly << 16) | lx, edgeCap entries per frame
	int* edgeCounts;          // per frame
	uint16_t* acc;            // [frames][T][accPitch], u16: a cell never exceeds 65535
	const int32_t* sinQ;      // [T]
	const int32_t* cosQ;      // [T]
	uint32_t* lineKeys;       // [frames * lineCap] sort keys: frameTag << strengthBits | strength -- DENSE: frame f's lines follow frame f-1's (min(count, lineCap) each)
	uint32_t* lineVals;       // [frames * lineCap] their accumulator cells: row * T + col
	uint8_t* nmsFlags;        // [frames][nmsGroups][nmsRows] NMS survivors: bit j of byte (group, row) = column 8 group + j
	int nmsRows;              // rows of a flag plane
	int* blockCounts;         // [frames][lineBlocks] NMS survivors per 64 accumulator rows (one row block of sht_lines_kernel); accumulated by sht_nms_kernel (zeroed per step)
	int lineBlocks;
	const int2* nmsRange;     // [nmsGroups] accumulator rows [x, y) the windows of the group's columns (+ one either side) can reach, widened by one row
	int nmsGroups;            // groups of 8 theta columns
	int* lineCounts;          // per frame
	const int* stepFlags;     // asynchronous steps: the hysteresis round flags of this step (device) ...
	int* hostStep;            // ... and where the host wants them: a device-mapped PINNED HOST slot, [0] = the line total, [kFrameSlot .. + 3] = the first four round flags;
	                          // written by one wave of sht_lines_kernel (nullptr: not an asynchronous step) -- a device-to-host copy per step was one more operation on the lane's chain
	int32_t* outCounts;       // the caller's per-frame line counts (device, may be nullptr): written with lineCounts by sht_lines_kernel -- a device copy per step was one more launch
	int* frameTotals;         // [frames * kFrameSlot] NMS survivors per frame, one counter per 128-byte line (sht_nms_kernel adds its row blocks, zeroed per step)
	unsigned int* lineTotal;  // sum over the frames of min(survivors, lineCap) = the key slots in use (written by sht_lines_kernel)
	size_t sortN;             // key slots the sort will cover: sht_lines_kernel zeroes [lineTotal, sortN) (0: nothing to pad -- the sort is sized after the fact)
	size_t bitsFrameStride, edgeCap, accFrameStride, lineCap;
	int W, H, wb;
	int R, T, accPitch, barrier;
	int threshold, nmsLastCol;
	int frames;
	int strengthBits;         // bits of the strength field of a line key (2^strengthBits > 2*max(W,H) >= any cell count)
};
// voting (sht_tiles_kernels.hip): image tiles, lane = theta
struct ShtTileArgs {
	const int32_t* kt;        // [tiles][T]  window constant K of (tile, theta): window row = (K - lx cosQ - ly sinQ) >> 16
	const int32_t* rowBase;   // [tiles][T]  accumulator row of window row 0
	uint8_t* partLo;          // [frames][tiles][Tpad][rwPitch]  theta-major partial accumulators (one window per tile and theta): low bytes of the counts
	uint8_t* partHi;          // same shape: high bytes, valid only for the (tile, theta) columns whose colFlag is set (some count of the column >= 256)
	uint8_t* colFlag;         // [frames][tiles][Tpad]  written by every vote workgroup for its 64 columns
	const int2* reach;        // [T]  accumulator rows [x, y) the tiles' windows of a theta cover (their union's hull)
	int* tileCounts;          // [frames][tiles] edges per tile
	int nx, ny, TW, TH, tiles;  // tile grid; TW % 32 == 0
	int Rw, rwPitch;          // window rows (<= 1264), pitch of a partial row (multiples of 16)
	int Tpad, groups;         // theta bins padded to groups * 64
	size_t tileCap;           // edge-list entries per tile (TW * TH)
};
constexpr int kShtMaxWindow = 1264;   // window rows of a vote workgroup: 1264 * 128 B = 158 KB of LDS
hipError_t launch_sht_compact_tiles(const ShtArgs& a, const ShtTileArgs& v, int frames, hipStream_t stream);
hipError_t launch_sht_vote_tiles(const ShtArgs& a, const ShtTileArgs& v, int frames, hipStream_t stream);
hipError_t launch_sht_reduce_tiles(const ShtArgs& a, const ShtTileArgs& v, int frames, hipStream_t stream);
hipError_t launch_bytes_to_bits(const uint8_t* edges, int W, int H, int S, size_t frameStride, uint32_t* ebits, int wb, size_t bitsFrameStride,
                                int frames, hipStream_t stream);
hipError_t launch_sht_lines(const ShtArgs& a, int frames, hipStream_t stream);
hipError_t launch_sht_decode(const uint32_t* keys, const uint32_t* vals, const int* counts, size_t lineCap, int frames, int T, int barrier, float thetaStep,
                             int maxLines, int strengthBits, void* lines /*compvhip_line*/, size_t outCap, hipStream_t stream);
int sht_nms_groups(int T);
size_t sht_nms_rows(int R);
int sht_lines_blocks(int R);
// acc [T][pitch] -> reference layout [R][stride]
// maxLines > 0: only the first min(count, lineCap, maxLines) lines of a frame are converted (what sht_decode_kernel wrote)
// a line whose theta is col * thetaStep takes cos / 1 / sin from the tables; any other theta (a refined line) is evaluated on the device
hipError_t launch_sht_cartesian(const void* lines /*compvhip_line*/, const int* counts, size_t lineCap, int maxLines, int frames, int T, const float* cosT,
                                const float* invSinT, float thetaStep, float widthF, float r, float* out /*[frames][lineCap][4]*/, hipStream_t stream);
hipError_t launch_sht_acc_transpose(const uint16_t* accT, int R, int T, int accPitch, int32_t* out, size_t outStride, hipStream_t stream);
// the line sort sized on the device (sht_sort_kernels.hip): counting sort on the strength, stable ranks counted in order inside chunks of lines
constexpr int kShtSortChunk = 8192;             // lines per chunk (one workgroup); a power of two below 65 536 (the chunk histogram is u16)
constexpr int kShtSortMaxStrengthBits = 13;     // 8192 strength bins: max(W, H) <= 4095
constexpr int kShtSortMaxChunks = 16;           // chunks per frame it is used for (line capacities up to 131 072 per frame)
struct ShtSortArgs {
	uint32_t* rankKeys;       // [frames * lineCap] per line, at its emission-order position (that of lineKeys / lineVals, which stay as they are: a replayed step
	                          // reads them again): (inverted strength << 13) | number of earlier lines of its chunk with the same strength
	uint16_t* chunkHist;      // [frames][chunks][8192] lines per inverted strength of a chunk (written whole by the chunks that have lines)
	uint32_t* strengthStart;  // [frames][8192] first slot of an inverted strength in the frame's sorted line list
	int chunks;               // chunks per frame = ceil(lineCap / 8192)
};
hipError_t launch_sht_sort_lines(const ShtArgs& a, const ShtSortArgs& q, int frames, float thetaStep, int maxLines, void* lines /*compvhip_line*/, size_t outCap,
                                 hipStream_t stream);
// one stable descending radix sort over the first n (key, value) slots; temp == nullptr queries tempBytes (for n = the capacity)
hipError_t sht_sort_pairs(void* temp, size_t& tempBytes, const uint32_t* keysIn, uint32_t* keysOut, const uint32_t* valsIn, uint32_t* valsOut, size_t n,
                          int keyBits, hipStream_t stream);

// ---- Hough SHT line segments and line refinement (sht_segments_kernels.hip, sht_fit_kernels.hip) ----------------------------------
// what both walks read: the edge pixels, the vote's tables and the lines (24 trailing bytes of ints: the structs derived from it keep the layout
// they had with these fields written out)
struct ShtLineSetArgs {
	const uint32_t* ebits;    // edge bit masks [frames][H][wb] (read when edges == nullptr)
	const uint8_t* edges;     // or byte edge maps [frames][H][S], non-zero = edge
	size_t bitsFrameStride, edgeFrameStride;
	int wb, S;
	const int32_t* sinQ;      // [T] the vote's Q16 tables
	const int32_t* cosQ;
	const compvhip_line* lines;   // [frames][lineCap]; only row / col are read
	const int32_t* lineCounts;    // [frames] lines found (may exceed lineCap)
	size_t lineCap;
	int nLines;               // lines considered per frame at most: min(lineCap, maxLines if > 0)
	int W, H, R, T, barrier;
};
struct ShtSegArgs : ShtLineSetArgs {
	int minLength, maxGap;
	int32_t* perLine;         // [frames][nLines] scratch: segments per line, then their exclusive prefix sums
	compvhip_segment* segs;   // [frames][segCap]
	size_t segCap;
	int32_t* segCounts;       // [frames] segments found (before clipping to segCap)
	int frame0;               // filled by the launcher
};
// phase 0: count the segments of every line; 1: exclusive scan per frame + segCounts; 2: write the segments
hipError_t launch_sht_segments(const ShtSegArgs& a, int frames, int phase, hipStream_t stream);

struct ShtFitArgs : ShtLineSetArgs {
	int halfWidth;            // 0 .. 8 rho cells either side of the line's
	const compvhip_segment* segs; // [frames][segCap] per-segment mode (nullptr: one record per line)
	const int32_t* segCounts;     // [frames] segments found (may exceed segCap)
	size_t segCap;
	compvhip_line_fit* fits;  // [frames][fitCap]
	size_t fitCap;
	int32_t* fitCounts;       // [frames] records (before clipping to fitCap)
	compvhip_line* refined;   // [frames][lineCap] the lines with the fitted rho / theta (per-line mode, may be nullptr)
	int frame0;               // filled by the launcher
};
static_assert(sizeof(ShtLineSetArgs) == 104 && sizeof(ShtSegArgs) == 152 && sizeof(ShtFitArgs) == 176, "kernel argument layout");
hipError_t launch_sht_fit(const ShtFitArgs& a, int frames, hipStream_t stream);

// ---- connected components of edge maps (components_kernels.hip) -------------------------------------------------
struct CompArgs {
	const uint32_t* bits;     // edge bit masks [frames][H][wb]: the plan's own, or the plan's packed copy of a byte map
	size_t bitsFrameStride;
	int wb;
	int W, H;
	int words;                // mask words of a row that hold columns < W: ceil(W / 32)
	uint32_t lastMask;        // the bits of word `words - 1` that are columns < W
	int conn8;                // 8-connectivity (else 4)
	int minPixels;
	int32_t* parent;          // [frames][H][ps]: parent words, then labels -- the caller's label map, or the plan's scratch (ps == W)
	size_t parentFrameStride;
	int ps;
	int wantLabels;           // parent is the caller's label map: finish it (ids on every foreground pixel, 0 elsewhere)
	compvhip_component* comps;    // [frames][compCap]
	size_t compCap;
	int32_t* compCounts;      // [frames] survivors (before clipping to compCap)
	int32_t* rowCounts;       // [frames][H] scratch: survivors whose root lies in a row, then their exclusive prefix sums
	int frame0;               // filled by the launcher
};
// phases 0..8 in launch order: tiles, tile borders, flatten, pixel counts, survivors per row, row scan, ids + records, boxes (+ labels of the
// non-root pixels), label map roots + background
hipError_t launch_components(const CompArgs& a, int frames, int phase, hipStream_t stream);

// ---- thresholding and morphology (morph_kernels.hip) --------------------------------------------------------------------------------
struct ThreshArgs {
	const uint8_t* in;        // [frames][H][S]; may be `out`
	uint8_t* out;
	const int32_t* levels;    // per-frame level (device; clipped to 0..255) or nullptr: t8 for every frame
	size_t frameStride;
	int W, H, S;
	int t8;
};
hipError_t launch_threshold(const ThreshArgs& a, int frames, hipStream_t stream);
struct AdaptArgs {
	const uint8_t* in;        // [frames][H][S]; must not overlap `out` (a tile reads the halo its neighbours write)
	uint8_t* out;
	size_t frameStride;
	int W, H, S;
	int r;                    // blockSize / 2: 1..15
	uint32_t k;               // the Q16 tap of the mean kernel
	int delta, maxVal, invert;
};
hipError_t launch_threshold_adaptive(const AdaptArgs& a, int frames, hipStream_t stream);
constexpr int kMorphMaxStrel = 31;
constexpr size_t kMorphGeneralMaxMembers = 15;   // compvhip_plan_morph sends a rectangle / cross of at most this many members to the general kernel
enum { kMorphGeneral = 0, kMorphRect = 1, kMorphCross = 2 };   // kernel of one basic operation
struct MorphArgs {
	const uint8_t* in;        // [frames][H][S]; must not overlap `out`
	uint8_t* out;
	size_t frameStride;
	int W, H, S;
	int sw, sh;               // odd, 1..31
	int dilate;               // max (else min)
	int replicate;            // border cells take in(y, x) (else 0)
	int kind;                 // kMorphGeneral: rows[] is read; kMorphRect / kMorphCross: sw and sh say it all
	uint32_t rows[kMorphMaxStrel];   // bit i of rows[j]: (j, i) is a member
};
hipError_t launch_morph(const MorphArgs& a, int frames, hipStream_t stream);

// ---- FAST corners (fast_kernels.hip) ----------------------------------------------------------------------------------------------------
struct FastArgs {
	const uint8_t* in;        // [frames][H][S]
	uint8_t* scores;          // [frames][H][S]: the caller's map or the plan's; must not overlap `in`
	size_t frameStride;
	int W, H, S;
	int t, N, nonmax;         // t in 0..255, N 9 or 12
	int maxFeatures;          // > 1: cut at the maxFeatures-th largest strength (hist and minScore are used)
	int* rowCounts;           // [frames][H] corners per row; ZEROED by the caller before the launch
	int* rowOffsets;          // [frames][H] their exclusive scan
	int* hist;                // [frames][256] corners per score; ZEROED by the caller before the launch
	int* minScore;            // [frames] the smallest score of the list
	compvhip_corner* corners; size_t cornerCap;   // [frames][cornerCap]
	int32_t* counts;          // [frames] corners before clipping
};
// stage 0: score + NMS (score map, row counts, histogram); stage 1: [cut level -> row recount ->] scan -> emit
hipError_t launch_fast(const FastArgs& a, int frames, int stage, hipStream_t stream);

// ---- brute-force Hamming matching (match_kernels.hip) ------------------------------------------------------------------------------------
constexpr int kMatchQueryBlock = 256;     // queries of one workgroup of the slice kernel: one per lane
constexpr int kMatchTrainSlice = 128;     // train rows one workgroup stages in LDS
constexpr int kMatchMaxKnn = 8;
constexpr int kMatchMaxDwords = 32;       // 128 descriptor bytes
struct MatchSliceArgs {
	const uint8_t* query;     // [pairs][queryCap] rows of queryStride bytes ([queryCap] rows when queryShared)
	const uint8_t* train;     // the same for the train side
	const int32_t* queryCounts; const int32_t* trainCounts;   // device counts per pair (one count on a shared side); nullptr: the capacity
	int queryCap, trainCap, queryStride, trainStride;
	int queryShared, trainShared;
	int descDwords;           // 1..32
	int knn;                  // 1..8
	int slices;               // (trainCap + kMatchTrainSlice - 1) / kMatchTrainSlice
	uint32_t* partial;        // [pairs][slices][knn][queryCap] keys: distance << 16 | row within the slice
	compvhip_match* matches;  // [pairs][knn][queryCap], 16-byte aligned
};
hipError_t launch_match_slices(const MatchSliceArgs& a, int pairs, hipStream_t stream);
hipError_t launch_match_merge(const MatchSliceArgs& a, int pairs, hipStream_t stream);
// the reference's own order among equal distances (partial is not used, but must be there): one lane per query walks every train row
hipError_t launch_match_reference(const MatchSliceArgs& a, int pairs, hipStream_t stream);
struct MatchGoodArgs {
	const compvhip_match* matches;   // [pairs][knn][queryCap]
	const compvhip_match* reverse;   // [pairs][trainCap]: the best query of every train row (crossCheck only)
	const int32_t* queryCounts; const int32_t* trainCounts;
	int queryCap, trainCap, trainShared, knn;
	double ratio; int maxDistance, crossCheck;
	compvhip_match* good; size_t goodCap;   // [pairs][goodCap], 16-byte aligned
	int32_t* counts;                 // [pairs] good matches before clipping
};
hipError_t launch_match_good(const MatchGoodArgs& a, int pairs, hipStream_t stream);

// ---- RANSAC homography (homography_kernels.hip) ---------------------------------------------------------------------------------------------
constexpr int kHomographySolveBlock = 64;    // tries of one workgroup of the solve kernel: one per lane, one wave (162 float64 of LDS per lane)
constexpr int kHomographyScoreBlock = 256;   // tries of one workgroup of the score kernel, and the points it stages per round
struct HomographyPointsArgs {
	const compvhip_match* good; int goodCap;          // [pairs][goodCap]
	const int32_t* goodCounts;                        // [pairs] (may exceed goodCap, may be negative); nullptr: goodCap
	const compvhip_keypoint* query; int queryCap;     // [pairs][queryCap]
	const compvhip_keypoint* train; int trainCap;     // [pairs][trainCap], or [trainCap] when trainShared
	int trainShared;
	double2* src; double2* dst; int pointCap;         // [pairs][pointCap]: train / query positions of the records kept
	int32_t* counts;                                  // [pairs] records kept
};
hipError_t launch_homography_points(const HomographyPointsArgs& a, int pairs, hipStream_t stream);
struct HomographyFindArgs {
	const double2* src; const double2* dst;           // [pairs][pointCap]
	const int32_t* counts; int pointCap;              // [pairs]; nullptr: pointCap
	int tries, maxTries;
	uint32_t seed; double threshold;
	const int32_t* quads;                             // nullptr or [pairs][tries][4], 16-byte aligned
	// scratch, [pairs][maxTries] each: 1 when the try has an H and an inverse; its Jacobi rotations; H then the inverse (18 float64); inlier count; variance
	int32_t* state; int32_t* rotations; double* hyp; int32_t* scoreCount; double* scoreVar;
	double2* selSrc; double2* selDst;                 // scratch [pairs][pointCap]: the inliers of the best try in index order
	compvhip_homography_result* results;              // [pairs]
	uint8_t* mask;                                    // nullptr or [pairs][pointCap]
};
hipError_t launch_homography_solve(const HomographyFindArgs& a, int pairs, hipStream_t stream);
hipError_t launch_homography_score(const HomographyFindArgs& a, int pairs, hipStream_t stream);
hipError_t launch_homography_refit(const HomographyFindArgs& a, int pairs, hipStream_t stream);
struct HomographyProjectArgs {
	const compvhip_homography_result* results;        // [pairs]
	const double2* points; int n, shared;             // [pairs][n], or [n] when shared
	double2* out;                                     // [pairs][n]
};
hipError_t launch_homography_project(const HomographyProjectArgs& a, int pairs, hipStream_t stream);

// ---- RANSAC line and parabola fits (curvefit_kernels.hip) -------------------------------------------------------------------------------------
constexpr int kCurvefitBlock = 256;          // tries of one workgroup of the score kernel and the points it stages per round; pixels of a gather round
struct CurvefitGatherArgs {
	const int32_t* labels; int W, H, labelStride;     // [frames][H][labelStride]
	const compvhip_component* comps; int compCap;     // [frames][compCap]
	const int32_t* compCounts;                        // [frames] (may exceed compCap, may be negative)
	double2* points; int pointCap;                    // [frames * compCap][pointCap]
	int32_t* counts;                                  // [frames * compCap] points taken
};
hipError_t launch_curvefit_gather(const CurvefitGatherArgs& a, int sets, hipStream_t stream);
struct CurvefitFindArgs {
	const double2* points;                            // [sets][pointCap]
	const int32_t* counts; int pointCap;              // [sets]; nullptr: pointCap
	int model, tries, maxTries;
	uint32_t seed; double threshold;
	const int32_t* samples;                           // nullptr or [sets][tries][m]
	int32_t* scoreCount;                              // scratch [sets][maxTries]: the inlier count of every try
	double2* sel;                                     // scratch [sets][pointCap]: the inliers of the best try in index order
	compvhip_curvefit_result* results;                // [sets]
	uint8_t* mask;                                    // nullptr or [sets][pointCap]
};
hipError_t launch_curvefit_score(const CurvefitFindArgs& a, int sets, hipStream_t stream);
hipError_t launch_curvefit_refit(const CurvefitFindArgs& a, int sets, hipStream_t stream);
struct CurvefitDistanceArgs {
	const double2* points; const int32_t* counts; int pointCap, model;
	const double* params;                             // [sets][3]
	double* out;                                      // [sets][pointCap]
};
hipError_t launch_curvefit_distances(const CurvefitDistanceArgs& a, int sets, hipStream_t stream);

// ---- ORB: keypoint orientation and rotated BRIEF (orb_kernels.hip) -------------------------------------------------------------------------
// the byte-read variant of orb_brief_kernel that ships: at 32 x 4K with 2000 keypoints a frame the two measured alike (0.0678 ms with the LDS patch, 0.0680 ms
// with bytes from global memory; docs/kernels/orb.md), so the first one built stays
constexpr bool kOrbBriefLdsDefault = true;
constexpr int kOrbBorder = 18;            // (31 + 5) >> 1: a keypoint lies this far from every border; a rotated pattern point reaches no further
struct OrbKeyArgs {
	const uint8_t* gray;      // [frames][H][S], the unblurred plane
	size_t frameStride;
	int W, H, S;
	const compvhip_corner* corners; size_t cornerCap;   // [frames][cornerCap]
	const int32_t* cornerCounts;                        // [frames] corners found (may exceed cornerCap, may be negative)
	int level; float scale;
	int32_t* index;           // [frames][keyCap] scratch: source index of the q-th survivor
	compvhip_keypoint* keys; size_t keyCap;             // [frames][keyCap]
	int32_t* keyCounts;       // [frames] survivors before clipping to keyCap
	int32_t* moments;         // nullptr or [frames][keyCap][2] = {m01, m10}
	// one level of a pyramid (nullptr: a list of its own, as above): the frame's records go behind the keyBase[f] records of the levels before, while they
	// fit in keyCap; keyTotal[f] = keyBase[f] + keyCounts[f].  index stays level-local.
	const int32_t* keyBase = nullptr; int32_t* keyTotal = nullptr;
};
hipError_t launch_orb_select(const OrbKeyArgs& a, int frames, hipStream_t stream);
hipError_t launch_orb_orient(const OrbKeyArgs& a, int frames, hipStream_t stream);
struct OrbDescArgs {
	const uint8_t* blurred;   // [frames][H][S], 4-byte aligned, S % 4 == 0
	size_t frameStride;
	int W, H, S;
	const compvhip_keypoint* keys; size_t keyCap;
	const int32_t* keyCounts;
	float scale;
	uint8_t* desc; size_t descStride;                   // row q of frame f at desc + (f * keyCap + q) * descStride; 4-byte aligned, descStride % 4 == 0
};
// lds: the tests read a patch staged in the LDS (else their bytes from global memory); the result does not depend on it
hipError_t launch_orb_brief(const OrbDescArgs& a, int frames, bool lds, hipStream_t stream);

// ---- ORB pyramid (orb_kernels.hip, scale_kernels.hip) ------------------------------------------------------------------------------------------
constexpr int kPyrMaxLevels = 16;
struct OrbLevelPlane {
	const uint8_t* blurred;   // [frames][H][S] of the level, or nullptr: an empty level (its keypoints get zero rows)
	size_t frameStride;
	int W, H, S;
	float scale;
};
struct OrbPyrDescArgs {     // one launch over the concatenated list: every keypoint is described on the plane of its own `level`
	OrbLevelPlane lv[kPyrMaxLevels];
	int levels;               // a keypoint's level outside 0 .. levels - 1: a zero row
	const compvhip_keypoint* keys; size_t keyCap;
	const int32_t* keyCounts;
	uint8_t* desc; size_t descStride;
};
hipError_t launch_orb_brief_pyramid(const OrbPyrDescArgs& a, int frames, bool lds, hipStream_t stream);
struct OrbPyrCountArgs {    // per-level counts [levels][frames] of the pyramid's own -> the caller's [frames][levels] arrays and totals
	const int32_t* totals;    // [frames] keypoints of the frame over all levels
	const int32_t* lvKeys;    // [active][frames] survivors per level
	const int32_t* lvCorners; // [active][frames] FAST counts per level
	int active, levels, frames;
	int32_t* keyCounts;       // [frames]
	int32_t* levelCounts;     // nullptr or [frames][levels]
	int32_t* levelCorners;    // nullptr or [frames][levels]
};
hipError_t launch_orb_pyramid_counts(const OrbPyrCountArgs& a, hipStream_t stream);

// CompVImageScaleBilinear (compv_image_scale_bilinear.cxx:48-88): one source batch, up to 16 destinations (the levels of a pyramid), one launch
struct ScaleLevel {
	uint8_t* out;             // [frames][H][S]
	size_t frameStride;
	int W, H, S;
	uint32_t sx, sy;          // (int)(((float)Win / (float)W) * 256.f), the same for y
	int copy;                 // the destination has the source's size: a copy, not the arithmetic
	int dwords;               // out, S and frameStride are multiples of 4: full groups of 4 pixels go out as one dword
	int tilesX;               // ceil(W / 256)
	int blockEnd;             // workgroups of the levels up to this one
};
struct ScaleArgs {
	const uint8_t* in;        // [frames][H][S]
	size_t frameStride;
	int W, H, S;
	int levels;
	ScaleLevel lv[kPyrMaxLevels];
};
// fills sx, sy, copy, dwords, tilesX of `lv` from the two sizes; false: a ratio outside (0, 256) or a size of 0
bool scale_level_init(ScaleLevel& lv, int Win, int Hin);
hipError_t launch_scale_bilinear(ScaleArgs& a, int frames, hipStream_t stream);   // fills blockEnd

// ---- remap and inverse warp (remap_kernels.hip) -----------------------------------------------------------------------------------------------
// CompVImageRemap::process / CompVImage::warpInverse: a per-pixel gather at coordinates that come from a float32 map or from the running-sum tables
// of a matrix (include/compv_hip.h, section "remap and inverse warp")
enum { kRemapMap = 0, kRemapWarp2 = 1, kRemapWarp3 = 2, kRemapUndist = 3 };   // coordinate source
enum { kRemapNearest = 0, kRemapBilinear = 1, kRemapBilinearF32 = 2, kRemapBicubic = 4, kRemapBicubicF32 = 5 };     // = COMPVHIP_INTERP_* (3 is unassigned)
constexpr int kRemapFramesPerGroup = 8;   // frames a workgroup loops over with one set of coordinates when the map / matrix is shared
struct RemapArgs {
	const uint8_t* in;        // [frames][H][S]
	size_t inFrameStride;
	int W, H, S;
	void* out;                // uint8 or float32 [frames][Hout][Sout]
	size_t outFrameStride;    // in elements, like Sout
	int Wout, Hout, Sout;
	const float* mapX; const float* mapY;   // kRemapMap: [1 or frames][Hout * Wout] each
	const float* tables;      // kRemapWarp2 / 3: [1 or frames] x { ac, df[, gi] of Wout values, by, ey[, hy] of Hout values }; kRemapUndist: [1 or frames] x 14 coefficients (undistort_math.hpp)
	size_t coordFrameStride;  // floats from one frame's map / tables to the next (ignored when they are shared)
	float left, right, top, bottom;   // the clipped ROI: inside the frame, or empty (left > right)
	int defaultValue;         // 0 .. 255
	int frames;
	int framesPerGroup, group0, tilesX, wide, mapVec;   // filled by launch_remap
	int originX, originY;     // kRemapUndist: output pixel (i, j) is pixel (originX + i, originY + j) of the undistorted frame; origin + size <= 32767
};
// perFrame: every frame has a map / tables of its own (coordFrameStride apart); otherwise all frames share the first.  S >= 2 (the bilinear forms load
// 2-byte pairs inside a row; the bicubic forms load 4-byte tap rows and need S >= 4); hipErrorInvalidValue for that, for a ROI that is neither empty nor inside the frame, and for sizes whose frame exceeds 2^31 bytes.
hipError_t launch_remap(const RemapArgs& a, int source, int interp, bool perFrame, hipStream_t stream);

// ---- HOG descriptors (hog_kernels.hip) ------------------------------------------------------------------------------------------------------------
// CompVHOG (COMPV_HOGS_ID): per-cell orientation histograms, then the blocks' normalised vectors (include/compv_hip.h, section "HOG descriptors").
// The geometry is worked out on the host (hogGeometry in api_features.cpp); every field below is resolved: no zero "default" is left.
struct HogArgs {
	const uint8_t* gray;      // [frames][H][S]
	size_t frameStride;
	int W, H, S;
	int cellW, cellH, strideW, strideH, nbins;
	int interp, gradientSigned, norm;   // hog::kInterp*, 0 / 1, hog::kNorm*
	int cellsX, cellsY, validX, validY;   // the map's cells; the cells that are computed (the others hold 0)
	float* cells;             // [frames][cellsY][cellsX][nbins]: the caller's, or the plan's scratch
	size_t cellsFrameStride;  // cellsY * cellsX * nbins
	int blocksX, blocksY, cpbX, cpbY, stepX, stepY, count;   // blocks; cells per block; map cells from one block to the next; cpbX * cpbY * nbins
	float* desc;              // [frames][descStride]
	size_t descStride;
	// filled by hog_plan_launch: the cells a wave takes (nx across, ny down, nx * ny <= 64), cell rows staged at a time, the staged rows' pitch in bytes,
	// whether whole dwords are loaded, the workgroups of a frame, the dynamic LDS of the cells kernel
	int nx, ny, rowsPerChunk, pitch, dwords, tilesX, tilesY, ldsBytes;
};
constexpr size_t kHogLdsLimit = 160 * 1024;      // LDS of a CU: histogram [nbins][64] float32 and the staged rows of one wave share it
constexpr size_t kHogTileBudget = 16 * 1024;     // staged rows of a wave: as many cell rows at a time as fit this (at least one)
// fills the launch fields of `a`; false: a cell so wide that three rows of ONE cell and the histogram do not fit a CU's LDS
bool hog_plan_launch(HogArgs& a);
hipError_t launch_hog_cells(const HogArgs& a, int frames, hipStream_t stream);
hipError_t launch_hog_blocks(const HogArgs& a, int frames, hipStream_t stream);

// ---- image statistics: integral images, histogram, equalisation, projections (stats_kernels.hip) -------------------------------------------------
// CompVImage::integral / histogramBuild / histogramEqualiz / histogramBuildProjectionX / Y (include/compv_hip.h, section "image statistics")
constexpr int kStatsBandRows = 16;      // rows of a band: one workgroup of the band-sums kernel, one wave of the integral kernel
constexpr int kStatsTile = 64;          // columns of a tile of the integral kernel: one per lane
constexpr int kStatsThreads = 256;      // threads of the band-sums kernel, four columns each: 1024 columns at a time (one wave, 256 columns, for frames of at most 256)
constexpr int kStatsMaxChunks = 128;    // row chunks (= workgroups) per frame of the histogram and the equalisation kernel
int stats_bands(int H);                 // ceil(H / kStatsBandRows)
int stats_row_chunks(int H, int frames);   // row chunks of at least 16 rows: 1024 / frames of them, 1 .. kStatsMaxChunks
struct StatsBandArgs {
	const uint8_t* in;        // [frames][H][S]
	size_t frameStride;
	int W, H, S, bands;
	uint64_t* colSum;         // [frames][bands][W] per band and column: the sum of the band's pixels (may be nullptr)
	uint64_t* colSq;          // the same for their squares (may be nullptr)
	int32_t* rowSum;          // [frames][H] the sum of every row = projY (may be nullptr)
};
hipError_t launch_stats_band_sums(const StatsBandArgs& a, int frames, hipStream_t stream);
// projX == nullptr: colSum / colSq (either may be nullptr) become their exclusive prefix sums down the bands, in place; otherwise projX [frames][W] = the
// total of colSum over the bands, and nothing else is written
hipError_t launch_stats_band_scan(uint64_t* colSum, uint64_t* colSq, int bands, int W, int32_t* projX, int frames, hipStream_t stream);
struct StatsIntegralArgs {
	const uint8_t* in;        // [frames][H][S]
	size_t frameStride;
	int W, H, S, bands;
	const uint64_t* edgeSum;  // [frames][bands][W]: what launch_stats_band_scan left (read with `sum`)
	const uint64_t* edgeSq;   // (read with `sumsq`)
	double* sum;              // [frames][H + 1][sumStride], or nullptr
	double* sumsq;            // likewise; not both nullptr
	size_t sumStride;         // >= W + 1, in elements
};
hipError_t launch_stats_integral(const StatsIntegralArgs& a, int frames, hipStream_t stream);
// part: [frames][chunks][256] partial histograms, chunks = stats_row_chunks(H, frames)
hipError_t launch_stats_hist(const uint8_t* in, int W, int H, int S, size_t frameStride, int frames, int chunks, uint32_t* part, hipStream_t stream);
// hist (may be nullptr): [frames][256] the sum of the partial ones; lut (may be nullptr): [frames][256] min(trunc(float32(running sum) * scaleF), 255)
hipError_t launch_stats_hist_finish(const uint32_t* part, int chunks, uint32_t* hist, float scaleF, uint8_t* lut, int frames, hipStream_t stream);
struct StatsEqualizeArgs {
	const uint8_t* in;        // [frames][H][S]
	uint8_t* out;             // [frames][H][S]; may be `in`
	const uint8_t* lut;       // [frames][256]
	size_t frameStride;
	int W, H, S;
};
hipError_t launch_stats_equalize(const StatsEqualizeArgs& a, int frames, int chunks, hipStream_t stream);

// ---- SVM prediction (svm_kernels.hip) ----------------------------------------------------------------------------------------------------------
constexpr int kSvmTile = 64;                 // queries and support vectors of one workgroup of svm_kvalues_kernel
struct SvmKvaluesArgs {
	const void* vectors; int f32;                     // [n][stride] float32 (f32 != 0) or float64
	int n; size_t stride;                             // stride >= dim, in elements
	const double* sv; int l, dim;                     // [l][dim]
	int rbf; double gamma;                            // rbf == 0: LINEAR
	const uint64_t* expTable;                         // [2048] (RBF)
	double* K;                                        // [n][l]
};
hipError_t launch_svm_kvalues(const SvmKvaluesArgs& a, hipStream_t stream);
struct SvmDecideArgs {
	const double* K; int n, l;                        // [n][l]
	int nrClass; const int32_t* nSV;                  // [nrClass]
	const double* svCoef;                             // [nrClass - 1][l]
	const double* rho;                                // [pairs]
	const int32_t* label;                             // [nrClass]
	int32_t* labels;                                  // [n]
	double* dec;                                      // nullptr or [n][pairs]
};
hipError_t launch_svm_decide(const SvmDecideArgs& a, hipStream_t stream);

// ---- lens undistortion: maps, points, projection (undistort_kernels.hip; the fused image form is remap_kernels.hip's kRemapUndist) ------------------
// A camera is a record of 14 coefficients of T (undistort_math.hpp); `coeffStride` is 14 when every frame / set has its own and 0 when all share the first.
struct UndistMapArgs {
	const void* coeffs;       // [1 or cameras][14] float32 or float64
	int coeffStride;
	void* mapX; void* mapY;   // [cameras][Hout * Wout] each, of the same type
	int Wout, Hout, originX, originY, cameras;
	int f64;
};
// Vector stores (16 bytes) where Wout % 4 == 0 and both planes are 16-byte aligned, element stores otherwise.  More than 65 535 cameras: sliced.
hipError_t launch_undist_map(const UndistMapArgs& a, hipStream_t stream);
struct UndistPointsArgs {
	const void* coeffs; int coeffStride;
	const void* in;           // [sets][n] {x, y} float32 or float64
	void* out;                // the same shape; in == out is served
	const int32_t* counts;    // nullptr, or [sets]: points of set s at and behind min(max(counts[s], 0), n) are neither read nor written
	int n, sets, f64;
};
hipError_t launch_undist_points(const UndistPointsArgs& a, hipStream_t stream);   // more than 65 535 sets: sliced
struct UndistProjectArgs {
	const double* coeffs; int coeffStride;
	const double* poses;      // [sets][12]: R row-major, then t
	const double* in;         // [sets][n] {x, y, z}
	double* out;              // [sets][n] {x, y}
	const int32_t* counts;    // as UndistPointsArgs
	int n, sets;
};
hipError_t launch_undist_project(const UndistProjectArgs& a, hipStream_t stream);   // more than 65 535 sets: sliced

// ---- image moments (moments_kernels.hip; the shape record is moments_math.hpp's) -----------------------------------------------------------------
constexpr int kMomentsRows = 16;             // image rows of one workgroup of moments_frames_kernel
constexpr int kMomentsCompRows = 16;         // label rows of one wave of moments_components_kernel
struct MomentsFramesArgs {
	const uint8_t* gray;      // [frames][H][S], any byte
	int W, H; size_t S;
	int frames, frame0;       // frame0: set by the launcher (slices)
	int unit;                 // != 0: a pixel counts gray != 0
	compvhip_moments* raw;    // [frames], zeroed by the launcher
};
// zeroes raw[0 .. frames), then the six sums of every frame.  More than 65 535 frames: sliced.
hipError_t launch_moments_frames(const MomentsFramesArgs& a, hipStream_t stream);
struct MomentsCompArgs {
	const int32_t* labels;    // [frames][H][labelStride]
	int W, H; size_t labelStride;
	const uint8_t* gray;      // nullptr (every pixel weighs 1) or [frames][H][S]
	size_t S;
	const compvhip_component* comps;   // [frames][compCap]: x0, y0 are read when box != 0
	int compCap; const int32_t* counts; // [frames]: ids 1 .. min(max(counts[f], 0), compCap) are served
	int frames, frame0;
	int unit, box;
	compvhip_moments* raw;    // [frames][compCap]: the served records are zeroed by the launcher, the others are not written
};
hipError_t launch_moments_components(const MomentsCompArgs& a, hipStream_t stream);   // more than 65 535 frames: sliced
// shape[g * cap + c] of raw[g * cap + c] for c < (counts ? min(max(counts[g], 0), cap) : cap), g < groups
struct MomentsShapeArgs {
	const compvhip_moments* raw; compvhip_moments_shape* shape;
	size_t groups; int cap; const int32_t* counts;
};
hipError_t launch_moments_shapes(const MomentsShapeArgs& a, hipStream_t stream);

// ---- PCA projection, mulABt, mean and covariance (pca_kernels.hip; the arithmetic is pca_math.hpp's) ------------------------------------------------
constexpr int kPcaTile = 32;                 // rows and components of one workgroup of pca_project_kernel
constexpr int kPcaChunk = 64;                // columns it stages at a time
// out[r][m] = dot16(in[r] (- mean), vectors[m], dim) (* scale), r < n, m < comps.  Row tiles ride in grid x, component tiles in y: comps <= 2^20
// keeps y below 65 535, so no launch is sliced.
struct PcaProjectArgs {
	const float* in; int n; size_t inStride;              // [n][inStride]
	const float* mean;                                    // [dim], or nullptr: rows are taken as they are
	const float* vectors; int comps; size_t vecStride;    // [comps][vecStride]
	int dim;
	float* out; size_t outStride;                         // [n][outStride]
	int scaled; float scale;                              // scaled != 0: one more rounded multiply
};
hipError_t launch_pca_project(const PcaProjectArgs& a, hipStream_t stream);
struct PcaMeanArgs {
	const float* obs; int n; size_t obsStride; int dim;   // [n][obsStride]
	float* mean;                                          // [dim]
};
hipError_t launch_pca_mean(const PcaMeanArgs& a, hipStream_t stream);
struct PcaCentreArgs {
	const float* obs; int n; size_t obsStride; int dim;
	const float* mean;
	float* centred; size_t nPad;                          // [dim][nPad]; columns n .. nPad - 1 are not written
};
hipError_t launch_pca_centre_transpose(const PcaCentreArgs& a, hipStream_t stream);

} // namespace compvhip
