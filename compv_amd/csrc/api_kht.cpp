// api_kht.cpp -- kernel-based Hough transform: the host entry points and the batched plan call (host stages on a KhtPool, GPU stages batched).
#include "api_internal.hpp"
#include "kht_pool.hpp"

#if defined(__linux__)
#include <sched.h>
#endif

// CPUs this process may really use at once: min(affinity mask, cgroup CPU quota) -- a container can show 256 logical CPUs and own 16 (cpu.max "1600000 100000");
// twice as many busy threads as the quota only makes the kernel throttle all of them (round 5: 32 threads on a 16-CPU quota, sort + sweep 0.69 -> 1.97 ms per frame)
size_t compvhip_api::hostCpuBudget()
{
	size_t n = std::thread::hardware_concurrency();
	if (!n) n = 4;
#if defined(__linux__)
	cpu_set_t set;
	if (sched_getaffinity(0, sizeof(set), &set) == 0) { const int c = CPU_COUNT(&set); if (c > 0) n = std::min<size_t>(n, static_cast<size_t>(c)); }
	if (FILE* f = fopen("/sys/fs/cgroup/cpu.max", "r")) {               // cgroup v2: "<quota|max> <period>"
		char q[64] = {}; long long period = 0;
		if (fscanf(f, "%63s %lld", q, &period) == 2 && strcmp(q, "max") != 0 && period > 0) {
			const long long quota = atoll(q);
			if (quota > 0) n = std::min<size_t>(n, static_cast<size_t>(std::max<long long>(1, quota / period)));
		}
		fclose(f);
	}
	else {
		long long quota = -1, period = 0;
		if (FILE* fq = fopen("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", "r")) { if (fscanf(fq, "%lld", &quota) != 1) quota = -1; fclose(fq); }
		if (FILE* fp = fopen("/sys/fs/cgroup/cpu/cpu.cfs_period_us", "r")) { if (fscanf(fp, "%lld", &period) != 1) period = 0; fclose(fp); }
		if (quota > 0 && period > 0) n = std::min<size_t>(n, static_cast<size_t>(std::max<long long>(1, quota / period)));
	}
#endif
	return std::max<size_t>(1, n);
}

// ---- KHT -----------------------------------------------------------------------------------------------------------------------
// All of it works on ONE KhtScratch (its stream, its device buffers) and reports failures through K.err: the batched entry point runs
// several of these at the same time on worker threads, so nothing below touches ctx->err or any other shared state (ctx->live is atomic).
#define KCHK(K, call) do { hipError_t e__ = (call); if (e__ != hipSuccess) { (K).err = std::string(#call) + ": " + hipGetErrorString(e__); return COMPVHIP_E_HIP; } } while (0)

// the reference's AVX (4) / SSE2 (2) kernel-height loops take n & ~(pack - 1) clusters of a frame; the rest go through the C code (other operation order)
static int khtSimdEnd(size_t n)
{
	const size_t pack = n >= 4 ? 4 : (n >= 2 ? 2 : 1);
	return static_cast<int>(pack > 1 ? (n & ~(pack - 1)) : 0);
}

// host linking (on K.plane, which it destroys), then cluster subdivision (kht_subdivide_kernel) and per-cluster statistics (kht_stats_kernel) on the GPU; kernels in cluster order
static int khtBuildKernels(compvhip_ctx* ctx, KhtScratch& K, size_t W, size_t H, double clusterMinDeviation, size_t clusterMinSize,
                           std::vector<KhtKernel>& kernels, double& hmax)
{
	using clk = std::chrono::steady_clock;
	auto ms = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
	kernels.clear(); hmax = 0.0;
	const auto t0 = clk::now();
	std::vector<KhtRange> strings;
	const size_t most = khtPlaneCount(K.plane);
	if (most > 0x7fffffffull) { K.err = "too many edge pixels"; return COMPVHIP_E_INVALID_PARAMETER; }
	if (K.linked.cap < most) {
		KCHK(K, hipSetDevice(ctx->device));
		KCHK(K, K.linked.reserve(most + most / 4 + 4096));   // (frames of a stream resemble each other: no reallocation for a slightly denser one)
	}
	const size_t nPts = khtLink(K.plane, clusterMinSize, K.linked, strings);
	const auto t1 = clk::now();
	K.stageMs[0] += ms(t0, t1);
	if (strings.empty()) return COMPVHIP_OK;

	// device: cluster subdivision (one wave per string), per-cluster statistics (one thread per cluster)
	std::vector<KhtStringDesc> descs(strings.size());
	size_t slots = 0;
	for (size_t i = 0; i < strings.size(); ++i) {
		descs[i].begin = static_cast<uint32_t>(strings[i].begin); descs[i].end = static_cast<uint32_t>(strings[i].end);
		descs[i].slot = static_cast<uint32_t>(slots);
		slots += khtSubdivSlots(strings[i].end - strings[i].begin, clusterMinSize);
	}
	KCHK(K, hipSetDevice(ctx->device));
	if (K.pts.cap < nPts) KCHK(K, K.pts.reserve(ctx, K.linked.cap));   // as large as the pinned arena it mirrors
	KCHK(K, K.strings.reserve(ctx, descs.size())); KCHK(K, K.counts32.reserve(ctx, descs.size() + 2));
	KCHK(K, K.spans.reserve(ctx, slots)); KCHK(K, K.scratch.reserve(ctx, slots)); KCHK(K, K.stack.reserve(ctx, slots)); KCHK(K, K.kernelsDev.reserve(ctx, slots));
	hipStream_t st = K.stream;
	KCHK(K, hipMemcpyAsync(K.pts, K.linked, nPts * sizeof(KhtPoint), hipMemcpyHostToDevice, st));
	KCHK(K, hipMemcpyAsync(K.strings, descs.data(), descs.size() * sizeof(KhtStringDesc), hipMemcpyHostToDevice, st));
	KhtSubdivArgs sv;
	sv.pts = K.pts; sv.strings = K.strings; sv.nStrings = static_cast<int>(descs.size());
	sv.minSize = static_cast<int>(std::min<size_t>(clusterMinSize, 0x7fffffff)); sv.minDev = clusterMinDeviation;
	sv.scratch = K.scratch; sv.stack = K.stack; sv.counts = K.counts32; sv.clusters = K.spans; sv.total = K.counts32 + descs.size(); sv.flagIndex = 1;
	KCHK(K, hipMemsetAsync(sv.total, 0, 2 * sizeof(uint32_t), st));   // [0] cluster total, [1] "recursion truncated" flag
	KhtBatchStrings one{};   // a batch of one frame
	one.frames = 1; one.stringBegin[0] = 0; one.stringBegin[1] = static_cast<uint32_t>(descs.size()); one.clusterBase[0] = 0;
	KCHK(K, launch_kht_subdivide(sv, one, st));
	uint32_t tot[2] = { 0, 0 };
	KCHK(K, hipMemcpyAsync(tot, sv.total, sizeof(tot), hipMemcpyDeviceToHost, st));
	KCHK(K, hipStreamSynchronize(st));
	if (tot[1]) { K.err = "cluster subdivision ran out of recursion slots"; return COMPVHIP_E_INVALID_STATE; } // cannot happen: clusterMinSize >= 2 is enforced and khtSubdivSlots bounds the depth for it
	const uint32_t nClusters = tot[0];
	const auto t2 = clk::now();
	K.stageMs[1] += ms(t1, t2);
	if (!nClusters) return COMPVHIP_OK;
	const size_t n = nClusters;
	KhtStatsArgs sa;
	sa.pts = K.pts; sa.clusters = K.spans;
	sa.hw = static_cast<double>(W) * 0.5; sa.hh = static_cast<double>(H) * 0.5;
	sa.out = K.kernelsDev;
	KhtBatchStats ones{};
	ones.frames = 1; ones.clusterBase[0] = 0; ones.n[0] = static_cast<int>(n); ones.simdEnd[0] = khtSimdEnd(n);
	KCHK(K, launch_kht_stats(sa, ones, st));
	kernels.resize(n);
	KCHK(K, hipMemcpyAsync(kernels.data(), K.kernelsDev, n * sizeof(KhtKernel), hipMemcpyDeviceToHost, st));
	KCHK(K, hipStreamSynchronize(st));
	khtFinishKernels(kernels, hmax);
	K.stageMs[2] += ms(t2, clk::now());
	return COMPVHIP_OK;
}

// the device tables of the line fields for this geometry (uploaded when it changes; synchronous: the host vectors die here)
static hipError_t khtCanonTabs(compvhip_ctx* ctx, KhtCanonTabs& t, const KhtAxes& ax, hipStream_t st)
{
	if (t.rho && t.W == ax.W && t.H == ax.H && t.dRho == ax.dRho && t.dTheta == ax.dThetaDeg) return hipSuccess;
	t.rho.release(); t.theta.release();   // tables of another geometry: exactly the new size, not the larger of the two
	std::vector<float> rho, theta;
	khtCanonTables(ax, rho, theta);
	hipError_t e = t.rho.reserve(ctx, rho.size());
	if (e == hipSuccess) e = t.theta.reserve(ctx, theta.size());
	if (e == hipSuccess) e = hipMemcpyAsync(t.rho, rho.data(), rho.size() * sizeof(float), hipMemcpyHostToDevice, st);
	if (e == hipSuccess) e = hipMemcpyAsync(t.theta, theta.data(), theta.size() * sizeof(float), hipMemcpyHostToDevice, st);
	if (e == hipSuccess) e = hipStreamSynchronize(st);
	if (e != hipSuccess) { t.rho.release(); t.theta.release(); return e; }   // no half-filled tables: t.rho == nullptr, the next call builds them
	t.W = ax.W; t.H = ax.H; t.dRho = ax.dRho; t.dTheta = ax.dThetaDeg;
	return hipSuccess;
}

// one frame, host edge map -> lines (the body of CompVHoughKht::process, houghkht.cxx:208-447) in the reference's order, or in the canonical order
// (compvhip_kht_opts.order) with the peak stage on the GPU; *found = the lines after the maxLines cut, of which out holds the first min(found, cap) (all of
// them in the reference order)
// (the frame's edge map is K.plane: packed by the caller, destroyed by the linker)
static int khtFrame(compvhip_ctx* ctx, KhtScratch& K, size_t W, size_t H, const KhtAxes& ax, int threshold, int maxLines,
                    double clusterMinDeviation, size_t clusterMinSize, double kernelMinHeight, int order, size_t cap, std::vector<KhtLine>& out, size_t* found, double* gs)
{
	using clk = std::chrono::steady_clock;
	auto msSince = [](clk::time_point a) { return std::chrono::duration<double, std::milli>(clk::now() - a).count(); };
	out.clear();
	*found = 0;
	std::vector<KhtKernel> kernels;
	double hmax = 0.0;
	const int rck = khtBuildKernels(ctx, K, W, H, clusterMinDeviation, clusterMinSize, kernels, hmax);
	if (rck) return rck;
	if (kernels.empty()) return COMPVHIP_OK;
	auto t3 = clk::now();
	const double GS = khtPruneAndScale(kernels, hmax, kernelMinHeight);
	if (kernels.empty()) return COMPVHIP_OK;
	if (gs) *gs = GS;
	std::vector<KhtVoteParams> params;
	khtVoteParams(ax, kernels, params);

	// device: Gaussian voting + smoothing/threshold
	KCHK(K, hipSetDevice(ctx->device));
	const int stride = static_cast<int>(alignUp(ax.rhoN + 2, 16));
	const size_t countsElems = (ax.T + 2) * static_cast<size_t>(stride);
	const size_t cellCap = ax.T * ax.rhoN;
	KCHK(K, K.counts.reserve(ctx, countsElems)); KCHK(K, K.params.reserve(ctx, params.size())); KCHK(K, K.cells.reserve(ctx, cellCap)); KCHK(K, K.cellCount.reserve(ctx, 1));
	hipStream_t st = K.stream;
	K.stageMs[3] += msSince(t3);
	t3 = clk::now();
	KCHK(K, hipMemsetAsync(K.counts, 0, countsElems * sizeof(int32_t), st));
	KCHK(K, hipMemsetAsync(K.cellCount, 0, sizeof(int), st));
	KCHK(K, hipMemcpyAsync(K.params, params.data(), params.size() * sizeof(KhtVoteParams), hipMemcpyHostToDevice, st));
	KhtGpuArgs a;
	a.params = K.params; a.nKernels = static_cast<int>(params.size()); a.counts = K.counts; a.stride = stride;
	a.rhoN = static_cast<int>(ax.rhoN); a.T = static_cast<int>(ax.T); a.dRho = ax.dRho; a.dThetaDeg = ax.dThetaDeg; a.gs = GS;
	a.threshold = threshold; a.cells = K.cells; a.cellCount = K.cellCount; a.cellCap = static_cast<int>(cellCap);
	KhtBatchVote onev{};
	onev.frames = 1; onev.paramsBase[0] = 0; onev.nKernels[0] = a.nKernels; onev.gs[0] = GS; onev.mapElems = countsElems; onev.cellCap = cellCap;
	KCHK(K, launch_kht_vote(a, onev, st));
	if (order == COMPVHIP_KHT_ORDER_CANONICAL) {
		// peaks, line test and sort on the device: only the lines come back
		KCHK(K, khtCanonTabs(ctx, K.tabs, ax, st));
		const size_t capDev = std::min(cap, cellCap);
		KCHK(K, K.canonLines.grow(ctx, capDev));
		KCHK(K, K.canonCount.reserve(ctx, 1));
		KCHK(K, launch_kht_canon_peaks(a, onev, st));
		KhtCanonOut o;
		o.rho = K.tabs.rho; o.theta = K.tabs.theta; o.lines = K.canonLines; o.cap = static_cast<int>(capDev); o.counts = K.canonCount; o.maxLines = maxLines;
		KCHK(K, launch_kht_canon_sort(a, onev, o, st));
		int32_t n = 0;
		KCHK(K, hipMemcpyAsync(&n, K.canonCount, sizeof(n), hipMemcpyDeviceToHost, st));
		KCHK(K, hipStreamSynchronize(st));
		if (n < 0) { K.err = "canonical KHT: merge scratch too small"; return COMPVHIP_E_INVALID_STATE; }   // cannot happen (kht_canon_sort_kernel)
		*found = static_cast<size_t>(n);
		out.resize(std::min(*found, capDev));
		if (!out.empty()) {
			KCHK(K, hipMemcpyAsync(out.data(), K.canonLines, out.size() * sizeof(KhtLine), hipMemcpyDeviceToHost, st));
			KCHK(K, hipStreamSynchronize(st));
		}
		K.stageMs[4] += msSince(t3);
		return COMPVHIP_OK;
	}
	KCHK(K, launch_kht_peaks(a, onev, st));
	int cellCount = 0;
	KCHK(K, hipMemcpyAsync(&cellCount, K.cellCount, sizeof(int), hipMemcpyDeviceToHost, st));
	KCHK(K, hipStreamSynchronize(st));
	std::vector<KhtCell>& cells = K.cellsHost;
	cells.resize(static_cast<size_t>(std::min<int>(cellCount, static_cast<int>(cellCap))));
	if (!cells.empty()) {
		KCHK(K, hipMemcpyAsync(cells.data(), K.cells, cells.size() * sizeof(KhtCell), hipMemcpyDeviceToHost, st));
		KCHK(K, hipStreamSynchronize(st));
	}
	K.stageMs[4] += msSince(t3);
	t3 = clk::now();
	// host: sort + sweep (order dependent, :1195-1247)
	khtPeaks(ax, cells, maxLines, out, K.peaks);
	*found = out.size();
	K.stageMs[5] += msSince(t3);
	return COMPVHIP_OK;
}

static int khtCheckParams(compvhip_ctx* ctx, size_t W, size_t H, float rho, float thetaDeg, int threshold, size_t clusterMinSize, double kernelMinHeight, KhtAxes& ax)
{
	if (!(rho > 0.f) || rho > 1.f || !(thetaDeg > 0.f) || threshold <= 0) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "rho in (0,1], theta > 0, threshold > 0"); // :146-163,491
	if (!clusterMinSize || !(kernelMinHeight >= 0.0)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "invalid KHT knob"); // :169-186 (the deviation is unchecked there)
	// Defined deviation: the reference's set() accepts a cluster size of 1 and its clusters_subdivision then recurses without bound on the first
	// collinear string (max_index stays at start_index, both "halves" hold >= 1 point: houghkht.cxx:795-821) -- a stack overflow, not a result.
	if (clusterMinSize < 2) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "clusterMinSize must be >= 2 (the reference's recursion does not terminate for 1)");
	if (!W || !H || W > 32767 || H > 32767) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "image size out of range");
	if (!khtAxes(W, H, rho, thetaDeg, ax)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "degenerate KHT parameter space");
	// the peak stage identifies a vote cell by the 32-bit key theta * 2 (rhoN + 2) + rho (KhtCell::order) and indexes the vote map with ints
	if (static_cast<uint64_t>(ax.T + 2) * 2u * (ax.rhoN + 2) >= (1ull << 32) || static_cast<uint64_t>(ax.T + 2) * (ax.rhoN + 2) > 0x7fffffffull)
		return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "KHT parameter space too fine for this image size ((T + 2) * 2 (rhoN + 2) must stay below 2^32)");
	return COMPVHIP_OK;
}

static void khtCopyLines(const std::vector<KhtLine>& out, compvhip_line* lines, size_t cap)
{
	const size_t ncopy = std::min(out.size(), cap);
	for (size_t i = 0; i < ncopy; ++i) {
		lines[i].rho = out[i].rho; lines[i].theta = out[i].theta; lines[i].strength = out[i].strength;
		lines[i].row = out[i].rhoIndex; lines[i].col = out[i].thetaIndex;
	}
}

int compvhip_houghkht_kernels_u8(compvhip_ctx* ctx, const uint8_t* edges, size_t W, size_t H, size_t S, double clusterMinDeviation, size_t clusterMinSize,
                                 double* kernels7, size_t cap, size_t* n, double* hmax)
{
	if (!ctx) return COMPVHIP_E_INVALID_PARAMETER;
	if (!edges || !n || (cap && !kernels7) || S < W || !W || !H || clusterMinSize < 2) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "null/invalid argument (clusterMinSize >= 2)");
	if (W > 32767 || H > 32767) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "image size out of range");
	std::vector<KhtKernel> kernels; double hm = 0.0;
	ctx->kht.stream = ctx->stream;
	memset(ctx->kht.stageMs, 0, sizeof(ctx->kht.stageMs));
	{
		const auto tp = std::chrono::steady_clock::now();
		khtPackBytes(edges, W, H, S, ctx->kht.plane);
		ctx->kht.stageMs[0] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tp).count();
	}
	const int rc = khtBuildKernels(ctx, ctx->kht, W, H, clusterMinDeviation, clusterMinSize, kernels, hm);
	if (rc) return fail(ctx, rc, ctx->kht.err.c_str());
	*n = kernels.size();
	if (hmax) *hmax = hm;
	for (size_t i = 0; i < std::min(kernels.size(), cap); ++i) {
		const KhtKernel& k = kernels[i];
		const double v[7] = { k.rho, k.theta, k.h, k.sigmaThetaSquare, k.sigmaRhoSquare, k.m2, k.sigmaRhoTimesTheta };
		memcpy(kernels7 + i * 7, v, sizeof(v));
	}
	if (kernels.size() > cap) return fail(ctx, COMPVHIP_E_OUT_OF_BOUND, "kernel buffer too small");
	return COMPVHIP_OK;
}

int compvhip_houghkht_link_u8(const uint8_t* edges, size_t W, size_t H, size_t S, size_t clusterMinSize, int32_t* xy, size_t cap, size_t* nPoints,
                              uint32_t* stringEnds, size_t stringCap, size_t* nStrings)
{
	if (!edges || !nPoints || !nStrings || (cap && !xy) || (stringCap && !stringEnds) || S < W || !W || !H || !clusterMinSize || W > 32767 || H > 32767)
		return COMPVHIP_E_INVALID_PARAMETER;
	try {
		KhtBitPlane plane;
		std::vector<KhtRange> strings;
		khtPackBytes(edges, W, H, S, plane);
		std::unique_ptr<KhtPoint[]> pts(new KhtPoint[khtPlaneCount(plane) + 1]);
		const size_t n = khtLink(plane, clusterMinSize, pts.get(), strings);
		*nPoints = n; *nStrings = strings.size();
		if (n > cap || strings.size() > stringCap) return COMPVHIP_E_OUT_OF_BOUND;
		for (size_t i = 0; i < n; ++i) { xy[2 * i] = pts[i].x; xy[2 * i + 1] = pts[i].y; }
		for (size_t i = 0; i < strings.size(); ++i) stringEnds[i] = static_cast<uint32_t>(strings[i].end);
	}
	catch (...) { return COMPVHIP_E_OUT_OF_MEMORY; }
	return COMPVHIP_OK;
}

int compvhip_houghkht_stage_ms(compvhip_ctx* ctx, double* ms6)
{
	if (!ctx || !ms6) return COMPVHIP_E_INVALID_PARAMETER;
	memcpy(ms6, ctx->kht.stageMs, sizeof(ctx->kht.stageMs));
	return COMPVHIP_OK;
}

static int khtHostEntry(compvhip_ctx* ctx, const uint8_t* edges, size_t W, size_t H, size_t S, float rho, float thetaDeg, int threshold, int maxLines,
                        double clusterMinDeviation, size_t clusterMinSize, double kernelMinHeight, int order, compvhip_line* lines, size_t cap, size_t* n, double* gs)
{
	if (!edges || !n || (cap && !lines) || S < W || !W || !H) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "null/invalid argument"); // houghkht.cxx:210-211
	KhtAxes ax;
	int rc = khtCheckParams(ctx, W, H, rho, thetaDeg, threshold, clusterMinSize, kernelMinHeight, ax);
	if (rc) return rc;
	*n = 0;
	ctx->kht.stream = ctx->stream;
	memset(ctx->kht.stageMs, 0, sizeof(ctx->kht.stageMs));
	std::vector<KhtLine> out;
	{
		const auto tp = std::chrono::steady_clock::now();
		khtPackBytes(edges, W, H, S, ctx->kht.plane);   // host bytes -> the linker's bit plane (the linker never touches the caller's map)
		ctx->kht.stageMs[0] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tp).count();
	}
	size_t found = 0;
	rc = khtFrame(ctx, ctx->kht, W, H, ax, threshold, maxLines, clusterMinDeviation, clusterMinSize, kernelMinHeight, order, cap, out, &found, gs);
	if (rc) return fail(ctx, rc, ctx->kht.err.c_str());
	*n = found;
	khtCopyLines(out, lines, cap);
	if (found > cap) return fail(ctx, COMPVHIP_E_OUT_OF_BOUND, "line buffer too small");
	return COMPVHIP_OK;
}

int compvhip_houghkht_u8(compvhip_ctx* ctx, const uint8_t* edges, size_t W, size_t H, size_t S, float rho, float thetaDeg, int threshold, int maxLines,
                         double clusterMinDeviation, size_t clusterMinSize, double kernelMinHeight, compvhip_line* lines, size_t cap, size_t* n, double* gs)
{
	if (!ctx) return COMPVHIP_E_INVALID_PARAMETER;
	return khtHostEntry(ctx, edges, W, H, S, rho, thetaDeg, threshold, maxLines, clusterMinDeviation, clusterMinSize, kernelMinHeight,
	                    COMPVHIP_KHT_ORDER_REFERENCE, lines, cap, n, gs);
}

// compvhip_kht_opts with its zero fields replaced by the defaults; false for an unknown order
static bool khtResolveOpts(const compvhip_kht_opts* o, compvhip_kht_opts& k)
{
	if (o->order != COMPVHIP_KHT_ORDER_REFERENCE && o->order != COMPVHIP_KHT_ORDER_CANONICAL) return false;
	k = *o;
	if (k.rho == 0.f) k.rho = 1.f;
	if (k.thetaDeg == 0.f) k.thetaDeg = 1.f;
	if (k.threshold == 0) k.threshold = 1;
	if (k.clusterMinDeviation == 0.0) k.clusterMinDeviation = 2.0;   // houghkht.cxx:38-40
	if (k.clusterMinSize == 0) k.clusterMinSize = 10;
	if (k.kernelMinHeight == 0.0) k.kernelMinHeight = 0.002;
	return true;
}

int compvhip_houghkht_ex_u8(compvhip_ctx* ctx, const uint8_t* edges, size_t W, size_t H, size_t S, const compvhip_kht_opts* opts,
                            compvhip_line* lines, size_t cap, size_t* n, double* gs)
{
	if (!ctx) return COMPVHIP_E_INVALID_PARAMETER;
	compvhip_kht_opts k;
	if (!opts || !khtResolveOpts(opts, k)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "null options or unknown KHT order");
	return khtHostEntry(ctx, edges, W, H, S, k.rho, k.thetaDeg, k.threshold, k.maxLines, k.clusterMinDeviation, k.clusterMinSize, k.kernelMinHeight,
	                    k.order, lines, cap, n, gs);
}

// CompVHoughKht::process on the plan's `frames` device edge maps.  The chain walk of the linker (Appendix A) is sequential per frame and
// stays on the host -- but frames are independent: a pool of host threads takes them in turn, each with its own HIP stream and scratch
// buffers.  A worker downloads its frame (pinned buffer, asynchronous copy on its stream), links it, and drives the GPU stages of that
// frame (subdivision, statistics, voting, peaks); while one worker links, the kernels and copies of the others run, so the GPU work
// and the PCIe transfers of the batch hide under the host stage that bounds it.
// ---- batched KHT (compvhip_plan_houghkht) ------------------------------------------------------------------------------------------------------
// The frames of a batch go through the stages TOGETHER: the host stages (bit-plane linking, prune / Gmin, sort + sweep: sequential per frame, independent
// between frames) run as parallel loops over the frames on a pool of host threads, the GPU stages are ONE launch each over the strings / clusters /
// kernels / vote maps of all frames (kht.hpp: the per-frame tables travel in the kernel arguments), with one upload and one download per stage.
// (Rounds 3-4 gave every worker thread its own stream and let it drive its frame's five small launches and four synchronisations: with 32 workers the
// GPU-touching stages took 5-9 x their single-frame time -- a launch / synchronisation pile-up, not compute.)
// one group of up to kKhtBatch frames
static int khtBatchGroup(compvhip_plan* p, KhtBatchState& B, KhtPool& pool, const uint8_t* d_edges, size_t G, const KhtAxes& ax, int threshold, int maxLines,
                         double clusterMinDeviation, size_t clusterMinSize, double kernelMinHeight, int order, compvhip_line* lines, size_t cap, size_t* counts, double* gs,
                         bool* overflow, std::string& err)
{
	using clk = std::chrono::steady_clock;
	auto msSince = [](clk::time_point a) { return std::chrono::duration<double, std::milli>(clk::now() - a).count(); };
	compvhip_ctx* ctx = p->ctx;
	const size_t W = p->W, H = p->H, S = p->S;
	const size_t wpr = (W + 31) / 32, words = wpr * H;
	hipStream_t st = B.stream;
	auto sleepSync = [&]() -> hipError_t {   // the stream's work so far, waited for without spinning
		hipError_t e = hipEventRecord(B.syncEv, st);
		return e != hipSuccess ? e : hipEventSynchronize(B.syncEv);
	};
	// (several groups run at the same time, each on its own controller thread: errors travel back as (code, text), only the caller touches ctx->err)
// (an early return must not leave asynchronous copies in flight towards this frame's stack arrays or the pinned state: drain the stream first, result ignored)
#define BCHK(call) do { hipError_t e__ = (call); if (e__ != hipSuccess) { err = std::string(#call) + ": " + hipGetErrorString(e__); (void)hipStreamSynchronize(st); return COMPVHIP_E_HIP; } } while (0)
	auto firstError = [&]() -> int {
		for (size_t f = 0; f < G; ++f)
			if (B.frames[f].code) { err = "frame " + std::to_string(f) + " of its group: " + B.frames[f].err; (void)hipStreamSynchronize(st); return B.frames[f].code; }
		return COMPVHIP_OK;
	};
	if (hipSetDevice(ctx->device) != hipSuccess) { err = "hipSetDevice"; return COMPVHIP_E_HIP; }
	auto guarded = [&](size_t f, const std::function<void(KhtBatchFrame&)>& body) {   // nothing may leave a pool thread (or an extern "C" entry point) as an exception
		KhtBatchFrame& fr = B.frames[f];
		if (fr.code) return;
		try { body(fr); }
		catch (const std::exception& ex) { fr.code = COMPVHIP_E_OUT_OF_MEMORY; fr.err = std::string("exception in a KHT stage: ") + ex.what(); }
		catch (...) { fr.code = COMPVHIP_E_OUT_OF_MEMORY; fr.err = "exception in a KHT stage"; }
	};
	for (size_t f = 0; f < G; ++f) {
		KhtBatchFrame& fr = B.frames[f];
		fr.code = COMPVHIP_OK; fr.err.clear(); fr.nClusters = 0; fr.kernels.clear(); fr.params.clear(); fr.cells.clear(); fr.cellCount = 0; fr.out.clear(); fr.haveGS = false;
		memset(fr.ms, 0, sizeof(fr.ms));
	}

	// ---- A. the edge maps leave the device as bit-mask rows (1/8 of the bytes over PCIe; the linker works on bits anyway): one kernel, one copy per frame ----
	BCHK(launch_bytes_to_bits(d_edges, static_cast<int>(W), static_cast<int>(H), static_cast<int>(S), S * H, B.dBits, static_cast<int>(wpr), words, static_cast<int>(G), st));
	for (size_t f = 0; f < G; ++f) {
		BCHK(hipMemcpyAsync(B.hostBits + f * words, B.dBits + f * words, words * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
		BCHK(hipEventRecord(B.ready[f], st));
	}
	pool.run(G, [&](size_t f) { guarded(f, [&](KhtBatchFrame& fr) {
		const auto t0 = clk::now();
		if (hipSetDevice(ctx->device) != hipSuccess || hipEventSynchronize(B.ready[f]) != hipSuccess) { fr.code = COMPVHIP_E_HIP; fr.err = "frame download"; return; }
		khtPlaneFromWords(B.hostBits + f * words, wpr, W, H, fr.plane);
		fr.most = khtPlaneCount(fr.plane);
		fr.ms[0] += msSince(t0);
	}); }, 'P');
	int rc = firstError();
	if (rc) return rc;
	size_t total = 0;
	for (size_t f = 0; f < G; ++f) { B.frames[f].ptsOff = total; total += B.frames[f].most; }
	if (total > 0x7fffffffull) { err = "too many edge pixels in the batch"; return COMPVHIP_E_INVALID_PARAMETER; }
	BCHK(B.linked.grow(total + 1));
	// ---- B. linking (Appendix A): sequential inside a frame, the frames in parallel; every frame's points go straight into its slice of the pinned arena ----
	// (longest first: the items are milliseconds long and few, the last ones decide when the group moves on)
	std::vector<size_t> byWork(G);
	for (size_t f = 0; f < G; ++f) byWork[f] = f;
	std::sort(byWork.begin(), byWork.end(), [&](size_t a, size_t b) { return B.frames[a].most > B.frames[b].most; });
	pool.run(G, [&](size_t i) { const size_t f = byWork[i]; guarded(f, [&](KhtBatchFrame& fr) {
		const auto t0 = clk::now();
		fr.nPts = khtLink(fr.plane, clusterMinSize, B.linked + fr.ptsOff, fr.strings);
		fr.ms[0] += msSince(t0);
	}); }, 'L');
	rc = firstError();
	if (rc) return rc;

	// ---- C. cluster subdivision of ALL strings: one upload per frame slice, one launch, one download ----
	auto tc = clk::now();
	size_t nStrings = 0, slots = 0;
	for (size_t f = 0; f < G; ++f) nStrings += B.frames[f].strings.size();
	KhtBatchStrings tabS{};
	tabS.frames = static_cast<int>(G);
	if (nStrings) {
		BCHK(B.stringsHost.grow(nStrings));
		size_t si = 0;
		for (size_t f = 0; f < G; ++f) {
			KhtBatchFrame& fr = B.frames[f];
			tabS.stringBegin[f] = static_cast<uint32_t>(si); tabS.clusterBase[f] = static_cast<uint32_t>(slots);
			fr.slotBase = slots;
			for (const KhtRange& r : fr.strings) {
				KhtStringDesc& d = B.stringsHost[si++];
				d.begin = static_cast<uint32_t>(fr.ptsOff + r.begin); d.end = static_cast<uint32_t>(fr.ptsOff + r.end); d.slot = static_cast<uint32_t>(slots);
				slots += khtSubdivSlots(r.end - r.begin, clusterMinSize);
			}
			fr.slots = slots - fr.slotBase;
		}
		for (size_t f = G; f <= static_cast<size_t>(kKhtBatch); ++f) tabS.stringBegin[f] = static_cast<uint32_t>(nStrings);
		tabS.stringBegin[G] = static_cast<uint32_t>(nStrings);
		if (slots > 0xffffffffull) { err = "too many cluster slots in the batch"; return COMPVHIP_E_INVALID_PARAMETER; }
		BCHK(B.pts.grow(ctx, total + 1));
		BCHK(B.strings.grow(ctx, nStrings)); BCHK(B.counts32.grow(ctx, nStrings));
		BCHK(B.spans.grow(ctx, slots)); BCHK(B.scratch.grow(ctx, slots)); BCHK(B.stack.grow(ctx, slots)); BCHK(B.kernelsDev.grow(ctx, slots));
		BCHK(B.kernelsHost.grow(slots));
		for (size_t f = 0; f < G; ++f) {
			const KhtBatchFrame& fr = B.frames[f];
			if (fr.nPts) BCHK(hipMemcpyAsync(B.pts + fr.ptsOff, B.linked + fr.ptsOff, fr.nPts * sizeof(KhtPoint), hipMemcpyHostToDevice, st));
		}
		BCHK(hipMemcpyAsync(B.strings, B.stringsHost, nStrings * sizeof(KhtStringDesc), hipMemcpyHostToDevice, st));
		KhtSubdivArgs sv;
		sv.pts = B.pts; sv.strings = B.strings; sv.nStrings = static_cast<int>(nStrings);
		sv.minSize = static_cast<int>(std::min<size_t>(clusterMinSize, 0x7fffffff)); sv.minDev = clusterMinDeviation;
		sv.scratch = B.scratch; sv.stack = B.stack; sv.counts = B.counts32; sv.clusters = B.spans; sv.total = B.totals; sv.flagIndex = kKhtBatch;
		BCHK(hipMemsetAsync(B.totals, 0, (kKhtBatch + 1) * sizeof(uint32_t), st));
		BCHK(launch_kht_subdivide(sv, tabS, st));
		uint32_t tot[kKhtBatch + 1];
		BCHK(hipMemcpyAsync(tot, B.totals, sizeof(tot), hipMemcpyDeviceToHost, st));
		BCHK(sleepSync());
		if (tot[kKhtBatch]) { err = "cluster subdivision ran out of recursion slots"; return COMPVHIP_E_INVALID_STATE; }   // cannot happen: clusterMinSize >= 2 is enforced and khtSubdivSlots bounds the depth for it
		for (size_t f = 0; f < G; ++f) B.frames[f].nClusters = B.frames[f].strings.empty() ? 0u : tot[f];
	}
	B.stageMs[1] += msSince(tc);

	// ---- D. per-cluster statistics of ALL clusters: one launch, one download per frame slice; acos / hmax, prune, Gmin and the vote parameters on the pool ----
	tc = clk::now();
	{
		KhtBatchStats tab{};
		tab.frames = static_cast<int>(G);
		bool any = false;
		for (size_t f = 0; f < G; ++f) {
			const KhtBatchFrame& fr = B.frames[f];
			tab.clusterBase[f] = static_cast<uint32_t>(fr.slotBase); tab.n[f] = static_cast<int>(fr.nClusters); tab.simdEnd[f] = khtSimdEnd(fr.nClusters);
			any = any || fr.nClusters;
		}
		if (any) {
			KhtStatsArgs sa;
			sa.pts = B.pts; sa.clusters = B.spans; sa.hw = static_cast<double>(W) * 0.5; sa.hh = static_cast<double>(H) * 0.5; sa.out = B.kernelsDev;
			BCHK(launch_kht_stats(sa, tab, st));
			for (size_t f = 0; f < G; ++f) {
				const KhtBatchFrame& fr = B.frames[f];
				if (fr.nClusters) BCHK(hipMemcpyAsync(B.kernelsHost + fr.slotBase, B.kernelsDev + fr.slotBase, fr.nClusters * sizeof(KhtKernel), hipMemcpyDeviceToHost, st));
			}
			BCHK(sleepSync());
		}
	}
	B.stageMs[2] += msSince(tc);
	pool.run(G, [&](size_t f) { guarded(f, [&](KhtBatchFrame& fr) {
		if (!fr.nClusters) return;
		auto t0 = clk::now();
		fr.kernels.assign(B.kernelsHost + fr.slotBase, B.kernelsHost + fr.slotBase + fr.nClusters);
		khtFinishKernels(fr.kernels, fr.hmax);
		fr.ms[2] += msSince(t0);
		t0 = clk::now();
		fr.GS = khtPruneAndScale(fr.kernels, fr.hmax, kernelMinHeight);
		if (!fr.kernels.empty()) { fr.haveGS = true; khtVoteParams(ax, fr.kernels, fr.params); }
		fr.ms[3] += msSince(t0);
	}); }, 'K');
	rc = firstError();
	if (rc) return rc;

	// ---- E. Gaussian voting + smoothing / threshold of ALL frames' vote maps: one launch each, the cell counts, then the cells ----
	// (canonical order: voting, then peaks + line test and the sort of every frame's lines on the GPU; the line counts, then the lines)
	const bool canon = order == COMPVHIP_KHT_ORDER_CANONICAL;
	int32_t lineCount[kKhtBatch] = {};
	tc = clk::now();
	const int stride = static_cast<int>(alignUp(ax.rhoN + 2, 16));
	const size_t mapElems = (ax.T + 2) * static_cast<size_t>(stride), cellCap = ax.T * ax.rhoN;
	KhtBatchVote tabV{};
	tabV.frames = static_cast<int>(G); tabV.mapElems = mapElems; tabV.cellCap = cellCap;
	size_t nParams = 0;
	for (size_t f = 0; f < G; ++f) {
		KhtBatchFrame& fr = B.frames[f];
		fr.paramsBase = nParams; nParams += fr.params.size();
		tabV.paramsBase[f] = static_cast<uint32_t>(fr.paramsBase); tabV.nKernels[f] = static_cast<int>(fr.params.size()); tabV.gs[f] = fr.GS;
	}
	if (nParams) {
		BCHK(B.counts.reserve(ctx, mapElems * G)); BCHK(B.cells.reserve(ctx, cellCap * G));
		BCHK(B.paramsHost.grow(nParams));
		BCHK(B.params.grow(ctx, nParams));
		for (size_t f = 0; f < G; ++f) { const KhtBatchFrame& fr = B.frames[f]; if (!fr.params.empty()) memcpy(B.paramsHost + fr.paramsBase, fr.params.data(), fr.params.size() * sizeof(KhtVoteParams)); }
		BCHK(hipMemcpyAsync(B.params, B.paramsHost, nParams * sizeof(KhtVoteParams), hipMemcpyHostToDevice, st));
		BCHK(hipMemsetAsync(B.counts, 0, mapElems * G * sizeof(int32_t), st));
		BCHK(hipMemsetAsync(B.cellCount, 0, kKhtBatch * sizeof(int), st));
		KhtGpuArgs a;
		a.params = B.params; a.nKernels = 0; a.counts = B.counts; a.stride = stride;
		a.rhoN = static_cast<int>(ax.rhoN); a.T = static_cast<int>(ax.T); a.dRho = ax.dRho; a.dThetaDeg = ax.dThetaDeg; a.gs = 1.0;
		a.threshold = threshold; a.cells = B.cells; a.cellCount = B.cellCount; a.cellCap = static_cast<int>(cellCap);
		BCHK(launch_kht_vote(a, tabV, st));
		if (canon) {
			BCHK(khtCanonTabs(ctx, B.tabs, ax, st));
			const size_t capDev = std::min(cap, cellCap);
			BCHK(B.canonLines.grow(ctx, capDev * G));
			BCHK(B.canonCounts.reserve(ctx, kKhtBatch));
			BCHK(launch_kht_canon_peaks(a, tabV, st));
			KhtCanonOut o;
			o.rho = B.tabs.rho; o.theta = B.tabs.theta; o.lines = B.canonLines; o.cap = static_cast<int>(capDev); o.counts = B.canonCounts; o.maxLines = maxLines;
			BCHK(launch_kht_canon_sort(a, tabV, o, st));
			BCHK(hipMemcpyAsync(lineCount, B.canonCounts, G * sizeof(int32_t), hipMemcpyDeviceToHost, st));
			BCHK(sleepSync());
			size_t nLines = 0;
			for (size_t f = 0; f < G; ++f) {
				if (B.frames[f].params.empty()) lineCount[f] = 0;   // (no launch covered it: nKernels == 0)
				if (lineCount[f] < 0) { err = "canonical KHT: merge scratch too small"; return COMPVHIP_E_INVALID_STATE; }   // cannot happen (kht_canon_sort_kernel)
				nLines += std::min(static_cast<size_t>(lineCount[f]), capDev);
			}
			if (nLines) {
				BCHK(B.canonLinesHost.grow(nLines));
				size_t off = 0;
				for (size_t f = 0; f < G; ++f) {
					const size_t nf = std::min(static_cast<size_t>(lineCount[f]), capDev);
					if (nf) BCHK(hipMemcpyAsync(B.canonLinesHost + off, B.canonLines + f * capDev, nf * sizeof(KhtLine), hipMemcpyDeviceToHost, st));
					off += nf;
				}
				BCHK(sleepSync());
				off = 0;
				for (size_t f = 0; f < G; ++f) {
					const size_t nf = std::min(static_cast<size_t>(lineCount[f]), capDev);
					for (size_t i = 0; i < nf; ++i) {
						const KhtLine& l = B.canonLinesHost[off + i];
						compvhip_line& d = lines[f * cap + i];
						d.rho = l.rho; d.theta = l.theta; d.strength = l.strength; d.row = l.rhoIndex; d.col = l.thetaIndex;
					}
					off += nf;
				}
			}
		}
		else {
			BCHK(launch_kht_peaks(a, tabV, st));
			int cc[kKhtBatch];
			BCHK(hipMemcpyAsync(cc, B.cellCount, sizeof(cc), hipMemcpyDeviceToHost, st));
			BCHK(sleepSync());
			size_t nCells = 0;
			for (size_t f = 0; f < G; ++f) {
				KhtBatchFrame& fr = B.frames[f];
				fr.cellCount = fr.params.empty() ? 0 : std::min<int>(cc[f], static_cast<int>(cellCap));
				fr.cellOff = nCells; nCells += static_cast<size_t>(fr.cellCount);
			}
			if (nCells) {
				BCHK(B.cellsHost.grow(nCells));
				for (size_t f = 0; f < G; ++f) {
					const KhtBatchFrame& fr = B.frames[f];
					if (fr.cellCount) BCHK(hipMemcpyAsync(B.cellsHost + fr.cellOff, B.cells + f * cellCap, static_cast<size_t>(fr.cellCount) * sizeof(KhtCell), hipMemcpyDeviceToHost, st));
				}
				BCHK(sleepSync());
			}
		}
	}
	if (canon) {
		B.stageMs[4] += msSince(tc);
		for (size_t f = 0; f < G; ++f) {
			const KhtBatchFrame& fr = B.frames[f];
			if (fr.haveGS && gs) gs[f] = fr.GS;
			counts[f] = static_cast<size_t>(lineCount[f]);
			if (counts[f] > cap) *overflow = true;
			B.stageMs[0] += fr.ms[0]; B.stageMs[2] += fr.ms[2]; B.stageMs[3] += fr.ms[3];
		}
		return COMPVHIP_OK;
	}
	B.stageMs[4] += msSince(tc);

	// ---- F. sort + sweep with the visited map (order dependent, :1195-1247): per frame, on the pool ----
	for (size_t f = 0; f < G; ++f) byWork[f] = f;
	std::sort(byWork.begin(), byWork.end(), [&](size_t a, size_t b) { return B.frames[a].cellCount > B.frames[b].cellCount; });
	pool.run(G, [&](size_t i) { const size_t f = byWork[i]; guarded(f, [&](KhtBatchFrame& fr) {
		if (fr.haveGS && gs) gs[f] = fr.GS;
		if (!fr.cellCount) { counts[f] = 0; return; }
		const auto t0 = clk::now();
		fr.cells.assign(B.cellsHost + fr.cellOff, B.cellsHost + fr.cellOff + fr.cellCount);
		// the WORKER's workspace, not the frame's: 32 frames x 1.6 MB of visited maps cycled through the caches (sort + sweep 0.69 ms for a frame alone, 1.9 in a batch)
		const int w = t_khtWorker;
		KhtPeaksWork& wk = (w >= 0 && static_cast<size_t>(w) < p->khtWork.size() && p->khtWork[w]) ? *p->khtWork[w] : fr.peaks;
		khtPeaks(ax, fr.cells, maxLines, fr.out, wk);
		counts[f] = fr.out.size();
		if (lines) khtCopyLines(fr.out, lines + f * cap, cap);
		fr.ms[5] += msSince(t0);
	}); }, 'S');
	rc = firstError();
	if (rc) return rc;
	for (size_t f = 0; f < G; ++f) {
		const KhtBatchFrame& fr = B.frames[f];
		B.stageMs[0] += fr.ms[0]; B.stageMs[2] += fr.ms[2]; B.stageMs[3] += fr.ms[3]; B.stageMs[5] += fr.ms[5];
		if (fr.out.size() > cap) *overflow = true;
	}
#undef BCHK
	return COMPVHIP_OK;
}

static int khtPlanEntry(compvhip_plan* p, const uint8_t* d_edges, float rho, float thetaDeg, int threshold, int maxLines, double clusterMinDeviation,
                        size_t clusterMinSize, double kernelMinHeight, int order, compvhip_line* lines, size_t cap, size_t* counts, double* gs, int hostThreads)
{
	compvhip_ctx* ctx = p->ctx;
	if (int rc = refuseBeyondLaunchLimit(ctx, p->frames, "compvhip_plan_houghkht")) return rc;
	if (!d_edges || !counts || (cap && !lines)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "null/invalid argument");
	const size_t W = p->W, H = p->H, S = p->S, F = p->frames;
	KhtAxes ax;
	int rc = khtCheckParams(ctx, W, H, rho, thetaDeg, threshold, clusterMinSize, kernelMinHeight, ax);
	if (rc) return rc;
	HIPCHK(ctx, hipSetDevice(ctx->device));
	unsigned hw = std::thread::hardware_concurrency();
	if (!hw) hw = 4;
	// default: what the host really grants (affinity mask, cgroup quota), at most 32, at most half the hardware threads
	size_t T = hostThreads > 0 ? static_cast<size_t>(hostThreads) : std::min<size_t>(std::min<size_t>(32, hostCpuBudget()), std::max<size_t>(1, hw / 2));
	T = std::min(T, F);
	// The frames go through the stages in GROUPS of kKhtGroup, up to four groups at a time, each with its own controller thread, stream, buffers and share
	// of the host threads: inside a group the stages are batched (one launch, one transfer per stage), and while one group is in a GPU stage the host
	// threads of the others link or sweep.  (One group of 32 frames: every stage waits for the slowest frame and the GPU stages -- 100 MB over PCIe per
	// 4K batch -- wait for all of them: 18-20 ms per batch against 10.9 ms for the thread-per-frame pipeline of round 4; measured)
	size_t group = kKhtGroup;
	if (const char* e = getenv("COMPVHIP_KHT_GROUP")) { const long v = atol(e); if (v >= 1 && v <= kKhtBatch) group = static_cast<size_t>(v); }   // lab knob
	const size_t nGroups = (F + group - 1) / group;
	// controllers = groups in flight.  A controller only enqueues GPU work, sleeps on it and posts its group's host stages to the shared workers, so there are
	// enough of them to keep the workers fed while some groups are on the GPU: all groups of a 32-frame batch, two groups per four workers otherwise.
	const size_t K = std::max<size_t>(1, std::min<size_t>(std::min<size_t>(std::max<size_t>(2, T / 2), kKhtMaxInFlight), nGroups));
	// The producer of d_edges may still be running on the caller's stream; the groups use private streams: drain the device first (the call is
	// synchronous and takes milliseconds -- the drain is not what bounds it)
	HIPCHK(ctx, hipDeviceSynchronize());
	const size_t G0 = std::min<size_t>(F, group), words = ((W + 31) / 32) * H;
	while (p->khtBatch.size() < K) {
		std::unique_ptr<KhtBatchState> b(new (std::nothrow) KhtBatchState());
		if (!b) return fail(ctx, COMPVHIP_E_OUT_OF_MEMORY, "KHT batch state");
		p->khtBatch.push_back(std::move(b));
	}
	for (size_t k = 0; k < K; ++k) {
		KhtBatchState& B = *p->khtBatch[k];
		if (!B.stream) HIPCHK(ctx, hipStreamCreateWithFlags(&B.stream, hipStreamNonBlocking));
		if (!B.syncEv) HIPCHK(ctx, hipEventCreateWithFlags(&B.syncEv, hipEventBlockingSync | hipEventDisableTiming));
		HIPCHK(ctx, B.dBits.reserve(ctx, words * G0));
		if (B.hostBits.reserve(words * G0) != hipSuccess) return fail(ctx, COMPVHIP_E_OUT_OF_MEMORY, "pinned bit planes");
		while (B.ready.size() < G0) { hipEvent_t e; HIPCHK(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming)); B.ready.push_back(e); }
		HIPCHK(ctx, B.totals.reserve(ctx, kKhtBatch + 1));
		HIPCHK(ctx, B.cellCount.reserve(ctx, kKhtBatch));
		try { if (B.frames.size() < G0) B.frames.resize(G0); }
		catch (...) { return fail(ctx, COMPVHIP_E_OUT_OF_MEMORY, "KHT batch state"); }
		memset(B.stageMs, 0, sizeof(B.stageMs));
	}
	for (size_t f = 0; f < F; ++f) counts[f] = 0;
	try {   // nothing may leave an extern "C" entry point as an exception (the vectors below allocate)
	const auto wall0 = std::chrono::steady_clock::now();
	std::atomic<size_t> nextGroup{0};
	std::vector<int> codes(K, COMPVHIP_OK);
	std::vector<std::string> errs(K);
	std::vector<size_t> badGroup(K, 0);
	std::atomic<int> overflowAny{0};
	while (p->khtWork.size() < T) p->khtWork.emplace_back(new KhtPeaksWork());
	KhtPool pool(T);   // the workers of this call, shared by every group in flight
	auto controller = [&](size_t k) {
		try {
			for (;;) {
				const size_t g = nextGroup.fetch_add(1);
				if (g >= nGroups) break;
				const size_t g0 = g * group, G = std::min<size_t>(group, F - g0);
				bool overflow = false;
				const int r = khtBatchGroup(p, *p->khtBatch[k], pool, d_edges + g0 * S * H, G, ax, threshold, maxLines, clusterMinDeviation, clusterMinSize, kernelMinHeight,
				                            order, lines ? lines + g0 * cap : nullptr, cap, counts + g0, gs ? gs + g0 : nullptr, &overflow, errs[k]);
				if (overflow) overflowAny.store(1);
				if (r) { codes[k] = r; badGroup[k] = g0; nextGroup.store(nGroups); break; }   // the other controllers finish the group they are in and stop
			}
		}
		catch (const std::exception& ex) { codes[k] = COMPVHIP_E_OUT_OF_MEMORY; errs[k] = std::string("exception in the batched KHT: ") + ex.what(); }   // nothing may leave a thread
		catch (...) { codes[k] = COMPVHIP_E_OUT_OF_MEMORY; errs[k] = "exception in the batched KHT"; }                                                   // (or an extern "C" entry point) as an exception
	};
	{
		std::vector<std::thread> ctl;
		try { for (size_t k = 1; k < K; ++k) ctl.emplace_back(controller, k); }
		catch (...) { /* the system refused a thread: the controllers that did start take all the groups */ }
		controller(0);
		for (std::thread& t : ctl) t.join();
	}
	p->khtWallMs = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
	p->khtThreads = static_cast<int>(T);
	memset(p->khtStageMs, 0, sizeof(p->khtStageMs));
	for (size_t k = 0; k < K; ++k) for (int i = 0; i < 6; ++i) p->khtStageMs[i] += p->khtBatch[k]->stageMs[i];
	for (size_t k = 0; k < K; ++k)
		if (codes[k]) return fail(ctx, codes[k], ("frames from " + std::to_string(badGroup[k]) + ": " + errs[k]).c_str());
	if (overflowAny.load()) return fail(ctx, COMPVHIP_E_OUT_OF_BOUND, "line buffer too small");
	}
	catch (const std::exception& ex) { return fail(ctx, COMPVHIP_E_OUT_OF_MEMORY, (std::string("exception in the batched KHT: ") + ex.what()).c_str()); }
	catch (...) { return fail(ctx, COMPVHIP_E_OUT_OF_MEMORY, "exception in the batched KHT"); }
	return COMPVHIP_OK;
}

int compvhip_plan_houghkht(compvhip_plan* p, const uint8_t* d_edges, float rho, float thetaDeg, int threshold, int maxLines, double clusterMinDeviation,
                           size_t clusterMinSize, double kernelMinHeight, compvhip_line* lines, size_t cap, size_t* counts, double* gs, int hostThreads)
{
	if (!p) return COMPVHIP_E_INVALID_PARAMETER;
	return khtPlanEntry(p, d_edges, rho, thetaDeg, threshold, maxLines, clusterMinDeviation, clusterMinSize, kernelMinHeight, COMPVHIP_KHT_ORDER_REFERENCE,
	                    lines, cap, counts, gs, hostThreads);
}

int compvhip_plan_houghkht_ex(compvhip_plan* p, const uint8_t* d_edges, const compvhip_kht_opts* opts, compvhip_line* lines, size_t cap, size_t* counts, double* gs)
{
	if (!p) return COMPVHIP_E_INVALID_PARAMETER;
	compvhip_kht_opts k;
	if (!opts || !khtResolveOpts(opts, k)) return fail(p->ctx, COMPVHIP_E_INVALID_PARAMETER, "null options or unknown KHT order");
	return khtPlanEntry(p, d_edges, k.rho, k.thetaDeg, k.threshold, k.maxLines, k.clusterMinDeviation, k.clusterMinSize, k.kernelMinHeight, k.order,
	                    lines, cap, counts, gs, k.hostThreads);
}

int compvhip_plan_houghkht_stage_ms(compvhip_plan* p, double* ms6, double* wallMs, int* threads)
{
	if (!p || !ms6) return COMPVHIP_E_INVALID_PARAMETER;
	memcpy(ms6, p->khtStageMs, sizeof(p->khtStageMs));
	if (wallMs) *wallMs = p->khtWallMs;
	if (threads) *threads = p->khtThreads;
	return COMPVHIP_OK;
}
