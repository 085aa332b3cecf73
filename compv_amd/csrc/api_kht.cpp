// api_kht.cpp -- kernel-based Hough transform: ONE driver of the stages over a group of frames (GPU stages batched, host stages per frame), run by the host
// entry points on a group of one frame and by the batched plan call on several groups at a time, with the host stages on a KhtPool.
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
// CompVHoughKht::process (houghkht.cxx:208-447) on a GROUP of 1 <= G <= kKhtBatch frames that go through the stages TOGETHER: the host stages (bit-plane
// linking, prune / Gmin, sort + sweep: sequential per frame, independent between frames) are loops over the frames, the GPU stages are ONE launch each over
// the strings / clusters / kernels / vote maps of all frames (kht.hpp: the per-frame tables travel in the kernel arguments, kht_group.hpp builds them), with
// one upload and one download per stage.  There is one driver: the plan call runs groups of kKhtGroup frames, several at a time, with the host loops on a
// pool of threads; the host entry points run a group of one frame on the calling thread.
// (Rounds 3-4 gave every worker thread its own stream and let it drive its frame's five small launches and four synchronisations: with 32 workers the
// GPU-touching stages took 5-9 x their single-frame time -- a launch / synchronisation pile-up, not compute.)
using KhtClock = std::chrono::steady_clock;
static double msSince(KhtClock::time_point a) { return std::chrono::duration<double, std::milli>(KhtClock::now() - a).count(); }

// One run of the stages over a group: the state, who runs the per-frame host loops, the call's resolved options and where its results go.  Several groups of
// a plan call run at the same time, each on its own controller thread: a stage touches nothing shared but ctx->live (atomic) and reports a failure as
// (code, err) -- only the exported function writes ctx->err.
struct KhtRun {
	compvhip_ctx* ctx; KhtGroupState& B;
	KhtPool* pool;                                                  // nullptr: a plain loop on the calling thread
	size_t G, W, H;
	const compvhip_kht_opts& k; const KhtAxes& ax;
	compvhip_line* lines; size_t cap; size_t* counts; double* gs;   // of frame f: lines + f * cap, counts[f], gs[f] (written when a kernel survives the pruning)
	std::vector<std::unique_ptr<KhtPeaksWork>>* work;               // the pool workers' sort + sweep workspaces (nullptr: the frames' own)
	bool overflow = false; std::string err;
};

// (an early return must not leave asynchronous copies in flight towards a stage's stack arrays or the pinned state: drain the stream first, result ignored)
static int khtFail(KhtRun& r, int code, std::string text)
{
	r.err = std::move(text);
	(void)hipStreamSynchronize(r.B.stream);
	return code;
}
#define KCHK(r, call) do { hipError_t e__ = (call); if (e__ != hipSuccess) return khtFail((r), COMPVHIP_E_HIP, std::string(#call) + ": " + hipGetErrorString(e__)); } while (0)

// body(f, frame) for the group's frames that have not failed, in the order byWork (nullptr: 0 .. G - 1), on the pool or on the calling thread; nothing leaves
// it as an exception (a pool thread, an extern "C" entry point).  Returns the first failed frame's code.
static int khtEachFrame(KhtRun& r, char tag, const size_t* byWork, const std::function<void(size_t, KhtFrameState&)>& body)
{
	const std::function<void(size_t)> item = [&](size_t i) {
		const size_t f = byWork ? byWork[i] : i;
		KhtFrameState& fr = r.B.frames[f];
		if (fr.code) return;
		try { body(f, fr); }
		catch (const std::exception& ex) { fr.code = COMPVHIP_E_OUT_OF_MEMORY; fr.err = std::string("exception in a KHT stage: ") + ex.what(); }
		catch (...) { fr.code = COMPVHIP_E_OUT_OF_MEMORY; fr.err = "exception in a KHT stage"; }
	};
	if (r.pool) r.pool->run(r.G, item, tag);
	else for (size_t i = 0; i < r.G; ++i) item(i);
	for (size_t f = 0; f < r.G; ++f)
		if (r.B.frames[f].code) return khtFail(r, r.B.frames[f].code, "frame " + std::to_string(f) + " of its group: " + r.B.frames[f].err);
	return COMPVHIP_OK;
}

// the frames by decreasing work(frame): the items are milliseconds long and few, the last ones decide when the group moves on
template <class Work>
static void khtLongestFirst(const KhtRun& r, size_t* byWork, Work work)
{
	for (size_t f = 0; f < r.G; ++f) byWork[f] = f;
	std::sort(byWork, byWork + r.G, [&](size_t a, size_t b) { return work(r.B.frames[a]) > work(r.B.frames[b]); });
}

// a run starts: the group's frames exist and are empty
static int khtBegin(KhtRun& r)
{
	KCHK(r, hipSetDevice(r.ctx->device));
	try { if (r.B.frames.size() < r.G) r.B.frames.resize(r.G); }
	catch (...) { return khtFail(r, COMPVHIP_E_OUT_OF_MEMORY, "KHT group state"); }
	for (size_t f = 0; f < r.G; ++f) {
		KhtFrameState& fr = r.B.frames[f];
		fr.code = COMPVHIP_OK; fr.err.clear(); fr.most = 0; fr.nPts = 0; fr.strings.clear(); fr.nClusters = 0; fr.kernels.clear(); fr.hmax = 0.0; fr.params.clear();
		fr.cells.clear(); fr.cellCount = 0; fr.out.clear(); fr.haveGS = false;
		memset(fr.ms, 0, sizeof(fr.ms));
	}
	return COMPVHIP_OK;
}

// ---- the planes (plan call): the edge maps leave the device as bit-mask rows (1/8 of the bytes over PCIe; the linker works on bits anyway): one kernel, one copy per frame ----
static int khtFetchPlanes(KhtRun& r, const uint8_t* d_edges, size_t S)
{
	KhtGroupState& B = r.B;
	const size_t W = r.W, H = r.H, wpr = (W + 31) / 32, words = wpr * H;
	KCHK(r, launch_bytes_to_bits(d_edges, static_cast<int>(W), static_cast<int>(H), static_cast<int>(S), S * H, B.dBits, static_cast<int>(wpr), words, static_cast<int>(r.G), B.stream));
	for (size_t f = 0; f < r.G; ++f) {
		KCHK(r, hipMemcpyAsync(B.hostBits + f * words, B.dBits + f * words, words * sizeof(uint32_t), hipMemcpyDeviceToHost, B.stream));
		KCHK(r, hipEventRecord(B.ready[f], B.stream));
	}
	return khtEachFrame(r, 'P', nullptr, [&](size_t f, KhtFrameState& fr) {
		const auto t0 = KhtClock::now();
		if (hipSetDevice(r.ctx->device) != hipSuccess || hipEventSynchronize(B.ready[f]) != hipSuccess) { fr.code = COMPVHIP_E_HIP; fr.err = "frame download"; return; }
		khtPlaneFromWords(B.hostBits + f * words, wpr, W, H, fr.plane);
		fr.most = khtPlaneCount(fr.plane);
		fr.ms[0] += msSince(t0);
	});
}

// ---- linking (Appendix A): sequential inside a frame, the frames in parallel; every frame's points go straight into its slice of the pinned arena ----
static int khtLinkFrames(KhtRun& r)
{
	KhtGroupState& B = r.B;
	size_t total = 0;
	for (size_t f = 0; f < r.G; ++f) { B.frames[f].ptsOff = total; total += B.frames[f].most; }
	if (total > 0x7fffffffull) return khtFail(r, COMPVHIP_E_INVALID_PARAMETER, "too many edge pixels");
	KCHK(r, B.linked.grow(total + 1));
	size_t byWork[kKhtBatch];
	khtLongestFirst(r, byWork, [](const KhtFrameState& fr) { return fr.most; });
	return khtEachFrame(r, 'L', byWork, [&](size_t, KhtFrameState& fr) {
		const auto t0 = KhtClock::now();
		fr.nPts = khtLink(fr.plane, r.k.clusterMinSize, B.linked + fr.ptsOff, fr.strings);
		fr.ms[0] += msSince(t0);
	});
}

// ---- cluster subdivision of ALL strings (kht_subdivide_kernel, one wave per string): one upload per frame slice, one launch, one download ----
static int khtSubdivide(KhtRun& r)
{
	KhtGroupState& B = r.B; compvhip_ctx* ctx = r.ctx; hipStream_t st = B.stream;
	const auto tc = KhtClock::now();
	const size_t G = r.G, total = B.frames[G - 1].ptsOff + B.frames[G - 1].most;
	size_t nStrings = 0, slots = 0;
	for (size_t f = 0; f < G; ++f) nStrings += B.frames[f].strings.size();
	if (nStrings) {
		KCHK(r, B.stringsHost.grow(nStrings));
		KhtBatchStrings tab;
		if (!khtStringTables(B.frames.data(), G, r.k.clusterMinSize, B.stringsHost.ptr, tab, slots)) return khtFail(r, COMPVHIP_E_INVALID_PARAMETER, "too many cluster slots");
		KCHK(r, B.pts.grow(ctx, total + 1));
		KCHK(r, B.strings.grow(ctx, nStrings)); KCHK(r, B.counts32.grow(ctx, nStrings)); KCHK(r, B.totals.reserve(ctx, kKhtBatch + 1));
		KCHK(r, B.spans.grow(ctx, slots)); KCHK(r, B.scratch.grow(ctx, slots)); KCHK(r, B.stack.grow(ctx, slots)); KCHK(r, B.kernelsDev.grow(ctx, slots));
		KCHK(r, B.kernelsHost.grow(slots));
		for (size_t f = 0; f < G; ++f) {
			const KhtFrameState& fr = B.frames[f];
			if (fr.nPts) KCHK(r, hipMemcpyAsync(B.pts + fr.ptsOff, B.linked + fr.ptsOff, fr.nPts * sizeof(KhtPoint), hipMemcpyHostToDevice, st));
		}
		KCHK(r, hipMemcpyAsync(B.strings, B.stringsHost, nStrings * sizeof(KhtStringDesc), hipMemcpyHostToDevice, st));
		KhtSubdivArgs sv;
		sv.pts = B.pts; sv.strings = B.strings; sv.nStrings = static_cast<int>(nStrings);
		sv.minSize = static_cast<int>(std::min<size_t>(r.k.clusterMinSize, 0x7fffffff)); sv.minDev = r.k.clusterMinDeviation;
		sv.scratch = B.scratch; sv.stack = B.stack; sv.counts = B.counts32; sv.clusters = B.spans; sv.total = B.totals; sv.flagIndex = kKhtBatch;
		KCHK(r, hipMemsetAsync(B.totals, 0, (kKhtBatch + 1) * sizeof(uint32_t), st));   // clusters per frame, then the "recursion truncated" flag
		KCHK(r, launch_kht_subdivide(sv, tab, st));
		uint32_t tot[kKhtBatch + 1];
		KCHK(r, hipMemcpyAsync(tot, B.totals, sizeof(tot), hipMemcpyDeviceToHost, st));
		KCHK(r, B.wait());
		if (tot[kKhtBatch]) return khtFail(r, COMPVHIP_E_INVALID_STATE, "cluster subdivision ran out of recursion slots");   // cannot happen: clusterMinSize >= 2 is enforced and khtSubdivSlots bounds the depth for it
		for (size_t f = 0; f < G; ++f) B.frames[f].nClusters = B.frames[f].strings.empty() ? 0u : tot[f];
	}
	B.stageMs[1] += msSince(tc);
	return COMPVHIP_OK;
}

// ---- per-cluster statistics of ALL clusters (kht_stats_kernel, one thread per cluster): one launch, one download per frame slice; then, per frame, acos /
// hmax and -- unless the run stops at the kernels (statsOnly) -- prune, Gmin and the vote parameters ----
static int khtKernels(KhtRun& r, bool statsOnly)
{
	KhtGroupState& B = r.B; hipStream_t st = B.stream;
	const auto tc = KhtClock::now();
	KhtBatchStats tab;
	if (khtStatsTable(B.frames.data(), r.G, tab)) {
		KhtStatsArgs sa;
		sa.pts = B.pts; sa.clusters = B.spans; sa.hw = static_cast<double>(r.W) * 0.5; sa.hh = static_cast<double>(r.H) * 0.5; sa.out = B.kernelsDev;
		KCHK(r, launch_kht_stats(sa, tab, st));
		for (size_t f = 0; f < r.G; ++f) {
			const KhtFrameState& fr = B.frames[f];
			if (fr.nClusters) KCHK(r, hipMemcpyAsync(B.kernelsHost + fr.slotBase, B.kernelsDev + fr.slotBase, fr.nClusters * sizeof(KhtKernel), hipMemcpyDeviceToHost, st));
		}
		KCHK(r, B.wait());
	}
	B.stageMs[2] += msSince(tc);
	return khtEachFrame(r, 'K', nullptr, [&](size_t, KhtFrameState& fr) {
		if (!fr.nClusters) return;
		auto t0 = KhtClock::now();
		fr.kernels.assign(B.kernelsHost + fr.slotBase, B.kernelsHost + fr.slotBase + fr.nClusters);
		khtFinishKernels(fr.kernels, fr.hmax);
		fr.ms[2] += msSince(t0);
		if (statsOnly) return;
		t0 = KhtClock::now();
		fr.GS = khtPruneAndScale(fr.kernels, fr.hmax, r.k.kernelMinHeight);
		if (!fr.kernels.empty()) { fr.haveGS = true; khtVoteParams(r.ax, fr.kernels, fr.params); }
		fr.ms[3] += msSince(t0);
	});
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

static_assert(sizeof(compvhip_line) == sizeof(KhtLine), "KhtLine has compvhip_line's layout (kht.hpp)");
static void khtCopyLines(const KhtLine* from, size_t n, compvhip_line* to) { if (n) memcpy(to, from, n * sizeof(KhtLine)); }

// reference order: smoothing / threshold of every vote map (kht_peaks_kernel), the cell counts, then the cells; the sweep follows on the host (khtSweep)
static int khtPeakCells(KhtRun& r, const KhtGpuArgs& a, const KhtBatchVote& tab)
{
	KhtGroupState& B = r.B; hipStream_t st = B.stream;
	KCHK(r, launch_kht_peaks(a, tab, st));
	int cc[kKhtBatch];
	KCHK(r, hipMemcpyAsync(cc, B.cellCount, sizeof(cc), hipMemcpyDeviceToHost, st));
	KCHK(r, B.wait());
	size_t nCells = 0;
	for (size_t f = 0; f < r.G; ++f) {
		KhtFrameState& fr = B.frames[f];
		fr.cellCount = fr.params.empty() ? 0 : std::min<int>(cc[f], static_cast<int>(tab.cellCap));   // (no launch covered a frame without kernels)
		fr.cellOff = nCells; nCells += static_cast<size_t>(fr.cellCount);
	}
	if (!nCells) return COMPVHIP_OK;
	KCHK(r, B.cellsHost.grow(nCells));
	for (size_t f = 0; f < r.G; ++f) {
		const KhtFrameState& fr = B.frames[f];
		if (fr.cellCount) KCHK(r, hipMemcpyAsync(B.cellsHost + fr.cellOff, B.cells + f * tab.cellCap, static_cast<size_t>(fr.cellCount) * sizeof(KhtCell), hipMemcpyDeviceToHost, st));
	}
	KCHK(r, B.wait());
	return COMPVHIP_OK;
}

// canonical order: peaks + line test (kht_canon_peaks_kernel) and the sort of every frame's lines (kht_canon_sort_kernel) on the GPU; the line counts, then
// the lines, which are final: counts[f] = the lines after the maxLines cut, of which the caller gets the first min(counts[f], cap)
static int khtCanonLines(KhtRun& r, const KhtGpuArgs& a, const KhtBatchVote& tab)
{
	KhtGroupState& B = r.B; compvhip_ctx* ctx = r.ctx; hipStream_t st = B.stream;
	KCHK(r, khtCanonTabs(ctx, B.tabs, r.ax, st));
	const size_t capDev = std::min(r.cap, tab.cellCap);
	KCHK(r, B.canonLines.grow(ctx, capDev * r.G));
	KCHK(r, B.canonCounts.reserve(ctx, kKhtBatch));
	KCHK(r, launch_kht_canon_peaks(a, tab, st));
	KhtCanonOut o;
	o.rho = B.tabs.rho; o.theta = B.tabs.theta; o.lines = B.canonLines; o.cap = static_cast<int>(capDev); o.counts = B.canonCounts; o.maxLines = r.k.maxLines;
	KCHK(r, launch_kht_canon_sort(a, tab, o, st));
	int32_t lineCount[kKhtBatch] = {};
	KCHK(r, hipMemcpyAsync(lineCount, B.canonCounts, r.G * sizeof(int32_t), hipMemcpyDeviceToHost, st));
	KCHK(r, B.wait());
	size_t nLines = 0, lineOff[kKhtBatch + 1];
	for (size_t f = 0; f < r.G; ++f) {
		if (B.frames[f].params.empty()) lineCount[f] = 0;   // (no launch covered it: nKernels == 0)
		if (lineCount[f] < 0) return khtFail(r, COMPVHIP_E_INVALID_STATE, "canonical KHT: merge scratch too small");   // cannot happen (kht_canon_sort_kernel)
		r.counts[f] = static_cast<size_t>(lineCount[f]);
		lineOff[f] = nLines; nLines += std::min(r.counts[f], capDev);
	}
	lineOff[r.G] = nLines;
	if (!nLines) return COMPVHIP_OK;
	KCHK(r, B.canonLinesHost.grow(nLines));
	for (size_t f = 0; f < r.G; ++f)
		if (lineOff[f + 1] > lineOff[f]) KCHK(r, hipMemcpyAsync(B.canonLinesHost + lineOff[f], B.canonLines + f * capDev, (lineOff[f + 1] - lineOff[f]) * sizeof(KhtLine), hipMemcpyDeviceToHost, st));
	KCHK(r, B.wait());
	for (size_t f = 0; f < r.G; ++f) khtCopyLines(B.canonLinesHost + lineOff[f], lineOff[f + 1] - lineOff[f], r.lines + f * r.cap);
	return COMPVHIP_OK;
}

// ---- Gaussian voting of ALL frames' kernels into their vote maps (kht_vote_kernel): one upload, one launch; then the peaks in the call's order ----
static int khtVote(KhtRun& r)
{
	KhtGroupState& B = r.B; compvhip_ctx* ctx = r.ctx; hipStream_t st = B.stream;
	const KhtAxes& ax = r.ax;
	const auto tc = KhtClock::now();
	const int stride = static_cast<int>(alignUp(ax.rhoN + 2, 16));
	const size_t mapElems = (ax.T + 2) * static_cast<size_t>(stride), cellCap = ax.T * ax.rhoN;
	KhtBatchVote tab;
	const size_t nParams = khtVoteTable(B.frames.data(), r.G, mapElems, cellCap, tab);
	if (nParams) {
		KCHK(r, B.counts.reserve(ctx, mapElems * r.G)); KCHK(r, B.cells.reserve(ctx, cellCap * r.G)); KCHK(r, B.cellCount.reserve(ctx, kKhtBatch));
		KCHK(r, B.paramsHost.grow(nParams));
		KCHK(r, B.params.grow(ctx, nParams));
		for (size_t f = 0; f < r.G; ++f) { const KhtFrameState& fr = B.frames[f]; if (!fr.params.empty()) memcpy(B.paramsHost + fr.paramsBase, fr.params.data(), fr.params.size() * sizeof(KhtVoteParams)); }
		KCHK(r, hipMemcpyAsync(B.params, B.paramsHost, nParams * sizeof(KhtVoteParams), hipMemcpyHostToDevice, st));
		KCHK(r, hipMemsetAsync(B.counts, 0, mapElems * r.G * sizeof(int32_t), st));
		KCHK(r, hipMemsetAsync(B.cellCount, 0, kKhtBatch * sizeof(int), st));
		KhtGpuArgs a;   // (nKernels and gs travel per frame, in the table)
		a.params = B.params; a.nKernels = 0; a.counts = B.counts; a.stride = stride;
		a.rhoN = static_cast<int>(ax.rhoN); a.T = static_cast<int>(ax.T); a.dRho = ax.dRho; a.dThetaDeg = ax.dThetaDeg; a.gs = 1.0;
		a.threshold = r.k.threshold; a.cells = B.cells; a.cellCount = B.cellCount; a.cellCap = static_cast<int>(cellCap);
		KCHK(r, launch_kht_vote(a, tab, st));
		if (const int rc = r.k.order == COMPVHIP_KHT_ORDER_CANONICAL ? khtCanonLines(r, a, tab) : khtPeakCells(r, a, tab)) return rc;
	}
	B.stageMs[4] += msSince(tc);
	return COMPVHIP_OK;
}

// ---- reference order: sort + sweep with the visited map (order dependent, :1195-1247), per frame ----
static int khtSweep(KhtRun& r)
{
	KhtGroupState& B = r.B;
	size_t byWork[kKhtBatch];
	khtLongestFirst(r, byWork, [](const KhtFrameState& fr) { return fr.cellCount; });
	return khtEachFrame(r, 'S', byWork, [&](size_t f, KhtFrameState& fr) {
		if (!fr.cellCount) return;
		const auto t0 = KhtClock::now();
		fr.cells.assign(B.cellsHost + fr.cellOff, B.cellsHost + fr.cellOff + fr.cellCount);
		// a pool WORKER's workspace, not the frame's: 32 frames x 1.6 MB of visited maps cycled through the caches (sort + sweep 0.69 ms for a frame alone, 1.9 in a batch)
		const int w = t_khtWorker;
		KhtPeaksWork& wk = (r.work && w >= 0 && static_cast<size_t>(w) < r.work->size() && (*r.work)[w]) ? *(*r.work)[w] : fr.peaks;
		khtPeaks(r.ax, fr.cells, r.k.maxLines, fr.out, wk);
		r.counts[f] = fr.out.size();
		khtCopyLines(fr.out.data(), std::min(fr.out.size(), r.cap), r.lines + f * r.cap);
		fr.ms[5] += msSince(t0);
	});
}

// The stages from the linking on, over frames whose planes are filled.  statsOnly: stop behind the kernels' statistics, before the pruning
// (compvhip_houghkht_kernels_u8).  Then the frames' GS, the "a frame has more lines than cap" mark and the frames' share of the stage clocks.
static int khtStages(KhtRun& r, bool statsOnly)
{
	int rc = khtLinkFrames(r);
	if (!rc) rc = khtSubdivide(r);
	if (!rc) rc = khtKernels(r, statsOnly);
	if (!rc && !statsOnly) rc = khtVote(r);
	if (!rc && !statsOnly && r.k.order == COMPVHIP_KHT_ORDER_REFERENCE) rc = khtSweep(r);
	if (rc) return rc;
	for (size_t f = 0; f < r.G; ++f) {
		const KhtFrameState& fr = r.B.frames[f];
		if (fr.haveGS && r.gs) r.gs[f] = fr.GS;
		if (!statsOnly && r.counts[f] > r.cap) r.overflow = true;
		for (int i = 0; i < 6; ++i) r.B.stageMs[i] += fr.ms[i];
	}
	return COMPVHIP_OK;
}

static int khtCheckParams(compvhip_ctx* ctx, size_t W, size_t H, const compvhip_kht_opts& k, KhtAxes& ax)
{
	if (!(k.rho > 0.f) || k.rho > 1.f || !(k.thetaDeg > 0.f) || k.threshold <= 0) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "rho in (0,1], theta > 0, threshold > 0"); // :146-163,491
	if (!k.clusterMinSize || !(k.kernelMinHeight >= 0.0)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "invalid KHT knob"); // :169-186 (the deviation is unchecked there)
	// Defined deviation: the reference's set() accepts a cluster size of 1 and its clusters_subdivision then recurses without bound on the first
	// collinear string (max_index stays at start_index, both "halves" hold >= 1 point: houghkht.cxx:795-821) -- a stack overflow, not a result.
	if (k.clusterMinSize < 2) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "clusterMinSize must be >= 2 (the reference's recursion does not terminate for 1)");
	if (!W || !H || W > 32767 || H > 32767) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "image size out of range");
	if (!khtAxes(W, H, k.rho, k.thetaDeg, ax)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "degenerate KHT parameter space");
	// the peak stage identifies a vote cell by the 32-bit key theta * 2 (rhoN + 2) + rho (KhtCell::order) and indexes the vote map with ints
	if (static_cast<uint64_t>(ax.T + 2) * 2u * (ax.rhoN + 2) >= (1ull << 32) || static_cast<uint64_t>(ax.T + 2) * (ax.rhoN + 2) > 0x7fffffffull)
		return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "KHT parameter space too fine for this image size ((T + 2) * 2 (rhoN + 2) must stay below 2^32)");
	return COMPVHIP_OK;
}

// the knobs of the loose-parameter exports as the options struct, taken as they are (no zero field stands for a default there)
static compvhip_kht_opts khtOpts(float rho, float thetaDeg, int threshold, int maxLines, double clusterMinDeviation, size_t clusterMinSize, double kernelMinHeight, int hostThreads)
{
	compvhip_kht_opts k{};
	k.rho = rho; k.thetaDeg = thetaDeg; k.threshold = threshold; k.maxLines = maxLines; k.clusterMinDeviation = clusterMinDeviation;
	k.clusterMinSize = clusterMinSize; k.kernelMinHeight = kernelMinHeight; k.hostThreads = hostThreads; k.order = COMPVHIP_KHT_ORDER_REFERENCE;
	return k;
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

// ---- the host entry points: the context's group of one frame, on the context's stream and the calling thread (no pool, no thread; the stages wait with
// hipStreamSynchronize).  The caller's bytes are packed into the frame's bit plane (the linker destroys its plane, never the caller's map), then the
// stages run from the linking on.  r.G == 1, r.B == ctx->kht.
static int khtHostRun(KhtRun& r, const uint8_t* edges, size_t S, bool statsOnly)
{
	r.B.stream = r.ctx->stream;
	memset(r.B.stageMs, 0, sizeof(r.B.stageMs));
	int rc = khtBegin(r);
	if (!rc) rc = khtEachFrame(r, 'P', nullptr, [&](size_t, KhtFrameState& fr) {
		const auto t0 = KhtClock::now();
		khtPackBytes(edges, r.W, r.H, S, fr.plane);
		fr.most = khtPlaneCount(fr.plane);
		fr.ms[0] += msSince(t0);
	});
	return rc ? rc : khtStages(r, statsOnly);
}

static int khtHostEntry(compvhip_ctx* ctx, const uint8_t* edges, size_t W, size_t H, size_t S, const compvhip_kht_opts& k, compvhip_line* lines, size_t cap, size_t* n, double* gs)
{
	if (!edges || !n || (cap && !lines) || S < W || !W || !H) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "null/invalid argument"); // houghkht.cxx:210-211
	KhtAxes ax;
	if (const int rc = khtCheckParams(ctx, W, H, k, ax)) return rc;
	*n = 0;
	KhtRun r{ ctx, ctx->kht, nullptr, 1, W, H, k, ax, lines, cap, n, gs, nullptr };
	if (const int rc = khtHostRun(r, edges, S, false)) return fail(ctx, rc, r.err.c_str());
	if (r.overflow) return fail(ctx, COMPVHIP_E_OUT_OF_BOUND, "line buffer too small");
	return COMPVHIP_OK;
}

int compvhip_houghkht_u8(compvhip_ctx* ctx, const uint8_t* edges, size_t W, size_t H, size_t S, float rho, float thetaDeg, int threshold, int maxLines,
                         double clusterMinDeviation, size_t clusterMinSize, double kernelMinHeight, compvhip_line* lines, size_t cap, size_t* n, double* gs)
{
	if (!ctx) return COMPVHIP_E_INVALID_PARAMETER;
	return khtHostEntry(ctx, edges, W, H, S, khtOpts(rho, thetaDeg, threshold, maxLines, clusterMinDeviation, clusterMinSize, kernelMinHeight, 0), lines, cap, n, gs);
}

int compvhip_houghkht_ex_u8(compvhip_ctx* ctx, const uint8_t* edges, size_t W, size_t H, size_t S, const compvhip_kht_opts* opts,
                            compvhip_line* lines, size_t cap, size_t* n, double* gs)
{
	if (!ctx) return COMPVHIP_E_INVALID_PARAMETER;
	compvhip_kht_opts k;
	if (!opts || !khtResolveOpts(opts, k)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "null options or unknown KHT order");
	return khtHostEntry(ctx, edges, W, H, S, k, lines, cap, n, gs);
}

// stage inspection: the kernels of the frame in cluster order and hmax, before the pruning
int compvhip_houghkht_kernels_u8(compvhip_ctx* ctx, const uint8_t* edges, size_t W, size_t H, size_t S, double clusterMinDeviation, size_t clusterMinSize,
                                 double* kernels7, size_t cap, size_t* n, double* hmax)
{
	if (!ctx) return COMPVHIP_E_INVALID_PARAMETER;
	if (!edges || !n || (cap && !kernels7) || S < W || !W || !H || clusterMinSize < 2) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "null/invalid argument (clusterMinSize >= 2)");
	if (W > 32767 || H > 32767) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "image size out of range");
	const compvhip_kht_opts k = khtOpts(1.f, 1.f, 1, 0, clusterMinDeviation, clusterMinSize, 0.0, 0);   // (only the two cluster knobs reach the stages that run)
	const KhtAxes ax{};
	KhtRun r{ ctx, ctx->kht, nullptr, 1, W, H, k, ax, nullptr, 0, nullptr, nullptr, nullptr };
	if (const int rc = khtHostRun(r, edges, S, true)) return fail(ctx, rc, r.err.c_str());
	const std::vector<KhtKernel>& kernels = ctx->kht.frames[0].kernels;
	*n = kernels.size();
	if (hmax) *hmax = ctx->kht.frames[0].hmax;
	for (size_t i = 0; i < std::min(kernels.size(), cap); ++i) {
		const KhtKernel& kk = kernels[i];
		const double v[7] = { kk.rho, kk.theta, kk.h, kk.sigmaThetaSquare, kk.sigmaRhoSquare, kk.m2, kk.sigmaRhoTimesTheta };
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

// ---- the plan call (compvhip_plan_houghkht, _ex): the frames go through the stages in GROUPS of kKhtGroup, several groups at a time, each with its own
// controller thread, state (stream, buffers, bit planes) and share of the host threads: inside a group the stages are batched (one launch, one transfer per
// stage), and while one group is in a GPU stage the host threads of the others link or sweep.  (One group of 32 frames: every stage waits for the slowest
// frame and the GPU stages -- 100 MB over PCIe per 4K batch -- wait for all of them: 18-20 ms per batch against 10.9 ms for the thread-per-frame pipeline of
// round 4; measured)

// the states of K groups in flight of up to G0 frames: a stream and a blocking-sync event of their own (a controller that waits for a GPU stage sleeps),
// the bit planes and their events
static int khtPlanStates(compvhip_plan* p, size_t K, size_t G0)
{
	compvhip_ctx* ctx = p->ctx;
	const size_t words = ((p->W + 31) / 32) * p->H;
	while (p->khtBatch.size() < K) {
		std::unique_ptr<KhtGroupState> b(new (std::nothrow) KhtGroupState());
		if (!b) return fail(ctx, COMPVHIP_E_OUT_OF_MEMORY, "KHT batch state");
		p->khtBatch.push_back(std::move(b));
	}
	for (size_t k = 0; k < K; ++k) {
		KhtGroupState& B = *p->khtBatch[k];
		if (!B.stream) { HIPCHK(ctx, hipStreamCreateWithFlags(&B.stream, hipStreamNonBlocking)); B.ownsStream = true; }
		if (!B.syncEv) HIPCHK(ctx, hipEventCreateWithFlags(&B.syncEv, hipEventBlockingSync | hipEventDisableTiming));
		HIPCHK(ctx, B.dBits.reserve(ctx, words * G0));
		if (B.hostBits.reserve(words * G0) != hipSuccess) return fail(ctx, COMPVHIP_E_OUT_OF_MEMORY, "pinned bit planes");
		while (B.ready.size() < G0) { hipEvent_t e; HIPCHK(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming)); B.ready.push_back(e); }
		memset(B.stageMs, 0, sizeof(B.stageMs));
	}
	return COMPVHIP_OK;
}

static int khtPlanEntry(compvhip_plan* p, const uint8_t* d_edges, const compvhip_kht_opts& k, compvhip_line* lines, size_t cap, size_t* counts, double* gs)
{
	compvhip_ctx* ctx = p->ctx;
	if (int rc = refuseBeyondLaunchLimit(ctx, p->frames, "compvhip_plan_houghkht")) return rc;
	if (!d_edges || !counts || (cap && !lines)) return fail(ctx, COMPVHIP_E_INVALID_PARAMETER, "null/invalid argument");
	const size_t W = p->W, H = p->H, S = p->S, F = p->frames;
	KhtAxes ax;
	if (const int rc = khtCheckParams(ctx, W, H, k, ax)) return rc;
	HIPCHK(ctx, hipSetDevice(ctx->device));
	unsigned hw = std::thread::hardware_concurrency();
	if (!hw) hw = 4;
	// default: what the host really grants (affinity mask, cgroup quota), at most 32, at most half the hardware threads
	size_t T = k.hostThreads > 0 ? static_cast<size_t>(k.hostThreads) : std::min<size_t>(std::min<size_t>(32, hostCpuBudget()), std::max<size_t>(1, hw / 2));
	T = std::min(T, F);
	size_t group = kKhtGroup;
	if (const char* e = getenv("COMPVHIP_KHT_GROUP")) { const long v = atol(e); if (v >= 1 && v <= kKhtBatch) group = static_cast<size_t>(v); }   // lab knob
	const size_t nGroups = (F + group - 1) / group;
	// controllers = groups in flight.  A controller only enqueues GPU work, sleeps on it and posts its group's host stages to the shared workers, so there are
	// enough of them to keep the workers fed while some groups are on the GPU: all groups of a 32-frame batch, two groups per four workers otherwise.
	const size_t K = std::max<size_t>(1, std::min<size_t>(std::min<size_t>(std::max<size_t>(2, T / 2), kKhtMaxInFlight), nGroups));
	// The producer of d_edges may still be running on the caller's stream; the groups use private streams: drain the device first (the call is
	// synchronous and takes milliseconds -- the drain is not what bounds it)
	HIPCHK(ctx, hipDeviceSynchronize());
	if (const int rc = khtPlanStates(p, K, std::min<size_t>(F, group))) return rc;
	for (size_t f = 0; f < F; ++f) counts[f] = 0;
	try {   // nothing may leave an extern "C" entry point as an exception (the vectors below allocate)
	const auto wall0 = KhtClock::now();
	std::atomic<size_t> nextGroup{0};
	std::vector<int> codes(K, COMPVHIP_OK);
	std::vector<std::string> errs(K);
	std::vector<size_t> badGroup(K, 0);
	std::atomic<int> overflowAny{0};
	while (p->khtWork.size() < T) p->khtWork.emplace_back(new KhtPeaksWork());
	KhtPool pool(T);   // the workers of this call, shared by every group in flight
	auto controller = [&](size_t c) {
		try {
			for (;;) {
				const size_t g = nextGroup.fetch_add(1);
				if (g >= nGroups) break;
				const size_t g0 = g * group, G = std::min<size_t>(group, F - g0);
				KhtRun r{ ctx, *p->khtBatch[c], &pool, G, W, H, k, ax, lines ? lines + g0 * cap : nullptr, cap, counts + g0, gs ? gs + g0 : nullptr, &p->khtWork };
				int rc = khtBegin(r);
				if (!rc) rc = khtFetchPlanes(r, d_edges + g0 * S * H, S);
				if (!rc) rc = khtStages(r, false);
				if (r.overflow) overflowAny.store(1);
				if (rc) { codes[c] = rc; errs[c] = r.err; badGroup[c] = g0; nextGroup.store(nGroups); break; }   // the other controllers finish the group they are in and stop
			}
		}
		catch (const std::exception& ex) { codes[c] = COMPVHIP_E_OUT_OF_MEMORY; errs[c] = std::string("exception in the batched KHT: ") + ex.what(); }   // nothing may leave a thread
		catch (...) { codes[c] = COMPVHIP_E_OUT_OF_MEMORY; errs[c] = "exception in the batched KHT"; }                                                   // (or an extern "C" entry point) as an exception
	};
	{
		std::vector<std::thread> ctl;
		try { for (size_t c = 1; c < K; ++c) ctl.emplace_back(controller, c); }
		catch (...) { /* the system refused a thread: the controllers that did start take all the groups */ }
		controller(0);
		for (std::thread& t : ctl) t.join();
	}
	p->khtWallMs = msSince(wall0);
	p->khtThreads = static_cast<int>(T);
	memset(p->khtStageMs, 0, sizeof(p->khtStageMs));
	for (size_t c = 0; c < K; ++c) for (int i = 0; i < 6; ++i) p->khtStageMs[i] += p->khtBatch[c]->stageMs[i];
	for (size_t c = 0; c < K; ++c)
		if (codes[c]) return fail(ctx, codes[c], ("frames from " + std::to_string(badGroup[c]) + ": " + errs[c]).c_str());
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
	return khtPlanEntry(p, d_edges, khtOpts(rho, thetaDeg, threshold, maxLines, clusterMinDeviation, clusterMinSize, kernelMinHeight, hostThreads), lines, cap, counts, gs);
}

int compvhip_plan_houghkht_ex(compvhip_plan* p, const uint8_t* d_edges, const compvhip_kht_opts* opts, compvhip_line* lines, size_t cap, size_t* counts, double* gs)
{
	if (!p) return COMPVHIP_E_INVALID_PARAMETER;
	compvhip_kht_opts k;
	if (!opts || !khtResolveOpts(opts, k)) return fail(p->ctx, COMPVHIP_E_INVALID_PARAMETER, "null options or unknown KHT order");
	return khtPlanEntry(p, d_edges, k, lines, cap, counts, gs);
}

int compvhip_plan_houghkht_stage_ms(compvhip_plan* p, double* ms6, double* wallMs, int* threads)
{
	if (!p || !ms6) return COMPVHIP_E_INVALID_PARAMETER;
	memcpy(ms6, p->khtStageMs, sizeof(p->khtStageMs));
	if (wallMs) *wallMs = p->khtWallMs;
	if (threads) *threads = p->khtThreads;
	return COMPVHIP_OK;
}
