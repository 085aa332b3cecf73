// kht_group_check.cpp -- the table arithmetic of a group of KHT frames (compv_amd/csrc/kht_group.hpp): the strings' descriptors and table, the cluster
// slots, the statistics and the vote tables, for a group of one frame (the host entry points), a group with an empty frame in the middle and a full group of
// kKhtBatch frames.  No HIP call, no GPU.  Built for the host with AddressSanitizer and UBSan by tests/test_kht_group_host.py.
#include "../../compv_amd/csrc/kht_group.hpp"

#include <cstdio>
#include <cstring>
#include <vector>

using namespace compvhip;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

// frames whose strings have the given lengths, laid out as the linker leaves them: a frame's strings one behind the other from its own point 0, the
// frames' points one behind the other in the group's arena
static std::vector<KhtFrameLayout> framesOf(const std::vector<std::vector<size_t>>& lengths)
{
	std::vector<KhtFrameLayout> frames(lengths.size());
	size_t arena = 0;
	for (size_t f = 0; f < lengths.size(); ++f) {
		size_t at = 0;
		for (size_t len : lengths[f]) { frames[f].strings.push_back({ at, at + len }); at += len; }
		frames[f].ptsOff = arena;
		arena += at + f;   // (khtLink may write fewer points than the plane has pixels: gaps between the frames' slices)
	}
	return frames;
}

// every slot of the three tables against sums recomputed here
static void checkGroup(const std::vector<std::vector<size_t>>& lengths, size_t minSize)
{
	const size_t G = lengths.size();
	std::vector<KhtFrameLayout> frames = framesOf(lengths);
	size_t nStrings = 0;
	for (const auto& l : lengths) nStrings += l.size();
	std::vector<KhtStringDesc> descs(nStrings + 1);
	const KhtStringDesc guard = { 0xdeadbeefu, 0xdeadbeefu, 0xdeadbeefu };
	descs[nStrings] = guard;
	KhtBatchStrings tab;
	memset(&tab, 0xff, sizeof(tab));
	size_t slots = ~static_cast<size_t>(0);
	CHECK(khtStringTables(frames.data(), G, minSize, descs.data(), tab, slots));
	CHECK(tab.frames == static_cast<int>(G));
	CHECK(memcmp(&descs[nStrings], &guard, sizeof(guard)) == 0);
	size_t si = 0, sum = 0;
	for (size_t f = 0; f < G; ++f) {
		CHECK(tab.stringBegin[f] == si && tab.clusterBase[f] == sum && frames[f].slotBase == sum);
		if (f) CHECK(tab.stringBegin[f] >= tab.stringBegin[f - 1]);
		size_t own = 0;
		for (size_t i = 0; i < lengths[f].size(); ++i, ++si) {
			const KhtRange& r = frames[f].strings[i];
			CHECK(descs[si].begin == frames[f].ptsOff + r.begin && descs[si].end == frames[f].ptsOff + r.end && descs[si].end - descs[si].begin == lengths[f][i]);
			CHECK(descs[si].slot == sum + own);
			own += khtSubdivSlots(lengths[f][i], minSize);
		}
		CHECK(frames[f].slots == own);
		sum += own;
	}
	CHECK(si == nStrings && slots == sum);
	for (size_t f = G; f <= static_cast<size_t>(kKhtBatch); ++f) CHECK(tab.stringBegin[f] == nStrings);
	for (size_t f = G; f < static_cast<size_t>(kKhtBatch); ++f) CHECK(tab.clusterBase[f] == 0);

	// statistics: as many clusters as the frame index says (0, 1, 2, ... : every branch of simdEnd), the last frame with as many as it has slots
	for (size_t f = 0; f < G; ++f) frames[f].nClusters = static_cast<uint32_t>(std::min(f, frames[f].slots));
	if (frames[G - 1].slots) frames[G - 1].nClusters = static_cast<uint32_t>(frames[G - 1].slots);
	KhtBatchStats st;
	memset(&st, 0xff, sizeof(st));
	const bool any = khtStatsTable(frames.data(), G, st);
	bool want = false;
	CHECK(st.frames == static_cast<int>(G));
	for (size_t f = 0; f < static_cast<size_t>(kKhtBatch); ++f) {
		const size_t n = f < G ? frames[f].nClusters : 0;
		want = want || n;
		CHECK(st.clusterBase[f] == (f < G ? frames[f].slotBase : 0) && st.n[f] == static_cast<int>(n));
		CHECK(st.simdEnd[f] == static_cast<int>(n >= 4 ? (n & ~static_cast<size_t>(3)) : n >= 2 ? (n & ~static_cast<size_t>(1)) : 0));
	}
	CHECK(any == want);

	// voting: f % 3 parameters per frame
	for (size_t f = 0; f < G; ++f) { frames[f].params.assign(f % 3, KhtVoteParams{}); frames[f].GS = 1.0 + static_cast<double>(f); }
	KhtBatchVote vt;
	memset(&vt, 0xff, sizeof(vt));
	const size_t nParams = khtVoteTable(frames.data(), G, 1000, 77, vt);
	CHECK(vt.frames == static_cast<int>(G) && vt.mapElems == 1000 && vt.cellCap == 77);
	size_t run = 0;
	for (size_t f = 0; f < G; ++f) {
		CHECK(vt.paramsBase[f] == run && frames[f].paramsBase == run && vt.nKernels[f] == static_cast<int>(f % 3) && vt.gs[f] == 1.0 + static_cast<double>(f));
		run += f % 3;
	}
	CHECK(nParams == run);
	for (size_t f = G; f < static_cast<size_t>(kKhtBatch); ++f) CHECK(vt.paramsBase[f] == 0 && vt.nKernels[f] == 0);
}

int main()
{
	const size_t minSize = 10;
	CHECK(khtSimdEnd(0) == 0 && khtSimdEnd(1) == 0 && khtSimdEnd(2) == 2 && khtSimdEnd(3) == 2 && khtSimdEnd(4) == 4 && khtSimdEnd(7) == 4 && khtSimdEnd(1001) == 1000);
	checkGroup({ {} }, minSize);                                      // a group of one frame without strings
	checkGroup({ { minSize, minSize + 1, 1000 } }, minSize);           // a group of one frame
	checkGroup({ { 12, 40 }, {}, { 1000, minSize, 33 } }, minSize);   // an empty frame in the middle
	checkGroup({ { minSize, minSize + 1, 1000 } }, 2);                // the smallest legal clusters: the most slots
	{
		std::vector<std::vector<size_t>> full(kKhtBatch);
		for (size_t f = 0; f < full.size(); ++f)
			for (size_t i = 0; i < f % 5; ++i) full[f].push_back(minSize + 7 * f + 131 * i);
		checkGroup(full, minSize);
	}
	{
		// fabricated lengths whose slot total passes 2^32 - 1: refused (a KhtRange is two size_t: no memory behind them)
		std::vector<KhtFrameLayout> frames(2);
		frames[0].strings = { { 0, 0x80000000ull } };
		frames[1].strings = { { 0, 0x80000000ull }, { 0x80000000ull, 0x80000010ull } };
		KhtStringDesc descs[3];
		KhtBatchStrings tab;
		size_t slots = 0;
		CHECK(!khtStringTables(frames.data(), 2, 2, descs, tab, slots));
		CHECK(slots > 0xffffffffull);
		frames[1].strings = { { 0, 0x7ffffff0ull } };                 // just below: accepted
		CHECK(khtStringTables(frames.data(), 2, 2, descs, tab, slots) && slots <= 0xffffffffull);
	}
	if (failures) { std::printf("kht_group_check: %d check(s) failed\n", failures); return 1; }
	std::printf("kht_group_check OK\n");
	return 0;
}
