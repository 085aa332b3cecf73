// kht_group.hpp -- the table arithmetic of a GROUP of KHT frames (api_kht.cpp): where the strings, cluster slots and vote parameters of every frame sit
// in the group's shared arrays, as the by-value tables of the batched launches (kht.hpp) say it.  The host entry point is a group of one frame.
// kht.hpp and the standard library only, no HIP call: tests/host/kht_group_check.cpp runs it without a GPU.
#pragma once
#include "kht.hpp"

namespace compvhip {

// the part of a frame's host state the tables are made from, and what they assign to the frame
struct KhtFrameLayout {
	std::vector<KhtRange> strings; size_t ptsOff = 0;   // the linker's strings (ranges of the frame's own points); where its points start in the group's arena
	size_t slotBase = 0, slots = 0;                     // khtStringTables: the frame's cluster slots in the group's arrays
	uint32_t nClusters = 0;
	std::vector<KhtVoteParams> params; double GS = 1.0;
	size_t paramsBase = 0;                              // khtVoteTable
};

// the reference's AVX (4) / SSE2 (2) kernel-height loops take n & ~(pack - 1) clusters of a frame; the rest go through the C code (other operation order)
inline int khtSimdEnd(size_t n)
{
	const size_t pack = n >= 4 ? 4 : (n >= 2 ? 2 : 1);
	return static_cast<int>(pack > 1 ? (n & ~(pack - 1)) : 0);
}

// Subdivision: the descriptors of all strings, frame after frame (descs: room for every frame's strings), the strings' table, every frame's slotBase / slots
// and the slot total.  false: the total does not fit the tables' 32 bits (nothing may be launched).
template <class Frame>
bool khtStringTables(Frame* frames, size_t G, size_t minSize, KhtStringDesc* descs, KhtBatchStrings& tab, size_t& slots)
{
	tab = KhtBatchStrings{};
	tab.frames = static_cast<int>(G);
	size_t si = 0;
	slots = 0;
	for (size_t f = 0; f < G; ++f) {
		Frame& fr = frames[f];
		tab.stringBegin[f] = static_cast<uint32_t>(si); tab.clusterBase[f] = static_cast<uint32_t>(slots);
		fr.slotBase = slots;
		for (const KhtRange& r : fr.strings) {
			KhtStringDesc& d = descs[si++];
			d.begin = static_cast<uint32_t>(fr.ptsOff + r.begin); d.end = static_cast<uint32_t>(fr.ptsOff + r.end); d.slot = static_cast<uint32_t>(slots);
			slots += khtSubdivSlots(r.end - r.begin, minSize);
		}
		fr.slots = slots - fr.slotBase;
	}
	for (size_t f = G; f <= static_cast<size_t>(kKhtBatch); ++f) tab.stringBegin[f] = static_cast<uint32_t>(si);
	return slots <= 0xffffffffull;
}

// Statistics: every frame's clusters (nClusters of them from slotBase).  false: no frame has any.
template <class Frame>
bool khtStatsTable(const Frame* frames, size_t G, KhtBatchStats& tab)
{
	tab = KhtBatchStats{};
	tab.frames = static_cast<int>(G);
	bool any = false;
	for (size_t f = 0; f < G; ++f) {
		const Frame& fr = frames[f];
		tab.clusterBase[f] = static_cast<uint32_t>(fr.slotBase); tab.n[f] = static_cast<int>(fr.nClusters); tab.simdEnd[f] = khtSimdEnd(fr.nClusters);
		any = any || fr.nClusters;
	}
	return any;
}

// Voting: every frame's paramsBase and the table; returns the number of vote parameters of the group
template <class Frame>
size_t khtVoteTable(Frame* frames, size_t G, size_t mapElems, size_t cellCap, KhtBatchVote& tab)
{
	tab = KhtBatchVote{};
	tab.frames = static_cast<int>(G); tab.mapElems = mapElems; tab.cellCap = cellCap;
	size_t n = 0;
	for (size_t f = 0; f < G; ++f) {
		Frame& fr = frames[f];
		fr.paramsBase = n; n += fr.params.size();
		tab.paramsBase[f] = static_cast<uint32_t>(fr.paramsBase); tab.nKernels[f] = static_cast<int>(fr.params.size()); tab.gs[f] = fr.GS;
	}
	return n;
}

} // namespace compvhip
