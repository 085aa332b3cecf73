// step_policy.hpp -- the decisions around an asynchronous step (compvhip_plan_pipeline_async / compvhip_plan_wait) as plain functions of plain values: what the
// plan remembers of its last steps, the sort range and the speculative rounds it predicts from that, and what a waited step's results mean.  No HIP header,
// no plan: api.cpp feeds them, tests/host/step_policy_check.cpp runs them on any machine.
#pragma once
#include <algorithm>
#include <cstddef>

namespace compvhip_api {

constexpr int kSpecRounds = 3;         // rounds enqueued speculatively between two convergence checks

// the last 8 values seen
struct Recent8 {
	unsigned int v[8] = {}; int n = 0;
	void push(unsigned int x)
	{
		v[n++ & 7] = x;
		if (n >= 16) n -= 8;   // the ring index keeps counting, "entries seen" saturates at 8
	}
	int seen() const { return std::min(n, 8); }
	unsigned int max() const   // over what has been seen (0: nothing)
	{
		unsigned int m = 0;
		for (int i = 0; i < seen(); ++i) m = std::max(m, v[i]);
		return m;
	}
	void reset() { n = 0; }
};

// Key slots the line sort of an asynchronous step covers, which cannot read the step's total before it enqueues the sort: the largest total of the plan's recent
// steps + 1/16 + 4096 slots (nothing seen yet, or just reset: everything), at most the capacity (lineCap * frames)
inline size_t asyncSortRange(const Recent8& totals, size_t capAll)
{
	if (!totals.seen()) return capAll;
	const unsigned int m = totals.max();
	return std::min(static_cast<size_t>(m) + (m >> 4) + 4096, capAll);
}

struct StepVerdict {
	int needed;    // hysteresis rounds the step needed = the first round that changed nothing, inclusive (more than were enqueued: one more than that, at least)
	bool sorted;   // the predicted range covered every line of the step
	bool replay;   // the step has to run again, synchronously
};

// rounds: speculative rounds the step enqueued; flags: its first four round flags (0 = the round changed nothing); total: its key slots in use; sortN: the
// range its sort covered; replayMark: an earlier step of the plan was replayed after this one ran.  A step is good when its last speculative round reached
// the fixed point and the sort covered its lines -- anything else, a slot nobody wrote included (total ~0u, flags 1: runStepAsync), is a replay.
inline StepVerdict stepVerdict(int rounds, const int flags[4], unsigned int total, size_t sortN, bool replayMark)
{
	StepVerdict v;
	const int looked = std::min(rounds, 4);
	v.needed = looked + 1;
	for (int i = 0; i < looked; ++i) if (flags[i] == 0) { v.needed = i + 1; break; }
	v.sorted = static_cast<size_t>(total) <= sortN;
	const int lastFlag = flags[std::max(0, looked - 1)];   // the flag of the step's last speculative round
	v.replay = !(lastFlag == 0 && v.sorted && !replayMark);
	return v;
}

// speculative rounds of the next step, from what the recent ones needed: a few steps first, then as many as they needed (at least 2, at most kSpecRounds)
inline int nextSpecRounds(const Recent8& rounds)
{
	if (rounds.seen() < 4) return kSpecRounds;
	return std::min(std::max<int>(2, static_cast<int>(rounds.max())), kSpecRounds);
}

} // namespace compvhip_api
