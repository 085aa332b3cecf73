// step_policy_check.cpp -- the decisions around an asynchronous pipeline step (compv_amd/csrc/step_policy.hpp): the ring of recent values, the predicted sort
// range, the verdict of a waited step and the next step's speculative rounds.  Every expected value follows from the rules as the header states them.
// A program of its own: standard library only, no GPU.  Prints "step_policy_check OK" and returns 0 when every check holds.
#include "../../compv_amd/csrc/step_policy.hpp"

#include <algorithm>
#include <cstdio>
#include <initializer_list>
#include <vector>

using namespace compvhip_api;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

static const size_t kCap = 32u * 65536u;   // lineCap * frames of the benchmark's plan

static Recent8 ringOf(std::initializer_list<unsigned int> values)
{
	Recent8 r;
	for (unsigned int x : values) r.push(x);
	return r;
}

static StepVerdict verdict(int rounds, std::initializer_list<int> flags, unsigned int total, size_t sortN, bool mark)
{
	int f[4] = { 0, 0, 0, 0 };
	std::copy(flags.begin(), flags.end(), f);
	return stepVerdict(rounds, f, total, sortN, mark);
}

int main()
{
	// ---- the ring and the sort range ----
	{
		Recent8 r;
		CHECK(r.seen() == 0 && r.max() == 0);
		CHECK(asyncSortRange(r, kCap) == kCap);                    // nothing seen: everything
		r.push(1000);
		CHECK(r.seen() == 1 && r.max() == 1000);
		CHECK(asyncSortRange(r, kCap) == 5158);                    // 1000 + 1000 / 16 + 4096
		CHECK(asyncSortRange(r, 4000) == 4000);                    // clamped to the capacity
		r.reset();
		CHECK(r.seen() == 0 && asyncSortRange(r, kCap) == kCap);   // after a reset: everything again
	}
	{
		Recent8 r = ringOf({ 100000 });
		CHECK(asyncSortRange(r, kCap) == 100000 + 6250 + 4096);
		for (int i = 0; i < 7; ++i) r.push(10);
		CHECK(r.seen() == 8 && r.max() == 100000);                 // still among the last 8
		r.push(10);
		CHECK(r.seen() == 8 && r.max() == 10);                     // the ninth push overwrote it
		CHECK(asyncSortRange(r, kCap) == 4106);
	}
	{
		// 40 pushes: after every one, the maximum is that of the last 8 values and the count has saturated at 8
		Recent8 r;
		std::vector<unsigned int> all;
		for (unsigned int i = 0; i < 40; ++i) {
			const unsigned int x = (i * 7919u) % 1000u + (i == 13 ? 50000u : 0u);
			r.push(x); all.push_back(x);
			const size_t n = std::min<size_t>(all.size(), 8);
			CHECK(r.seen() == static_cast<int>(n));
			CHECK(r.max() == *std::max_element(all.end() - static_cast<long>(n), all.end()));
			CHECK(asyncSortRange(r, kCap) == static_cast<size_t>(r.max()) + (r.max() >> 4) + 4096);
		}
		Recent8 last8;
		for (size_t i = all.size() - 8; i < all.size(); ++i) last8.push(all[i]);
		CHECK(asyncSortRange(r, kCap) == asyncSortRange(last8, kCap));
	}
	CHECK(asyncSortRange(ringOf({ 0xffffffffu }), kCap) == kCap);   // no 32-bit wrap in max + max / 16 + 4096

	// ---- the verdict of a waited step ----
	{
		StepVerdict v = verdict(3, { 1, 1, 0 }, 500, 5158, false);
		CHECK(v.needed == 3 && v.sorted && !v.replay);
		v = verdict(3, { 1, 0, 0 }, 500, 5158, false);
		CHECK(v.needed == 2 && v.sorted && !v.replay);
		v = verdict(2, { 1, 1 }, 500, 5158, false);
		CHECK(v.needed == 3 && v.sorted && v.replay);              // the last enqueued round still changed something
		v = verdict(3, { 1, 1, 1, 0 }, 500, 5158, false);
		CHECK(v.needed == 4 && v.replay);                          // flags[3] belongs to a round that was not enqueued
		v = verdict(3, { 1, 1, 0 }, 5159, 5158, false);
		CHECK(v.needed == 3 && !v.sorted && v.replay);             // more lines than the sort covered
		v = verdict(3, { 1, 1, 0 }, 5158, 5158, false);
		CHECK(v.sorted && !v.replay);                              // exactly covered
		v = verdict(3, { 1, 1, 0 }, 500, 5158, true);
		CHECK(v.needed == 3 && v.sorted && v.replay);              // an earlier step was replayed over this one's outputs
		v = verdict(0, { 0, 1, 1, 1 }, 500, 5158, false);
		CHECK(v.needed == 1 && !v.replay);                         // no rounds enqueued: flags[0] decides
		v = verdict(0, { 1, 0, 0, 0 }, 500, 5158, false);
		CHECK(v.needed == 1 && v.replay);
		v = verdict(7, { 1, 1, 1, 0 }, 500, 5158, false);
		CHECK(v.needed == 4 && !v.replay);                         // only four flags are reported: the fourth stands for the last round
		v = verdict(4, { 1, 1, 1, 1 }, 500, 5158, false);
		CHECK(v.needed == 5 && v.replay);
		// the slot as runStepAsync resets it (total ~0u, flags 1), for every number of rounds and even when the sort covered the whole capacity
		for (int rounds = 0; rounds <= 4; ++rounds) {
			v = verdict(rounds, { 1, 1, 1, 1 }, ~0u, kCap, false);
			CHECK(!v.sorted && v.replay && v.needed == rounds + 1);
		}
	}

	// ---- the next step's speculative rounds ----
	CHECK(nextSpecRounds(Recent8()) == kSpecRounds);
	CHECK(nextSpecRounds(ringOf({ 1, 1, 1 })) == kSpecRounds);      // fewer than 4 entries
	CHECK(nextSpecRounds(ringOf({ 1, 1, 1, 1 })) == 2);             // at least 2
	CHECK(nextSpecRounds(ringOf({ 1, 1, 1, 3 })) == 3);
	CHECK(nextSpecRounds(ringOf({ 2, 2, 2, 2 })) == 2);
	CHECK(nextSpecRounds(ringOf({ 1, 5, 1, 1 })) == 3);             // at most kSpecRounds
	CHECK(nextSpecRounds(ringOf({ 3, 1, 1, 1, 1, 1, 1, 1 })) == 3);
	CHECK(nextSpecRounds(ringOf({ 3, 1, 1, 1, 1, 1, 1, 1, 1 })) == 2);   // the 3 is forgotten after 8 more steps

	if (failures) { std::printf("step_policy_check: %d failure(s)\n", failures); return 1; }
	std::printf("step_policy_check OK\n");
	return 0;
}
