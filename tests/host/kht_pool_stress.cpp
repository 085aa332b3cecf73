// Stand-alone stress of KhtPool (compv_amd/csrc/kht_pool.hpp), built with -fsanitize=thread and with -fsanitize=address,undefined by
// tests/test_kht_pool_host.py.  Pools asked for 0, 1, 3 and 8 workers; four controller threads per pool, each posting 50 jobs of
// 37..40 items under the stage tags L, K, S, P ('K': the posting controller works along).  Every item must run exactly once, and run() may only
// return when all of its items have returned.  Any violation: exit status 1.
#include "../../compv_amd/csrc/kht_pool.hpp"

#include <cstdio>

namespace {
constexpr int kControllers = 4, kRuns = 50;
const char kTags[4] = { 'L', 'K', 'S', 'P' };

// workers: threads asked for.  The constructor starts max(1, workers) of them, so a request of 0 runs on one worker; run() works itself only in a pool whose
// every thread the system refused, which this program cannot bring about.
bool stress(size_t workers)
{
	KhtPool pool(workers);
	std::atomic<long> total{0};
	std::atomic<bool> ok{true};
	long expected[kControllers] = {};
	auto controller = [&](int c) {
		for (int r = 0; r < kRuns; ++r) {
			const size_t n = 37 + static_cast<size_t>((c + r) % 4);
			std::vector<int> slots(n, 0);   // slot i is written by item i alone; read after run() has returned
			pool.run(n, [&](size_t i) { ++slots[i]; total.fetch_add(1, std::memory_order_relaxed); }, kTags[(c + r) % 4]);
			for (size_t i = 0; i < n; ++i)
				if (slots[i] != 1) { fprintf(stderr, "workers %zu controller %d run %d: item %zu ran %d times\n", workers, c, r, i, slots[i]); ok = false; }
			expected[c] += static_cast<long>(n);
		}
		bool ran = false;
		pool.run(0, [&](size_t) { ran = true; }, 'L');   // nothing to do: returns at once
		if (ran) { fprintf(stderr, "workers %zu: run(0) called an item\n", workers); ok = false; }
	};
	std::vector<std::thread> ctl;
	for (int c = 1; c < kControllers; ++c) ctl.emplace_back(controller, c);
	controller(0);
	for (std::thread& t : ctl) t.join();
	long want = 0;
	for (long e : expected) want += e;
	if (total.load() != want) { fprintf(stderr, "workers %zu: %ld items ran, %ld were posted\n", workers, total.load(), want); ok = false; }
	return ok;
}
} // namespace

int main()
{
	bool ok = true;
	for (size_t workers : { size_t(0), size_t(1), size_t(3), size_t(8) }) ok = stress(workers) && ok;
	if (!ok) return 1;
	puts("kht_pool_stress OK");
	return 0;
}
