// kht_pool.hpp -- the host work pool of compvhip_plan_houghkht (api_kht.cpp).  Standard library only: tests/host/kht_pool_stress.cpp runs it under the
// thread and address sanitizers without a GPU.
#pragma once
#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <deque>
#include <functional>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>

// The host workers of ONE compvhip_plan_houghkht call, shared by the controllers of all groups in flight: run(n, fn) queues fn(0) .. fn(n - 1) and blocks until
// every item has returned; the workers take items from the OLDEST job that still has some, so while one group waits for a GPU stage its controller sleeps
// and the workers link / sweep the frames of the other groups.  (Rounds 4-5 gave every controller a private pool of threads / controllers workers: all
// groups reached their GPU stages together and the workers of a waiting group idled -- 0.46 ms per 4K frame at 16 threads against 0.30 here.)
// The callers do not work along: `threads` workers are what runs, whatever the number of controllers.
inline thread_local int t_khtWorker = -1;   // index of the pool worker running the current item (-1: not a pool worker)
class KhtPool {
	struct Job {
		const std::function<void(size_t)>* fn; size_t n, next = 0;   // next: guarded by the pool's mutex
		std::atomic<size_t> left; char tag;
		Job(const std::function<void(size_t)>* f, size_t count, char t) : fn(f), n(count), left(count), tag(t) {}
	};
	struct Span { int worker; char tag; double t0, t1; };
public:
	explicit KhtPool(size_t threads)
	{
		trace_ = getenv("COMPVHIP_KHT_TRACE") != nullptr;   // lab: one line per item on stderr when the pool goes (worker, stage tag, start, end in ms)
		born_ = std::chrono::steady_clock::now();
		try { for (size_t t = 0; t < std::max<size_t>(1, threads); ++t) pool_.emplace_back([this, t] { t_khtWorker = static_cast<int>(t); loop(); }); }
		catch (...) { /* the system refused another thread: the ones that started share the work (none at all: run() works itself) */ }
	}
	~KhtPool()
	{
		{ std::lock_guard<std::mutex> g(m_); quit_ = true; }
		cv_.notify_all();
		for (std::thread& t : pool_) t.join();
		if (trace_) for (const Span& sp : spans_) fprintf(stderr, "khtpool w%02d %c %8.3f %8.3f\n", sp.worker, sp.tag, sp.t0, sp.t1);
	}
	size_t workers() const { return pool_.size(); }
	void run(size_t n, const std::function<void(size_t)>& fn, char tag = '?')
	{
		if (!n) return;
		if (pool_.empty()) { for (size_t i = 0; i < n; ++i) fn(i); return; }
		std::shared_ptr<Job> job = std::make_shared<Job>(&fn, n, tag);
		{
			// by stage priority (prio()), then by arrival
			std::lock_guard<std::mutex> g(m_);
			auto it = jobs_.begin();
			while (it != jobs_.end() && prio((*it)->tag) >= prio(tag)) ++it;
			jobs_.insert(it, job);
		}
		cv_.notify_all();
		if (tag == 'K') {
			// The prune items are short (0.2 ms) and gate their group's second GPU stage: when they are posted every worker is usually in the middle of a 3 ms
			// link of another group, and the group -- and, 4 ms later, the workers -- would wait for one to come free.  The posting controller works along.
			for (;;) {
				size_t i;
				{
					std::lock_guard<std::mutex> g(m_);
					if (job->next >= job->n) break;
					i = job->next++;
					if (job->next >= job->n) jobs_.erase(std::remove(jobs_.begin(), jobs_.end(), job), jobs_.end());
				}
				fn(i);
				job->left.fetch_sub(1);
			}
		}
		std::unique_lock<std::mutex> lk(m_);
		done_.wait(lk, [&] { return job->left.load() == 0; });   // every item has RETURNED: fn may go out of scope
	}
private:
	// the stage with the longest way to go first: a frame that is not linked yet still needs 3 ms of link + two GPU stages + 2 ms of sweep, a sweep is the end of its frame
	// and fills whatever gap is left (sweeps before links: 17.8 ms per 32 x 4K batch on 16 workers against 14.4)
	static int prio(char tag) { return tag == 'K' ? 3 : (tag == 'L' || tag == 'P') ? 2 : 1; }
	void loop()
	{
		for (;;) {
			std::shared_ptr<Job> job; size_t i = 0;
			{
				std::unique_lock<std::mutex> lk(m_);
				cv_.wait(lk, [&] { return quit_ || !jobs_.empty(); });
				if (jobs_.empty()) return;   // quit_
				job = jobs_.front();
				i = job->next++;
				if (job->next >= job->n) jobs_.pop_front();
			}
			const auto t0 = std::chrono::steady_clock::now();
			(*job->fn)(i);
			if (trace_) {
				const auto t1 = std::chrono::steady_clock::now();
				std::lock_guard<std::mutex> g(m_);
				spans_.push_back({ t_khtWorker, job->tag, std::chrono::duration<double, std::milli>(t0 - born_).count(), std::chrono::duration<double, std::milli>(t1 - born_).count() });
			}
			if (job->left.fetch_sub(1) == 1) { std::lock_guard<std::mutex> g(m_); done_.notify_all(); }
		}
	}
	bool trace_ = false; std::chrono::steady_clock::time_point born_; std::vector<Span> spans_;
	std::vector<std::thread> pool_;
	std::mutex m_; std::condition_variable cv_, done_;
	std::deque<std::shared_ptr<Job>> jobs_;
	bool quit_ = false;
};
