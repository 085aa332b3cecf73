// host_call_check.cpp -- HostCall (compv_amd/csrc/host_call.hpp), the frame of the calls that stage the caller's host memory, on a runtime of this program's
// own: the five runtime functions the header calls are DEFINED here (a definition in the executable takes precedence over the shared library's), record what
// they were asked and answer from a script.  On a machine without a GPU the real ones only ever fail, which cannot show a drain; on one with a GPU no test may
// provoke a failure.  Shown: the order and number of the operations and synchronisations on the success path, a failure scripted at every step in turn, a
// failure before anything was enqueued, a failing wait(), and the drain behind an early return.  Built for the host with AddressSanitizer and UBSan by
// tests/test_host_call_host.py.
#include "../../compv_amd/csrc/host_call.hpp"

#include <cstdio>
#include <string>
#include <type_traits>
#include <vector>

using compvhip_api::HostCall;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

static_assert(!std::is_copy_constructible<HostCall>::value && !std::is_copy_assignable<HostCall>::value, "a frame is not copied");

// ---- the scripted runtime ----
static std::vector<std::string> calls;          // what the runtime was asked, in order
static int failAt = -1;                         // the runtime call (index into `calls`) that fails ...
static hipError_t failWith = hipSuccess;        // ... and with what
static hipStream_t const kStream = reinterpret_cast<hipStream_t>(0x5eed);

static hipError_t record(const char* op, hipStream_t st, bool onStream)
{
	if (onStream && st != kStream) { std::printf("FAILED: %s on a stream that is not the frame's\n", op); ++failures; }
	calls.push_back(op);
	return static_cast<int>(calls.size()) - 1 == failAt ? failWith : hipSuccess;
}
static const char* kindName(hipMemcpyKind k, const char* h2d, const char* d2h) { return k == hipMemcpyHostToDevice ? h2d : k == hipMemcpyDeviceToHost ? d2h : "copy of an unexpected kind"; }

extern "C" {
hipError_t hipMemcpyAsync(void*, const void*, size_t, hipMemcpyKind kind, hipStream_t st) { return record(kindName(kind, "h2d", "d2h"), st, true); }
hipError_t hipMemcpy2DAsync(void*, size_t, const void*, size_t, size_t, size_t, hipMemcpyKind kind, hipStream_t st) { return record(kindName(kind, "h2d2D", "d2h2D"), st, true); }
hipError_t hipMemcpy(void*, const void*, size_t, hipMemcpyKind kind) { return record(kindName(kind, "blocking h2d", "d2hNow"), nullptr, false); }
hipError_t hipMemcpy2D(void*, size_t, const void*, size_t, size_t, size_t, hipMemcpyKind kind) { return record(kindName(kind, "blocking h2d2D", "d2hNow2D"), nullptr, false); }
hipError_t hipStreamSynchronize(hipStream_t st) { return record("sync", st, true); }
}

static void script(int at = -1, hipError_t with = hipSuccess) { calls.clear(); failAt = at; failWith = with; }
static int count(const char* op) { int n = 0; for (const auto& c : calls) n += c == op; return n; }
static std::string joined() { std::string s; for (const auto& c : calls) { if (!s.empty()) s += ' '; s += c; } return s; }

// a reserve or a launch: not a runtime call of the header's, so it is recorded here; fails when this step is the scripted one
static int stepFail = -1;                       // the frame step (index into kSteps) whose reserve / launch fails
static hipError_t other(const char* op, int index) { calls.push_back(op); return index == stepFail ? hipErrorInvalidValue : hipSuccess; }
// what the library's HOSTSTEP does: the call is not made behind a failure
#define STEP(hc, call, what) do { if ((hc).ok()) (hc).step((call), what); } while (0)

// The sequence of a host form: a plane up, a reserve, a list up, a launch, a plane and a record down -- six steps, then what follows a wait.
static char host[64], dev[64];
struct Step { const char* op; const char* what; bool runtime; };
static const Step kSteps[] = { { "h2d2D", "plane upload", true }, { "reserve", "reserve", false }, { "h2d", "list upload", true }, { "launch", "launch", false },
	                           { "d2h2D", "plane download", true }, { "d2h", "record download", true } };
constexpr int kStepCount = sizeof(kSteps) / sizeof(kSteps[0]);

static void enqueueAll(HostCall& hc)
{
	hc.upload2D(dev, 16, host, 32, 8, 2, kSteps[0].what);
	STEP(hc, other("reserve", 1), kSteps[1].what);
	hc.upload(dev, host, 16, kSteps[2].what);
	STEP(hc, other("launch", 3), kSteps[3].what);
	hc.download2D(host, 32, dev, 16, 8, 2, kSteps[4].what);
	hc.download(host, dev, 16, kSteps[5].what);
}

// leaves in the middle of the sequence, as a call does whose plan-level call refused
static int leavesEarly(bool early)
{
	HostCall hc(kStream);
	hc.upload2D(dev, 16, host, 32, 8, 2);
	if (early) return 7;
	hc.download(host, dev, 16);
	return hc.wait() ? 0 : 1;
}

int main()
{
	// 1. every step succeeds: each operation once, in order, one synchronisation at wait(), the blocking copies behind it, none added by the destructor
	script();
	{
		HostCall hc(kStream);
		enqueueAll(hc);
		CHECK(hc.ok() && hc.what() == nullptr && hc.error() == hipSuccess);
		CHECK(hc.wait());
		CHECK(hc.downloadNow(host, dev, 16) && hc.downloadNow2D(host, 32, dev, 16, 8, 2));
		CHECK(hc.ok());
	}
	CHECK(joined() == "h2d2D reserve h2d launch d2h2D d2h sync d2hNow d2hNow2D");

	// 2. a failure scripted at each step in turn: nothing behind it is issued (the wait, the blocking copies and a later step included), the status is that
	// step's error and name, and leaving the scope synchronises exactly once -- the first step is a copy, so something was enqueued every time
	for (int k = 0; k < kStepCount; ++k) {
		script(kSteps[k].runtime ? k : -1, hipErrorLaunchFailure);   // (every step records one call: step k is call k)
		stepFail = kSteps[k].runtime ? -1 : k;
		const hipError_t expected = kSteps[k].runtime ? hipErrorLaunchFailure : hipErrorInvalidValue;
		{
			HostCall hc(kStream);
			enqueueAll(hc);
			CHECK(!hc.ok() && hc.error() == expected && std::string(hc.what()) == kSteps[k].what);
			CHECK(!hc.downloadNow(host, dev, 16) && !hc.upload(dev, host, 16) && !hc.step(hipErrorOutOfMemory, "later"));
			CHECK(hc.error() == expected && std::string(hc.what()) == kSteps[k].what);          // the FIRST failure is kept
			CHECK(static_cast<int>(calls.size()) == k + 1 && calls.back() == kSteps[k].op);     // steps 0 .. k were issued, nothing else
			CHECK(count("sync") == 0);
		}
		CHECK(static_cast<int>(calls.size()) == k + 2 && calls.back() == std::string("sync"));
		stepFail = -1;
	}

	// 3. a failure before anything was enqueued (the reserve in front of the first copy): no synchronisation at all, by wait() or by the destructor
	script();
	{
		HostCall hc(kStream);
		CHECK(!hc.step(hipErrorOutOfMemory, "reserve") && hc.error() == hipErrorOutOfMemory && std::string(hc.what()) == "reserve");
		enqueueAll(hc);
		CHECK(!hc.wait());
	}
	CHECK(calls.empty());

	// 4. a failing wait(): reported with its name, and not repeated by the destructor
	script(1, hipErrorIllegalAddress);
	{
		HostCall hc(kStream);
		CHECK(hc.upload(dev, host, 16));
		CHECK(!hc.wait() && hc.error() == hipErrorIllegalAddress && std::string(hc.what()) == "hipStreamSynchronize");
		CHECK(!hc.wait());                       // nothing pending behind a failure: nothing to drain
	}
	CHECK(joined() == "h2d sync");

	// 5. wait() behind a failed copy still drains what was enqueued (a stack variable may be its source), once; the copy's error stays
	script(1, hipErrorInvalidValue);
	{
		HostCall hc(kStream);
		CHECK(hc.upload(dev, host, 16) && !hc.download(host, dev, 16, "count"));
		CHECK(!hc.wait() && hc.error() == hipErrorInvalidValue && std::string(hc.what()) == "count");
	}
	CHECK(joined() == "h2d d2h sync");

	// 6. an early return in the middle of a sequence drains; the whole sequence synchronises once, at its wait()
	script();
	CHECK(leavesEarly(true) == 7 && joined() == "h2d2D sync");
	script();
	CHECK(leavesEarly(false) == 0 && joined() == "h2d2D d2h sync");

	// 7. slices: a wait() per slice, copies behind the last wait() are drained by the destructor, a frame that enqueued nothing synchronises nothing
	script();
	{
		HostCall hc(kStream);
		for (int slice = 0; slice < 2; ++slice) { hc.upload(dev, host, 16); hc.download(host, dev, 16); CHECK(hc.wait()); }
		hc.download(host, dev, 16);
	}
	CHECK(joined() == "h2d d2h sync h2d d2h sync d2h sync");
	script();
	{
		HostCall hc(kStream);
		CHECK(hc.step(hipSuccess, "reserve"));
	}
	CHECK(calls.empty());

	if (failures) return 1;
	std::printf("host_call_check OK\n");
	return 0;
}
