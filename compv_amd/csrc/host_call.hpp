// host_call.hpp -- the frame of a call that stages the CALLER's host memory (the `*_u8`, `*_host` and `*_f64` entry points of api*.cpp).  Such a call returns
// only when no copy from or to the caller's memory is still in flight, on failure as on success: the frame is a local of the call, every copy goes through
// it, and its destructor waits for the stream on whichever path the scope is left.  The first failure sticks: the steps behind it are skipped, and the frame
// keeps its error and the name of the step.  Declare it BEHIND the call's own DevBuf locals, temporary handles and the stack variables a copy reads or
// writes, so that it drains before they go.  Depends on the HIP runtime alone: tests/host/host_call_check.cpp runs it without the rest of the library.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

namespace compvhip_api {
class HostCall {
public:
	explicit HostCall(hipStream_t stream) : st(stream) {}
	HostCall(const HostCall&) = delete; HostCall& operator=(const HostCall&) = delete;
	~HostCall() { if (pending) (void)hipStreamSynchronize(st); }
	bool ok() const { return err == hipSuccess; }
	hipError_t error() const { return err; }
	const char* what() const { return name; }          // the step that failed (nullptr while ok)
	// The result of a step that copies nothing of the caller's: a reserve, a launch.  (Its argument has been evaluated by the time this runs: a call site
	// that must not run behind a failure asks ok() first, as HOSTSTEP of api_internal.hpp does.)
	bool step(hipError_t e, const char* what) { if (ok() && e != hipSuccess) { err = e; name = what; } return ok(); }
	// asynchronous copies between the caller's memory and the device on the frame's stream, 1-D, or pitched with `rows` rows of `bytes` bytes
	bool upload(void* dst, const void* src, size_t bytes, const char* what = "upload") { return enqueue() && step(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st), what); }
	bool download(void* dst, const void* src, size_t bytes, const char* what = "download") { return enqueue() && step(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st), what); }
	bool upload2D(void* dst, size_t dstPitch, const void* src, size_t srcPitch, size_t bytes, size_t rows, const char* what = "upload") { return enqueue() && step(hipMemcpy2DAsync(dst, dstPitch, src, srcPitch, bytes, rows, hipMemcpyHostToDevice, st), what); }
	bool download2D(void* dst, size_t dstPitch, const void* src, size_t srcPitch, size_t bytes, size_t rows, const char* what = "download") { return enqueue() && step(hipMemcpy2DAsync(dst, dstPitch, src, srcPitch, bytes, rows, hipMemcpyDeviceToHost, st), what); }
	// blocking device-to-host copies, complete on return: for records whose number a wait() has just made known
	bool downloadNow(void* dst, const void* src, size_t bytes, const char* what = "download") { return ok() && step(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost), what); }
	bool downloadNow2D(void* dst, size_t dstPitch, const void* src, size_t srcPitch, size_t bytes, size_t rows, const char* what = "download") { return ok() && step(hipMemcpy2D(dst, dstPitch, src, srcPitch, bytes, rows, hipMemcpyDeviceToHost), what); }
	// Waits for the stream now: a result is needed mid-call, a stack variable was the source of a copy, or the staging is used again.  Behind a failure it
	// still drains what the frame enqueued, and does nothing when there is nothing to drain.
	bool wait() { if (!ok() && !pending) return false; pending = false; return step(hipStreamSynchronize(st), "hipStreamSynchronize"); }

private:
	// a copy is about to be enqueued; a failed enqueue counts as pending too (a pitched copy from pageable memory may have started)
	bool enqueue() { if (ok()) pending = true; return ok(); }
	hipStream_t st; hipError_t err = hipSuccess; const char* name = nullptr;
	bool pending = false;          // something was enqueued through the frame since the last wait()
};
} // namespace compvhip_api
