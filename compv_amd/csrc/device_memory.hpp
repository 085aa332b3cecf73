// device_memory.hpp -- the buffers that own the device and pinned host memory of the C ABI's host side (api*.cpp).  A handle's members are DevBuf / PinBuf
// (they free themselves when the handle is deleted) or raw pointers that VIEW one of them.  Depends on the HIP runtime alone: tests/host/device_memory_check.cpp
// runs it without the rest of the library.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstring>

namespace compvhip_api {
using LiveCount = std::atomic<long>;   // hipMalloc / hipFree balance of a context (compvhip_live_allocations)

// compvhip_debug_alloc_fill (test hook, process-wide): -1 = off; 0 .. 255 = every block dmalloc or PinBuf::reserve has just ALLOCATED is filled with that
// byte before anyone sees it.  A buffer that is reused (cap >= n) is not touched.  Off, it costs one relaxed load per allocation; no launch path reads it.
inline std::atomic<int> allocFill{-1};

// the device fill is complete when this returns: the plans run on non-blocking streams, which do not order against the null stream, and what a plain
// hipMemset waits for is the runtime's business -- so the device is waited for
inline hipError_t fillFresh(void* p, size_t bytes, int byte)
{
	const hipError_t e = hipMemset(p, byte, bytes);
	return e != hipSuccess ? e : hipDeviceSynchronize();
}

template <typename T>
hipError_t dmalloc(LiveCount* live, T** p, size_t count)
{
	*p = nullptr;
	if (!count) return hipSuccess;
	hipError_t e = hipMalloc(reinterpret_cast<void**>(p), count * sizeof(T));
	if (e != hipSuccess) { *p = nullptr; return e; }
	const int fill = allocFill.load(std::memory_order_relaxed);
	if (fill >= 0 && (e = fillFresh(*p, count * sizeof(T), fill)) != hipSuccess) { (void)hipFree(*p); *p = nullptr; return e; }   // never counted
	if (live) ++*live;
	return e;
}
template <typename T>
void dfree(LiveCount* live, T*& p)
{
	if (p) { (void)hipFree(p); if (live) --*live; p = nullptr; }
}

// Growable device memory: a pointer and its capacity in elements, one hipMalloc through dmalloc / dfree, counted once in owner->live -- the owner is the
// context (or whatever has a LiveCount member of that name), remembered from the first allocation on, so that release and the destructor take no argument.
// (reserve / grow name the owner, not the counter, so that a call site reads -- and a failed HIPCHK reports -- `buf.reserve(ctx, n)` as it always has;
// a null owner counts nowhere, as a null context did for dmalloc.)  A request that fits reuses the buffer; after a failed allocation it is {nullptr, 0}, so a later, smaller request allocates again instead of trusting a
// stale capacity.  Move-only; a moved-from buffer is empty.
template <typename T>
struct DevBuf {
	T* ptr = nullptr; size_t cap = 0; LiveCount* live = nullptr;
	DevBuf() = default;
	DevBuf(const DevBuf&) = delete;
	DevBuf& operator=(const DevBuf&) = delete;
	DevBuf(DevBuf&& o) noexcept : ptr(o.ptr), cap(o.cap), live(o.live) { o.ptr = nullptr; o.cap = 0; }
	DevBuf& operator=(DevBuf&& o) noexcept
	{
		if (this != &o) { release(); ptr = o.ptr; cap = o.cap; live = o.live; o.ptr = nullptr; o.cap = 0; }
		return *this;
	}
	~DevBuf() { release(); }
	operator T*() const { return ptr; }
	template <typename Owner>
	hipError_t reserve(Owner* owner, size_t n)   // room for n elements: exactly n when it has to allocate
	{
		if (cap >= n) return hipSuccess;
		release();
		LiveCount* const count = owner ? &owner->live : nullptr;
		const hipError_t e = dmalloc(count, &ptr, n);
		if (e == hipSuccess) { cap = n; live = count; }
		return e;
	}
	// n + 25 % + 1024 when it has to allocate (frames of a stream resemble each other: no reallocation for a slightly denser one)
	template <typename Owner>
	hipError_t grow(Owner* owner, size_t n) { return cap >= n ? hipSuccess : reserve(owner, n + n / 4 + 1024); }
	void release() { dfree(live, ptr); cap = 0; }
};
// the same for pinned host memory (not counted)
template <typename T>
struct PinBuf {
	T* ptr = nullptr; size_t cap = 0;
	PinBuf() = default;
	PinBuf(const PinBuf&) = delete;
	PinBuf& operator=(const PinBuf&) = delete;
	PinBuf(PinBuf&& o) noexcept : ptr(o.ptr), cap(o.cap) { o.ptr = nullptr; o.cap = 0; }
	PinBuf& operator=(PinBuf&& o) noexcept
	{
		if (this != &o) { release(); ptr = o.ptr; cap = o.cap; o.ptr = nullptr; o.cap = 0; }
		return *this;
	}
	~PinBuf() { release(); }
	operator T*() const { return ptr; }
	hipError_t reserve(size_t n, unsigned int flags = hipHostMallocDefault)
	{
		if (cap >= n) return hipSuccess;
		release();
		const hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&ptr), n * sizeof(T), flags);
		if (e != hipSuccess) { ptr = nullptr; return e; }
		const int fill = allocFill.load(std::memory_order_relaxed);
		if (fill >= 0) std::memset(ptr, fill, n * sizeof(T));
		cap = n;
		return e;
	}
	hipError_t grow(size_t n) { return cap >= n ? hipSuccess : reserve(n + n / 4 + 1024); }
	void release() { if (ptr) (void)hipHostFree(ptr); ptr = nullptr; cap = 0; }
};
} // namespace compvhip_api
