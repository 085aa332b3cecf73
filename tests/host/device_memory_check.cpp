// device_memory_check.cpp -- DevBuf / PinBuf (compv_amd/csrc/device_memory.hpp) where every allocation FAILS: run on a machine without a GPU, where hipMalloc and
// hipHostMalloc return an error and a null pointer.  These are the paths no GPU test reaches: the {nullptr, 0} state after a failed reserve / grow,
// reserve(0), release and destruction of empty buffers, the moves, and the same failures with the fill of fresh allocations (compvhip_debug_alloc_fill)
// switched on: nothing filled, freed or counted.  Built for the host with AddressSanitizer and UBSan by tests/test_device_memory_host.py.
#include "../../compv_amd/csrc/device_memory.hpp"

#include <cstdint>
#include <cstdio>
#include <type_traits>
#include <utility>

using namespace compvhip_api;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

static_assert(!std::is_copy_constructible<DevBuf<int>>::value && !std::is_copy_assignable<DevBuf<int>>::value, "DevBuf is move-only");
static_assert(!std::is_copy_constructible<PinBuf<int>>::value && !std::is_copy_assignable<PinBuf<int>>::value, "PinBuf is move-only");
static_assert(std::is_nothrow_move_constructible<DevBuf<int>>::value && std::is_nothrow_move_assignable<DevBuf<int>>::value, "DevBuf moves");
static_assert(std::is_nothrow_move_constructible<PinBuf<int>>::value && std::is_nothrow_move_assignable<PinBuf<int>>::value, "PinBuf moves");

template <typename B> static bool empty(const B& b) { return b.ptr == nullptr && b.cap == 0; }

struct Owner { LiveCount live{0}; };   // what reserve / grow count in: the context in the library

int main()
{
	Owner owner;
	LiveCount& live = owner.live;
	{
		void* probe = nullptr;
		if (hipMalloc(&probe, 16) == hipSuccess) {   // a GPU after all: the wrapper should not have started this program
			(void)hipFree(probe);
			std::printf("device_memory_check: hipMalloc succeeded, nothing checked\n");
			return 2;
		}
	}
	{
		DevBuf<int32_t> d;
		CHECK(empty(d) && static_cast<int32_t*>(d) == nullptr);
		d.release();                                       // of an empty buffer: nothing happens
		CHECK(empty(d) && live.load() == 0);
		CHECK(d.reserve(&owner, 0) == hipSuccess);         // nothing to allocate
		CHECK(empty(d) && live.load() == 0);
		CHECK(d.reserve(&owner, 1000) != hipSuccess);
		CHECK(empty(d) && live.load() == 0);
		CHECK(d.grow(&owner, 10) != hipSuccess);           // asks for 10 + 2 + 1024
		CHECK(empty(d) && live.load() == 0);
		CHECK(d.reserve(&owner, 0) == hipSuccess);         // a failure leaves no stale capacity, and no stale error either
		CHECK(empty(d));
		CHECK(d.reserve(static_cast<Owner*>(nullptr), 16) != hipSuccess && empty(d));   // no owner: counted nowhere, not dereferenced
	}   // destructor of an empty buffer
	CHECK(live.load() == 0);
	{
		PinBuf<uint8_t> h;
		CHECK(empty(h));
		h.release();
		CHECK(h.reserve(0) == hipSuccess && empty(h));
		CHECK(h.reserve(4096) != hipSuccess && empty(h));
		CHECK(h.reserve(4096, hipHostMallocMapped) != hipSuccess && empty(h));
		CHECK(h.grow(1) != hipSuccess && empty(h));
	}
	{
		// The moves, on buffers that hold something: no allocation succeeds here, so the block is this program's own and is taken back before anything
		// could hand it to hipFree.  The count says one allocation throughout: nothing is counted twice, nothing is dropped.
		static int32_t block[8];
		DevBuf<int32_t> a;
		a.ptr = block; a.cap = 8; a.live = &live; live = 1;
		DevBuf<int32_t> b(std::move(a));
		CHECK(empty(a) && b.ptr == block && b.cap == 8 && b.live == &live && live.load() == 1);
		DevBuf<int32_t> c;
		c = std::move(b);
		CHECK(empty(b) && c.ptr == block && c.cap == 8 && c.live == &live && live.load() == 1);
		c = std::move(*&c);                                // self-assignment keeps it
		CHECK(c.ptr == block && c.cap == 8 && live.load() == 1);
		a.release(); b.release();                          // the moved-from ones are empty: nothing is freed or counted
		CHECK(live.load() == 1);
		CHECK(c.reserve(&owner, 8) == hipSuccess && c.ptr == block);   // fits: reused, no allocation tried
		c.ptr = nullptr; c.cap = 0; live = 0;              // take the block back
		a = std::move(c);                                  // empty into empty
		CHECK(empty(a) && empty(c) && live.load() == 0);

		static uint8_t bytes[16];
		PinBuf<uint8_t> p;
		p.ptr = bytes; p.cap = 16;
		PinBuf<uint8_t> q(std::move(p));
		CHECK(empty(p) && q.ptr == bytes && q.cap == 16);
		PinBuf<uint8_t> r;
		r = std::move(q);
		CHECK(empty(q) && r.ptr == bytes && r.cap == 16);
		CHECK(r.reserve(16) == hipSuccess && r.ptr == bytes);
		r.ptr = nullptr; r.cap = 0;
		CHECK(empty(a) && empty(b) && empty(c) && empty(p) && empty(q) && empty(r));   // nothing of this program's reaches hipFree / hipHostFree in the destructors
	}
	CHECK(live.load() == 0);
	for (const int byte : {0xFF, 0x01, 0x00}) {
		// the fill of fresh allocations (compvhip_debug_alloc_fill) switched on, the allocation fails: nothing is filled, freed or counted, the buffer stays empty
		allocFill.store(byte);
		DevBuf<int32_t> d;
		CHECK(d.reserve(&owner, 1000) != hipSuccess && empty(d) && live.load() == 0);
		CHECK(d.grow(&owner, 10) != hipSuccess && empty(d) && live.load() == 0);
		CHECK(d.reserve(&owner, 0) == hipSuccess && empty(d) && live.load() == 0);
		int32_t* raw = reinterpret_cast<int32_t*>(&owner);
		CHECK(dmalloc(&live, &raw, 16) != hipSuccess && raw == nullptr && live.load() == 0);
		PinBuf<uint8_t> h;
		CHECK(h.reserve(4096) != hipSuccess && empty(h));
		CHECK(h.reserve(4096, hipHostMallocMapped) != hipSuccess && empty(h));
		CHECK(h.grow(1) != hipSuccess && empty(h));
		CHECK(h.reserve(0) == hipSuccess && empty(h));
		static uint8_t bytes[16] = {7, 7, 7, 7, 7, 7, 7, 7, 7, 7, 7, 7, 7, 7, 7, 7};
		h.ptr = bytes; h.cap = 16;
		CHECK(h.reserve(16) == hipSuccess && h.ptr == bytes && bytes[0] == 7 && bytes[15] == 7);   // fits: reused and NOT filled
		h.ptr = nullptr; h.cap = 0;
		CHECK(allocFill.load() == byte);
	}
	allocFill.store(-1);
	CHECK(live.load() == 0);
	if (failures) return 1;
	std::printf("device_memory_check OK\n");
	return 0;
}
