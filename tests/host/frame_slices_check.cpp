// frame_slices_check.cpp -- for_frame_slices (compv_amd/csrc/frame_slices.hpp): the slices it hands out, and that it stops at the first error.
// A program of its own: standard library only, no GPU.  Prints "frame_slices_check OK" and returns 0 when every check holds.
#include "../../compv_amd/csrc/frame_slices.hpp"

#include <cstdio>
#include <utility>
#include <vector>

using compvhip::for_frame_slices;
using Slices = std::vector<std::pair<int, int>>;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

static void expectSlices(int frames, const Slices& want)
{
	Slices got;
	const int rc = for_frame_slices(frames, [&](int f0, int nf) { got.emplace_back(f0, nf); return 0; });
	CHECK(rc == 0);
	CHECK(got == want);
	// whatever the exact list: every slice fits the grid dimension, and together they tile [0, frames)
	int next = 0;
	for (const auto& s : got) {
		CHECK(s.first == next);
		CHECK(s.second >= 1 && s.second <= 65535);
		next = s.first + s.second;
	}
	CHECK(next == (frames > 0 ? frames : 0));
}

enum class Status { ok = 0, bad = 7 };   // a status type that is not int, as hipError_t is not

int main()
{
	expectSlices(0, {});
	expectSlices(-3, {});
	expectSlices(1, { { 0, 1 } });
	expectSlices(65535, { { 0, 65535 } });
	expectSlices(65536, { { 0, 65535 }, { 65535, 1 } });
	expectSlices(131070, { { 0, 65535 }, { 65535, 65535 } });
	expectSlices(131071, { { 0, 65535 }, { 65535, 65535 }, { 131070, 1 } });

	// a failure in the second of three slices: returned as it is, and the third slice is not started
	int calls = 0;
	const Status st = for_frame_slices(131071, [&](int, int) { return ++calls == 2 ? Status::bad : Status::ok; });
	CHECK(st == Status::bad);
	CHECK(calls == 2);
	const Status fine = for_frame_slices(131071, [&](int, int) { return Status::ok; });
	CHECK(fine == Status::ok);

	if (failures) return 1;
	std::printf("frame_slices_check OK\n");
	return 0;
}
