// frame_slices.hpp -- batches whose frame index rides in a grid dimension limited to 65 535 (blockIdx.y / .z) are launched in slices.
// Host-side, standard library only.
#pragma once

namespace compvhip {

constexpr int kMaxFramesPerLaunch = 65535;

// Calls fn(f0, nf) for consecutive slices [f0, f0 + nf) of [0, frames), 1 <= nf <= 65 535 each.  fn returns a status whose value-initialised
// value means success (hipError_t, int): the first other value ends the loop and is returned.  frames <= 0: success, no call.
template <typename Fn>
auto for_frame_slices(int frames, Fn&& fn) -> decltype(fn(0, 0))
{
	using Status = decltype(fn(0, 0));
	for (int f0 = 0; f0 < frames;) {
		const int nf = frames - f0 < kMaxFramesPerLaunch ? frames - f0 : kMaxFramesPerLaunch;
		const Status s = fn(f0, nf);
		if (s != Status{}) return s;
		f0 += nf;
	}
	return Status{};
}

} // namespace compvhip
