// pca_f32_floor.hip -- the instruction floor tools/pca_bench.py measures beside pca_project_kernel: a bare loop of INDEPENDENT float32 multiplies and adds,
// no memory traffic, 32 chains per lane (pairs of neighbours, so the compiler may pack them as it may in the kernel) so that no operation waits for
// another.  Built by tools/pca_bench.py into tools/_libs/ with -ffp-contract=off (a multiply and an add, never an FMA: the mix the PCA kernel may use).
// pca_f32_floor_ms -> milliseconds of one launch (HIP events, default stream), < 0 on error.
#include <hip/hip_runtime.h>

namespace {
constexpr int kChains = 32;

__global__ __launch_bounds__(256) void pca_f32_floor_kernel(float* out, int iters, float m, float c)
{
	float x[kChains];
#pragma unroll
	for (int k = 0; k < kChains; ++k) x[k] = 1.f + 1e-3f * (threadIdx.x + k);
	for (int i = 0; i < iters; ++i) {
#pragma unroll
		for (int k = 0; k < kChains; ++k) { x[k] = x[k] * m; x[k] = x[k] + c; }
	}
	float s = 0.f;
#pragma unroll
	for (int k = 0; k < kChains; ++k) s += x[k];
	out[static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x] = s;
}
}

// operations of one launch: blocks * 256 lanes * iters * 32 chains * 2
extern "C" __attribute__((visibility("default"))) float pca_f32_floor_ms(float* d_out, int blocks, int iters)
{
	hipEvent_t a, b;
	if (blocks < 1 || iters < 1 || !d_out || hipEventCreate(&a) != hipSuccess) return -1.f;
	if (hipEventCreate(&b) != hipSuccess) { (void)hipEventDestroy(a); return -1.f; }
	float ms = -1.f;
	(void)hipEventRecord(a, nullptr);
	pca_f32_floor_kernel<<<dim3(static_cast<unsigned>(blocks)), dim3(256), 0, nullptr>>>(d_out, iters, 0.999999f, 1e-6f);
	(void)hipEventRecord(b, nullptr);
	if (hipGetLastError() != hipSuccess || hipEventSynchronize(b) != hipSuccess || hipEventElapsedTime(&ms, a, b) != hipSuccess) ms = -1.f;
	(void)hipEventDestroy(a);
	(void)hipEventDestroy(b);
	return ms;
}
