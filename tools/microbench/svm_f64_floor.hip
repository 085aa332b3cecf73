// svm_f64_floor.hip -- the instruction floor tools/svm_bench.py measures beside svm_kvalues_kernel: a bare loop of INDEPENDENT float64 multiplies and adds,
// no memory traffic, 16 chains per lane so that no operation waits for another.  Built by tools/svm_bench.py into tools/_libs/ with -ffp-contract=off (a
// multiply and an add, never an FMA: the mix the SVM kernel may use).  svm_f64_floor_ms -> milliseconds of one launch (HIP events, default stream), < 0 on error.
#include <hip/hip_runtime.h>

namespace {
constexpr int kChains = 16;

__global__ __launch_bounds__(256) void svm_f64_floor_kernel(double* out, int iters, double m, double c)
{
	double x[kChains];
#pragma unroll
	for (int k = 0; k < kChains; ++k) x[k] = 1.0 + 1e-3 * (threadIdx.x + k);
	for (int i = 0; i < iters; ++i) {
#pragma unroll
		for (int k = 0; k < kChains; ++k) { x[k] = x[k] * m; x[k] = x[k] + c; }
	}
	double s = 0.0;
#pragma unroll
	for (int k = 0; k < kChains; ++k) s += x[k];
	out[static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x] = s;
}
}

// operations of one launch: blocks * 256 lanes * iters * 16 chains * 2
extern "C" __attribute__((visibility("default"))) float svm_f64_floor_ms(double* d_out, int blocks, int iters)
{
	hipEvent_t a, b;
	if (blocks < 1 || iters < 1 || !d_out || hipEventCreate(&a) != hipSuccess) return -1.f;
	if (hipEventCreate(&b) != hipSuccess) { (void)hipEventDestroy(a); return -1.f; }
	float ms = -1.f;
	(void)hipEventRecord(a, nullptr);
	svm_f64_floor_kernel<<<dim3(static_cast<unsigned>(blocks)), dim3(256), 0, nullptr>>>(d_out, iters, 0.999999, 1e-6);
	(void)hipEventRecord(b, nullptr);
	if (hipGetLastError() != hipSuccess || hipEventSynchronize(b) != hipSuccess || hipEventElapsedTime(&ms, a, b) != hipSuccess) ms = -1.f;
	(void)hipEventDestroy(a);
	(void)hipEventDestroy(b);
	return ms;
}
