// svm_kernels.hip -- C-SVC prediction (CompVMachineLearningSVM::predict -> svm_predict_values, base/ml/libsvm-322/libsvm.cxx) for gfx950: n query
// vectors against l support vectors of D dimensions in float64, RBF and LINEAR.  The definition is in include/compv_hip.h ("SVM prediction", items
// A - F); the arithmetic is svm_math.hpp.
//
//   svm_kvalues_kernel   a workgroup of 256 lanes owns 64 queries x 64 support vectors.  It stages 32 columns of both in the LDS as float64 (a float32
//                        query is widened there, which is exact), row-major with a pitch of 33 doubles: lanes of a wave read rows 66 dwords apart, 2
//                        banks each, without conflict.  A lane keeps 4 x 4 (query, SV) pairs -- queries ty, ty + 16, .., SVs tx, tx + 16, .. -- with
//                        the four accumulators of item B per pair (one for LINEAR).  A chunk is a multiple of 16 columns, so a 16-group of the
//                        reference's tree never straddles two; the pair / single tail runs once behind the last whole group.  Then the lane sums,
//                        * (-gamma) and exp_ref with the table staged in the same LDS, and K[n][l].
//   svm_decide_kernel    a wave per query: item E.  The four accumulators of the two dots of every class pair are 8 independent work items spread
//                        over the lanes (the order inside each is the reference's); then a lane per pair folds them into the decision value, and
//                        lane 0 counts the votes in pair order.
// No atomics: every output element has one writer.  No FMA: the Makefile builds with -ffp-contract=off, and a contracted d * d + s would round once
// where the reference rounds twice -- the last bit of K would differ.  No MFMA: v_mfma_f64 accumulates in an order of its own.  Every store is a plain
// C++ store.
#include "kernels.hpp"
#include "svm_math.hpp"

namespace compvhip {
namespace {

using namespace svm;

constexpr int kTile = kSvmTile;               // queries and support vectors of a workgroup
constexpr int kReg = 4;                       // per lane: kReg x kReg pairs
constexpr int kChunk = 32;                    // columns staged at a time: a multiple of 16
constexpr int kPitch = kChunk + 1;            // doubles per staged row
constexpr int kThreads = 256;                 // 16 x 16 lanes
static_assert(kTile == 16 * kReg && kChunk % 16 == 0 && 2 * kTile * kPitch >= kExpTable, "svm_kvalues_kernel: tile / staging geometry");

// the exponential's table as the kernel sees it: staged as doubles of the same bits
struct LdsTable {
	const double* p;
	__device__ uint64_t operator[](int i) const { return bits_of(p[i]); }
};

template <bool RBF>
__global__ __launch_bounds__(kThreads) void svm_kvalues_kernel(SvmKvaluesArgs a)
{
	__shared__ double s_mem[2 * kTile * kPitch];
	double* const s_q = s_mem;
	double* const s_v = s_mem + kTile * kPitch;
	constexpr int kAcc = RBF ? 4 : 1;
	const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
	const unsigned vTiles = (static_cast<unsigned>(a.l) + kTile - 1) / kTile;
	const int q0 = static_cast<int>(blockIdx.x / vTiles) * kTile, v0 = static_cast<int>(blockIdx.x % vTiles) * kTile;

	double acc[kReg][kReg][kAcc];
#pragma unroll
	for (int i = 0; i < kReg; ++i)
#pragma unroll
		for (int j = 0; j < kReg; ++j)
#pragma unroll
			for (int k = 0; k < kAcc; ++k) acc[i][j][k] = 0.0;

	// columns [k0, k0 + kc) of the tile's rows; rows behind n or l and columns behind kc read nothing and stage 0
	auto stage = [&](int k0, int kc) {
		for (int idx = tid; idx < kTile * kChunk; idx += kThreads) {
			const int r = idx / kChunk, c = idx % kChunk;
			double qv = 0.0, vv = 0.0;
			if (c < kc) {
				if (q0 + r < a.n) {
					const size_t off = static_cast<size_t>(q0 + r) * a.stride + static_cast<size_t>(k0 + c);
					qv = a.f32 ? static_cast<double>(static_cast<const float*>(a.vectors)[off]) : static_cast<const double*>(a.vectors)[off];
				}
				if (v0 + r < a.l) vv = a.sv[static_cast<size_t>(v0 + r) * a.dim + static_cast<size_t>(k0 + c)];
			}
			s_q[r * kPitch + c] = qv;
			s_v[r * kPitch + c] = vv;
		}
	};

	const int d16 = a.dim & ~15;
	for (int k0 = 0; k0 < d16; k0 += kChunk) {
		const int kc = min(kChunk, d16 - k0);          // 16 or 32
		stage(k0, kc);
		__syncthreads();
		for (int g = 0; g < kc; g += 16) {
			if constexpr (RBF) {
#pragma unroll
				for (int j = 0; j < 4; ++j) {          // accumulator j: the columns g + j, + 4, + 8, + 12
					double qa[kReg][4], vb[kReg][4];
#pragma unroll
					for (int i = 0; i < kReg; ++i)
#pragma unroll
						for (int m = 0; m < 4; ++m) {
							qa[i][m] = s_q[(ty + 16 * i) * kPitch + g + j + 4 * m];
							vb[i][m] = s_v[(tx + 16 * i) * kPitch + g + j + 4 * m];
						}
#pragma unroll
					for (int i = 0; i < kReg; ++i)
#pragma unroll
						for (int jj = 0; jj < kReg; ++jj)
							dotsub_lane(acc[i][jj][j], qa[i][0], qa[i][1], qa[i][2], qa[i][3], vb[jj][0], vb[jj][1], vb[jj][2], vb[jj][3]);
				}
			}
			else {
				for (int c = g; c < g + 16; ++c) {
					double qa[kReg], vb[kReg];
#pragma unroll
					for (int i = 0; i < kReg; ++i) { qa[i] = s_q[(ty + 16 * i) * kPitch + c]; vb[i] = s_v[(tx + 16 * i) * kPitch + c]; }
#pragma unroll
					for (int i = 0; i < kReg; ++i)
#pragma unroll
						for (int jj = 0; jj < kReg; ++jj) acc[i][jj][0] += qa[i] * vb[jj];
				}
			}
		}
		__syncthreads();          // the next chunk (or the tail, or the table) overwrites the staging
	}

	const int nt = a.dim - d16;          // 0 .. 15 columns behind the last whole group
	if (nt) {
		stage(d16, nt);
		__syncthreads();
		for (int c = 0; c < nt; ++c) {
			// RBF: pairs of columns into accumulators 0 and 1, a last single column (an even c) into 0; LINEAR: the one accumulator
			const int lane = c & 1;
			double qa[kReg], vb[kReg];
#pragma unroll
			for (int i = 0; i < kReg; ++i) { qa[i] = s_q[(ty + 16 * i) * kPitch + c]; vb[i] = s_v[(tx + 16 * i) * kPitch + c]; }
#pragma unroll
			for (int i = 0; i < kReg; ++i)
#pragma unroll
				for (int jj = 0; jj < kReg; ++jj) {
					if constexpr (RBF) {
						if (lane == 0) dotsub_one(acc[i][jj][0], qa[i], vb[jj]);
						else dotsub_one(acc[i][jj][1], qa[i], vb[jj]);
					}
					else acc[i][jj][0] += qa[i] * vb[jj];
				}
		}
		__syncthreads();
	}

	if constexpr (RBF) {
		for (int idx = tid; idx < kExpTable; idx += kThreads) s_mem[idx] = double_of(a.expTable[idx]);
		__syncthreads();
	}
	const LdsTable tab = { s_mem };
	const double gm = -a.gamma;
#pragma unroll
	for (int i = 0; i < kReg; ++i)
#pragma unroll
		for (int jj = 0; jj < kReg; ++jj) {
			const int q = q0 + ty + 16 * i, v = v0 + tx + 16 * jj;
			if (q < a.n && v < a.l) {
				double k;
				if constexpr (RBF) k = exp_ref(lanes_sum(acc[i][jj][0], acc[i][jj][1], acc[i][jj][2], acc[i][jj][3]) * gm, tab);
				else k = acc[i][jj][0];
				a.K[static_cast<size_t>(q) * a.l + v] = k;
			}
		}
}

constexpr int kDecideThreads = 64;

__global__ __launch_bounds__(kDecideThreads) void svm_decide_kernel(SvmDecideArgs a)
{
	__shared__ double s_part[8 * kMaxPairs];
	__shared__ int s_start[kMaxClasses], s_votes[kMaxClasses];
	__shared__ uint8_t s_first[kMaxPairs];          // the pair votes for its first class
	const int tid = threadIdx.x, nc = a.nrClass, P = nc * (nc - 1) / 2;
	const size_t q = blockIdx.x;
	const double* K = a.K + q * a.l;
	if (tid == 0) {
		int s = 0;
		for (int c = 0; c < nc; ++c) { s_start[c] = s; s += a.nSV[c]; s_votes[c] = 0; }
	}
	__syncthreads();
	for (int w = tid; w < 8 * P; w += kDecideThreads) {
		const int p = w >> 3, second = (w >> 2) & 1, j = w & 3;
		int ci, cj;
		pair_classes(p, nc, ci, cj);
		// sumi: sv_coef[cj - 1] over class ci's segment; sumj: sv_coef[ci] over class cj's
		const int cls = second ? cj : ci, row = second ? ci : cj - 1;
		s_part[w] = dot_lane_total(a.svCoef + static_cast<size_t>(row) * a.l + s_start[cls], K + s_start[cls], a.nSV[cls], j);
	}
	__syncthreads();
	for (int p = tid; p < P; p += kDecideThreads) {
		const double* s = s_part + 8 * p;
		const double sumi = lanes_sum(s[0], s[1], s[2], s[3]), sumj = lanes_sum(s[4], s[5], s[6], s[7]);
		const double d = (sumi + sumj) - a.rho[p];
		if (a.dec) a.dec[q * P + p] = d;
		s_first[p] = d > 0 ? 1 : 0;
	}
	__syncthreads();
	if (tid == 0) {
		int p = 0;
		for (int i = 0; i < nc; ++i)
			for (int j = i + 1; j < nc; ++j, ++p) ++s_votes[s_first[p] ? i : j];
		a.labels[q] = a.label[vote_winner(s_votes, nc)];
	}
}

} // namespace

hipError_t launch_svm_kvalues(const SvmKvaluesArgs& a, hipStream_t stream)
{
	const size_t tiles = ((static_cast<size_t>(a.n) + kTile - 1) / kTile) * ((static_cast<size_t>(a.l) + kTile - 1) / kTile);
	if (a.n < 1 || a.l < 1 || a.dim < 1 || tiles > 0x7fffffffull) return hipErrorInvalidValue;
	if (a.rbf) svm_kvalues_kernel<true><<<dim3(static_cast<unsigned>(tiles)), dim3(kThreads), 0, stream>>>(a);
	else svm_kvalues_kernel<false><<<dim3(static_cast<unsigned>(tiles)), dim3(kThreads), 0, stream>>>(a);
	return hipGetLastError();
}

hipError_t launch_svm_decide(const SvmDecideArgs& a, hipStream_t stream)
{
	if (a.n < 1 || a.nrClass < 2 || a.nrClass > svm::kMaxClasses) return hipErrorInvalidValue;
	svm_decide_kernel<<<dim3(static_cast<unsigned>(a.n)), dim3(kDecideThreads), 0, stream>>>(a);
	return hipGetLastError();
}

} // namespace compvhip
