// kernels_match_guided.hip -- guided matching (sift3d_match_guided, include/sift3d_hip.h): the matcher's best and second
// best of a row over the targets inside a spatial gate around the row's predicted position, instead of over all targets.
// No reference counterpart for the gate; the scoring is muBruteMatcher::calMatches (reference Src/cMatcher.cc:40-79) on the gated
// columns: s += (double)(a[k] * b[k]) with k ascending, strict '>' from FLT_MIN, ties to the lower column.
//   k_gate_points  a table of fp32 positions -> what poi_grid_build indexes: the floors as int (pts) and the exact values as
//                  doubles (disp).  A position with a non-finite coordinate or one beyond +-2^24 gets a floor the index refuses.
//   k_match_gated  one wave per query row.  The wave walks the PoiWindow of the row's position in chunks of 64 entries, applies the
//                  fp32 gate test to every entry (the index only narrows, the gate decides), compacts the passing columns into a queue
//                  and scores the queue 64 columns at a time: the PRODUCTS of a piece of 32 k are formed cooperatively (eight lanes
//                  per chain, 16-byte loads along the rows), parked in the wave's LDS block, and lane c then adds the products of
//                  chain c in order -- the scheme of k_rescore (kernels_match.hip).  A batch is folded into the row's running
//                  (best, second) by (score descending, column ascending) among the scores > FLT_MIN, which is what the reference's
//                  scan in ascending column order yields; the rule does not depend on the order of the walk.  No float atomics.
// The relation "column j is in the gate of row i" is fabsf(tar[j][c] - pred[i][c]) <= radius in fp32 for c = 0, 1, 2.  fabsf(a - b)
// equals fabsf(b - a) bit for bit, so the reverse pass (queries: target positions, index: the predicted positions) walks the same
// relation transposed with the same kernel.
#include <float.h>

#include "call_state.h"
#include "poi_window.h"

namespace s3d {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int KD = kDesc;
constexpr int kWaves = 4;                  // query rows of a workgroup
constexpr int kBatch = 64;                 // chains scored at a time: one per lane
constexpr int kPiece = 32;                 // k indices of a piece: eight lanes of 16 bytes per chain
constexpr int kPitch = kPiece + 4;         // floats between the chains' product rows (16-byte aligned)
constexpr int kQueue = 2 * kBatch;         // gated columns waiting for a batch: fewer than kBatch before a chunk adds up to 64
static_assert(KD % kPiece == 0, "a descriptor row is a whole number of pieces");

__device__ inline bool gate_coord_ok(float c) { return fabsf(c) <= (float)kCoordMax; }  // false for NaN and +-inf

__global__ __launch_bounds__(256) void k_gate_points(const float *__restrict__ xyz, int n, int *__restrict__ pts, double *__restrict__ disp) {
	const int i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n) return;
	const float x = xyz[3 * (size_t)i], y = xyz[3 * (size_t)i + 1], z = xyz[3 * (size_t)i + 2];
	const bool ok = gate_coord_ok(x) && gate_coord_ok(y) && gate_coord_ok(z);
	const float c[3] = {x, y, z};
	for (int a = 0; a < 3; a++) {
		pts[3 * (size_t)i + a] = ok ? (int)floorf(c[a]) : kCoordMax + 1;  // (coord_ok refuses the point)
		disp[3 * (size_t)i + a] = (double)c[a];
	}
}

// is (s, j) ahead of (bs, bj) in the order (score descending, column ascending)?  j < 0: no entry
__device__ inline bool ahead(double s, int j, double bs, int bj) { return j >= 0 && (bj < 0 || s > bs || (s == bs && j < bj)); }

// the first of the wave's (s, j) entries in that order, in every lane (j < 0 where no lane holds one)
__device__ inline void wave_first(double &s, int &j) {
	for (int off = 32; off > 0; off >>= 1) {
		const double os = __shfl_xor(s, off, 64);
		const int oj = __shfl_xor(j, off, 64);
		if (ahead(os, oj, s, j)) { s = os; j = oj; }
	}
}

__global__ __launch_bounds__(64 * kWaves) void k_match_gated(const float *__restrict__ A, const float *__restrict__ qxyz,
                                                              const int *__restrict__ row_ids, int nrows, const float *__restrict__ B,
                                                              PoiIndex ix, float radius, int half_width, float *__restrict__ gd,
                                                              float *__restrict__ sd, int *__restrict__ gi, int *__restrict__ si,
                                                              int *__restrict__ cnt) {
	__shared__ __attribute__((aligned(16))) float s_prod[kWaves][kBatch * kPitch];
	__shared__ int s_queue[kWaves][kQueue];
	const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
	const int r = blockIdx.x * kWaves + wv;
	if (r >= nrows) return;  // wave-uniform; the kernel has no workgroup barrier
	const int row = __builtin_amdgcn_readfirstlane(row_ids ? row_ids[r] : r);
	const float qx = qxyz[3 * (size_t)row], qy = qxyz[3 * (size_t)row + 1], qz = qxyz[3 * (size_t)row + 2];
	float *P = s_prod[wv];
	int *Q = s_queue[wv];
	const int oct = lane >> 3, l8 = lane & 7;
	const float *arow = A + (size_t)row * KD + 4 * l8;

	double b1 = FLT_MIN, b2 = FLT_MIN;  // the row's running best and second, the same in every lane
	int j1 = -1, j2 = -1;
	int fill = 0, gated = 0;

	// scores the first nc <= kBatch columns of the queue and folds them into (b1, j1, b2, j2)
	auto score = [&](int nc) {
		const int j = lane < nc ? Q[lane] : -1;
		double s = 0.0;
#pragma unroll 1
		for (int k0 = 0; k0 < KD; k0 += kPiece) {
			const f32x4 av = *reinterpret_cast<const f32x4 *>(arow + k0);
			for (int c = oct; c < nc; c += 8) {  // chain c: eight lanes, four products each
				const f32x4 bv = *reinterpret_cast<const f32x4 *>(B + (size_t)Q[c] * KD + k0 + 4 * l8);
				*reinterpret_cast<f32x4 *>(P + c * kPitch + 4 * l8) = f32x4{av.x * bv.x, av.y * bv.y, av.z * bv.z, av.w * bv.w};
			}
			__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
			__builtin_amdgcn_wave_barrier();
			__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
			if (lane < nc) {
				const f32x4 *pc = reinterpret_cast<const f32x4 *>(P + lane * kPitch);
#pragma unroll
				for (int q = 0; q < kPiece / 4; q++) {
					const f32x4 v = pc[q];
					s += (double)v.x; s += (double)v.y; s += (double)v.z; s += (double)v.w;
				}
			}
			__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
			__builtin_amdgcn_wave_barrier();  // the block is rewritten by the next piece
			__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
		}
		// the reference never chooses a score that is NaN or <= FLT_MIN
		const bool live = j >= 0 && s > (double)FLT_MIN;
		double c1 = s, c2 = s;
		int k1 = live ? j : -1;
		wave_first(c1, k1);
		int k2 = live && j != k1 ? j : -1;
		wave_first(c2, k2);
		// the batch's first two (c1, k1), (c2, k2) against the running two: a new best is followed by the better of its own second and
		// the old best; otherwise the batch's best may still be the second.  (Written as selects of values: with conditional
		// assignments the compiler kept the four running values in scratch memory.)
		const bool first = ahead(c1, k1, b1, j1), over_b1 = ahead(c2, k2, b1, j1), over_b2 = ahead(c1, k1, b2, j2);
		const double n2 = first ? (over_b1 ? c2 : b1) : (over_b2 ? c1 : b2);
		const int m2 = first ? (over_b1 ? k2 : j1) : (over_b2 ? k1 : j2);
		b1 = first ? c1 : b1; j1 = first ? k1 : j1;
		b2 = n2; j2 = m2;
	};

	if (gate_coord_ok(qx) && gate_coord_ok(qy) && gate_coord_ok(qz)) {
		const PoiWindow<true> win(ix.g, ix.start, ix.ncells, (int)floorf(qx), (int)floorf(qy), (int)floorf(qz), half_width);
		for (int t0 = 0; t0 < win.total; t0 += 64) {
			const int t = t0 + lane;
			bool in = false;
			int col = -1;
			if (t < win.total) {
				const int e = win.entry(t);
				// the gate, in fp32 as the contract writes it: one rounded subtraction per component
				const float dx = (float)ix.S.u[e] - qx, dy = (float)ix.S.v[e] - qy, dz = (float)ix.S.w[e] - qz;
				in = fabsf(dx) <= radius && fabsf(dy) <= radius && fabsf(dz) <= radius;
				col = ix.S.idx[e];
			}
			const unsigned long long mask = __ballot(in);
			if (in) Q[fill + __popcll(mask & ((1ull << lane) - 1ull))] = col;
			const int add = __popcll(mask);
			fill += add;
			gated += add;
			__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
			__builtin_amdgcn_wave_barrier();
			__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
			if (fill >= kBatch) {
				score(kBatch);
				const int rest = fill - kBatch;  // < kBatch: moved to the front (the two halves of the queue do not overlap)
				if (lane < rest) Q[lane] = Q[kBatch + lane];
				fill = rest;
				__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
				__builtin_amdgcn_wave_barrier();
				__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
			}
		}
		if (fill > 0) score(fill);
	}
	if (lane == 0) {
		gd[row] = (float)(2 - 2 * b1);
		sd[row] = (float)(2 - 2 * b2);
		gi[row] = j1;
		si[row] = j2;
		if (cnt) cnt[row] = gated;
	}
}

}  // namespace

void launch_gate_points(const float *d_xyz, int n, int *d_pts, double *d_disp, hipStream_t st) {
	if (n > 0) hipLaunchKernelGGL(k_gate_points, dim3((n + 255) / 256), dim3(256), 0, st, d_xyz, n, d_pts, d_disp);
}

void launch_match_gated(const float *d_a, const float *d_qxyz, const int *d_row_ids, int nrows, const float *d_b, const PoiIndex &ix,
                        float radius, int half_width, float *d_gd, float *d_sd, int *d_gi, int *d_si, int *d_cnt, hipStream_t st) {
	if (nrows > 0)
		hipLaunchKernelGGL(k_match_gated, dim3((nrows + kWaves - 1) / kWaves), dim3(64 * kWaves), 0, st, d_a, d_qxyz, d_row_ids, nrows, d_b, ix,
		                   radius, half_width, d_gd, d_sd, d_gi, d_si, d_cnt);
}

}  // namespace s3d
