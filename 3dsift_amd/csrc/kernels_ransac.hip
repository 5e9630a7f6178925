// kernels_ransac.hip -- RANSAC affine fits of matched pairs (sift3d_fit_affine / sift3d_fit_affine_local, include/sift3d_hip.h).
// No reference counterpart.  The numerical contract (sampler, minimal solve, scoring, refit, neighbour order) is written out in the
// header; every fp64 expression here follows it term by term (the library builds with -ffp-contract=off, and the pragma of
// sift3d_internal.h keeps FMA contraction off in this unit as well).  The sampler, the scoring expression, the running top-k and the
// record writer are shared with the rigid fits (kernels_rigid.hip) through ransac_kit.h.
//
// Global fit, three launches on one stream:
//   k_ransac_hyp     one thread per hypothesis: 4 draws + the minimal solve; 12 doubles SoA, count = 0 (-1: degenerate)
//   k_ransac_score   grid (hypothesis tiles of 256) x (pair chunks of 256): the chunk is staged in LDS as doubles and read at a
//                    wave-uniform address (broadcast); each lane scores its hypothesis and adds its count (integer atomics: any
//                    order gives the same sums)
//   k_ransac_refit   one workgroup: argmax (count, -h), the refit rounds (sums in a fixed order: per-thread strided loop, xor
//                    butterfly in the wave, waves in index order) and the final mask
// Local fits, one launch: k_ransac_local gives a wave to each point -- the k nearest pairs by a running top-k held one entry per lane
// (chunks of 64 pairs are skipped by a ballot against the current k-th entry), then one candidate per lane, hypotheses 64 at a time
// one per lane (candidates read by readlane: scalar broadcast), and the refit with wave sums.
#include "sift3d_internal.h"

#include "ransac_kit.h"

#include <float.h>
#include <limits.h>

#include <algorithm>

namespace s3d {
namespace {

using namespace ransac_kit;

// cofactor inverse of M; false when |det| >= min_det does not hold (NaN included)
__device__ inline bool inv3(const double M[3][3], double min_det, double inv[3][3]) {
	double C[3][3];
#pragma unroll
	for (int r = 0; r < 3; r++) {
		const int r1 = r == 0 ? 1 : 0, r2 = r == 2 ? 1 : 2;
#pragma unroll
		for (int c = 0; c < 3; c++) {
			const int c1 = c == 0 ? 1 : 0, c2 = c == 2 ? 1 : 2;
			const double v = M[r1][c1] * M[r2][c2] - M[r1][c2] * M[r2][c1];
			C[r][c] = ((r + c) & 1) ? -v : v;
		}
	}
	const double det = (M[0][0] * C[0][0] + M[0][1] * C[0][1]) + M[0][2] * C[0][2];
	if (!(fabs(det) >= min_det)) return false;
#pragma unroll
	for (int i = 0; i < 3; i++)
#pragma unroll
		for (int j = 0; j < 3; j++) inv[i][j] = C[j][i] / det;
	return true;
}

// A = [N inv | t0 - (N inv) p0]
__device__ inline void affine_from(const double N[3][3], const double inv[3][3], const double p0[3], const double t0[3], double A[12]) {
#pragma unroll
	for (int i = 0; i < 3; i++) {
#pragma unroll
		for (int j = 0; j < 3; j++) A[4 * i + j] = (N[i][0] * inv[0][j] + N[i][1] * inv[1][j]) + N[i][2] * inv[2][j];
		A[4 * i + 3] = t0[i] - ((A[4 * i] * p0[0] + A[4 * i + 1] * p0[1]) + A[4 * i + 2] * p0[2]);
	}
}

// minimal solve of the samples P[j] -> T[j]; false: degenerate
__device__ inline bool solve_minimal(const double P[4][3], const double T[4][3], double min_det, double A[12]) {
	double M[3][3], N[3][3], inv[3][3];
#pragma unroll
	for (int k = 1; k < 4; k++)
#pragma unroll
		for (int i = 0; i < 3; i++) { M[i][k - 1] = P[k][i] - P[0][i]; N[i][k - 1] = T[k][i] - T[0][i]; }
	if (!inv3(M, min_det, inv)) return false;
	affine_from(N, inv, P[0], T[0], A);
	return true;
}

// The refit rounds of the contract on the inliers of A (hyp on entry).  each(f) calls f(r, t) for the calling thread's candidates;
// sum(v) replaces each element of the array v by its total over all threads of the problem, the same bits in every thread.
template <class Each, class Sum>
__device__ void refit(const Each &each, const Sum &sum, double A[12], double tau2, double min_det, int refine, int &status, int &inliers,
                      double &sumd2) {
	for (int round = 0;; round++) {
		double v[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // count, sum r, sum t, sum d2
		each([&](const double r[3], const double t[3]) {
			const double d2 = resid2(A, r[0], r[1], r[2], t[0], t[1], t[2]);
			if (d2 <= tau2) {
				v[0] += 1.0;
				for (int i = 0; i < 3; i++) { v[1 + i] += r[i]; v[4 + i] += t[i]; }
				v[7] += d2;
			}
		});
		sum(v);
		inliers = (int)v[0];
		sumd2 = v[7];
		if (round == refine || inliers < 4) return;
		double rb[3], tb[3];
		for (int i = 0; i < 3; i++) { rb[i] = v[1 + i] / v[0]; tb[i] = v[4 + i] / v[0]; }
		double w[15];  // Cov upper triangle (00 01 02 11 12 22), S row-major
		for (int i = 0; i < 15; i++) w[i] = 0.0;
		each([&](const double r[3], const double t[3]) {
			if (resid2(A, r[0], r[1], r[2], t[0], t[1], t[2]) <= tau2) {
				const double d0 = r[0] - rb[0], d1 = r[1] - rb[1], d2 = r[2] - rb[2];
				w[0] += d0 * d0; w[1] += d0 * d1; w[2] += d0 * d2; w[3] += d1 * d1; w[4] += d1 * d2; w[5] += d2 * d2;
				for (int i = 0; i < 3; i++) {
					const double e = t[i] - tb[i];
					w[6 + 3 * i] += e * d0; w[7 + 3 * i] += e * d1; w[8 + 3 * i] += e * d2;
				}
			}
		});
		sum(w);
		const double Cov[3][3] = {{w[0], w[1], w[2]}, {w[1], w[3], w[4]}, {w[2], w[4], w[5]}};
		const double S[3][3] = {{w[6], w[7], w[8]}, {w[9], w[10], w[11]}, {w[12], w[13], w[14]}};
		double inv[3][3];
		if (!inv3(Cov, min_det, inv)) { status = 3; return; }
		affine_from(S, inv, rb, tb, A);
	}
}

// ---- global fit -----------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void k_ransac_hyp(const float *__restrict__ pairs, int n, int H, uint32_t s, double min_det,
                                                    double *__restrict__ hyp /* 12 x H */, int *__restrict__ count) {
	const int h = blockIdx.x * 256 + threadIdx.x;
	if (h >= H) return;
	uint32_t idx[4];
	draw<4>(fmix32(s + 0u), (uint32_t)h, (uint32_t)n, idx);
	double P[4][3], T[4][3], A[12];
	for (int j = 0; j < 4; j++)
		for (int i = 0; i < 3; i++) { P[j][i] = pairs[(size_t)idx[j] * 6 + i]; T[j][i] = pairs[(size_t)idx[j] * 6 + 3 + i]; }
	const bool ok = solve_minimal(P, T, min_det, A);
	for (int i = 0; i < 12; i++) hyp[(size_t)i * H + h] = ok ? A[i] : 0.0;
	count[h] = ok ? 0 : -1;
}

__global__ __launch_bounds__(256) void k_ransac_score(const float *__restrict__ pairs, int n, int H, const double *__restrict__ hyp,
                                                      double tau2, int *__restrict__ count) {
	__shared__ double2 sp[kChunk][3];  // (rx, ry) (rz, tx) (ty, tz)
	double *flat = &sp[0][0].x;
	const int h = blockIdx.x * 256 + threadIdx.x;
	const bool live = h < H && count[h] >= 0;
	double A[12];
	for (int i = 0; i < 12; i++) A[i] = live ? hyp[(size_t)i * H + h] : 0.0;
	int c = 0;
	for (int c0 = blockIdx.y * kChunk; c0 < n; c0 += gridDim.y * kChunk) {  // (one chunk per workgroup unless n > 65535 chunks)
		const int cnt = min(kChunk, n - c0);
		__syncthreads();
		for (int i = threadIdx.x; i < cnt * 6; i += 256) flat[i] = (double)pairs[(size_t)c0 * 6 + i];
		__syncthreads();
		if (live)
			for (int j = 0; j < cnt; j++) {
				const double2 a = sp[j][0], b = sp[j][1], d = sp[j][2];
				c += resid2(A, a.x, a.y, b.x, b.y, d.x, d.y) <= tau2;
			}
	}
	if (c) atomicAdd(&count[h], c);
}

__global__ __launch_bounds__(kRefitThreads) void k_ransac_refit(const float *__restrict__ pairs, int n, int H, const double *__restrict__ hyp,
                                                                const int *__restrict__ count, double tau2, double min_det, int refine,
                                                                sift3d_affine_fit *__restrict__ out, unsigned char *__restrict__ mask) {
	constexpr int NW = kRefitThreads / 64;
	__shared__ double red[NW][16];
	__shared__ unsigned long long kred[NW];
	const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
	const unsigned long long key = best_key(count, H, kred);  // the most inliers, ties to the smallest h; 0 = degenerate
	if (key == 0) {
		const double Z[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
		if (tid == 0) write_fit(out, Z, Z, 2, n, -1, 0, 0, 0.0);
		for (int i = tid; i < n; i += kRefitThreads) mask[i] = 0;
		return;
	}
	const int bh = (int)(0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFu)), bc = (int)(key >> 32);
	double A[12], A0[12];
	for (int i = 0; i < 12; i++) A[i] = A0[i] = hyp[(size_t)i * H + bh];

	auto each = [&](auto &&f) {
		for (int i = tid; i < n; i += kRefitThreads) {
			const float *p = pairs + (size_t)i * 6;
			const double r[3] = {p[0], p[1], p[2]}, t[3] = {p[3], p[4], p[5]};
			f(r, t);
		}
	};
	auto sum = [&](auto &v) {
		constexpr int nv = sizeof(v) / sizeof(double);
#pragma unroll
		for (int k = 0; k < nv; k++) v[k] = wave_sum(v[k]);
		if (lane == 0)
#pragma unroll
			for (int k = 0; k < nv; k++) red[wv][k] = v[k];
		__syncthreads();
#pragma unroll
		for (int k = 0; k < nv; k++) {
			double s = 0.0;
#pragma unroll
			for (int w = 0; w < NW; w++) s += red[w][k];
			v[k] = s;
		}
		__syncthreads();
	};
	int status = 0, inliers = 0;
	double sumd2 = 0.0;
	refit(each, sum, A, tau2, min_det, refine, status, inliers, sumd2);
	for (int i = tid; i < n; i += kRefitThreads) {
		const float *p = pairs + (size_t)i * 6;
		mask[i] = resid2(A, p[0], p[1], p[2], p[3], p[4], p[5]) <= tau2 ? 1 : 0;
	}
	if (tid == 0) write_fit(out, A, A0, status, n, bh, bc, inliers, sumd2);
}

// ---- local fits -----------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void k_ransac_local(const float *__restrict__ pairs, int n, const float *__restrict__ pts, int m, int k,
                                                      float r2 /* radius^2 (fp32), < 0: no limit */, int H, uint32_t s, double tau2, double min_det,
                                                      int refine, sift3d_affine_fit *__restrict__ out, int *__restrict__ nbrs /* may be null */) {
	const int lane = threadIdx.x & 63, p = blockIdx.x * 4 + (threadIdx.x >> 6);
	if (p >= m) return;  // (whole waves: no workgroup barrier below)
	const float qx = pts[(size_t)p * 3], qy = pts[(size_t)p * 3 + 1], qz = pts[(size_t)p * 3 + 2];

	// phase 1: lane l < k holds entry l of the sorted list (d2, i)
	float myd;
	int myi;
	const int c = topk_neighbours(pairs, n, qx, qy, qz, k, r2, lane, myd, myi);
	if (nbrs && lane < k) nbrs[(size_t)p * k + lane] = lane < c ? myi : -1;
	const double Z[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
	if (c < 4) {
		if (lane == 0) write_fit(out + p, Z, Z, 1, c, -1, 0, 0, 0.0);
		return;
	}

	// phase 2: candidate `lane` (< c) in registers
	float cr[6];
	for (int j = 0; j < 6; j++) cr[j] = lane < c ? pairs[(size_t)myi * 6 + j] : 0.f;
	const uint32_t sp = fmix32(s + (uint32_t)p);
	unsigned long long best = 0;
	for (int hb = 0; hb < H; hb += 64) {
		const int h = hb + lane;
		uint32_t idx[4];
		draw<4>(sp, (uint32_t)h, (uint32_t)c, idx);
		double P[4][3], T[4][3], A[12];
		for (int j = 0; j < 4; j++)
			for (int i = 0; i < 3; i++) { P[j][i] = __shfl(cr[i], (int)idx[j]); T[j][i] = __shfl(cr[3 + i], (int)idx[j]); }
		const bool ok = solve_minimal(P, T, min_det, A) && h < H;
		int cnt = 0;
		for (int j = 0; j < c; j++)
			cnt += resid2(A, readlane_f(cr[0], j), readlane_f(cr[1], j), readlane_f(cr[2], j), readlane_f(cr[3], j), readlane_f(cr[4], j),
			              readlane_f(cr[5], j)) <= tau2;
		if (ok) best = max(best, ((unsigned long long)(unsigned)cnt << 32) | (0xFFFFFFFFu - (unsigned)h));
	}
	for (int off = 32; off > 0; off >>= 1) best = max(best, (unsigned long long)__shfl_xor(best, off));
	if (best == 0) {
		if (lane == 0) write_fit(out + p, Z, Z, 2, c, -1, 0, 0, 0.0);
		return;
	}
	const int bh = (int)(0xFFFFFFFFu - (unsigned)(best & 0xFFFFFFFFu)), bc = (int)(best >> 32);
	// the best hypothesis again, in every lane (uniform draws: the same bits as its lane had)
	double A[12], A0[12];
	{
		uint32_t idx[4];
		draw<4>(sp, (uint32_t)bh, (uint32_t)c, idx);
		double P[4][3], T[4][3];
		for (int j = 0; j < 4; j++)
			for (int i = 0; i < 3; i++) { P[j][i] = __shfl(cr[i], (int)idx[j]); T[j][i] = __shfl(cr[3 + i], (int)idx[j]); }
		solve_minimal(P, T, min_det, A);
		for (int i = 0; i < 12; i++) A0[i] = A[i];
	}
	auto each = [&](auto &&f) {
		if (lane < c) {
			const double r[3] = {cr[0], cr[1], cr[2]}, t[3] = {cr[3], cr[4], cr[5]};
			f(r, t);
		}
	};
	auto sum = [&](auto &v) {
		constexpr int nv = sizeof(v) / sizeof(double);
#pragma unroll
		for (int j = 0; j < nv; j++) v[j] = wave_sum(v[j]);
	};
	int status = 0, inliers = 0;
	double sumd2 = 0.0;
	refit(each, sum, A, tau2, min_det, refine, status, inliers, sumd2);
	if (lane == 0) write_fit(out + p, A, A0, status, c, bh, bc, inliers, sumd2);
}

}  // namespace

uint32_t ransac_seed(uint32_t seed) { return fmix32(seed ^ 0x9E3779B9u); }

void launch_ransac_score(const float *d_pairs, int n, int H, const double *d_hyp, double tau2, int *d_count, hipStream_t st) {
	hipLaunchKernelGGL(k_ransac_score, dim3((H + 255) / 256, std::min((n + kChunk - 1) / kChunk, 65535)), dim3(256), 0, st, d_pairs, n, H, d_hyp, tau2, d_count);
}

void launch_ransac_global(const float *d_pairs, int n, int H, uint32_t s, double tau2, double min_det, int refine, double *d_hyp, int *d_count,
                          sift3d_affine_fit *d_out, unsigned char *d_mask, hipStream_t st) {
	hipLaunchKernelGGL(k_ransac_hyp, dim3((H + 255) / 256), dim3(256), 0, st, d_pairs, n, H, s, min_det, d_hyp, d_count);
	launch_ransac_score(d_pairs, n, H, d_hyp, tau2, d_count, st);
	hipLaunchKernelGGL(k_ransac_refit, dim3(1), dim3(kRefitThreads), 0, st, d_pairs, n, H, d_hyp, d_count, tau2, min_det, refine, d_out, d_mask);
}

void launch_ransac_local(const float *d_pairs, int n, const float *d_pts, int m, int k, float r2, int H, uint32_t s, double tau2, double min_det,
                         int refine, sift3d_affine_fit *d_out, int *d_nbrs, hipStream_t st) {
	hipLaunchKernelGGL(k_ransac_local, dim3((m + 3) / 4), dim3(256), 0, st, d_pairs, n, d_pts, m, k, r2, H, s, tau2, min_det, refine, d_out, d_nbrs);
}

}  // namespace s3d
