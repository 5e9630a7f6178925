// kernels_rigid.hip -- RANSAC rigid and similarity fits of matched pairs (sift3d_fit_rigid / sift3d_fit_rigid_local,
// include/sift3d_hip.h).  No reference counterpart.  The numerical contract (sampler, triad, scoring, Horn refit, Jacobi) is written
// out in the header; every fp64 expression here follows it term by term (the library builds with -ffp-contract=off, and the pragma
// of sift3d_internal.h keeps FMA contraction off in this unit as well).  What the affine fits share lives in ransac_kit.h; the
// triad, the Jacobi and the Horn refit, which the per-body fits (kernels_bodyfit.hip) run as well, in rigid_kit.h.
//
// Global fit, three launches on one stream:
//   k_rigid_hyp      one thread per hypothesis: 3 draws + the triad; 12 doubles SoA, count = 0 (-1: degenerate)
//   k_ransac_score   the affine fit's scoring kernel as it is (kernels_ransac.hip): it reads 12 doubles per hypothesis
//   k_rigid_refit    one workgroup: argmax (count, -h), the refit rounds (sums in the fixed order of k_ransac_refit) and the final
//                    mask; every thread runs the 4x4 Jacobi on the same sums (no broadcast, no extra barrier)
// Local fits, one launch: k_rigid_local gives a wave to each point -- the top-k of the affine local fit, one candidate per lane,
// hypotheses 64 at a time one per lane, the refit with wave sums.  The Jacobi runs once per refit round, never per hypothesis.
#include "sift3d_internal.h"

#include "rigid_kit.h"

#include <float.h>
#include <limits.h>

#include <algorithm>

namespace s3d {
namespace {

using namespace rigid_kit;

// ---- global fit -----------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void k_rigid_hyp(const float *__restrict__ pairs, int n, int H, uint32_t s, double md2, int model,
                                                   double *__restrict__ hyp /* 12 x H */, int *__restrict__ count) {
	const int h = blockIdx.x * 256 + threadIdx.x;
	if (h >= H) return;
	uint32_t idx[3];
	draw<3>(fmix32(s + 0u), (uint32_t)h, (uint32_t)n, idx);
	double P[3][3], T[3][3], A[12];
	for (int j = 0; j < 3; j++)
		for (int i = 0; i < 3; i++) { P[j][i] = pairs[(size_t)idx[j] * 6 + i]; T[j][i] = pairs[(size_t)idx[j] * 6 + 3 + i]; }
	const bool ok = solve_triad(P, T, md2, model, A);
	for (int i = 0; i < 12; i++) hyp[(size_t)i * H + h] = ok ? A[i] : 0.0;
	count[h] = ok ? 0 : -1;
}

__global__ __launch_bounds__(kRefitThreads) void k_rigid_refit(const float *__restrict__ pairs, int n, int H, const double *__restrict__ hyp,
                                                               const int *__restrict__ count, double tau2, double md2, int model, int refine,
                                                               sift3d_affine_fit *__restrict__ out, unsigned char *__restrict__ mask) {
	constexpr int NW = kRefitThreads / 64;
	__shared__ double red[NW][16];
	__shared__ unsigned long long kred[NW];
	const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
	const unsigned long long key = best_key(count, H, kred);
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
		static_assert(nv <= 16, "red holds 16 sums per wave");
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
	refit_rigid(each, sum, A, tau2, md2, model, refine, status, inliers, sumd2);
	for (int i = tid; i < n; i += kRefitThreads) {
		const float *p = pairs + (size_t)i * 6;
		mask[i] = resid2(A, p[0], p[1], p[2], p[3], p[4], p[5]) <= tau2 ? 1 : 0;
	}
	if (tid == 0) write_fit(out, A, A0, status, n, bh, bc, inliers, sumd2);
}

// ---- local fits -----------------------------------------------------------------------------------------------------------------

// the samples of hypothesis h over the c candidates the lanes hold (cr: candidate `lane`)
__device__ inline void gather_triad(const float cr[6], uint32_t sp, uint32_t h, uint32_t c, double P[3][3], double T[3][3]) {
	uint32_t idx[3];
	draw<3>(sp, h, c, idx);
	for (int j = 0; j < 3; j++)
		for (int i = 0; i < 3; i++) { P[j][i] = __shfl(cr[i], (int)idx[j]); T[j][i] = __shfl(cr[3 + i], (int)idx[j]); }
}

__global__ __launch_bounds__(256) void k_rigid_local(const float *__restrict__ pairs, int n, const float *__restrict__ pts, int m, int k,
                                                     float r2 /* radius^2 (fp32), < 0: no limit */, int H, uint32_t s, double tau2, double md2,
                                                     int model, int refine, sift3d_affine_fit *__restrict__ out,
                                                     int *__restrict__ nbrs /* may be null */) {
	const int lane = threadIdx.x & 63, p = blockIdx.x * 4 + (threadIdx.x >> 6);
	if (p >= m) return;  // (whole waves: no workgroup barrier below)
	const float qx = pts[(size_t)p * 3], qy = pts[(size_t)p * 3 + 1], qz = pts[(size_t)p * 3 + 2];

	// phase 1: lane l < k holds entry l of the sorted list (d2, i)
	float myd;
	int myi;
	const int c = topk_neighbours(pairs, n, qx, qy, qz, k, r2, lane, myd, myi);
	if (nbrs && lane < k) nbrs[(size_t)p * k + lane] = lane < c ? myi : -1;
	const double Z[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
	if (c < 3) {
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
		double P[3][3], T[3][3], A[12];
		gather_triad(cr, sp, (uint32_t)h, (uint32_t)c, P, T);
		const bool ok = solve_triad(P, T, md2, model, A) && h < H;
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
		double P[3][3], T[3][3];
		gather_triad(cr, sp, (uint32_t)bh, (uint32_t)c, P, T);
		solve_triad(P, T, md2, model, A);
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
	refit_rigid(each, sum, A, tau2, md2, model, refine, status, inliers, sumd2);
	if (lane == 0) write_fit(out + p, A, A0, status, c, bh, bc, inliers, sumd2);
}

}  // namespace

void launch_rigid_global(const float *d_pairs, int n, int H, uint32_t s, double tau2, double min_det, int model, int refine, double *d_hyp,
                         int *d_count, sift3d_affine_fit *d_out, unsigned char *d_mask, hipStream_t st) {
	const double md2 = min_det * min_det;
	hipLaunchKernelGGL(k_rigid_hyp, dim3((H + 255) / 256), dim3(256), 0, st, d_pairs, n, H, s, md2, model, d_hyp, d_count);
	launch_ransac_score(d_pairs, n, H, d_hyp, tau2, d_count, st);
	hipLaunchKernelGGL(k_rigid_refit, dim3(1), dim3(kRefitThreads), 0, st, d_pairs, n, H, d_hyp, d_count, tau2, md2, model, refine, d_out, d_mask);
}

void launch_rigid_local(const float *d_pairs, int n, const float *d_pts, int m, int k, float r2, int H, uint32_t s, double tau2, double min_det,
                        int model, int refine, sift3d_affine_fit *d_out, int *d_nbrs, hipStream_t st) {
	hipLaunchKernelGGL(k_rigid_local, dim3((m + 3) / 4), dim3(256), 0, st, d_pairs, n, d_pts, m, k, r2, H, s, tau2, min_det * min_det, model, refine,
	                   d_out, d_nbrs);
}

}  // namespace s3d
