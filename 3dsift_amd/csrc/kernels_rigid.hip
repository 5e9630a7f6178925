// kernels_rigid.hip -- RANSAC rigid and similarity fits of matched pairs (sift3d_fit_rigid / sift3d_fit_rigid_local,
// include/sift3d_hip.h).  No reference counterpart.  The numerical contract (sampler, triad, scoring, Horn refit, Jacobi) is written
// out in the header; every fp64 expression here follows it term by term (the library builds with -ffp-contract=off, and the pragma
// of sift3d_internal.h keeps FMA contraction off in this unit as well).  What the affine fits share lives in ransac_kit.h.
//
// Global fit, three launches on one stream:
//   k_rigid_hyp      one thread per hypothesis: 3 draws + the triad; 12 doubles SoA, count = 0 (-1: degenerate)
//   k_ransac_score   the affine fit's scoring kernel as it is (kernels_ransac.hip): it reads 12 doubles per hypothesis
//   k_rigid_refit    one workgroup: argmax (count, -h), the refit rounds (sums in the fixed order of k_ransac_refit) and the final
//                    mask; every thread runs the 4x4 Jacobi on the same sums (no broadcast, no extra barrier)
// Local fits, one launch: k_rigid_local gives a wave to each point -- the top-k of the affine local fit, one candidate per lane,
// hypotheses 64 at a time one per lane, the refit with wave sums.  The Jacobi runs once per refit round, never per hypothesis.
#include "sift3d_internal.h"

#include "ransac_kit.h"

#include <float.h>
#include <limits.h>

#include <algorithm>

namespace s3d {
namespace {

using namespace ransac_kit;

__device__ inline double dot3(const double u[3], const double v[3]) { return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]; }

__device__ inline void cross3(const double u[3], const double v[3], double w[3]) {
	w[0] = u[1] * v[2] - u[2] * v[1];
	w[1] = u[2] * v[0] - u[0] * v[2];
	w[2] = u[0] * v[1] - u[1] * v[0];
}

// the frame (x, y, z) of the edges a = Q1 - Q0, b = Q2 - Q0: x = a / |a|, z = (a x b) / |a x b|, y = z x x; cc = (a x b).(a x b),
// len = (a.a + b.b) + (b - a).(b - a)
__device__ inline void triad_frame(const double Q[3][3], double x[3], double y[3], double z[3], double &cc, double &len) {
	double a[3], b[3], c[3], d[3];
#pragma unroll
	for (int i = 0; i < 3; i++) { a[i] = Q[1][i] - Q[0][i]; b[i] = Q[2][i] - Q[0][i]; }
	cross3(a, b, c);
	const double aa = dot3(a, a);
	cc = dot3(c, c);
	const double na = sqrt(aa), nc = sqrt(cc);
#pragma unroll
	for (int i = 0; i < 3; i++) { x[i] = a[i] / na; z[i] = c[i] / nc; d[i] = b[i] - a[i]; }
	cross3(z, x, y);
	len = (aa + dot3(b, b)) + dot3(d, d);
}

// A = [L | t0 - L p0]
__device__ inline void with_offset(const double L[3][3], const double p0[3], const double t0[3], double A[12]) {
#pragma unroll
	for (int i = 0; i < 3; i++) {
#pragma unroll
		for (int j = 0; j < 3; j++) A[4 * i + j] = L[i][j];
		A[4 * i + 3] = t0[i] - ((L[i][0] * p0[0] + L[i][1] * p0[1]) + L[i][2] * p0[2]);
	}
}

// minimal solve of the samples P[j] -> T[j] (j < 3); md2 = min_det * min_det; false: degenerate
__device__ inline bool solve_triad(const double P[3][3], const double T[3][3], double md2, int model, double A[12]) {
	double x[3], y[3], z[3], xt[3], yt[3], zt[3], cc, cct, len, lent;
	triad_frame(P, x, y, z, cc, len);
	triad_frame(T, xt, yt, zt, cct, lent);
	if (!(cc >= md2) || !(cct > 0.0)) return false;
	const double s = model == 1 ? sqrt(lent / len) : 1.0;
	double L[3][3];
#pragma unroll
	for (int i = 0; i < 3; i++)
#pragma unroll
		for (int j = 0; j < 3; j++) {
			const double r = (xt[i] * x[j] + yt[i] * y[j]) + zt[i] * z[j];
			L[i][j] = model == 1 ? s * r : r;
		}
	with_offset(L, P[0], T[0], A);
	return true;
}

// index of (i, j) in the upper triangle 00 01 02 03 11 12 13 22 23 33
__device__ constexpr int sym(int i, int j) { return i <= j ? 4 * i - i * (i - 1) / 2 + (j - i) : 4 * j - j * (j - 1) / 2 + (i - j); }

// unit eigenvector of the largest eigenvalue of the symmetric 4x4 a (upper triangle, destroyed): 8 cyclic Jacobi sweeps
__device__ inline void top_eigenvector4(double a[10], double q[4]) {
	double v[4][4];
#pragma unroll
	for (int i = 0; i < 4; i++)
#pragma unroll
		for (int j = 0; j < 4; j++) v[i][j] = i == j ? 1.0 : 0.0;
#pragma unroll 1
	for (int sweep = 0; sweep < 8; sweep++) {
#pragma unroll
		for (int pl = 0; pl < 6; pl++) {
			constexpr int PP[6] = {0, 0, 0, 1, 1, 2}, QQ[6] = {1, 2, 3, 2, 3, 3};
			const int p = PP[pl], qq = QQ[pl];
			const double apq = a[sym(p, qq)];
			if (apq == 0.0) continue;
			const double theta = (a[sym(qq, qq)] - a[sym(p, p)]) / (2.0 * apq);
			const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
			const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
			a[sym(p, p)] -= t * apq;
			a[sym(qq, qq)] += t * apq;
			a[sym(p, qq)] = 0.0;
#pragma unroll
			for (int r = 0; r < 4; r++) {
				if (r != p && r != qq) {
					const double arp = a[sym(r, p)], arq = a[sym(r, qq)];
					a[sym(r, p)] = c * arp - s * arq;
					a[sym(r, qq)] = s * arp + c * arq;
				}
				const double vrp = v[r][p], vrq = v[r][qq];
				v[r][p] = c * vrp - s * vrq;
				v[r][qq] = s * vrp + c * vrq;
			}
		}
	}
	int best = 0;
	double top = a[sym(0, 0)];
#pragma unroll
	for (int i = 1; i < 4; i++)
		if (a[sym(i, i)] > top) { top = a[sym(i, i)]; best = i; }
#pragma unroll
	for (int r = 0; r < 4; r++) q[r] = best == 0 ? v[r][0] : best == 1 ? v[r][1] : best == 2 ? v[r][2] : v[r][3];
	const double nq = sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
#pragma unroll
	for (int r = 0; r < 4; r++) q[r] /= nq;
}

// The refit rounds of the contract (Horn's quaternion method) on the inliers of A (hyp on entry).  each / sum: as in the affine
// refit of kernels_ransac.hip.
template <class Each, class Sum>
__device__ void refit_rigid(const Each &each, const Sum &sum, double A[12], double tau2, double md2, int model, int refine, int &status,
                            int &inliers, double &sumd2) {
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
		if (round == refine || inliers < 3) return;
		double rb[3], tb[3];
		for (int i = 0; i < 3; i++) { rb[i] = v[1 + i] / v[0]; tb[i] = v[4 + i] / v[0]; }
		double w[16];  // Cov upper triangle (00 01 02 11 12 22), S_ab = sum d_a e_b row-major, sum e.e
		for (int i = 0; i < 16; i++) w[i] = 0.0;
		each([&](const double r[3], const double t[3]) {
			if (resid2(A, r[0], r[1], r[2], t[0], t[1], t[2]) <= tau2) {
				const double d[3] = {r[0] - rb[0], r[1] - rb[1], r[2] - rb[2]};
				const double e[3] = {t[0] - tb[0], t[1] - tb[1], t[2] - tb[2]};
				w[0] += d[0] * d[0]; w[1] += d[0] * d[1]; w[2] += d[0] * d[2]; w[3] += d[1] * d[1]; w[4] += d[1] * d[2]; w[5] += d[2] * d[2];
				for (int i = 0; i < 3; i++) { w[6 + 3 * i] += d[i] * e[0]; w[7 + 3 * i] += d[i] * e[1]; w[8 + 3 * i] += d[i] * e[2]; }
				w[15] += dot3(e, e);
			}
		});
		sum(w);
		const double C00 = w[0], C01 = w[1], C02 = w[2], C11 = w[3], C12 = w[4], C22 = w[5];
		const double e2 = ((C00 * C11 - C01 * C01) + (C00 * C22 - C02 * C02)) + (C11 * C22 - C12 * C12);
		if (!(e2 >= md2)) { status = 3; return; }
		const double Sxx = w[6], Sxy = w[7], Sxz = w[8], Syx = w[9], Syy = w[10], Syz = w[11], Szx = w[12], Szy = w[13], Szz = w[14];
		double N[10] = {(Sxx + Syy) + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx, (Sxx - Syy) - Szz, Sxy + Syx, Szx + Sxz, (-Sxx + Syy) - Szz,
		                Syz + Szy, (-Sxx - Syy) + Szz};
		double q[4];
		top_eigenvector4(N, q);
		const double qw = q[0], qx = q[1], qy = q[2], qz = q[3];
		const double ww = qw * qw, xx = qx * qx, yy = qy * qy, zz = qz * qz;
		const double s = model == 1 ? sqrt(w[15] / ((C00 + C11) + C22)) : 1.0;
		double L[3][3] = {{((ww + xx) - yy) - zz, 2.0 * (qx * qy - qw * qz), 2.0 * (qx * qz + qw * qy)},
		                  {2.0 * (qx * qy + qw * qz), ((ww - xx) + yy) - zz, 2.0 * (qy * qz - qw * qx)},
		                  {2.0 * (qx * qz - qw * qy), 2.0 * (qy * qz + qw * qx), ((ww - xx) - yy) + zz}};
		if (model == 1)
			for (int i = 0; i < 3; i++)
				for (int j = 0; j < 3; j++) L[i][j] = s * L[i][j];
		with_offset(L, rb, tb, A);
	}
}

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
