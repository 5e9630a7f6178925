// kernels_icgn2.hip -- second-order (30-parameter) IC-GN (sift3d_icgn2, include/sift3d_hip.h, which states the numerical contract).
// No reference counterpart.  The structure of kernels_icgn.hip: one workgroup of 256 threads per point of interest (POI), two launches
// on one stream; the walk over the subset and the per-voxel sample of T are shared with it (icgn_subset.h).
//   k_icgn2_prepare  the status 5 / 2 / 4 / 3 checks, Rm, dR and the constants of the subset in fp64, in passes over the subset (R's
//                    subset is cache resident) so that no pass holds more than 35 fp64 sums per thread: one pass per component for
//                    sum SD^T and sum SD^T (R - Rm) (22 sums), one pass per gradient pair for H (35 sums: H(i, j) is g_a g_b times a
//                    monomial of degree <= 4, and there are 35 of those; the 1/2 of the squares is applied afterwards, exactly); the
//                    30 x 30 fp64 Cholesky of H in LDS (a column per step, the trailing update spread over the workgroup) and H^-1 by
//                    30 column solves in LDS; a record per POI (Icgn2State) with H^-1's lower triangle for the second launch
//   k_icgn2_iterate  every iteration inside the launch: one pass over the subset per iteration gathers 33 sums at the current warp
//                    (sum T', sum T'^2, the 30 sums SD^T T' and sum R'T'), reduced in a fixed order.  The step is formed across
//                    threads -- thread j the right-hand side b_j, thread i the row i of H^-1 b, both through LDS -- and wave 0 alone
//                    composes the warp: lane i holds row i of M(dp) in registers, the 10 x 10 LU with partial pivoting and the three
//                    row solves exchange rows by shuffles (no LDS, no barrier), lanes 0..2 form the new parameters of one component
//                    each and test its axis of the domain rule.  Four barriers per pass; p lives in LDS between the passes.
// The per-voxel sample of T is fp32 (position, weights, gather); the products g T' xi' and every per-thread sum are fp64, as is the
// reduction.  That is not a luxury: the fp32 rounding of T' is a perturbation e of T', which reaches dp as H^-1 SD^T e, a least-squares
// projection damped by 1 / sigma_min(SD); a product g T' rounded to fp32 is not of that form, enters b directly and is amplified by
// 1 / lambda_min(H) = 1 / sigma_min^2 -- 3e-4 voxel at r = 2 where the fp32 sample alone costs 1e-6 (measured).  No
// float atomics: two calls give the same bits.
#include "icgn_subset.h"

#include <math.h>

namespace s3d {
namespace {

using namespace icgn;

constexpr int kP = 30;                    // parameters: 10 per component
constexpr int kTri = kP * (kP + 1) / 2;   // the lower triangle of H^-1
constexpr int kMono = 35;                 // monomials of degree <= 4 in (dx, dy, dz)
constexpr int kCompSums = 22;             // per component: 10 sum SD, 10 sum SD R', and (used once) dR^2, sum R'
constexpr int kIterSums = 33;             // sum T', sum T'^2, 30 sum SD T', sum R'T' (T' = T - Tc)

struct Icgn2State {
	double hinv[kTri];  // H^-1 (symmetric): (i, j), j <= i, at i (i + 1) / 2 + j
	double c1[kP];      // sum SD^T (R - Rm)
	double c2[kP];      // sum SD^T
	double dr;          // dR
	double sr;          // sum (R - Rm) as the iterate kernel forms R' (fp32 R - (float)Rm): zncc's correction term
	float rm;           // (float)Rm
	int status;         // kRun, or the final status the prepare kernel wrote
};

// the ten terms of a component: c, cx, cy, cz, cxx, cyy, czz, cxy, cxz, cyz
__device__ inline int term_ex(int k) { return (k == 1) + (k == 7) + (k == 8) + 2 * (k == 4); }
__device__ inline int term_ey(int k) { return (k == 2) + (k == 7) + (k == 9) + 2 * (k == 5); }
__device__ inline int term_ez(int k) { return (k == 3) + (k == 8) + (k == 9) + 2 * (k == 6); }
__device__ inline double term_half(int k) { return (k >= 4 && k <= 6) ? 0.5 : 1.0; }

// index of dx^i dy^j dz^k in the order the H passes enumerate the monomials: i, then j <= 4 - i, then k <= 4 - i - j
__device__ inline int mono_index(int i, int j, int k) {
	int at = 0;
	for (int a = 0; a < i; a++) at += (5 - a) * (6 - a) / 2;
	for (int b = 0; b < j; b++) at += 5 - i - b;
	return at + k;
}

__device__ inline void write_result(sift3d_icgn2_result *o, const double *p, double zncc, double last, int it, int status) {
	for (int k = 0; k < kP; k++) o->p[k] = p ? p[k] : 0.0;
	o->zncc = zncc;
	o->last_step = last;
	o->iterations = it;
	o->status = status;
	o->reserved[0] = o->reserved[1] = 0;
}

// one axis of the domain rule (fp64; a NaN is outside): the 8 corners of the affine part of e (the ten terms of component a), widened
// by B_a = r^2 (|cxx| / 2 + |cyy| / 2 + |czz| / 2 + |cxy| + |cxz| + |cyz|); with zero second-order terms the first-order rule
__device__ inline bool axis_in_domain(const double e[10], int a, int qa, int r, int n, bool cubic) {
	const double fx = (a == 0 ? 1.0 + e[1] : e[1]), fy = (a == 1 ? 1.0 + e[2] : e[2]), fz = (a == 2 ? 1.0 + e[3] : e[3]);
	double mn = INFINITY, mx = -INFINITY;
	bool ok = true;
#pragma unroll
	for (int c = 0; c < 8; c++) {
		const double dx = (c & 1) ? r : -r, dy = (c & 2) ? r : -r, dz = (c & 4) ? r : -r;
		const double v = ((double)qa + ((fx * dx + fy * dy) + fz * dz)) + e[0];
		ok = ok && (v == v);
		mn = v < mn ? v : mn;
		mx = v > mx ? v : mx;
	}
	const double B = ((double)r * (double)r) * ((((0.5 * fabs(e[4]) + 0.5 * fabs(e[5])) + 0.5 * fabs(e[6])) + fabs(e[7])) + fabs(e[8]) + fabs(e[9]));
	const double lo = floor(mn - B), hi = floor(mx + B);
	return ok && (cubic ? (lo - 1.0 >= 0.0 && hi + 2.0 <= (double)(n - 1)) : (lo >= 0.0 && hi + 1.0 <= (double)(n - 1)));
}

// ---- prepare ---------------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(kThreads) void k_icgn2_prepare(IcgnVol R, IcgnVol T, const int *__restrict__ pts, const double *__restrict__ init,
                                                           int r, int cubic, Icgn2State *__restrict__ state, sift3d_icgn2_result *__restrict__ out) {
	__shared__ double red[kWaves][kMono];
	__shared__ double sums[2 + 2 * kP];  // dR^2, sum R', 30 sum SD, 30 sum SD R'
	__shared__ double hp[6][kMono];      // the H pieces: gradient pair x monomial
	__shared__ double A[kP][kP + 1];
	__shared__ double Y[kP][kP + 1];
	__shared__ int s_fail;
	const int poi = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
	const int q[3] = {pts[3 * poi], pts[3 * poi + 1], pts[3 * poi + 2]};
	const double *p0 = init ? init + kP * (size_t)poi : nullptr;
	const int bad = (p0 && tid < kP) ? !isfinite(p0[tid]) : 0;
	const bool finite = !__syncthreads_or(bad);
	Icgn2State *S = state + poi;
	int status = kRun;
	if (!finite) status = 5;
	else if (q[0] - r - 1 < 0 || q[0] + r + 1 > R.nx - 1 || q[1] - r - 1 < 0 || q[1] + r + 1 > R.ny - 1 || q[2] - r - 1 < 0 ||
	         q[2] + r + 1 > R.nz - 1)
		status = 2;
	if (status != kRun) {  // uniform: the whole workgroup leaves
		if (tid == 0) {
			S->status = status;
			write_result(out + poi, p0, 0.0, 0.0, 0, status);
		}
		return;
	}
	const int D = 2 * r + 1, N = D * D * D;
	const SubsetWalk W(r);
	const float *Rq = R.d + vidx(R, q[0], q[1], q[2]);
	const int sy = R.nx, sz = R.nx * R.ny;
	const double Rm = subset_mean(R, q, r, red);
	const float rmf = (float)Rm;
	// a pass per component a: sum SD and sum SD R' of its ten terms (and, kept from a = 0, dR^2 and sum R')
#pragma unroll 1
	for (int a = 0; a < 3; a++) {
		double acc[kCompSums];
#pragma unroll
		for (int k = 0; k < kCompSums; k++) acc[k] = 0.0;
		const int ga = a == 0 ? 1 : (a == 1 ? sy : sz);
		int dx, dy, dz;
		W.start(tid, dx, dy, dz);
		for (int i = tid; i < N; i += kThreads) {
			const float *c = Rq + (dz * sz + dy * sy + dx);
			const double g = (double)(0.5f * (c[ga] - c[-ga]));
			const double rv = (double)c[0] - Rm;
			const double x = dx, y = dy, z = dz;
			const double v[10] = {1.0, x, y, z, 0.5 * (x * x), 0.5 * (y * y), 0.5 * (z * z), x * y, x * z, y * z};
#pragma unroll
			for (int k = 0; k < 10; k++) {
				acc[k] += g * v[k];
				acc[10 + k] += (g * v[k]) * rv;
			}
			acc[20] += rv * rv;
			acc[21] += (double)(c[0] - rmf);
			W.next(dx, dy, dz);
		}
#pragma unroll
		for (int k = 0; k < kCompSums; k++) {
			const double x = wave_sum(acc[k]);
			if (lane == 0) red[wv][k] = x;
		}
		__syncthreads();
		if (tid < kCompSums) {
			const double t = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
			if (tid < 10) sums[2 + 10 * a + tid] = t;
			else if (tid < 20) sums[2 + kP + 10 * a + (tid - 10)] = t;
			else if (a == 0) sums[tid - 20] = t;
		}
		__syncthreads();
	}
	// a pass per gradient pair (0,0) (0,1) (0,2) (1,1) (1,2) (2,2): sum g_a g_b dx^i dy^j dz^k, i + j + k <= 4
#pragma unroll 1
	for (int pp = 0; pp < 6; pp++) {
		const int a = pp < 3 ? 0 : (pp < 5 ? 1 : 2), b = pp < 3 ? pp : (pp < 5 ? pp - 2 : 2);
		const int ga = a == 0 ? 1 : (a == 1 ? sy : sz), gb = b == 0 ? 1 : (b == 1 ? sy : sz);
		double acc[kMono];
#pragma unroll
		for (int k = 0; k < kMono; k++) acc[k] = 0.0;
		int dx, dy, dz;
		W.start(tid, dx, dy, dz);
		for (int i = tid; i < N; i += kThreads) {
			const float *c = Rq + (dz * sz + dy * sy + dx);
			const double w = (double)(0.5f * (c[ga] - c[-ga])) * (double)(0.5f * (c[gb] - c[-gb]));
			double px[5], py[5], pz[5];
			px[0] = py[0] = pz[0] = 1.0;
#pragma unroll
			for (int e = 1; e < 5; e++) {
				px[e] = px[e - 1] * (double)dx;
				py[e] = py[e - 1] * (double)dy;
				pz[e] = pz[e - 1] * (double)dz;
			}
			int at = 0;
#pragma unroll
			for (int ei = 0; ei < 5; ei++)
#pragma unroll
				for (int ej = 0; ej < 5 - ei; ej++)
#pragma unroll
					for (int ek = 0; ek < 5 - ei - ej; ek++, at++) acc[at] += w * ((px[ei] * py[ej]) * pz[ek]);
			W.next(dx, dy, dz);
		}
#pragma unroll
		for (int k = 0; k < kMono; k++) {
			const double x = wave_sum(acc[k]);
			if (lane == 0) red[wv][k] = x;
		}
		__syncthreads();
		if (tid < kMono) hp[pp][tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
		__syncthreads();
	}
	const double dr = sqrt(sums[0]);
	for (int e = tid; e < kP * kP; e += kThreads) {
		const int i = e / kP, j = e % kP;
		int a = i / 10, b = j / 10;
		const int ki = i % 10, kj = j % 10;
		if (a > b) { const int t = a; a = b; b = t; }
		const int pp = a == 0 ? b : (a == 1 ? 2 + b : 5);
		A[i][j] = hp[pp][mono_index(term_ex(ki) + term_ex(kj), term_ey(ki) + term_ey(kj), term_ez(ki) + term_ez(kj))] * (term_half(ki) * term_half(kj));
	}
	if (cholesky_lds<kP>(A, &s_fail, !(dr > 0.0))) {
		if (tid == 0) {
			S->status = 4;
			write_result(out + poi, p0, 0.0, 0.0, 0, 4);
		}
		return;
	}
	// H^-1: thread c solves L y = e_c, then L^T x = y, in its column of Y
	if (tid < kP) {
		const int c = tid;
		for (int i = 0; i < kP; i++) {
			double t = (i == c) ? 1.0 : 0.0;
			for (int j = 0; j < i; j++) t -= A[i][j] * Y[j][c];
			Y[i][c] = t / A[i][i];
		}
		for (int i = kP - 1; i >= 0; i--) {
			double t = Y[i][c];
			for (int j = i + 1; j < kP; j++) t -= A[j][i] * Y[j][c];
			Y[i][c] = t / A[i][i];
		}
		S->c2[c] = sums[2 + c];
		S->c1[c] = sums[2 + kP + c];
	}
	__syncthreads();
	for (int e = tid; e < kTri; e += kThreads) {
		int i = 0;
		while ((i + 1) * (i + 2) / 2 <= e) i++;
		S->hinv[e] = Y[i][e - i * (i + 1) / 2];
	}
	if (tid == 0) {
		bool dom = true;
		for (int a = 0; a < 3; a++) {
			double e[10];
			for (int k = 0; k < 10; k++) e[k] = p0 ? p0[10 * a + k] : 0.0;
			dom = axis_in_domain(e, a, q[a], r, a == 0 ? T.nx : (a == 1 ? T.ny : T.nz), cubic) && dom;
		}
		S->dr = dr;
		S->sr = sums[1];
		S->rm = rmf;
		S->status = dom ? kRun : 3;
		if (!dom) write_result(out + poi, p0, 0.0, 0.0, 0, 3);
	}
}

// ---- iterate ---------------------------------------------------------------------------------------------------------------------

// a value every lane holds alike, moved to a scalar register: the 30 fp32 warp coefficients stay out of the vector registers
__device__ inline float uniform(float x) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(x))); }

// one pass over the subset at the warp p (LDS): the wave sums of the 33 sums go to red, which the caller reads behind a barrier.  T is
// shifted by Tc as in the first-order kernel (kernels_icgn.hip, subset_pass).  Returns Tc - (float)Rm.
template <int KIND>
__device__ inline double subset_pass(const IcgnVol &R, const IcgnVol &T, const int q[3], int r, float rmf, const double *p,
                                   double (*red)[kIterSums]) {
	constexpr bool CUBIC = KIND != kLinear;
	const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
	const int D = 2 * r + 1, N = D * D * D;
	const SubsetWalk W(r);
	// position of offset d: (c + d) + o(d), c = floor(q + u) and d integers, o = frac(q + u) + (F - I) d + the quadratic part in fp32:
	// with d kept out of the fp32 sum, o stays of the order of 1 and carries the position to 1e-7 voxel at every radius (F d itself
	// would cost an ulp of |d|, which the 30-parameter solve of a small subset amplifies)
	int ci[3];
	float cf[3], F[9], Q[18];
#pragma unroll
	for (int a = 0; a < 3; a++) {
		const double c = (double)q[a] + p[10 * a];
		const double fl = floor(c);
		ci[a] = (int)fl;
		cf[a] = uniform((float)(c - fl));
#pragma unroll
		for (int b = 0; b < 3; b++) F[3 * a + b] = uniform((float)p[10 * a + 1 + b]);
#pragma unroll
		for (int k = 0; k < 6; k++) Q[6 * a + k] = uniform((float)p[10 * a + 4 + k]);
	}
	const int lo = CUBIC ? 1 : 0;
	const int hx = T.nx - (CUBIC ? 3 : 2), hy = T.ny - (CUBIC ? 3 : 2), hz = T.nz - (CUBIC ? 3 : 2);
	const size_t tsy = (size_t)T.nx, tsz = (size_t)T.nx * T.ny;
	const float *Rq = R.d + vidx(R, q[0], q[1], q[2]);
	const int sy = R.nx, sz = R.nx * R.ny;
	const float tc = T.d[vidx(T, min(max(ci[0], lo), hx), min(max(ci[1], lo), hy), min(max(ci[2], lo), hz))];
	double acc[kP];
#pragma unroll
	for (int k = 0; k < kP; k++) acc[k] = 0.0;
	float rt = 0.f;  // sum R'T': zncc only
	double sT = 0.0, sTT = 0.0;
	int dx, dy, dz;
	W.start(tid, dx, dy, dz);
#pragma unroll 1
	for (int i = tid; i < N; i += kThreads) {
		const float fx = (float)dx, fy = (float)dy, fz = (float)dz;
		// xi'(d): exact in fp32 (|d| <= 32)
		const float mo[10] = {1.f, fx, fy, fz, 0.5f * (fx * fx), 0.5f * (fy * fy), 0.5f * (fz * fz), fx * fy, fx * fz, fy * fz};
		float o[3];
#pragma unroll
		for (int a = 0; a < 3; a++) {
			const float *Qa = Q + 6 * a;
			const float lin = (F[3 * a] * fx + F[3 * a + 1] * fy) + F[3 * a + 2] * fz;
			const float quad = ((((Qa[0] * mo[4] + Qa[1] * mo[5]) + Qa[2] * mo[6]) + Qa[3] * mo[7]) + Qa[4] * mo[8]) + Qa[5] * mo[9];
			o[a] = cf[a] + (lin + quad);
		}
		const int cd[3] = {ci[0] + dx, ci[1] + dy, ci[2] + dz};
		const float tp = sample_shifted<KIND>(T, cd, o, tc, lo, hx, hy, hz, tsy, tsz);
		const float *c = Rq + (dz * sz + dy * sy + dx);
		const float g[3] = {0.5f * (c[1] - c[-1]), 0.5f * (c[sy] - c[-sy]), 0.5f * (c[sz] - c[-sz])};
		const float rp = c[0] - rmf;
		sT += (double)tp;
		sTT = fma((double)tp, (double)tp, sTT);
		const double td = (double)tp, xd = (double)dx, yd = (double)dy, zd = (double)dz;
		rt = fmaf(rp, tp, rt);
#pragma unroll
		for (int a = 0; a < 3; a++) {
			// fp64 products and sums: g T' is exact, so the fp32 rounding stays a perturbation of T' (which the least-squares solve
			// damps by 1 / sigma_min(SD)); a rounded product enters b directly and is amplified by 1 / lambda_min(H)
			const double gt = (double)g[a] * td, gx = gt * xd, gy = gt * yd, gz = gt * zd;
			double *A = acc + 10 * a;
			A[0] += gt;
			A[1] += gx;
			A[2] += gy;
			A[3] += gz;
			A[4] = fma(0.5 * gx, xd, A[4]);
			A[5] = fma(0.5 * gy, yd, A[5]);
			A[6] = fma(0.5 * gz, zd, A[6]);
			A[7] = fma(gx, yd, A[7]);
			A[8] = fma(gx, zd, A[8]);
			A[9] = fma(gy, zd, A[9]);
		}
		W.next(dx, dy, dz);
	}
	{
		const double x = wave_sum(sT), y = wave_sum(sTT);
		if (lane == 0) {
			red[wv][0] = x;
			red[wv][1] = y;
		}
	}
#pragma unroll
	for (int k = 0; k <= kP; k++) {
		const double x = wave_sum(k < kP ? acc[k] : (double)rt);
		if (lane == 0) red[wv][2 + k] = x;
	}
	return (double)tc - (double)rmf;
}

// A B as polynomials in (1, dx, dy, dz, dx^2, dy^2, dz^2, dx dy, dx dz, dy dz), the terms of degree 3 and 4 dropped
__device__ inline void truncated_product(const double A[10], const double B[10], double o[10]) {
	o[0] = A[0] * B[0];
#pragma unroll
	for (int k = 1; k <= 3; k++) {
		o[k] = A[0] * B[k] + A[k] * B[0];
		o[3 + k] = (A[0] * B[3 + k] + A[3 + k] * B[0]) + A[k] * B[k];
	}
	o[7] = (A[0] * B[7] + A[7] * B[0]) + (A[1] * B[2] + A[2] * B[1]);
	o[8] = (A[0] * B[8] + A[8] * B[0]) + (A[1] * B[3] + A[3] * B[1]);
	o[9] = (A[0] * B[9] + A[9] * B[0]) + (A[2] * B[3] + A[3] * B[2]);
}

// wave 0, all 64 lanes: the step dp (LDS) -> its norm, M(dp), the LU, p <- the parameters of M(p) M(dp)^-1, the domain test.
// Leaves s_ctl = 0 and the new p in s_p, or s_ctl = 6 / 3 and s_p as it was; s_last in every case.
__device__ inline void compose_in_wave(const double *s_dp, double *s_p, double *s_last, int *s_ctl, const int q[3], int r, const IcgnVol &T,
                                       bool cubic) {
	const int lane = threadIdx.x & 63;
	double cd[3][10];  // the position polynomials of dp: e_{1+a} + the terms, the squares with their 1/2
	bool fin = true;
	double n0 = 0.0, n1 = 0.0, n2 = 0.0, n3 = 0.0;
#pragma unroll
	for (int a = 0; a < 3; a++)
#pragma unroll
		for (int k = 0; k < 10; k++) {
			const double v = s_dp[10 * a + k];
			fin = fin && isfinite(v);
			if (k == 0) n0 += v * v;
			else if (k < 4) n1 += v * v;
			else if (k < 7) n2 += v * v;
			else n3 += v * v;
			cd[a][k] = (k >= 4 && k <= 6 ? 0.5 * v : v) + (k == 1 + a ? 1.0 : 0.0);
		}
	const double r2 = (double)r * (double)r;
	const double last = sqrt((n0 + r2 * n1) + (r2 * r2) * (0.25 * n2 + n3));
	if (!fin) {
		if (lane == 0) {
			*s_last = last;
			*s_ctl = 6;
		}
		return;
	}
	// row `lane` of M(dp) (lanes >= 10 carry row 0 and are never read)
	double m[10];
	{
		const int i = lane < 10 ? lane : 0, n = i - 4;
		const int ia = i < 4 ? (i > 0 ? i - 1 : 0) : (n < 3 ? n : (n == 5 ? 1 : 0)), ib = i < 4 ? ia : (n < 3 ? n : (n == 3 ? 1 : 2));
		double A[10], B[10], P[10];
#pragma unroll
		for (int k = 0; k < 10; k++) {
			A[k] = ia == 0 ? cd[0][k] : (ia == 1 ? cd[1][k] : cd[2][k]);
			B[k] = ib == 0 ? cd[0][k] : (ib == 1 ? cd[1][k] : cd[2][k]);
		}
		truncated_product(A, B, P);
#pragma unroll
		for (int k = 0; k < 10; k++) m[k] = i == 0 ? (k == 0 ? 1.0 : 0.0) : (i < 4 ? A[k] : P[k]);
	}
	// P M = L U, partial pivoting: the first entry of largest magnitude in the column (a NaN is never larger); every choice is uniform
	int perm = lane;
	bool singular = false;
#pragma unroll
	for (int k = 0; k < 10; k++) {
		if (singular) break;
		double best = -1.0;
		int bi = k;
#pragma unroll
		for (int i = k; i < 10; i++) {
			const double v = fabs(__shfl(m[k], i));
			if (v > best) {
				best = v;
				bi = i;
			}
		}
		if (bi != k) {
			const int src = lane == k ? bi : (lane == bi ? k : lane);
#pragma unroll
			for (int j = 0; j < 10; j++) m[j] = __shfl(m[j], src);
			perm = __shfl(perm, src);
		}
		const double pv = __shfl(m[k], k);
		if (!(pv != 0.0) || !isfinite(pv)) {
			singular = true;
		} else {
			double pr[10];
#pragma unroll
			for (int j = k + 1; j < 10; j++) pr[j] = __shfl(m[j], k);
			if (lane > k) {
				const double l = m[k] / pv;
				m[k] = l;
#pragma unroll
				for (int j = k + 1; j < 10; j++) m[j] = m[j] - l * pr[j];
			}
		}
	}
	if (singular) {
		if (lane == 0) {
			*s_last = last;
			*s_ctl = 6;
		}
		return;
	}
	// lane a < 3: x M(dp) = row 1 + a of M(p), i.e. (x P^T) L U = b
	const int a = lane < 3 ? lane : 0;
	double z[10], y[10], x[10];
#pragma unroll
	for (int j = 0; j < 10; j++) {
		double t = s_p[10 * a + j] * (j >= 4 && j <= 6 ? 0.5 : 1.0) + (j == 1 + a ? 1.0 : 0.0);
#pragma unroll
		for (int i = 0; i < j; i++) t -= z[i] * __shfl(m[j], i);
		z[j] = t / __shfl(m[j], j);
	}
#pragma unroll
	for (int j = 9; j >= 0; j--) {
		double t = z[j];
#pragma unroll
		for (int i = j + 1; i < 10; i++) t -= y[i] * __shfl(m[j], i);
		y[j] = t;
	}
#pragma unroll
	for (int c = 0; c < 10; c++) x[c] = 0.0;
#pragma unroll
	for (int i = 0; i < 10; i++) {
		const int pm = __shfl(perm, i);
#pragma unroll
		for (int c = 0; c < 10; c++) x[c] = pm == c ? y[i] : x[c];
	}
	double pn[10];
#pragma unroll
	for (int k = 0; k < 10; k++) {
		const double v = x[k] - (k == 1 + a ? 1.0 : 0.0);
		pn[k] = (k >= 4 && k <= 6) ? 2.0 * v : v;
	}
	const bool ok = axis_in_domain(pn, a, a == 0 ? q[0] : (a == 1 ? q[1] : q[2]), r, a == 0 ? T.nx : (a == 1 ? T.ny : T.nz), cubic);
	const bool all = (__ballot(ok) & 7ull) == 7ull;
	if (all && lane < 3) {
#pragma unroll
		for (int k = 0; k < 10; k++) s_p[10 * a + k] = pn[k];
	}
	if (lane == 0) {
		*s_last = last;
		*s_ctl = all ? 0 : 3;
	}
}

template <int KIND>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(2))) void k_icgn2_iterate(IcgnVol R, IcgnVol T, const int *__restrict__ pts, const double *__restrict__ init,
                                                           int r, int max_it, double tol, const Icgn2State *__restrict__ state,
                                                           sift3d_icgn2_result *__restrict__ out) {
	__shared__ double red[kWaves][kIterSums];
	__shared__ double cst[kTri + 2 * kP + 2];  // H^-1, c1, c2, dR, sum R': read after each pass, not held in registers across it
	__shared__ double s_p[kP], s_b[kP], s_dp[kP];
	__shared__ double s_last;
	__shared__ int s_ctl;
	const int poi = blockIdx.x, tid = threadIdx.x;
	const Icgn2State *S = state + poi;
	if (S->status != kRun) return;  // the prepare kernel wrote the result
	for (int e = tid; e < kTri + 2 * kP; e += kThreads) cst[e] = e < kTri ? S->hinv[e] : (e < kTri + kP ? S->c1[e - kTri] : S->c2[e - kTri - kP]);
	if (tid < kP) s_p[tid] = init ? init[kP * (size_t)poi + tid] : 0.0;
	if (tid == 0) {
		cst[kTri + 2 * kP] = S->dr;
		cst[kTri + 2 * kP + 1] = S->sr;
		s_last = 0.0;
	}
	__syncthreads();
	const int q[3] = {pts[3 * poi], pts[3 * poi + 1], pts[3 * poi + 2]};
	const float rmf = S->rm;
	int it = 0, status = kRun;
	bool done = false;
	for (;;) {
		const double sh = subset_pass<KIND>(R, T, q, r, rmf, s_p, red);
		__syncthreads();
		const double N = (double)((2 * r + 1) * (2 * r + 1) * (2 * r + 1)), dr = cst[kTri + 2 * kP], sr = cst[kTri + 2 * kP + 1];
		const double s0 = ((red[0][0] + red[1][0]) + red[2][0]) + red[3][0], s1 = ((red[0][1] + red[1][1]) + red[2][1]) + red[3][1];
		const double srt = ((red[0][2 + kP] + red[1][2 + kP]) + red[2][2 + kP]) + red[3][2 + kP];
		const double tm = s0 / N;
		const double dt2 = s1 - s0 * tm;
		const double ttm = (s1 + 2.0 * sh * s0) + (N * sh) * sh;  // sum (T - Rm)^2 from the sums of T' = T - Tc
		const bool flat = !(dt2 > 1e-10 * ttm);  // dT = 0 to rounding
		const double dt = flat ? 0.0 : sqrt(dt2);
		const double zncc = flat ? 0.0 : (srt - tm * sr) / (dr * dt);
		if (done || flat) {
			if (tid == 0) write_result(out + poi, s_p, done ? zncc : 0.0, s_last, it, done ? status : 4);
			return;
		}
		if (tid < kP) {
			const double sj = ((red[0][2 + tid] + red[1][2 + tid]) + red[2][2 + tid]) + red[3][2 + tid];
			s_b[tid] = cst[kTri + tid] - (dr / dt) * (sj - tm * cst[kTri + kP + tid]);
		}
		__syncthreads();
		if (tid < kP) {
			double t = 0.0;
			for (int j = 0; j < kP; j++) t += cst[tid >= j ? tid * (tid + 1) / 2 + j : j * (j + 1) / 2 + tid] * s_b[j];
			s_dp[tid] = -t;
		}
		__syncthreads();
		if (tid < 64) compose_in_wave(s_dp, s_p, &s_last, &s_ctl, q, r, T, KIND != kLinear);
		__syncthreads();
		const double last = s_last;
		const int ctl = s_ctl;
		if (ctl != 0) {
			if (tid == 0) write_result(out + poi, s_p, zncc, last, it, ctl);
			return;
		}
		it++;
		if (last < tol) {
			status = 0;
			done = true;
		} else if (it >= max_it) {
			status = 1;
			done = true;
		}
	}
}

}  // namespace

size_t icgn2_state_bytes() { return sizeof(Icgn2State); }

void launch_icgn2(IcgnVol R, IcgnVol T, const int *d_pts, int m, const double *d_init, int r, int max_it, double tol, int kind, void *d_state,
                  sift3d_icgn2_result *d_out, hipStream_t st) {
	Icgn2State *S = static_cast<Icgn2State *>(d_state);
	hipLaunchKernelGGL(k_icgn2_prepare, dim3(m), dim3(kThreads), 0, st, R, T, d_pts, d_init, r, kind != kLinear, S, d_out);
	hipLaunchKernelGGL(by_kind(kind, k_icgn2_iterate<kKeys>, k_icgn2_iterate<kLinear>, k_icgn2_iterate<kBspline>), dim3(m), dim3(kThreads), 0, st, R,
	                   T, d_pts, d_init, r, max_it, tol, S, d_out);
}

}  // namespace s3d
