// kernels_icgn.hip -- IC-GN displacement refinement (sift3d_icgn, include/sift3d_hip.h, which states the numerical contract).
// No reference counterpart.  One workgroup of 256 threads per point of interest (POI), two launches on one stream:
//   k_icgn_prepare  the status 5 / 2 / 4 / 3 checks, Rm, dR and the constants of the subset: sum SD^T (R - Rm), sum SD^T and
//                   H = sum SD^T SD (60 distinct sums: 6 gradient pairs x 10 monomials of (1, dx, dy, dz)), all accumulated in fp64;
//                   the 12 x 12 fp64 Cholesky of H in LDS (a column per step, the trailing update spread over the workgroup) and
//                   H^-1 by 12 column solves; a record per POI (IcgnState) for the second launch
//   k_icgn_iterate  every iteration inside the launch: one pass over the subset per iteration gathers 15 sums at the current warp
//                   (sum T', sum T'^2, sum R'T' and the 12 sums SD^T T', with T' = T(W) - Tc and R' = R - Rm; Tc: T's voxel under the subset centre), reduced in a fixed
//                   order (xor butterfly in the wave, waves in index order); every thread then forms the same step from the sums
//                   (fp64, redundantly: no broadcast and one barrier per pass), composes the warp, tests convergence and the 8 corners.
//                   The pass after the last update gives zncc at the returned p.
// SD is recomputed per voxel from R (6 cached loads; a 12-float table per voxel does not fit in LDS at r = 16).  Per-voxel arithmetic is
// fp32 (positions relative to floor(q + u), so the fraction keeps its bits); per-thread sums are fp32 except sum T' and sum T'^2
// (fp64: the variance is their difference); the reduction is fp64.  No float atomics: two calls give the same bits.
// sift3d_icgn_bspline runs the same two launches with the cubic B-spline weights on the prefiltered T (kernels_bspline.hip): the
// third instantiation of k_icgn_iterate.
// sift3d_icgn_masked runs the MASKED instantiations of both kernels behind k_mask_active: every sum skips the voxels that are not
// active (one byte load per voxel and pass; a wave whose voxels are all inactive branches over the body), the walk is the unmasked
// one, and the active count n of a POI -- an int per POI beside the state records, IcgnState keeps its size -- takes N's place.  The
// unmasked instantiations are the kernels as they were: every masked piece stands under `if constexpr`.
// sift3d_icgn_labelled runs the masked instantiations once more with an IcgnLabels in the IcgnMask's place: the volume read per
// voxel and pass is the int volume of interior labels (k_label_interior) and the test is `== L_i`, the label under the POI's own
// voxel, which the prepare kernel reads once, leaves beside the active counts and the iterate kernel reads back.  The kind of the
// last kernel argument tells the two apart, so the byte-masked instantiations keep their names and their code.
#include "icgn_subset.h"

#include <math.h>

#include <type_traits>

namespace s3d {
namespace {

using namespace icgn;

constexpr int kPrepSums = 86;  // dR^2, sum R', 12 sum SD, 12 sum SD R', 60 H pieces
constexpr int kIterSums = 15;  // sum T', sum T'^2, 12 sum SD T', sum R'T' (T' = T - Tc)

struct IcgnState {
	double hinv[144];  // H^-1, row-major
	double c1[12];     // sum SD^T (R - Rm)
	double c2[12];     // sum SD^T
	double dr;         // dR
	double sr;         // sum (R - Rm) as the iterate kernel forms R' (fp32 R - (float)Rm): zncc's correction term
	float rm;          // (float)Rm, the shift of T and R in the iterate kernel
	int status;        // kRun, or the final status the prepare kernel wrote
};

// the position of the subset offset d under p (fp64, the contract's order): q + F d + (u, v, w)
__device__ inline void warp_point(const double p[12], const int q[3], double dx, double dy, double dz, double o[3]) {
#pragma unroll
	for (int a = 0; a < 3; a++) {
		const double *g = p + 4 * a;
		const double fx = (a == 0 ? 1.0 + g[1] : g[1]), fy = (a == 1 ? 1.0 + g[2] : g[2]), fz = (a == 2 ? 1.0 + g[3] : g[3]);
		o[a] = ((double)q[a] + ((fx * dx + fy * dy) + fz * dz)) + g[0];
	}
}

// every tap of the warped subset inside T: the 8 corners decide (a NaN position is outside)
__device__ inline bool in_domain(const double p[12], const int q[3], int r, const IcgnVol &T, bool cubic) {
	const int n[3] = {T.nx, T.ny, T.nz};
	bool ok = true;
#pragma unroll
	for (int c = 0; c < 8; c++) {
		double o[3];
		warp_point(p, q, (c & 1) ? r : -r, (c & 2) ? r : -r, (c & 4) ? r : -r, o);
#pragma unroll
		for (int a = 0; a < 3; a++) {
			const double f = floor(o[a]);
			ok = ok && (cubic ? (f - 1.0 >= 0.0 && f + 2.0 <= (double)(n[a] - 1)) : (f >= 0.0 && f + 1.0 <= (double)(n[a] - 1)));
		}
	}
	return ok;
}

__device__ inline void write_result(sift3d_icgn_result *o, const double p[12], double zncc, double last, int it, int status) {
#pragma unroll
	for (int k = 0; k < 12; k++) o->p[k] = p[k];
	o->zncc = zncc;
	o->last_step = last;
	o->iterations = it;
	o->status = status;
	o->reserved[0] = o->reserved[1] = 0;
}

// ---- prepare ---------------------------------------------------------------------------------------------------------------------

__device__ inline int h_piece(int i, int j) {  // H(i, j) -> index into the 60 H pieces
	int a = i >> 2, b = j >> 2, mi = i & 3, mj = j & 3;
	if (a > b) { int t = a; a = b; b = t; }
	if (mi > mj) { int t = mi; mi = mj; mj = t; }
	const int pp = a == 0 ? b : (a == 1 ? 2 + b : 5);                          // (0,0) (0,1) (0,2) (1,1) (1,2) (2,2)
	const int mm = mi == 0 ? mj : (mi == 1 ? 3 + mj : (mi == 2 ? 5 + mj : 9));  // (0,0..3) (1,1..3) (2,2..3) (3,3)
	return pp * 10 + mm;
}

// The masked instantiations take one more kernel argument, the IcgnMask; the unmasked ones take none (MASK is empty), so their
// signature and kernel-argument segment are what they were.
__device__ inline IcgnMask mask_of() { return IcgnMask{nullptr, nullptr, 0.f}; }
__device__ inline IcgnMask mask_of(IcgnMask m) { return m; }
__device__ inline IcgnLabels mask_of(IcgnLabels m) { return m; }
// the volume a masked form tests per voxel: the active bytes, or the interior labels
__device__ inline const unsigned char *active_of(const IcgnMask &m) { return m.act; }
__device__ inline const int *active_of(const IcgnLabels &m) { return m.interior; }
template <class... MASK>
constexpr bool kLabelled = (std::is_same<MASK, IcgnLabels>::value || ...);

template <bool MASKED, class... MASK>
__global__ __launch_bounds__(kThreads) void k_icgn_prepare(IcgnVol R, IcgnVol T, const int *__restrict__ pts, const double *__restrict__ init,
                                                          int r, int cubic, IcgnState *__restrict__ state, sift3d_icgn_result *__restrict__ out,
                                                          MASK... mask) {
	static_assert(sizeof...(MASK) == (MASKED ? 1 : 0), "the masked instantiation takes the IcgnMask");
	constexpr bool LABELLED = kLabelled<MASK...>;
	const auto M = mask_of(mask...);
	typedef typename std::remove_cv<typename std::remove_pointer<decltype(active_of(M))>::type>::type Act;  // a byte, or an int label
	__shared__ double red[kWaves][kPrepSums];
	__shared__ double A[12][13];
	__shared__ int s_fail;
	const int poi = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
	const int q[3] = {pts[3 * poi], pts[3 * poi + 1], pts[3 * poi + 2]};
	double p[12];
	bool finite = true;
#pragma unroll
	for (int k = 0; k < 12; k++) {
		p[k] = init ? init[12 * (size_t)poi + k] : 0.0;
		finite = finite && isfinite(p[k]);
	}
	IcgnState *S = state + poi;
	Act want = 0;  // labelled: L_i, the label under q (0 outside R); uniform, one scalar load
	if constexpr (LABELLED) {
		if (q[0] >= 0 && q[0] < R.nx && q[1] >= 0 && q[1] < R.ny && q[2] >= 0 && q[2] < R.nz) want = M.labels[vidx(R, q[0], q[1], q[2])];
		if (tid == 0) M.label[poi] = want;
	}
	int status = kRun;
	if (!finite) status = 5;
	else if (q[0] - r - 1 < 0 || q[0] + r + 1 > R.nx - 1 || q[1] - r - 1 < 0 || q[1] + r + 1 > R.ny - 1 || q[2] - r - 1 < 0 ||
	         q[2] + r + 1 > R.nz - 1)
		status = 2;
	if (status != kRun) {  // uniform: the whole workgroup leaves
		if (tid == 0) {
			S->status = status;
			write_result(out + poi, p, 0.0, 0.0, 0, status);
			if constexpr (MASKED) M.n[poi] = 0;  // no voxel is read
		}
		return;
	}
	const int D = 2 * r + 1, N = D * D * D;
	const SubsetWalk W(r);
	const float *Rq = R.d + vidx(R, q[0], q[1], q[2]);
	const int sy = R.nx, sz = R.nx * R.ny;
	// pass 1: Rm (masked: and the active count, status 7)
	const Act *Aq = MASKED ? active_of(M) + vidx(R, q[0], q[1], q[2]) : nullptr;
	int n = N;
	if constexpr (LABELLED) {
		if (want <= 0) {  // uniform: no body under q, n = 0 and no voxel is read
			if (tid == 0) {
				M.n[poi] = 0;
				S->status = 7;
				write_result(out + poi, p, 0.0, 0.0, 0, 7);
			}
			return;
		}
	}
	const double Rm = subset_mean<kPrepSums, MASKED, Act>(R, q, r, red, Aq, &n, want);
	if constexpr (MASKED) {
		const bool few = n == 0 || (double)n < (double)M.min_fraction * (double)N;  // uniform: every thread holds the same n
		if (tid == 0) {
			M.n[poi] = n;
			if (few) {
				S->status = 7;
				write_result(out + poi, p, 0.0, 0.0, 0, 7);
			}
		}
		if (few) return;
	}
	const float rmf = (float)Rm;
	// pass 2: the constants
	double acc[kPrepSums];
#pragma unroll
	for (int k = 0; k < kPrepSums; k++) acc[k] = 0.0;
	{
		int dx, dy, dz;
		W.start(tid, dx, dy, dz);
		for (int i = tid; i < N; i += kThreads) {
			bool on = true;
			if constexpr (MASKED) on = voxel_on(Aq[dz * sz + dy * sy + dx], want);
			if (on) {
				const float *c = Rq + (dz * sz + dy * sy + dx);
				const float gxf = 0.5f * (c[1] - c[-1]), gyf = 0.5f * (c[sy] - c[-sy]), gzf = 0.5f * (c[sz] - c[-sz]);
				const double rv = (double)c[0] - Rm;
				const double g[3] = {(double)gxf, (double)gyf, (double)gzf};
				const double v[4] = {1.0, (double)dx, (double)dy, (double)dz};
				acc[0] += rv * rv;
				acc[1] += (double)(c[0] - rmf);
#pragma unroll
				for (int a = 0; a < 3; a++)
#pragma unroll
					for (int k = 0; k < 4; k++) {
						acc[2 + 4 * a + k] += g[a] * v[k];
						acc[14 + 4 * a + k] += (g[a] * v[k]) * rv;
					}
				int pp = 0;
#pragma unroll
				for (int a = 0; a < 3; a++)
#pragma unroll
					for (int b = a; b < 3; b++, pp++) {
						const double w = g[a] * g[b];
						int mm = 0;
#pragma unroll
						for (int mi = 0; mi < 4; mi++)
#pragma unroll
							for (int mj = mi; mj < 4; mj++, mm++) acc[26 + pp * 10 + mm] += w * (v[mi] * v[mj]);
					}
			}
			W.next(dx, dy, dz);
		}
	}
#pragma unroll
	for (int k = 0; k < kPrepSums; k++) {
		const double x = wave_sum(acc[k]);
		if (lane == 0) red[wv][k] = x;
	}
	__syncthreads();
	if (tid < kPrepSums) red[0][tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
	__syncthreads();
	const double dr = sqrt(red[0][0]);
	if (tid < 144) {
		const int i = tid / 12, j = tid % 12;
		A[i][j] = red[0][26 + h_piece(i, j)];
	}
	if (cholesky_lds<12>(A, &s_fail, !(dr > 0.0))) {
		if (tid == 0) {
			S->status = 4;
			write_result(out + poi, p, 0.0, 0.0, 0, 4);
		}
		return;
	}
	// H^-1: thread c solves L y = e_c, then L^T x = y in place (registers, fully unrolled)
	if (tid < 12) {
		const int c = tid;
		double y[12];
#pragma unroll
		for (int i = 0; i < 12; i++) {
			double t = (i == c) ? 1.0 : 0.0;
#pragma unroll
			for (int j = 0; j < i; j++) t -= A[i][j] * y[j];
			y[i] = t / A[i][i];
		}
#pragma unroll
		for (int i = 11; i >= 0; i--) {
			double t = y[i];
#pragma unroll
			for (int j = i + 1; j < 12; j++) t -= A[j][i] * y[j];
			y[i] = t / A[i][i];
		}
#pragma unroll
		for (int i = 0; i < 12; i++) S->hinv[12 * i + c] = y[i];
		S->c2[c] = red[0][2 + c];
		S->c1[c] = red[0][14 + c];
	}
	if (tid == 0) {
		const bool dom = in_domain(p, q, r, T, cubic);
		S->dr = dr;
		S->sr = red[0][1];
		S->rm = rmf;
		S->status = dom ? kRun : 3;
		if (!dom) write_result(out + poi, p, 0.0, 0.0, 0, 3);
	}
}

// ---- iterate ---------------------------------------------------------------------------------------------------------------------

// one pass over the subset at the warp p: the 15 sums, reduced (every thread returns the same values).  T is shifted by Tc, the voxel of T
// at the base tap of the subset's centre (any constant serves: ZNSSD does not change when T is shifted), and the taps are shifted
// before they are weighted: a constant T gives T' = 0 exactly, T scaled by a power of two scales T' exactly, and an offset common to
// the taps leaves the interpolation's rounding.  Tc is one voxel: an outlier there (a hot voxel |Tc - Tm| >> dT) makes every T' large
// and costs the fp32 sums that many ulps, as a T far brighter than R did under the shift by Rm; a mean of T would need a pass of its
// own.  Returns Tc - (float)Rm, which turns the sums into those of T - Rm.
// MASKED: Aq is the active byte of the voxel q; the body is skipped for an inactive voxel (neither R nor T is read there).  Labelled:
// Aq is the interior label of the voxel q and `want` the POI's label (voxel_on, icgn_subset.h).
template <int KIND, bool MASKED, class Act>
__device__ inline double subset_pass(const IcgnVol &R, const IcgnVol &T, const int q[3], int r, float rmf, const double p[12],
                                   double (*red)[kIterSums], double sums[kIterSums], const Act *Aq, Act want) {
	constexpr bool CUBIC = KIND != kLinear;  // 64 taps
	const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
	const int D = 2 * r + 1, N = D * D * D;
	const SubsetWalk W(r);
	// position of offset d: c + o(d), c = floor(q + u) (integer), o = frac(q + u) + F d in fp32
	int ci[3];
	float cf[3], F[9];
#pragma unroll
	for (int a = 0; a < 3; a++) {
		const double c = (double)q[a] + p[4 * a];
		const double fl = floor(c);
		ci[a] = (int)fl;
		cf[a] = (float)(c - fl);
#pragma unroll
		for (int b = 0; b < 3; b++) F[3 * a + b] = (float)((a == b ? 1.0 : 0.0) + p[4 * a + 1 + b]);
	}
	const int lo = CUBIC ? 1 : 0;
	const int hx = T.nx - (CUBIC ? 3 : 2), hy = T.ny - (CUBIC ? 3 : 2), hz = T.nz - (CUBIC ? 3 : 2);
	const size_t tsy = (size_t)T.nx, tsz = (size_t)T.nx * T.ny;
	const float *Rq = R.d + vidx(R, q[0], q[1], q[2]);
	const int sy = R.nx, sz = R.nx * R.ny;
	const float tc = T.d[vidx(T, min(max(ci[0], lo), hx), min(max(ci[1], lo), hy), min(max(ci[2], lo), hz))];
	float acc[13];
#pragma unroll
	for (int k = 0; k < 13; k++) acc[k] = 0.f;
	double sT = 0.0, sTT = 0.0;
	int dx, dy, dz;
	W.start(tid, dx, dy, dz);
#pragma unroll 1
	for (int i = tid; i < N; i += kThreads) {
		bool on = true;
		if constexpr (MASKED) on = voxel_on(Aq[dz * sz + dy * sy + dx], want);
		if (on) {
			const float fx = (float)dx, fy = (float)dy, fz = (float)dz;
			float o[3];
#pragma unroll
			for (int a = 0; a < 3; a++) o[a] = cf[a] + ((F[3 * a] * fx + F[3 * a + 1] * fy) + F[3 * a + 2] * fz);
			const float tv = sample_shifted<KIND>(T, ci, o, tc, lo, hx, hy, hz, tsy, tsz);
			const float *c = Rq + (dz * sz + dy * sy + dx);
			const float g[3] = {0.5f * (c[1] - c[-1]), 0.5f * (c[sy] - c[-sy]), 0.5f * (c[sz] - c[-sz])};
			const float tp = tv, rp = c[0] - rmf;
			sT += (double)tp;
			sTT = fma((double)tp, (double)tp, sTT);
			acc[12] = fmaf(rp, tp, acc[12]);
#pragma unroll
			for (int a = 0; a < 3; a++) {
				const float gt = g[a] * tp;
				acc[4 * a] += gt;
				acc[4 * a + 1] = fmaf(gt, fx, acc[4 * a + 1]);
				acc[4 * a + 2] = fmaf(gt, fy, acc[4 * a + 2]);
				acc[4 * a + 3] = fmaf(gt, fz, acc[4 * a + 3]);
			}
		}
		W.next(dx, dy, dz);
	}
	double v[kIterSums];
	v[0] = sT;
	v[1] = sTT;
#pragma unroll
	for (int k = 0; k < 13; k++) v[2 + k] = (double)acc[k];
#pragma unroll
	for (int k = 0; k < kIterSums; k++) {
		const double x = wave_sum(v[k]);
		if (lane == 0) red[wv][k] = x;
	}
	__syncthreads();
#pragma unroll
	for (int k = 0; k < kIterSums; k++) sums[k] = ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k];
	return (double)tc - (double)rmf;
}

template <int KIND, bool MASKED, class... MASK>
__global__ __launch_bounds__(kThreads) void k_icgn_iterate(IcgnVol R, IcgnVol T, const int *__restrict__ pts, const double *__restrict__ init,
                                                          int r, int max_it, double tol, const IcgnState *__restrict__ state,
                                                          sift3d_icgn_result *__restrict__ out, MASK... mask) {
	static_assert(sizeof...(MASK) == (MASKED ? 1 : 0), "the masked instantiation takes the IcgnMask");
	const auto M = mask_of(mask...);
	typedef typename std::remove_cv<typename std::remove_pointer<decltype(active_of(M))>::type>::type Act;
	__shared__ double red[2][kWaves][kIterSums];  // by pass parity: one barrier per pass
	__shared__ double cst[168];                   // H^-1, c1, c2: read in the solve only (not held in registers across the passes)
	const int poi = blockIdx.x;
	const IcgnState *S = state + poi;
	if (S->status != kRun) return;  // the prepare kernel wrote the result
	if (threadIdx.x < 168) cst[threadIdx.x] = threadIdx.x < 144 ? S->hinv[threadIdx.x] : (threadIdx.x < 156 ? S->c1[threadIdx.x - 144] : S->c2[threadIdx.x - 156]);
	__syncthreads();
	const int q[3] = {pts[3 * poi], pts[3 * poi + 1], pts[3 * poi + 2]};
	double p[12];
#pragma unroll
	for (int k = 0; k < 12; k++) p[k] = init ? init[12 * (size_t)poi + k] : 0.0;
	// (masked: N is the POI's active count, which the prepare kernel left beside the state records)
	const double N = MASKED ? (double)M.n[poi] : (double)((2 * r + 1) * (2 * r + 1) * (2 * r + 1)), dr = S->dr, sr = S->sr, r2 = (double)r * (double)r;
	const Act *Aq = MASKED ? active_of(M) + vidx(R, q[0], q[1], q[2]) : nullptr;
	Act want = 0;
	if constexpr (kLabelled<MASK...>) want = M.label[poi];  // (> 0: the prepare kernel ended every other POI)
	const float rmf = S->rm;
	int it = 0, status = kRun;
	double last = 0.0;
	bool done = false;
	for (int pass = 0;; pass++) {
		double s[kIterSums];
		const double sh = subset_pass<KIND, MASKED, Act>(R, T, q, r, rmf, p, red[pass & 1], s, Aq, want);
		// s: 0 sum T', 1 sum T'^2, 2..13 sum SD T', 14 sum R'T'
		const double tm = s[0] / N;
		const double dt2 = s[1] - s[0] * tm;
		const double ttm = (s[1] + 2.0 * sh * s[0]) + (N * sh) * sh;  // sum (T - Rm)^2 from the sums of T' = T - Tc
		const bool flat = !(dt2 > 1e-10 * ttm);  // dT = 0 to rounding
		const double dt = flat ? 0.0 : sqrt(dt2);
		const double zncc = flat ? 0.0 : (s[14] - tm * sr) / (dr * dt);
		if (done) {
			if (threadIdx.x == 0) write_result(out + poi, p, zncc, last, it, status);
			return;
		}
		if (flat) {
			if (threadIdx.x == 0) write_result(out + poi, p, 0.0, last, it, 4);
			return;
		}
		const double k = dr / dt;
		double b[12], dp[12];
#pragma unroll
		for (int j = 0; j < 12; j++) b[j] = cst[144 + j] - k * (s[2 + j] - tm * cst[156 + j]);
		bool fin = true;
#pragma unroll
		for (int i = 0; i < 12; i++) {
			double t = 0.0;
#pragma unroll
			for (int j = 0; j < 12; j++) t += cst[12 * i + j] * b[j];
			dp[i] = -t;
			fin = fin && isfinite(dp[i]);
		}
		double g2 = 0.0;
#pragma unroll
		for (int a = 0; a < 3; a++) g2 += (dp[4 * a + 1] * dp[4 * a + 1] + dp[4 * a + 2] * dp[4 * a + 2]) + dp[4 * a + 3] * dp[4 * a + 3];
		last = sqrt(((dp[0] * dp[0] + dp[4] * dp[4]) + dp[8] * dp[8]) + r2 * g2);
		// M(p) <- M(p) . M(dp)^-1: F <- F Fd^-1, t <- t - F Fd^-1 td
		double Fd[9], Fp[9], inv[9];
#pragma unroll
		for (int a = 0; a < 3; a++)
#pragma unroll
			for (int c = 0; c < 3; c++) {
				Fd[3 * a + c] = (a == c ? 1.0 : 0.0) + dp[4 * a + 1 + c];
				Fp[3 * a + c] = (a == c ? 1.0 : 0.0) + p[4 * a + 1 + c];
			}
		inv[0] = Fd[4] * Fd[8] - Fd[5] * Fd[7];
		inv[3] = -(Fd[3] * Fd[8] - Fd[5] * Fd[6]);
		inv[6] = Fd[3] * Fd[7] - Fd[4] * Fd[6];
		const double det = (Fd[0] * inv[0] + Fd[1] * inv[3]) + Fd[2] * inv[6];
		if (!fin || !(det != 0.0) || !isfinite(det)) {
			if (threadIdx.x == 0) write_result(out + poi, p, zncc, last, it, 6);
			return;
		}
		inv[1] = -(Fd[1] * Fd[8] - Fd[2] * Fd[7]);
		inv[4] = Fd[0] * Fd[8] - Fd[2] * Fd[6];
		inv[7] = -(Fd[0] * Fd[7] - Fd[1] * Fd[6]);
		inv[2] = Fd[1] * Fd[5] - Fd[2] * Fd[4];
		inv[5] = -(Fd[0] * Fd[5] - Fd[2] * Fd[3]);
		inv[8] = Fd[0] * Fd[4] - Fd[1] * Fd[3];
#pragma unroll
		for (int e = 0; e < 9; e++) inv[e] = inv[e] / det;
		double pn[12], ti[3];
#pragma unroll
		for (int a = 0; a < 3; a++) ti[a] = -((inv[3 * a] * dp[0] + inv[3 * a + 1] * dp[4]) + inv[3 * a + 2] * dp[8]);
#pragma unroll
		for (int a = 0; a < 3; a++) {
			pn[4 * a] = ((Fp[3 * a] * ti[0] + Fp[3 * a + 1] * ti[1]) + Fp[3 * a + 2] * ti[2]) + p[4 * a];
#pragma unroll
			for (int c = 0; c < 3; c++)
				pn[4 * a + 1 + c] = ((Fp[3 * a] * inv[c] + Fp[3 * a + 1] * inv[3 + c]) + Fp[3 * a + 2] * inv[6 + c]) - (a == c ? 1.0 : 0.0);
		}
		if (!in_domain(pn, q, r, T, KIND != kLinear)) {
			if (threadIdx.x == 0) write_result(out + poi, p, zncc, last, it, 3);
			return;
		}
#pragma unroll
		for (int e = 0; e < 12; e++) p[e] = pn[e];
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

size_t icgn_state_bytes() { return sizeof(IcgnState); }

void launch_icgn(IcgnVol R, IcgnVol T, const int *d_pts, int m, const double *d_init, int r, int max_it, double tol, int kind, void *d_state,
                 sift3d_icgn_result *d_out, hipStream_t st) {
	IcgnState *S = static_cast<IcgnState *>(d_state);
	hipLaunchKernelGGL(k_icgn_prepare<false>, dim3(m), dim3(kThreads), 0, st, R, T, d_pts, d_init, r, kind != kLinear, S, d_out);
	hipLaunchKernelGGL(by_kind(kind, k_icgn_iterate<kKeys, false>, k_icgn_iterate<kLinear, false>, k_icgn_iterate<kBspline, false>), dim3(m),
	                   dim3(kThreads), 0, st, R, T, d_pts, d_init, r, max_it, tol, S, d_out);
}

void launch_icgn_masked(IcgnVol R, IcgnVol T, const int *d_pts, int m, const double *d_init, int r, int max_it, double tol, int kind, void *d_state,
                        sift3d_icgn_result *d_out, IcgnMask M, hipStream_t st) {
	IcgnState *S = static_cast<IcgnState *>(d_state);
	hipLaunchKernelGGL((k_icgn_prepare<true, IcgnMask>), dim3(m), dim3(kThreads), 0, st, R, T, d_pts, d_init, r, kind != kLinear, S, d_out, M);
	hipLaunchKernelGGL(by_kind(kind, k_icgn_iterate<kKeys, true, IcgnMask>, k_icgn_iterate<kLinear, true, IcgnMask>, k_icgn_iterate<kBspline, true, IcgnMask>), dim3(m),
	                   dim3(kThreads), 0, st, R, T, d_pts, d_init, r, max_it, tol, S, d_out, M);
}

void launch_icgn_labelled(IcgnVol R, IcgnVol T, const int *d_pts, int m, const double *d_init, int r, int max_it, double tol, int kind,
                          void *d_state, sift3d_icgn_result *d_out, IcgnLabels M, hipStream_t st) {
	IcgnState *S = static_cast<IcgnState *>(d_state);
	hipLaunchKernelGGL((k_icgn_prepare<true, IcgnLabels>), dim3(m), dim3(kThreads), 0, st, R, T, d_pts, d_init, r, kind != kLinear, S, d_out, M);
	hipLaunchKernelGGL(by_kind(kind, k_icgn_iterate<kKeys, true, IcgnLabels>, k_icgn_iterate<kLinear, true, IcgnLabels>, k_icgn_iterate<kBspline, true, IcgnLabels>), dim3(m),
	                   dim3(kThreads), 0, st, R, T, d_pts, d_init, r, max_it, tol, S, d_out, M);
}

}  // namespace s3d
