// rigid_kit.h -- the device functions of the rigid / similarity model that every kernel fitting it shares (kernels_rigid.hip: the global
// and the per-point fits; kernels_bodyfit.hip: the per-body fits): the triad (minimal solve), the 4x4 Jacobi and the Horn refit rounds.
// Every fp64 expression follows the contract of include/sift3d_hip.h ("RANSAC rigid and similarity fits") term by term; include after
// sift3d_internal.h, whose pragma keeps FMA contraction off.  Every function is inline, so each kernel file compiles its own copy.
#ifndef S3D_RIGID_KIT_H
#define S3D_RIGID_KIT_H

#include "ransac_kit.h"

namespace s3d {
namespace rigid_kit {

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

}  // namespace rigid_kit
}  // namespace s3d

#endif
