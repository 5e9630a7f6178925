// kernels_subset.hip -- subset screening (sift3d_subset_quality, include/sift3d_hip.h, which states the numerical contract): the texture
// sums of the cube around a POI at every radius of r_min .. r_max, and the smallest radius whose criterion reaches the threshold.
// No reference counterpart.  One workgroup of 256 threads per point of interest (POI), direct loads (k_icgn_prepare's form):
//   block      the cube of r_min is one block: voxel i = (dz, dy, dx) in linear order, dx fastest, thread t takes i = t, t + 256, ...
//   shells     then the Chebyshev shells k = r_min + 1 .. feasible, one at a time.  Voxel j of shell k (D = 2k + 1):
//                j <  D^2           the face dz = -k:  dy = j / D - k, dx = j % D - k
//                j <  2 D^2         the face dz = +k, likewise
//                else j' = j - 2 D^2: dz = j' / 8k - k + 1 and t = j' % 8k walks the ring of that plane:
//                  t < D  the row dy = -k (dx = t - k);  t < 2D  the row dy = +k (dx = t - D - k);
//                  else t' = t - 2D: dy = t' / 2 - k + 1, dx = -k (t' even) or +k (t' odd)
//              thread t takes j = t, t + 256, ...: lanes run along x on the faces and rows.
//   sums       per voxel 7 loads (the voxel and its six axial neighbours); 8 fp64 sums (S, Q, Gxx Gyy Gzz Gxy Gxz Gyz) and the material
//              count per thread, reduced in a fixed order: xor butterfly in the wave, waves in index order through LDS (two buffers
//              in turn: one barrier per shell), then added to the running totals.  Every thread holds the same totals and forms the
//              same decision from them (redundantly, as k_icgn_iterate forms its step): no broadcast, the branch is uniform.
//   stop       the walk ends at the first radius that qualifies; thread 0 writes the record.  No float atomics.
// tests/subset_cases.py restates this walk order for the seam tests.
#include "sift3d_internal.h"

#include <math.h>

namespace s3d {
namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kSums = 8;  // S, Q, Gxx, Gyy, Gzz, Gxy, Gxz, Gyz

__device__ inline double wave_sum(double x) {
	for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off);
	return x;
}

__device__ inline int wave_isum(int x) {
	for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off);
	return x;
}

// one Jacobi rotation of the symmetric 3 x 3 matrix in the plane (p, q); r is the third index (kernels_strain.hip's)
__device__ inline void jacobi_rotate(double &app, double &aqq, double &apq, double &arp, double &arq) {
	if (apq == 0.0) return;
	const double theta = (aqq - app) / (2.0 * apq);
	const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
	const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
	app -= t * apq;
	aqq += t * apq;
	apq = 0.0;
	const double rp = c * arp - s * arq, rq = s * arp + c * arq;
	arp = rp;
	arq = rq;
}

// eigenvalues of G (tot[2..7]: xx yy zz xy xz yz), descending; three NaN where an entry of G is not finite
__device__ inline void eigenvalues(const double *tot, bool finite, double e[3]) {
	if (!finite) {
		e[0] = e[1] = e[2] = NAN;
		return;
	}
	double a00 = tot[2], a11 = tot[3], a22 = tot[4], a01 = tot[5], a02 = tot[6], a12 = tot[7];
#pragma unroll 1
	for (int sweep = 0; sweep < 8; sweep++) {
		jacobi_rotate(a00, a11, a01, a02, a12);
		jacobi_rotate(a00, a22, a02, a01, a12);
		jacobi_rotate(a11, a22, a12, a01, a02);
	}
	e[0] = fmax(a00, fmax(a11, a22));
	e[2] = fmin(a00, fmin(a11, a22));
	e[1] = ((a00 + a11) + a22) - e[0] - e[2];
}

// the voxel at c into the thread's sums: sy, sz R's strides, rc the shift R[q]
__device__ inline void add_voxel(const float *c, long long sy, long long sz, float rc, double level, double acc[kSums], int &mat) {
	const float v = c[0];
	const float gxf = 0.5f * (c[1] - c[-1]), gyf = 0.5f * (c[sy] - c[-sy]), gzf = 0.5f * (c[sz] - c[-sz]);
	const double a = (double)v - (double)rc;
	const double gx = (double)gxf, gy = (double)gyf, gz = (double)gzf;
	acc[0] += a;
	acc[1] += a * a;
	acc[2] += gx * gx;
	acc[3] += gy * gy;
	acc[4] += gz * gz;
	acc[5] += gx * gy;
	acc[6] += gx * gz;
	acc[7] += gy * gz;
	mat += ((double)v >= level) ? 1 : 0;
}

__global__ __launch_bounds__(kThreads) void k_subset_quality(IcgnVol R, const int *__restrict__ pts, SubsetParams P,
                                                            sift3d_subset_result *__restrict__ out) {
	__shared__ double red[2][kWaves][kSums];
	__shared__ int redi[2][kWaves];
	const int poi = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
	const int q[3] = {pts[3 * (size_t)poi], pts[3 * (size_t)poi + 1], pts[3 * (size_t)poi + 2]};
	sift3d_subset_result *o = out + poi;
	// feasible: the largest rho <= r_max with q - rho - 1 >= 0 and q + rho + 1 <= n - 1 on every axis (64-bit: q is any int)
	long long room = P.r_max;
	{
		const int n[3] = {R.nx, R.ny, R.nz};
#pragma unroll
		for (int a = 0; a < 3; a++) {
			const long long lo = (long long)q[a] - 1, hi = (long long)n[a] - 2 - (long long)q[a];
			room = lo < room ? lo : room;
			room = hi < room ? hi : room;
		}
	}
	if (room < (long long)P.r_min) {  // uniform: the whole workgroup leaves, no voxel read
		if (tid == 0) {
			o->mean = 0.0;
			o->dR = 0.0;
			for (int k = 0; k < 6; k++) o->G[k] = 0.0;
			for (int k = 0; k < 3; k++) o->eig[k] = 0.0;
			o->radius = 0;
			o->status = 2;
			o->feasible = 0;
			o->material = 0;
		}
		return;
	}
	const int feasible = (int)room;
	const long long sy = R.nx, sz = (long long)R.nx * R.ny;
	const float *Rq = R.d + (((size_t)q[2] * R.ny + q[1]) * R.nx + q[0]);
	const float rc = Rq[0];
	double tot[kSums];
#pragma unroll
	for (int k = 0; k < kSums; k++) tot[k] = 0.0;
	int material = 0, radius = P.r_min, buf = 0;
	bool qualifies = false, gfinite = false;
	double eig[3] = {0.0, 0.0, 0.0};
	for (int rho = P.r_min;; rho++) {
		double acc[kSums];
#pragma unroll
		for (int k = 0; k < kSums; k++) acc[k] = 0.0;
		int mat = 0;
		const int D = 2 * rho + 1, DD = D * D;
		if (rho == P.r_min) {
			const int N = DD * D;
			for (int i = tid; i < N; i += kThreads) {
				const int z = i / DD, rem = i - z * DD, y = rem / D, x = rem - y * D;
				add_voxel(Rq + ((z - rho) * sz + (y - rho) * sy + (x - rho)), sy, sz, rc, P.level, acc, mat);
			}
		} else {
			const int ring = 8 * rho, n_shell = 2 * DD + ring * (D - 2);
			for (int j = tid; j < n_shell; j += kThreads) {
				int dx, dy, dz;
				if (j < 2 * DD) {
					const int f = j < DD ? j : j - DD;
					dz = j < DD ? -rho : rho;
					dy = f / D;
					dx = f - dy * D - rho;
					dy -= rho;
				} else {
					const int jj = j - 2 * DD, p = jj / ring, t = jj - p * ring;
					dz = p - rho + 1;
					if (t < 2 * D) {
						dy = t < D ? -rho : rho;
						dx = (t < D ? t : t - D) - rho;
					} else {
						const int tt = t - 2 * D;
						dy = (tt >> 1) - rho + 1;
						dx = (tt & 1) ? rho : -rho;
					}
				}
				add_voxel(Rq + (dz * sz + dy * sy + dx), sy, sz, rc, P.level, acc, mat);
			}
		}
#pragma unroll
		for (int k = 0; k < kSums; k++) {
			const double x = wave_sum(acc[k]);
			if (lane == 0) red[buf][wv][k] = x;
		}
		mat = wave_isum(mat);
		if (lane == 0) redi[buf][wv] = mat;
		__syncthreads();
#pragma unroll
		for (int k = 0; k < kSums; k++) tot[k] += ((red[buf][0][k] + red[buf][1][k]) + red[buf][2][k]) + red[buf][3][k];
		material += ((redi[buf][0] + redi[buf][1]) + redi[buf][2]) + redi[buf][3];
		buf ^= 1;  // the next shell writes the other buffer; this one is written again only behind the next barrier
		radius = rho;
		// the criterion at rho: not finite where an entry of G is not
		gfinite = true;
#pragma unroll
		for (int k = 2; k < kSums; k++) gfinite = gfinite && isfinite(tot[k]);
		double c = NAN;
		if (P.criterion == 0) {
			if (gfinite) c = fmin(tot[2], fmin(tot[3], tot[4]));
		} else {
			eigenvalues(tot, gfinite, eig);
			c = eig[2];
		}
		qualifies = isfinite(c) && c >= P.threshold;
		if (qualifies || rho >= feasible) break;  // uniform: every thread holds the same totals
	}
	if (tid != 0) return;
	if (P.criterion == 0) eigenvalues(tot, gfinite, eig);
	const double Nd = (double)(2 * radius + 1) * (double)(2 * radius + 1) * (double)(2 * radius + 1);
	const double var = tot[1] - tot[0] * tot[0] / Nd;
	o->mean = (double)rc + tot[0] / Nd;
	o->dR = sqrt(var < 0.0 ? 0.0 : var);
#pragma unroll
	for (int k = 0; k < 6; k++) o->G[k] = tot[2 + k];
	o->eig[0] = eig[0];
	o->eig[1] = eig[1];
	o->eig[2] = eig[2];
	o->radius = radius;
	o->status = !qualifies ? 1 : ((double)material < P.fraction_min * Nd ? 3 : 0);
	o->feasible = feasible;
	o->material = material;
}

}  // namespace

void launch_subset_quality(IcgnVol R, const int *d_pts, int m, SubsetParams P, sift3d_subset_result *d_out, hipStream_t st) {
	hipLaunchKernelGGL(k_subset_quality, dim3(m), dim3(kThreads), 0, st, R, d_pts, P, d_out);
}

}  // namespace s3d
