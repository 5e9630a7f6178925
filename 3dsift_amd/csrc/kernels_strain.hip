// kernels_strain.hip -- strain fields from the displacements of the POIs (sift3d_strain, include/sift3d_hip.h, which states the
// numerical contract).  No reference counterpart.  A POI's neighbours come from the POI index (kernels_poigrid.hip), so a window is 9
// contiguous runs of the sorted arrays (poi_window.h).
//   fit        one wave per POI.  The 9 runs are walked as one sequence, lane l taking entries l, l + 64, ...: coordinates and
//              displacements are SoA, so a wave reads them coalesced.  Three walks: count and lowest index (u0), the 21 sums, the
//              residual.  Sums are fp64, reduced by an xor butterfly: a fixed order, the same value in every lane.  Every lane solves
//              the 3 x 3 system (Cholesky) and the eigenvalues (cyclic Jacobi), lane 0 writes the record.  No float atomics.
#include "poi_window.h"

#include <math.h>

namespace s3d {
namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr double kPivotRel = 1e-9;

__device__ inline int wave_min(int x) {
	for (int off = 32; off > 0; off >>= 1) x = min(x, __shfl_xor(x, off));
	return x;
}
__device__ inline double wave_sum(double x) {
	for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off);
	return x;
}

// one Jacobi rotation of the symmetric 3 x 3 matrix in the plane (p, q); r is the third index
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

__device__ inline void write_failed(sift3d_strain_result *o, int n, int status) {
	for (int k = 0; k < 3; k++) o->disp[k] = o->principal[k] = 0.0;
	for (int k = 0; k < 9; k++) o->G[k] = 0.0;
	for (int k = 0; k < 6; k++) o->E[k] = 0.0;
	o->equivalent = 0.0;
	o->rms = 0.0;
	o->neighbours = n;
	o->status = status;
}

// Labelled (sift3d_strain_labelled): a neighbour also has the POI's own label, which is positive, and the lanes share out the entries
// of that label (walk_matching, poi_window.h); the plain instantiation reads no label and walks as it always did
template <bool Labelled>
__global__ __launch_bounds__(kThreads) void k_strain_fit(const int *__restrict__ pts, const double *__restrict__ disp,
                                                        const int *__restrict__ label, int m, PoiGrid g, const int *__restrict__ start,
                                                        int ncells, PoiSorted S, int radius, int min_nb, int measure,
                                                        sift3d_strain_result *__restrict__ out) {
	const int lane = threadIdx.x & 63;
	const int i = blockIdx.x * kWaves + (threadIdx.x >> 6);
	if (i >= m) return;
	const int x = pts[3 * (size_t)i], y = pts[3 * (size_t)i + 1], z = pts[3 * (size_t)i + 2];
	if (!(coord_ok(x) && coord_ok(y) && coord_ok(z))) {
		if (lane == 0) write_failed(out + i, 0, 2);
		return;
	}
	int own = 0;
	if constexpr (Labelled) {
		own = label[i];
		if (own <= 0) {
			if (lane == 0) write_failed(out + i, 0, 1);
			return;
		}
	}
	const PoiWindow<false> W(g, start, ncells, x, y, z, radius);
	const int total = W.total;
	auto inside = [&](int j) { return abs(S.x[j] - x) <= radius && abs(S.y[j] - y) <= radius && abs(S.z[j] - z) <= radius; };
	// f(j) for the lane's share of the window's entries: every 64th of them, or (labelled) every 64th of those of the POI's label
	auto walk = [&](auto f) {
		if constexpr (Labelled)
			walk_matching(W, lane, [&](int j) { return label[S.idx[j]] == own; }, f);
		else
			for (int t = lane; t < total; t += 64) f(W.entry(t));
	};

	// walk 1: the neighbour count and the lowest index among them
	int n = 0, first = 0x7fffffff;
	walk([&](int j) {
		if (inside(j)) {
			n++;
			first = min(first, S.idx[j]);
		}
	});
	n = wave_isum(n);
	first = wave_min(first);
	if (n < min_nb) {
		if (lane == 0) write_failed(out + i, n, 1);
		return;
	}
	const double u0[3] = {disp[3 * (size_t)first], disp[3 * (size_t)first + 1], disp[3 * (size_t)first + 2]};

	// walk 2: S1 = sum d, S2 = sum d d^T, U = sum (u - u0), P[c][a] = sum (u_c - u0_c) d_a
	double s1[3] = {0, 0, 0}, s2[6] = {0, 0, 0, 0, 0, 0}, U[3] = {0, 0, 0}, P[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
	walk([&](int j) {
		if (!inside(j)) return;
		const double d[3] = {(double)(S.x[j] - x), (double)(S.y[j] - y), (double)(S.z[j] - z)};
		const double a[3] = {S.u[j] - u0[0], S.v[j] - u0[1], S.w[j] - u0[2]};
#pragma unroll
		for (int c = 0; c < 3; c++) {
			s1[c] += d[c];
			U[c] += a[c];
#pragma unroll
			for (int b = 0; b < 3; b++) P[c][b] += a[c] * d[b];
		}
		s2[0] += d[0] * d[0]; s2[1] += d[0] * d[1]; s2[2] += d[0] * d[2];
		s2[3] += d[1] * d[1]; s2[4] += d[1] * d[2]; s2[5] += d[2] * d[2];
	});
#pragma unroll
	for (int c = 0; c < 3; c++) {
		s1[c] = wave_sum(s1[c]);
		U[c] = wave_sum(U[c]);
#pragma unroll
		for (int b = 0; b < 3; b++) P[c][b] = wave_sum(P[c][b]);
	}
#pragma unroll
	for (int k = 0; k < 6; k++) s2[k] = wave_sum(s2[k]);

	// C = S2 - S1 S1^T / n and its Cholesky factor; a pivot at or under 1e-9 of C's largest diagonal entry (or NaN): degenerate window
	const double dn = (double)n;
	const double c00 = s2[0] - s1[0] * s1[0] / dn, c01 = s2[1] - s1[0] * s1[1] / dn, c02 = s2[2] - s1[0] * s1[2] / dn;
	const double c11 = s2[3] - s1[1] * s1[1] / dn, c12 = s2[4] - s1[1] * s1[2] / dn, c22 = s2[5] - s1[2] * s1[2] / dn;
	const double floor_p = kPivotRel * fmax(c00, fmax(c11, c22));
	bool ok = c00 > floor_p;
	const double l00 = sqrt(c00), l10 = c01 / l00, l20 = c02 / l00;
	const double p1 = c11 - l10 * l10;
	ok = ok && p1 > floor_p;
	const double l11 = sqrt(p1), l21 = (c12 - l20 * l10) / l11;
	const double p2 = (c22 - l20 * l20) - l21 * l21;
	ok = ok && p2 > floor_p;
	if (!ok) {
		if (lane == 0) write_failed(out + i, n, 4);
		return;
	}
	const double l22 = sqrt(p2);
	double G[3][3], dsp[3];
#pragma unroll
	for (int c = 0; c < 3; c++) {
		const double b0 = P[c][0] - s1[0] * U[c] / dn, b1 = P[c][1] - s1[1] * U[c] / dn, b2 = P[c][2] - s1[2] * U[c] / dn;
		const double y0 = b0 / l00, y1 = (b1 - l10 * y0) / l11, y2 = ((b2 - l20 * y0) - l21 * y1) / l22;
		G[c][2] = y2 / l22;
		G[c][1] = (y1 - l21 * G[c][2]) / l11;
		G[c][0] = ((y0 - l10 * G[c][1]) - l20 * G[c][2]) / l00;
		dsp[c] = (u0[c] + U[c] / dn) - ((G[c][0] * s1[0] + G[c][1] * s1[1]) + G[c][2] * s1[2]) / dn;
	}

	// walk 3: the residual of the fitted plane
	double rs = 0;
	walk([&](int j) {
		if (!inside(j)) return;
		const double d[3] = {(double)(S.x[j] - x), (double)(S.y[j] - y), (double)(S.z[j] - z)};
		const double uj[3] = {S.u[j], S.v[j], S.w[j]};
#pragma unroll
		for (int c = 0; c < 3; c++) {
			const double e = (uj[c] - dsp[c]) - ((G[c][0] * d[0] + G[c][1] * d[1]) + G[c][2] * d[2]);
			rs += e * e;
		}
	});
	rs = wave_sum(rs);

	// E of the chosen measure (xx yy zz xy yz zx), its eigenvalues and the equivalent strain
	double exx = G[0][0], eyy = G[1][1], ezz = G[2][2];
	double exy = 0.5 * (G[0][1] + G[1][0]), eyz = 0.5 * (G[1][2] + G[2][1]), ezx = 0.5 * (G[2][0] + G[0][2]);
	if (measure == 0) {
		exx += 0.5 * ((G[0][0] * G[0][0] + G[1][0] * G[1][0]) + G[2][0] * G[2][0]);
		eyy += 0.5 * ((G[0][1] * G[0][1] + G[1][1] * G[1][1]) + G[2][1] * G[2][1]);
		ezz += 0.5 * ((G[0][2] * G[0][2] + G[1][2] * G[1][2]) + G[2][2] * G[2][2]);
		exy += 0.5 * ((G[0][0] * G[0][1] + G[1][0] * G[1][1]) + G[2][0] * G[2][1]);
		eyz += 0.5 * ((G[0][1] * G[0][2] + G[1][1] * G[1][2]) + G[2][1] * G[2][2]);
		ezx += 0.5 * ((G[0][2] * G[0][0] + G[1][2] * G[1][0]) + G[2][2] * G[2][0]);
	}
	double a00 = exx, a11 = eyy, a22 = ezz, a01 = exy, a12 = eyz, a02 = ezx;
#pragma unroll 1
	for (int sweep = 0; sweep < 8; sweep++) {
		jacobi_rotate(a00, a11, a01, a02, a12);
		jacobi_rotate(a00, a22, a02, a01, a12);
		jacobi_rotate(a11, a22, a12, a01, a02);
	}
	const double e_hi = fmax(a00, fmax(a11, a22)), e_lo = fmin(a00, fmin(a11, a22));
	const double e_mid = ((a00 + a11) + a22) - e_hi - e_lo;
	const double mean = ((exx + eyy) + ezz) / 3.0;
	const double dx = exx - mean, dy = eyy - mean, dz = ezz - mean;
	const double dev2 = ((dx * dx + dy * dy) + dz * dz) + 2.0 * ((exy * exy + eyz * eyz) + ezx * ezx);

	if (lane == 0) {
		sift3d_strain_result *o = out + i;
#pragma unroll
		for (int c = 0; c < 3; c++) {
			o->disp[c] = dsp[c];
#pragma unroll
			for (int b = 0; b < 3; b++) o->G[3 * c + b] = G[c][b];
		}
		o->E[0] = exx; o->E[1] = eyy; o->E[2] = ezz; o->E[3] = exy; o->E[4] = eyz; o->E[5] = ezx;
		o->principal[0] = e_hi; o->principal[1] = e_mid; o->principal[2] = e_lo;
		o->equivalent = sqrt(2.0 / 3.0 * dev2);
		o->rms = sqrt(rs / (3.0 * dn));
		o->neighbours = n;
		o->status = 0;
	}
}

int blocks_for(size_t n, int per) { return (int)((n + per - 1) / per); }
}  // namespace

void launch_strain_fit(const int *d_pts, const double *d_disp, const int *d_label, int m, const PoiIndex &ix, int radius, int min_nb,
                       int measure, sift3d_strain_result *d_out, hipStream_t st) {
	const dim3 grid(blocks_for(m, kWaves)), block(kThreads);
	if (d_label)
		hipLaunchKernelGGL(k_strain_fit<true>, grid, block, 0, st, d_pts, d_disp, d_label, m, ix.g, ix.start, ix.ncells, ix.S, radius, min_nb,
		                   measure, d_out);
	else
		hipLaunchKernelGGL(k_strain_fit<false>, grid, block, 0, st, d_pts, d_disp, d_label, m, ix.g, ix.start, ix.ncells, ix.S, radius, min_nb,
		                   measure, d_out);
}

}  // namespace s3d
