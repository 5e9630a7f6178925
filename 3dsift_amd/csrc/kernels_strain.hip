// kernels_strain.hip -- strain fields from the displacements of the POIs (sift3d_strain, include/sift3d_hip.h, which states the
// numerical contract).  No reference counterpart.  A POI's neighbours are found through a uniform cell grid over the bounding box of
// the contributing POIs; the side of a cell is at least the window's half width, so a window touches at most 3 x 3 x 3 cells.
//   mark       per POI: does it contribute (valid byte, finite displacement, |coordinate| <= 2^24)?  The bounding box of the
//              contributing POIs by integer atomic min (the maxima as minima of the negated coordinate).  The host reads the box and
//              chooses the grid (entry_strain.hip).
//   bin        a count per cell by integer atomics, an exclusive scan (tiles of 4096 cells, the tile sums by one workgroup), then the
//              placement: POIs take a slot of their cell's segment by atomic (any order), and every slot is then ranked by the number of
//              POIs of its segment with a smaller index -- the sorted arrays list a cell's POIs in ascending index whatever order the
//              atomics gave.  Cells consecutive in x are consecutive in memory: the cells a window touches are 9 contiguous runs.
//              The ranking costs k^2 per cell of k POIs, which is what the fits of those k POIs cost as well.
//   fit        one wave per POI.  The 9 runs are walked as one sequence, lane l taking entries l, l + 64, ...: coordinates and
//              displacements are SoA, so a wave reads them coalesced.  Three walks: count and lowest index (u0), the 21 sums, the
//              residual.  Sums are fp64, reduced by an xor butterfly: a fixed order, the same value in every lane.  Every lane solves
//              the 3 x 3 system (Cholesky) and the eigenvalues (cyclic Jacobi), lane 0 writes the record.  No float atomics.
#include "sift3d_internal.h"

#include <math.h>

namespace s3d {
namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kScanItems = 16;                      // cells per thread of a scan tile
constexpr int kScanTile = kThreads * kScanItems;
constexpr int kCoordMax = 1 << 24;
constexpr double kPivotRel = 1e-9;

__device__ inline bool coord_ok(int v) { return v <= kCoordMax && v >= -kCoordMax; }
__device__ inline int wave_min(int x) {
	for (int off = 32; off > 0; off >>= 1) x = min(x, __shfl_xor(x, off));
	return x;
}
__device__ inline int wave_isum(int x) {
	for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off);
	return x;
}
__device__ inline double wave_sum(double x) {
	for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off);
	return x;
}
// floor(a / s), s > 0
__device__ inline int floor_div(int a, int s) { return a >= 0 ? a / s : -((-a + s - 1) / s); }

// cell[i] = 1 where POI i contributes, else -1; box = (min x, min y, min z, min -x, min -y, min -z), preset to a value above 2^24
__global__ __launch_bounds__(kThreads) void k_strain_mark(const int *__restrict__ pts, const double *__restrict__ disp,
                                                         const unsigned char *__restrict__ valid, int m, int *__restrict__ cell,
                                                         int *__restrict__ box) {
	const int i = blockIdx.x * kThreads + threadIdx.x;
	bool on = false;
	int q[3] = {0, 0, 0};
	if (i < m) {
		for (int a = 0; a < 3; a++) q[a] = pts[3 * (size_t)i + a];
		on = (!valid || valid[i]) && coord_ok(q[0]) && coord_ok(q[1]) && coord_ok(q[2]);
		for (int a = 0; a < 3; a++) on = on && isfinite(disp[3 * (size_t)i + a]);
		cell[i] = on ? 1 : -1;
	}
	const int big = 0x7f7f7f7f;
	for (int a = 0; a < 3; a++) {
		const int lo = wave_min(on ? q[a] : big), hi = wave_min(on ? -q[a] : big);
		if ((threadIdx.x & 63) == 0 && lo != big) {
			atomicMin(&box[a], lo);
			atomicMin(&box[3 + a], hi);
		}
	}
}

__device__ inline int cell_of(const StrainGrid &g, int x, int y, int z) {
	return (((z - g.z0) / g.side) * g.ny + (y - g.y0) / g.side) * g.nx + (x - g.x0) / g.side;
}

// cell[i]: 1 -> the POI's cell; cnt[c] = POIs of cell c
__global__ __launch_bounds__(kThreads) void k_strain_count(const int *__restrict__ pts, int m, StrainGrid g, int *__restrict__ cell,
                                                          int *__restrict__ cnt) {
	const int i = blockIdx.x * kThreads + threadIdx.x;
	if (i >= m || cell[i] < 0) return;
	const int c = cell_of(g, pts[3 * (size_t)i], pts[3 * (size_t)i + 1], pts[3 * (size_t)i + 2]);
	cell[i] = c;
	atomicAdd(&cnt[c], 1);
}

// inclusive scan of one value per thread over the workgroup; returns the thread's inclusive sum
__device__ inline int block_scan(int v, int *sh) {
	const int t = threadIdx.x;
	sh[t] = v;
	__syncthreads();
	for (int off = 1; off < kThreads; off <<= 1) {
		const int add = t >= off ? sh[t - off] : 0;
		__syncthreads();
		sh[t] += add;
		__syncthreads();
	}
	const int r = sh[t];
	__syncthreads();
	return r;
}

// out[i] = sum of in[tile start .. i) within each tile of kScanTile entries; tiles[b] = the tile's total
__global__ __launch_bounds__(kThreads) void k_strain_scan_tiles(const int *__restrict__ in, int *__restrict__ out, int n, int *__restrict__ tiles) {
	__shared__ int sh[kThreads];
	const size_t base = (size_t)blockIdx.x * kScanTile + (size_t)threadIdx.x * kScanItems;
	int v[kScanItems], sum = 0;
#pragma unroll
	for (int k = 0; k < kScanItems; k++) {
		v[k] = base + k < (size_t)n ? in[base + k] : 0;
		sum += v[k];
	}
	const int incl = block_scan(sum, sh);
	int run = incl - sum;
#pragma unroll
	for (int k = 0; k < kScanItems; k++) {
		if (base + k < (size_t)n) out[base + k] = run;
		run += v[k];
	}
	if (threadIdx.x == kThreads - 1) tiles[blockIdx.x] = incl;
}

// tiles[0 .. nt) -> their exclusive sums, by one workgroup
__global__ __launch_bounds__(kThreads) void k_strain_scan_sums(int *__restrict__ tiles, int nt) {
	__shared__ int sh[kThreads];
	int carry = 0;
	for (int base = 0; base < nt; base += kThreads) {
		const int i = base + threadIdx.x;
		const int v = i < nt ? tiles[i] : 0;
		const int incl = block_scan(v, sh);
		if (i < nt) tiles[i] = carry + incl - v;
		if (threadIdx.x == kThreads - 1) sh[0] = incl;
		__syncthreads();
		carry += sh[0];
		__syncthreads();
	}
}

__global__ __launch_bounds__(kThreads) void k_strain_scan_add(int *__restrict__ out, int n, const int *__restrict__ tiles) {
	const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
	if (i < (size_t)n) out[i] += tiles[i / kScanTile];
}

// a slot of the cell's segment per contributing POI, in the order the atomics give
__global__ __launch_bounds__(kThreads) void k_strain_scatter(const int *__restrict__ cell, int m, const int *__restrict__ start,
                                                            int *__restrict__ fill, int *__restrict__ slots) {
	const int i = blockIdx.x * kThreads + threadIdx.x;
	if (i >= m || cell[i] < 0) return;
	const int c = cell[i];
	slots[start[c] + atomicAdd(&fill[c], 1)] = i;
}

// slot s holds POI i of cell c: its place is the cell's start + the number of POIs of the cell with a smaller index
__global__ __launch_bounds__(kThreads) void k_strain_place(const int *__restrict__ slots, const int *__restrict__ cell, const int *__restrict__ start,
                                                          int ncells, const int *__restrict__ pts, const double *__restrict__ disp,
                                                          StrainSorted S) {
	const int s = blockIdx.x * kThreads + threadIdx.x;
	if (s >= start[ncells]) return;
	const int i = slots[s], c = cell[i];
	const int a = start[c], b = start[c + 1];
	int rank = 0;
	for (int t = a; t < b; t++) rank += slots[t] < i ? 1 : 0;
	const int d = a + rank;
	S.x[d] = pts[3 * (size_t)i];
	S.y[d] = pts[3 * (size_t)i + 1];
	S.z[d] = pts[3 * (size_t)i + 2];
	S.idx[d] = i;
	S.u[d] = disp[3 * (size_t)i];
	S.v[d] = disp[3 * (size_t)i + 1];
	S.w[d] = disp[3 * (size_t)i + 2];
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

__global__ __launch_bounds__(kThreads) void k_strain_fit(const int *__restrict__ pts, const double *__restrict__ disp, int m, StrainGrid g,
                                                        const int *__restrict__ start, int ncells, StrainSorted S, int radius, int min_nb,
                                                        int measure, sift3d_strain_result *__restrict__ out) {
	const int lane = threadIdx.x & 63;
	const int i = blockIdx.x * kWaves + (threadIdx.x >> 6);
	if (i >= m) return;
	const int x = pts[3 * (size_t)i], y = pts[3 * (size_t)i + 1], z = pts[3 * (size_t)i + 2];
	if (!(coord_ok(x) && coord_ok(y) && coord_ok(z))) {
		if (lane == 0) write_failed(out + i, 0, 2);
		return;
	}
	// the cells the window touches, per axis (none where the window misses the grid)
	const int lox = max(floor_div(x - radius - g.x0, g.side), 0), hix = min(floor_div(x + radius - g.x0, g.side), g.nx - 1);
	const int loy = max(floor_div(y - radius - g.y0, g.side), 0), hiy = min(floor_div(y + radius - g.y0, g.side), g.ny - 1);
	const int loz = max(floor_div(z - radius - g.z0, g.side), 0), hiz = min(floor_div(z + radius - g.z0, g.side), g.nz - 1);
	const int nc = start[ncells];
	// the runs: rb[k] the first entry of run k, cum[k] the entries of the runs before it
	int rb[9], cum[10];
	cum[0] = 0;
#pragma unroll
	for (int k = 0; k < 9; k++) {
		const int zz = loz + k / 3, yy = loy + k % 3;
		int b = 0, e = 0;
		if (zz <= hiz && yy <= hiy && lox <= hix) {
			const int row = (zz * g.ny + yy) * g.nx;
			b = min(max(start[row + lox], 0), nc);
			e = min(max(start[row + hix + 1], b), nc);
		}
		rb[k] = b;
		cum[k + 1] = cum[k] + (e - b);
	}
	const int total = cum[9];
	auto entry = [&](int t) {
		int j = rb[0] + t;
#pragma unroll
		for (int k = 1; k < 9; k++)
			if (t >= cum[k]) j = rb[k] + (t - cum[k]);
		return j;
	};
	auto inside = [&](int j) { return abs(S.x[j] - x) <= radius && abs(S.y[j] - y) <= radius && abs(S.z[j] - z) <= radius; };

	// walk 1: the neighbour count and the lowest index among them
	int n = 0, first = 0x7fffffff;
	for (int t = lane; t < total; t += 64) {
		const int j = entry(t);
		if (inside(j)) {
			n++;
			first = min(first, S.idx[j]);
		}
	}
	n = wave_isum(n);
	first = wave_min(first);
	if (n < min_nb) {
		if (lane == 0) write_failed(out + i, n, 1);
		return;
	}
	const double u0[3] = {disp[3 * (size_t)first], disp[3 * (size_t)first + 1], disp[3 * (size_t)first + 2]};

	// walk 2: S1 = sum d, S2 = sum d d^T, U = sum (u - u0), P[c][a] = sum (u_c - u0_c) d_a
	double s1[3] = {0, 0, 0}, s2[6] = {0, 0, 0, 0, 0, 0}, U[3] = {0, 0, 0}, P[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
	for (int t = lane; t < total; t += 64) {
		const int j = entry(t);
		if (!inside(j)) continue;
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
	}
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
	for (int t = lane; t < total; t += 64) {
		const int j = entry(t);
		if (!inside(j)) continue;
		const double d[3] = {(double)(S.x[j] - x), (double)(S.y[j] - y), (double)(S.z[j] - z)};
		const double uj[3] = {S.u[j], S.v[j], S.w[j]};
#pragma unroll
		for (int c = 0; c < 3; c++) {
			const double e = (uj[c] - dsp[c]) - ((G[c][0] * d[0] + G[c][1] * d[1]) + G[c][2] * d[2]);
			rs += e * e;
		}
	}
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

size_t strain_scan_tiles(size_t n) { return (n + kScanTile - 1) / kScanTile; }

void launch_strain_mark(const int *d_pts, const double *d_disp, const unsigned char *d_valid, int m, int *d_cell, int *d_box, hipStream_t st) {
	hipLaunchKernelGGL(k_strain_mark, dim3(blocks_for(m, kThreads)), dim3(kThreads), 0, st, d_pts, d_disp, d_valid, m, d_cell, d_box);
}

hipError_t launch_strain_bin(const int *d_pts, const double *d_disp, int m, StrainGrid g, int *d_cell, int *d_cnt, int *d_start, int *d_tiles,
                             int *d_slots, StrainSorted S, hipStream_t st) {
	const int ncells = g.nx * g.ny * g.nz, n = ncells + 1, nt = (int)strain_scan_tiles(n);
	const int bm = blocks_for(m, kThreads);
	hipLaunchKernelGGL(k_strain_count, dim3(bm), dim3(kThreads), 0, st, d_pts, m, g, d_cell, d_cnt);
	hipLaunchKernelGGL(k_strain_scan_tiles, dim3(nt), dim3(kThreads), 0, st, d_cnt, d_start, n, d_tiles);
	hipLaunchKernelGGL(k_strain_scan_sums, dim3(1), dim3(kThreads), 0, st, d_tiles, nt);
	hipLaunchKernelGGL(k_strain_scan_add, dim3(blocks_for(n, kThreads)), dim3(kThreads), 0, st, d_start, n, d_tiles);
	const hipError_t e = hipMemsetAsync(d_cnt, 0, sizeof(int) * (size_t)ncells, st);  // the counts become the fill marks of the scatter
	if (e != hipSuccess) return e;
	hipLaunchKernelGGL(k_strain_scatter, dim3(bm), dim3(kThreads), 0, st, d_cell, m, d_start, d_cnt, d_slots);
	hipLaunchKernelGGL(k_strain_place, dim3(bm), dim3(kThreads), 0, st, d_slots, d_cell, d_start, ncells, d_pts, d_disp, S);
	return hipGetLastError();
}

void launch_strain_fit(const int *d_pts, const double *d_disp, int m, StrainGrid g, const int *d_start, StrainSorted S, int radius, int min_nb,
                       int measure, sift3d_strain_result *d_out, hipStream_t st) {
	hipLaunchKernelGGL(k_strain_fit, dim3(blocks_for(m, kWaves)), dim3(kThreads), 0, st, d_pts, d_disp, m, g, d_start, g.nx * g.ny * g.nz, S, radius,
	                   min_nb, measure, d_out);
}

}  // namespace s3d
