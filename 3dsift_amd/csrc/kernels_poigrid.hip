// kernels_poigrid.hip -- the spatial index over a call's POIs (poi_grid.h), which the strain fit (kernels_strain.hip) and
// the median test (kernels_validate.hip) walk.  No reference counterpart.  A POI's neighbours are found through a uniform cell grid over
// the bounding box of the contributing POIs; the side of a cell is at least the window's half width, so a window touches at most
// 3 x 3 x 3 cells (poi_window.h).
//   mark       per POI: does it contribute (valid byte, finite displacement, |coordinate| <= 2^24)?  The bounding box of the
//              contributing POIs by integer atomic min (the maxima as minima of the negated coordinate).  The host reads the box and
//              chooses the grid (poi_choose_grid).
//   bin        a count per cell by integer atomics, an exclusive scan (tiles of 4096 cells, the tile sums by one workgroup), then the
//              placement: POIs take a slot of their cell's segment by atomic (any order), and every slot is then ranked by the number of
//              POIs of its segment with a smaller index -- the sorted arrays list a cell's POIs in ascending index whatever order the
//              atomics gave.  Cells consecutive in x are consecutive in memory: the cells a window touches are 9 contiguous runs.
//              The ranking costs k^2 per cell of k POIs, which is what the fits of those k POIs cost as well.
#include "call_state.h"
#include "poi_window.h"

#include <math.h>

namespace s3d {
namespace {

constexpr int kThreads = 256;
constexpr int kScanItems = kPoiScanTile / kThreads;  // cells per thread of a scan tile

__device__ inline int wave_min(int x) {
	for (int off = 32; off > 0; off >>= 1) x = min(x, __shfl_xor(x, off));
	return x;
}

// cell[i] = 1 where POI i contributes, else -1; box = (min x, min y, min z, min -x, min -y, min -z), preset to kPoiBoxEmpty
__global__ __launch_bounds__(kThreads) void k_poi_mark(const int *__restrict__ pts, const double *__restrict__ disp,
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
	const int big = kPoiBoxEmpty;
	for (int a = 0; a < 3; a++) {
		const int lo = wave_min(on ? q[a] : big), hi = wave_min(on ? -q[a] : big);
		if ((threadIdx.x & 63) == 0 && lo != big) {
			atomicMin(&box[a], lo);
			atomicMin(&box[3 + a], hi);
		}
	}
}

__device__ inline int cell_of(const PoiGrid &g, int x, int y, int z) {
	return (((z - g.z0) / g.side) * g.ny + (y - g.y0) / g.side) * g.nx + (x - g.x0) / g.side;
}

// cell[i]: 1 -> the POI's cell; cnt[c] = POIs of cell c
__global__ __launch_bounds__(kThreads) void k_poi_count(const int *__restrict__ pts, int m, PoiGrid g, int *__restrict__ cell,
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

// out[i] = sum of in[tile start .. i) within each tile of kPoiScanTile entries; tiles[b] = the tile's total
__global__ __launch_bounds__(kThreads) void k_poi_scan_tiles(const int *__restrict__ in, int *__restrict__ out, int n, int *__restrict__ tiles) {
	__shared__ int sh[kThreads];
	const size_t base = (size_t)blockIdx.x * kPoiScanTile + (size_t)threadIdx.x * kScanItems;
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
__global__ __launch_bounds__(kThreads) void k_poi_scan_sums(int *__restrict__ tiles, int nt) {
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

__global__ __launch_bounds__(kThreads) void k_poi_scan_add(int *__restrict__ out, int n, const int *__restrict__ tiles) {
	const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
	if (i < (size_t)n) out[i] += tiles[i / kPoiScanTile];
}

// a slot of the cell's segment per contributing POI, in the order the atomics give
__global__ __launch_bounds__(kThreads) void k_poi_scatter(const int *__restrict__ cell, int m, const int *__restrict__ start,
                                                         int *__restrict__ fill, int *__restrict__ slots) {
	const int i = blockIdx.x * kThreads + threadIdx.x;
	if (i >= m || cell[i] < 0) return;
	const int c = cell[i];
	slots[start[c] + atomicAdd(&fill[c], 1)] = i;
}

// slot s holds POI i of cell c: its place is the cell's start + the number of POIs of the cell with a smaller index
__global__ __launch_bounds__(kThreads) void k_poi_place(const int *__restrict__ slots, const int *__restrict__ cell, const int *__restrict__ start,
                                                       int ncells, const int *__restrict__ pts, const double *__restrict__ disp, PoiSorted S) {
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

int blocks_for(size_t n, int per) { return (int)((n + per - 1) / per); }
}  // namespace

int poi_grid_build(const PoiGridPlan &P, char *A, const int *d_pts, const double *d_disp, const unsigned char *d_valid, int m, int radius,
                   CallTemps &T, hipStream_t st, PoiIndex &ix) {
	int *d_box = reinterpret_cast<int *>(A + P.o_box), *d_cell = reinterpret_cast<int *>(A + P.o_cell), *d_slots = reinterpret_cast<int *>(A + P.o_slots);
	int *si = reinterpret_cast<int *>(A + P.o_si);
	double *sd = reinterpret_cast<double *>(A + P.o_sd);
	const size_t ni = P.wi / sizeof(int), nd = P.wd / sizeof(double);
	const PoiSorted S = {si, si + ni, si + 2 * ni, si + 3 * ni, sd, sd + nd, sd + 2 * nd};
	const int bm = blocks_for(m, kThreads);
	S3D_HIP_ST(st, hipMemsetAsync(d_box, kPoiBoxEmpty & 0xff, sizeof(int) * 6, st));
	hipLaunchKernelGGL(k_poi_mark, dim3(bm), dim3(kThreads), 0, st, d_pts, d_disp, d_valid, m, d_cell, d_box);
	S3D_HIP_ST(st, hipGetLastError());
	int box[6];
	S3D_HIP_ST(st, hipMemcpyAsync(box, d_box, sizeof(box), hipMemcpyDeviceToHost, st));
	S3D_HIP_ST(st, hipStreamSynchronize(st));
	const PoiGrid g = poi_choose_grid(box, radius);
	// block b: [counts per cell (then the scatter's fill marks) | cell starts | the scan's tile sums]; the scan runs over ncells + 1 values
	const int ncells = g.nx * g.ny * g.nz, n = ncells + 1, nt = (int)poi_scan_tiles(n);
	const size_t wc = al256(sizeof(int) * (size_t)n);
	S3D_HIP(hipMalloc(&T.b, 2 * wc + sizeof(int) * (size_t)nt));
	int *d_cnt = reinterpret_cast<int *>(T.b), *d_start = reinterpret_cast<int *>(T.b + wc), *d_tiles = reinterpret_cast<int *>(T.b + 2 * wc);
	S3D_HIP_ST(st, hipMemsetAsync(d_cnt, 0, sizeof(int) * (size_t)n, st));
	hipLaunchKernelGGL(k_poi_count, dim3(bm), dim3(kThreads), 0, st, d_pts, m, g, d_cell, d_cnt);
	hipLaunchKernelGGL(k_poi_scan_tiles, dim3(nt), dim3(kThreads), 0, st, d_cnt, d_start, n, d_tiles);
	hipLaunchKernelGGL(k_poi_scan_sums, dim3(1), dim3(kThreads), 0, st, d_tiles, nt);
	hipLaunchKernelGGL(k_poi_scan_add, dim3(blocks_for(n, kThreads)), dim3(kThreads), 0, st, d_start, n, d_tiles);
	S3D_HIP_ST(st, hipMemsetAsync(d_cnt, 0, sizeof(int) * (size_t)ncells, st));  // the counts become the fill marks of the scatter
	hipLaunchKernelGGL(k_poi_scatter, dim3(bm), dim3(kThreads), 0, st, d_cell, m, d_start, d_cnt, d_slots);
	hipLaunchKernelGGL(k_poi_place, dim3(bm), dim3(kThreads), 0, st, d_slots, d_cell, d_start, ncells, d_pts, d_disp, S);
	S3D_HIP_ST(st, hipGetLastError());
	ix = PoiIndex{g, ncells, d_cell, d_start, S};
	return SIFT3D_OK;
}

}  // namespace s3d
