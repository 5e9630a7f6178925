// kernels_detect_full.hip -- the opt-in detection rules of sift3d_set_detect_options (include/sift3d_hip.h): the full 3x3x3x3
// scale-space extremum test (80 neighbours) and the sub-voxel quadratic refinement.  No reference counterpart: the reference has
// one rule, IsExtrema_neighbor (Src/cSIFT3D.cc:884-911, restated by k_mark in kernels_detect.hip), which stays the default.
//
//   k_mark_full : the same ballot words and block counts as k_mark (word index ((lvl * nz + z) * ny + y) * wpr + xw, one count per
//                 block of `rows` rows), so k_scan / k_emit / k_emit_multi turn them into the ordered extrema list unchanged.  Lanes run
//                 along x (coalesced); the voxels above the peak threshold (a few per cent) are pushed into a wave-private LDS queue
//                 by ballot rank; 64 queued candidates at a time, one per lane, take the neighbourhood test -- the 26 in-level
//                 neighbours first (the cheapest rejections), then the 54 voxels of the levels below and above -- and, with refine
//                 on, the fp64 fit, which clears a rejected candidate.  Every DoG level is materialised when options are set (the
//                 run does not elide DoG[0] / DoG[nd-1] nor the last Gaussian level), so all reads are plain loads.
//   k_refine    : one thread per extremum; an accepted one (slot >= 0) refits its 3x3x3x3 block -> sift3d_refined[slot].
//
// The fit is fp64 arithmetic on the fp32 DoG samples in ONE fixed order, with FP contraction off (a Python float restatement in
// tests/detect_full_ref.py reproduces every decision and value bit for bit).
#include <math.h>

#include <algorithm>

#include "sift3d_internal.h"

#pragma clang fp contract(off)

namespace s3d {

// 3x3x3x3 fit at voxel i of level `cur` (prev / next: the DoG levels below / above, same dims).  d = -H^-1 g (axis order x, y, z, s),
// contrast = D0 + 0.5 g.d, Hs = the spatial 3x3 block of H.  false: a pivot of the elimination is exactly 0.
__device__ __noinline__ bool quad_fit(const float *cur, const float *prev, const float *next, size_t i, long long sy, long long sz,
                                      double d[4], double &contrast, double Hs[3][3]) {
	const long long o[3] = {1, sy, sz};
	const float *c = cur + i, *pm = prev + i, *pp = next + i;
	const double D0 = (double)c[0];
	double g[4], H[4][4];
	for (int a = 0; a < 3; a++) {
		const double dp = (double)c[o[a]], dm = (double)c[-o[a]];
		g[a] = 0.5 * (dp - dm);
		H[a][a] = (dp + dm) - 2.0 * D0;
	}
	{
		const double dp = (double)pp[0], dm = (double)pm[0];
		g[3] = 0.5 * (dp - dm);
		H[3][3] = (dp + dm) - 2.0 * D0;
	}
	for (int a = 0; a < 3; a++)
		for (int b = a + 1; b < 3; b++) {
			const double app = (double)c[o[a] + o[b]], apm = (double)c[o[a] - o[b]], amp = (double)c[-o[a] + o[b]], amm = (double)c[-o[a] - o[b]];
			H[a][b] = H[b][a] = 0.25 * (((app - apm) - amp) + amm);
		}
	for (int a = 0; a < 3; a++) {  // (axis a, scale): D++ = next at +a, D+- = prev at +a, D-+ = next at -a, D-- = prev at -a
		const double app = (double)pp[o[a]], apm = (double)pm[o[a]], amp = (double)pp[-o[a]], amm = (double)pm[-o[a]];
		H[a][3] = H[3][a] = 0.25 * (((app - apm) - amp) + amm);
	}
	double A[4][5];
	for (int r = 0; r < 4; r++) {
		for (int k = 0; k < 4; k++) A[r][k] = H[r][k];
		A[r][4] = -g[r];
	}
	for (int k = 0; k < 4; k++) {
		int p = k;
		for (int r = k + 1; r < 4; r++)
			if (fabs(A[r][k]) > fabs(A[p][k])) p = r;
		if (p != k)
			for (int cc = 0; cc < 5; cc++) { const double t = A[k][cc]; A[k][cc] = A[p][cc]; A[p][cc] = t; }
		if (A[k][k] == 0.0) return false;
		for (int r = k + 1; r < 4; r++) {
			const double f = A[r][k] / A[k][k];
			for (int cc = k; cc < 5; cc++) A[r][cc] = A[r][cc] - f * A[k][cc];
		}
	}
	for (int k = 3; k >= 0; k--) {
		double s = A[k][4];
		for (int cc = k + 1; cc < 4; cc++) s = s - A[k][cc] * d[cc];
		d[k] = s / A[k][k];
	}
	contrast = D0 + 0.5 * (((g[0] * d[0] + g[1] * d[1]) + g[2] * d[2]) + g[3] * d[3]);
	for (int a = 0; a < 3; a++)
		for (int b = 0; b < 3; b++) Hs[a][b] = H[a][b];
	return true;
}

// the rejection tests of a fitted candidate (absmax = max|level| of the keypoint's DoG level)
__device__ __forceinline__ bool fit_accepts(const DetectOpts &opt, const double d[4], double contrast, const double Hs[3][3], float absmax) {
	if (opt.max_offset > 0.0f) {
		const double m = (double)opt.max_offset;
		for (int a = 0; a < 4; a++)
			if (fabs(d[a]) > m) return false;
	}
	if (opt.contrast_thresh > 0.0f) {
		const float thr = opt.contrast_thresh * absmax;  // fp32 product, like the peak threshold
		if (fabs(contrast) < (double)thr) return false;
	}
	if (opt.edge_ratio > 0.0f) {
		const double tr = (Hs[0][0] + Hs[1][1]) + Hs[2][2];
		const double det = (Hs[0][0] * (Hs[1][1] * Hs[2][2] - Hs[1][2] * Hs[2][1]) - Hs[0][1] * (Hs[1][0] * Hs[2][2] - Hs[1][2] * Hs[2][0])) +
		                   Hs[0][2] * (Hs[1][0] * Hs[2][1] - Hs[1][1] * Hs[2][0]);
		const double r = (double)opt.edge_ratio, q = 2.0 * r + 1.0;
		const double lim = ((q * q) * q) / (r * r);
		if (!(tr * det > 0.0 && ((tr * tr) * tr) / det < lim)) return false;
	}
	return true;
}

// v strictly above (mx) / below every value of the rows of a 3x3 block of one level around p (skip_centre: the centre itself is v)
__device__ __forceinline__ bool beats_block(float v, bool mx, const float *p, long long sy, long long sz, bool skip_centre) {
	for (int dz = -1; dz <= 1; dz++)
		for (int dy = -1; dy <= 1; dy++) {
			const float *r = p + dz * sz + dy * sy;
			for (int dx = -1; dx <= 1; dx++) {
				if (skip_centre && dz == 0 && dy == 0 && dx == 0) continue;
				const float w = r[dx];
				if (mx ? !(v > w) : !(v < w)) return false;
			}
		}
	return true;
}

constexpr int kFullThreads = 256;
constexpr int kFullQueue = 128;  // >= 63 left over + one word's 64 (drained after every word)
__global__ void __launch_bounds__(kFullThreads) k_mark_full(DetectLevels L, int nx, int ny, ZRange zr, int nyb, int rows, float peak_thresh,
                                                            DetectOpts opt, unsigned long long *__restrict__ masks,
                                                            unsigned *__restrict__ block_counts) {
	__shared__ unsigned s_cnt[kFullThreads / 64];
	__shared__ uint2 s_q[kFullThreads / 64][kFullQueue];  // (value bits, (row within the wave) << 12 | word << 6 | lane)
	extern __shared__ unsigned long long s_mask_full[];   // [wave][row of the wave][word of the segment]
	const int segw = min((nx + 63) >> 6, 64);
	const int b = blockIdx.x;
	const int nz = zr.zo1 - zr.zo0;
	const int yb = b % nyb, zi = (b / nyb) % nz, lvl = b / (nyb * nz);
	const int z = zr.zo0 + zi;
	const int zg = z + zr.zoff;
	const float *__restrict__ cur = L.cur[lvl];
	const float *__restrict__ prev = L.prev[lvl];
	const float *__restrict__ next = L.next[lvl];
	const float absmax = __uint_as_float(*L.absmax_bits[lvl]);
	const float thr = peak_thresh * absmax;
	const int wpr = (nx + 63) >> 6;
	const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
	const long long sy = nx, sz = (long long)nx * ny;
	const bool z_in = zg >= 1 && zg <= zr.nzg - 2;
	const int y0 = yb * rows;
	const int wrows = rows / 4;
	const int nrows = min(rows, ny - y0);
	const int swid = __builtin_amdgcn_readfirstlane(wid);
	const int r_lo = swid * wrows, r_hi = min(nrows, (swid + 1) * wrows);
	uint2 *q = s_q[swid];
	unsigned long long *mloc = s_mask_full + (size_t)swid * wrows * segw;
	for (int i = lane; i < wrows * segw; i += 64) mloc[i] = 0ull;
	const unsigned long long lt = (1ull << lane) - 1ull;
	const size_t plane0 = (size_t)sz * (size_t)z + (size_t)sy * (size_t)y0;
	const bool full = opt.neighbours == 80;
	int qn = 0;  // wave-uniform
	// `n` queued candidates from entry `first`, one per lane
	auto evaluate = [&](int first, int n, int seg0) {
		if (lane >= n) return;
		const uint2 qe = q[first + lane];
		const float v = __uint_as_float(qe.x);
		const unsigned id = qe.y;
		const int rr = (int)((id >> 12) & 15), xw = (int)((id >> 6) & 63), bit = (int)(id & 63);
		const int x = (seg0 + xw) * 64 + bit;
		const size_t i = plane0 + (size_t)sy * (size_t)(r_lo + rr) + (size_t)x;
		const float *c = cur + i;
		const float w0 = c[1];
		const bool mx = v > w0;
		if (!(mx || v < w0)) return;
		bool hit;
		if (full) {
			hit = beats_block(v, mx, c, sy, sz, true) && beats_block(v, mx, prev + i, sy, sz, false) && beats_block(v, mx, next + i, sy, sz, false);
		} else {  // the reference's eight neighbours (the x + 1 one is w0)
			const float n1 = c[-1], n3 = c[sy], n4 = c[-sy], n5 = c[sz], n6 = c[-sz], n0 = prev[i], n7 = next[i];
			hit = mx ? (v > n0 && v > n1 && v > n3 && v > n4 && v > n5 && v > n6 && v > n7)
			         : (v < n0 && v < n1 && v < n3 && v < n4 && v < n5 && v < n6 && v < n7);
		}
		if (hit && opt.refine) {
			double d[4], contrast, Hs[3][3];
			hit = quad_fit(cur, prev, next, i, sy, sz, d, contrast, Hs) && fit_accepts(opt, d, contrast, Hs, absmax);
		}
		if (hit) atomicOr(&mloc[rr * segw + xw], 1ull << bit);
	};
	unsigned cnt = 0;
	for (int seg0 = 0; seg0 < wpr; seg0 += 64) {
		const int seg1 = min(wpr, seg0 + 64);
		for (int ry = r_lo; ry < r_hi; ry++) {
			const int y = y0 + ry;
			if (!(z_in && y >= 1 && y <= ny - 2)) continue;  // wave-uniform
			const float *row = cur + plane0 + (size_t)sy * (size_t)ry;
			for (int xw = seg0; xw < seg1; xw++) {
				const int x = xw * 64 + lane;
				const bool in = x >= 1 && x <= nx - 2;
				const float v = in ? row[x] : 0.0f;
				const bool cnd = in && fabsf(v) > thr;  // == (v > thr || v < -thr)
				const unsigned long long m = __ballot(cnd);
				if (cnd) q[qn + (int)__popcll(m & lt)] = make_uint2(__float_as_uint(v), (unsigned)(((ry - r_lo) << 12) | ((xw - seg0) << 6) | lane));
				qn += (int)__popcll(m);
				if (qn >= 64) {  // entries are consumed from the END so the front stays in place
					qn -= 64;
					evaluate(qn, 64, seg0);
				}
			}
		}
		if (qn > 0) evaluate(0, qn, seg0);
		qn = 0;
		__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
		__builtin_amdgcn_wave_barrier();
		__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
		for (int ry = r_lo; ry < r_hi; ry++) {
			unsigned long long *mrow = masks + ((size_t)(lvl * nz + zi) * ny + (y0 + ry)) * wpr;
			for (int xw = seg0 + lane; xw < seg1; xw += 64) {
				const unsigned long long m = mloc[(ry - r_lo) * segw + xw - seg0];
				mrow[xw] = m;
				cnt += (unsigned)__popcll(m);
				mloc[(ry - r_lo) * segw + xw - seg0] = 0ull;
			}
		}
	}
#pragma unroll
	for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
	if (lane == 0) s_cnt[wid] = cnt;
	__syncthreads();
	if (threadIdx.x == 0) block_counts[b] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
}

void launch_mark_full(const DetectLevels &L, int nlevels, int nx, int ny, const ZRange &zr, int rows, float peak_thresh, const DetectOpts &opt,
                      const DetectBufs &b, hipStream_t st) {
	const int nyb = (ny + rows - 1) / rows;
	const int nzl = zr.zo1 - zr.zo0;
	if (nzl <= 0) return;
	const unsigned nblocks = (unsigned)(nlevels * nzl * nyb);
	if (nblocks == 0) return;
	const size_t mask_lds = sizeof(unsigned long long) * (kFullThreads / 64) * (rows / 4) * (size_t)std::min((nx + 63) >> 6, 64);
	hipLaunchKernelGGL(k_mark_full, dim3(nblocks), dim3(kFullThreads), mask_lds, st, L, nx, ny, zr, nyb, rows, peak_thresh, opt, b.masks,
	                   b.block_counts);
}

// one thread per extremum; the accepted ones (slot >= 0, like k_finalize) write out[slot].  (Not through d_order: the descriptor stage
// leaves that list in its processing order.)
__global__ void __launch_bounds__(256) k_refine(const DevKp *__restrict__ kps, const unsigned *__restrict__ d_count, unsigned cap, unsigned kp_cap,
                                                DogTable T, int num_kp_levels, sift3d_refined *__restrict__ out) {
	const unsigned n = min(*d_count, cap);
	for (unsigned e = blockIdx.x * blockDim.x + threadIdx.x; e < n; e += gridDim.x * blockDim.x) {
		const DevKp k = kps[e];
		if (k.slot < 0 || (unsigned)k.slot >= kp_cap) continue;
		const unsigned s = (unsigned)k.slot;
		const int o = k.octave - T.octave_base, lv = k.level;
		const long long nxo = T.nx[o], sz = (long long)T.nx[o] * T.ny[o];
		const size_t i = (size_t)k.z * (size_t)sz + (size_t)k.y * (size_t)nxo + (size_t)k.x;
		double d[4] = {0.0, 0.0, 0.0, 0.0}, contrast = 0.0, Hs[3][3];
		if (!quad_fit(T.d[o][lv], T.d[o][lv - 1], T.d[o][lv + 1], i, nxo, sz, d, contrast, Hs)) contrast = (double)T.d[o][lv][i];  // (never: detection rejected it)
		const double f = (double)(1 << k.octave);  // the factor of sift3d_keypoint.rx (k_finalize)
		sift3d_refined r;
		r.rx = (float)(((double)k.x + d[0]) * f);
		r.ry = (float)(((double)k.y + d[1]) * f);
		r.rz = (float)(((double)k.z + d[2]) * f);
		r.scale = (float)((double)k.scale * exp2(d[3] / (double)num_kp_levels));
		for (int a = 0; a < 4; a++) r.offset[a] = (float)d[a];
		r.contrast = (float)contrast;
		out[s] = r;
	}
}

void launch_refine(const DevKp *kps, const unsigned *d_count, unsigned cap, unsigned kp_cap, const DogTable &T, int num_kp_levels,
                   sift3d_refined *out, hipStream_t st) {
	hipLaunchKernelGGL(k_refine, dim3(64), dim3(256), 0, st, kps, d_count, cap, kp_cap, T, num_kp_levels, out);
}

}  // namespace s3d
