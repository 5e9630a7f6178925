// kernels_search.hip -- ZNCC integer search (sift3d_zncc_search, include/sift3d_hip.h, which states the numerical contract).
// No reference counterpart.  One workgroup of 256 threads per point of interest (POI); a launch has at most kMaxGroups workgroups and
// each walks its POIs in turn, so the score table (one double per candidate, needed for zncc_second) is a scratch per workgroup.
//   checks     status 2, then Rm and dR over the subset (fp64, two passes over R), status 4, then the admissible range of e per axis in
//              64-bit arithmetic (status 3 when it is empty on an axis) and Tc, the level the sums are centred on: the voxel nearest
//              to the mean of T over the subset at q + g clamped into T (fp64, two passes over it), so that no one voxel sets it
//   chunks     the candidates are taken in chunks of `ec` planes of ez (at most kThreads * kK candidates); slot f = tid + kThreads k of a
//              chunk is candidate (ezl, ey, ex) = (f / E^2, f / E % E, f % E): consecutive lanes own candidates consecutive in ex, so a
//              wave reads consecutive LDS words of T and one word of R (a broadcast).  A thread owns kK candidates and their 3 sums
//              (sum T', sum T'^2, sum R'T' with T' = T - Tc, R' = R - (float)Rm): fp32 along a row of the subset, fp64 across rows.
//   slabs      per chunk the subset is walked in slabs of `zs` planes of dz.  LDS holds the slab of R' (zs D^2 floats) and the planes
//              of T' that the chunk's candidates see under it (zs + ec - 1 planes of W^2 floats, W = 2 (r + s) + 1 the side of the search
//              window).  A voxel of the window outside T is staged as 0 and never enters a score: only admissible candidates are scored.
//   result     argmax of (score, lowest candidate index) per thread, then the wave (xor butterfly) and the waves in index order;
//              zncc_second from the score table, every thread re-reading the slots it wrote.  No float atomics.
// ec and zs are chosen on the host (search_plan) so that the image fits in kLdsFloats: 63 KiB, two workgroups per CU.
#include "sift3d_internal.h"

#include <math.h>

namespace s3d {
namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kK = 5;                  // candidates per thread and chunk
constexpr int kLdsFloats = 16128;      // 63 KiB of dynamic LDS
constexpr int kMaxGroups = 512;        // two resident workgroups on each of 256 CUs
constexpr double kUnscored = -3.0;     // a score table entry that was not scored (scores lie in [-1, 1] up to rounding)
constexpr long long kMaxGuess = 1 << 24;

struct SearchPlan {
	int ec;  // planes of ez per candidate chunk
	int zs;  // planes of dz per slab
};

SearchPlan search_plan(int r, int s) {
	const int D = 2 * r + 1, E = 2 * s + 1, W = D + 2 * s;
	SearchPlan p;
	p.ec = kThreads * kK / (E * E);
	if (p.ec < 1) p.ec = 1;
	if (p.ec > E) p.ec = E;
	while (p.ec > 1 && p.ec * W * W + D * D > kLdsFloats) p.ec--;
	p.zs = (kLdsFloats - (p.ec - 1) * W * W) / (W * W + D * D);
	if (p.zs > D) p.zs = D;
	return p;
}

__device__ inline double wave_sum(double x) {
	for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off);
	return x;
}

// sums of a and b over the workgroup, in a fixed order; every thread returns the same values
__device__ inline void block_sum2(double &a, double &b, double (*red)[2]) {
	const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
	a = wave_sum(a);
	b = wave_sum(b);
	if (lane == 0) { red[wv][0] = a; red[wv][1] = b; }
	__syncthreads();
	a = ((red[0][0] + red[1][0]) + red[2][0]) + red[3][0];
	b = ((red[0][1] + red[1][1]) + red[2][1]) + red[3][1];
	__syncthreads();
}

__device__ inline void write_result(sift3d_search_result *o, int dx, int dy, int dz, int status, double zncc, double second, int cand) {
	o->d[0] = dx; o->d[1] = dy; o->d[2] = dz;
	o->status = status;
	o->zncc = zncc;
	o->zncc_second = second;
	o->candidates = cand;
	o->reserved[0] = o->reserved[1] = o->reserved[2] = 0;
}

__global__ __launch_bounds__(kThreads) void k_zncc_search(IcgnVol R, IcgnVol T, const int *__restrict__ pts, const int *__restrict__ guess, int m,
                                                         int r, int s, int ec, int zs, double *__restrict__ scores,
                                                         sift3d_search_result *__restrict__ out) {
	extern __shared__ float lds[];
	__shared__ double red[kWaves][2];
	__shared__ int redi[kWaves][2];
	const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
	const int D = 2 * r + 1, E = 2 * s + 1, W = D + 2 * s, N = D * D * D, EE = E * E, DD = D * D, WW = W * W;
	float *Tw = lds, *Rs = lds + (zs + ec - 1) * WW;
	double *sc = scores + (size_t)blockIdx.x * ((size_t)EE * E);
	const int tn[3] = {T.nx, T.ny, T.nz};
	for (int poi = blockIdx.x; poi < m; poi += gridDim.x) {  // every branch below is uniform over the workgroup
		const int q[3] = {pts[3 * poi], pts[3 * poi + 1], pts[3 * poi + 2]};
		const int g[3] = {guess ? guess[3 * poi] : 0, guess ? guess[3 * poi + 1] : 0, guess ? guess[3 * poi + 2] : 0};
		sift3d_search_result *o = out + poi;
		if (q[0] < r || q[0] > R.nx - 1 - r || q[1] < r || q[1] > R.ny - 1 - r || q[2] < r || q[2] > R.nz - 1 - r) {
			if (tid == 0) write_result(o, g[0], g[1], g[2], 2, 0.0, -2.0, 0);
			continue;
		}
		// Rm, then dR and sum R' as the chunks form R' (fp32 R - (float)Rm): zncc's correction term
		const float *Rq = R.d + (((size_t)(q[2] - r) * R.ny + (q[1] - r)) * R.nx + (q[0] - r));
		const size_t rsy = (size_t)R.nx, rsz = (size_t)R.nx * R.ny;
		double a = 0.0, b = 0.0;
		for (int i = tid; i < N; i += kThreads) {
			const int dz = i / DD, rem = i - dz * DD, dy = rem / D, dx = rem - dy * D;
			a += (double)Rq[dz * rsz + dy * rsy + dx];
		}
		block_sum2(a, b, red);
		const double Rm = a / (double)N;
		const float rmf = (float)Rm;
		a = 0.0;
		b = 0.0;
		for (int i = tid; i < N; i += kThreads) {
			const int dz = i / DD, rem = i - dz * DD, dy = rem / D, dx = rem - dy * D;
			const float v = Rq[dz * rsz + dy * rsy + dx];
			const double rv = (double)v - Rm;
			a += rv * rv;
			b += (double)(v - rmf);
		}
		block_sum2(a, b, red);
		const double dr = sqrt(a), sr = b;
		if (!(dr > 0.0) || !isfinite(dr)) {
			if (tid == 0) write_result(o, g[0], g[1], g[2], 4, 0.0, -2.0, 0);
			continue;
		}
		// admissible e + s per axis: q + g + e - r >= 0 and q + g + e + r <= n - 1
		int lo[3], hi[3];
		long long base[3];  // T coordinate of the window's first voxel
		bool any = true;
#pragma unroll
		for (int ax = 0; ax < 3; ax++) {
			const long long c = (long long)q[ax] + (long long)g[ax];
			const long long l = (long long)r - c + s, h = (long long)tn[ax] - 1 - r - c + s;
			const bool far = (long long)g[ax] > kMaxGuess || (long long)g[ax] < -kMaxGuess;
			lo[ax] = (int)(l < 0 ? 0 : (l > E ? E : l));
			hi[ax] = (int)(h > E - 1 ? E - 1 : (h < -1 ? -1 : h));
			any = any && !far && lo[ax] <= hi[ax];
			base[ax] = c - s - r;
		}
		if (!any) {
			if (tid == 0) write_result(o, g[0], g[1], g[2], 3, 0.0, -2.0, 0);
			continue;
		}
		// Tc: over the subset of T at q + g clamped into T (the admissible candidate nearest to e = 0), the finite voxel nearest to the
		// fp64 mean of the finite voxels, the lowest index among equals; 0 when no voxel is finite
		float tc;
		{
			long long c[3];
#pragma unroll
			for (int ax = 0; ax < 3; ax++) {
				c[ax] = (long long)q[ax] + (long long)g[ax];
				c[ax] = c[ax] < r ? r : (c[ax] > tn[ax] - 1 - r ? tn[ax] - 1 - r : c[ax]);  // tn >= D: a candidate is admissible
			}
			const float *Tq = T.d + (((size_t)(c[2] - r) * T.ny + (size_t)(c[1] - r)) * T.nx + (size_t)(c[0] - r));
			const size_t tsy = (size_t)T.nx, tsz = (size_t)T.nx * T.ny;
			a = 0.0;
			b = 0.0;
			for (int i = tid; i < N; i += kThreads) {
				const int dz = i / DD, rem = i - dz * DD, dy = rem / D, dx = rem - dy * D;
				const float v = Tq[dz * tsz + dy * tsy + dx];
				if (isfinite(v)) { a += (double)v; b += 1.0; }
			}
			block_sum2(a, b, red);
			const double tmean = a / b;
			double nd = INFINITY;
			int ni = 0x7fffffff;
			for (int i = tid; i < N; i += kThreads) {
				const int dz = i / DD, rem = i - dz * DD, dy = rem / D, dx = rem - dy * D;
				const float v = Tq[dz * tsz + dy * tsy + dx];
				const double dv = fabs((double)v - tmean);
				if (isfinite(v) && dv < nd) { nd = dv; ni = i; }
			}
			for (int sft = 32; sft > 0; sft >>= 1) {
				const double od = __shfl_xor(nd, sft);
				const int oi = __shfl_xor(ni, sft);
				if (od < nd || (od == nd && oi < ni)) { nd = od; ni = oi; }
			}
			if (lane == 0) { red[wv][0] = nd; redi[wv][0] = ni; }
			__syncthreads();
			nd = red[0][0];
			ni = redi[0][0];
			for (int w = 1; w < kWaves; w++)
				if (red[w][0] < nd || (red[w][0] == nd && redi[w][0] < ni)) { nd = red[w][0]; ni = redi[w][0]; }
			__syncthreads();
			tc = 0.f;
			if (ni != 0x7fffffff) {
				const int dz = ni / DD, rem = ni - dz * DD, dy = rem / D, dx = rem - dy * D;
				tc = Tq[dz * tsz + dy * tsy + dx];
			}
		}
		const double sh = (double)tc - (double)rmf, Nd = (double)N;
		double best = kUnscored;
		int bestF = 0x7fffffff, count = 0;
		for (int e0 = lo[2]; e0 <= hi[2]; e0 += ec) {
			const int ecn = min(ec, hi[2] - e0 + 1);
			int off[kK];
			bool valid[kK], adm[kK];
			double S1[kK], S2[kK], S3[kK];
#pragma unroll
			for (int k = 0; k < kK; k++) {
				const int f = tid + kThreads * k, ezl = f / EE, rem = f - ezl * EE, ey = rem / E, ex = rem - ey * E;
				valid[k] = ezl < ecn;
				adm[k] = valid[k] && ey >= lo[1] && ey <= hi[1] && ex >= lo[0] && ex <= hi[0];
				off[k] = valid[k] ? (ezl * W + ey) * W + ex : 0;
				S1[k] = S2[k] = S3[k] = 0.0;
			}
			for (int z0 = 0; z0 < D; z0 += zs) {
				const int zsn = min(zs, D - z0), np = zsn + ecn - 1;
				__syncthreads();  // the previous slab has been read
				for (int i = tid; i < np * WW; i += kThreads) {
					const int p = i / WW, rem = i - p * WW, wy = rem / W, wx = rem - wy * W;
					const long long tz = base[2] + z0 + e0 + p, ty = base[1] + wy, tx = base[0] + wx;
					const bool in = tz >= 0 && tz < T.nz && ty >= 0 && ty < T.ny && tx >= 0 && tx < T.nx;
					Tw[i] = in ? T.d[((size_t)tz * T.ny + (size_t)ty) * T.nx + (size_t)tx] - tc : 0.f;
				}
				for (int i = tid; i < zsn * DD; i += kThreads) {
					const int dz = i / DD, rem = i - dz * DD, dy = rem / D, dx = rem - dy * D;
					Rs[i] = Rq[(z0 + dz) * rsz + dy * rsy + dx] - rmf;
				}
				__syncthreads();
				for (int dz = 0; dz < zsn; dz++)
					for (int dy = 0; dy < D; dy++) {
						const float *rrow = Rs + (dz * D + dy) * D;
						const float *trow = Tw + (dz * W + dy) * W;
						float a1[kK], a2[kK], a3[kK];
#pragma unroll
						for (int k = 0; k < kK; k++) a1[k] = a2[k] = a3[k] = 0.f;
						for (int dx = 0; dx < D; dx++) {
							const float rv = rrow[dx];
#pragma unroll
							for (int k = 0; k < kK; k++) {
								const float t = trow[off[k] + dx];
								a1[k] += t;
								a2[k] = fmaf(t, t, a2[k]);
								a3[k] = fmaf(rv, t, a3[k]);
							}
						}
#pragma unroll
						for (int k = 0; k < kK; k++) {
							S1[k] += (double)a1[k];
							S2[k] += (double)a2[k];
							S3[k] += (double)a3[k];
						}
					}
			}
#pragma unroll
			for (int k = 0; k < kK; k++) {
				if (!valid[k]) continue;
				const int f = tid + kThreads * k, F = e0 * EE + f;
				double score = kUnscored;
				if (adm[k]) {
					const double tm = S1[k] / Nd;
					const double dt2 = S2[k] - S1[k] * tm;
					const double ttm = (S2[k] + 2.0 * sh * S1[k]) + (Nd * sh) * sh;  // sum (T - Rm)^2 from the sums of T - Tc
					if (dt2 > 1e-10 * ttm) {                                          // false for dT = 0 to rounding and for NaN
						const double z = (S3[k] - tm * sr) / (dr * sqrt(dt2));
						if (isfinite(z)) {
							score = z;
							count++;
							if (z > best || (z == best && F < bestF)) { best = z; bestF = F; }
						}
					}
				}
				sc[F] = score;
			}
		}
		// the best candidate of the workgroup: the wave, then the waves in index order
		for (int sft = 32; sft > 0; sft >>= 1) {
			const double ob = __shfl_xor(best, sft);
			const int oF = __shfl_xor(bestF, sft);
			count += __shfl_xor(count, sft);
			if (ob > best || (ob == best && oF < bestF)) { best = ob; bestF = oF; }
		}
		if (lane == 0) { red[wv][0] = best; redi[wv][0] = bestF; redi[wv][1] = count; }
		__syncthreads();
		best = red[0][0];
		bestF = redi[0][0];
		count = redi[0][1];
		for (int w = 1; w < kWaves; w++) {
			const double ob = red[w][0];
			const int oF = redi[w][0];
			count += redi[w][1];
			if (ob > best || (ob == best && oF < bestF)) { best = ob; bestF = oF; }
		}
		__syncthreads();
		if (count == 0) {
			if (tid == 0) write_result(o, g[0], g[1], g[2], 3, 0.0, -2.0, 0);
			continue;
		}
		const int bz = bestF / EE, brem = bestF - bz * EE, by = brem / E, bx = brem - by * E;
		double second = -2.0;
		for (int e0 = lo[2]; e0 <= hi[2]; e0 += ec) {
			const int ecn = min(ec, hi[2] - e0 + 1);
#pragma unroll
			for (int k = 0; k < kK; k++) {
				const int f = tid + kThreads * k, ezl = f / EE, rem = f - ezl * EE, ey = rem / E, ex = rem - ey * E;
				if (ezl >= ecn) continue;
				const double v = sc[e0 * EE + f];  // written by this thread
				const int cheb = max(max(abs(e0 + ezl - bz), abs(ey - by)), abs(ex - bx));
				if (v > -2.5 && cheb > 1 && v > second) second = v;
			}
		}
		for (int sft = 32; sft > 0; sft >>= 1) second = fmax(second, __shfl_xor(second, sft));
		if (lane == 0) red[wv][0] = second;
		__syncthreads();
		second = fmax(fmax(red[0][0], red[1][0]), fmax(red[2][0], red[3][0]));
		__syncthreads();
		if (tid == 0) write_result(o, g[0] + (bx - s), g[1] + (by - s), g[2] + (bz - s), 0, best, second, count);
	}
}

}  // namespace

int search_groups(int m) { return m < kMaxGroups ? m : kMaxGroups; }

size_t search_score_bytes(int m, int s) {
	const size_t E = 2 * (size_t)s + 1;
	return sizeof(double) * E * E * E * (size_t)search_groups(m);
}

void launch_zncc_search(IcgnVol R, IcgnVol T, const int *d_pts, int m, const int *d_guess, int r, int s, double *d_scores,
                        sift3d_search_result *d_out, hipStream_t st) {
	const SearchPlan p = search_plan(r, s);
	const int D = 2 * r + 1, W = D + 2 * s;
	const size_t lds = sizeof(float) * ((size_t)(p.zs + p.ec - 1) * W * W + (size_t)p.zs * D * D);
	hipLaunchKernelGGL(k_zncc_search, dim3(search_groups(m)), dim3(kThreads), lds, st, R, T, d_pts, d_guess, m, r, s, p.ec, p.zs, d_scores, d_out);
}

}  // namespace s3d
