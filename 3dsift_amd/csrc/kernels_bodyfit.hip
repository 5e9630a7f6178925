// kernels_bodyfit.hip -- one RANSAC rigid / similarity fit per body (sift3d_fit_rigid_bodies, include/sift3d_hip.h) and the label at
// a real-valued position (sift3d_labels_at_positions).  No reference counterpart.  The numerical contract is sift3d_fit_rigid's; the
// sampler, the scoring expression and the record writer come from ransac_kit.h, the triad and the Horn refit from rigid_kit.h, so
// every fp64 expression is the one the global and the per-point fits evaluate.
//
// The pairs of a body arrive as a segment of an index list: list[off[L-1] .. off[L]) holds the pair indices of body L in ascending
// order (the entry builds it with a stable counting sort on the host).
//   k_rigid_bodies   one workgroup of 256 threads per body.  Hypotheses run 256 at a time, one per thread (draw, three gathers through
//                    the list, the triad); the body's candidates are staged through LDS 256 at a time and every thread scores its
//                    hypothesis on them (broadcast reads); (count, -h) is reduced over the workgroup.  Every thread then solves the best
//                    hypothesis again (uniform draws: the bits its thread had) and runs the refit rounds with the candidates strided by
//                    thread and the sums reduced as k_rigid_refit reduces them, so a body's sums are the global fit's on the same
//                    list.  The mask bytes are written through the list; the entry zeroed them, so a body of status 1 or 2 and a pair
//                    of no body write nothing.
//   k_labels_at_pos  one thread per position: the voxel nearest to it, 0 outside the volume.
#include "sift3d_internal.h"

#include "rigid_kit.h"

namespace s3d {
namespace {

using namespace rigid_kit;

constexpr int kBodyThreads = kRefitThreads;  // the refit's sums are k_rigid_refit's: the same stride and the same reduction

__global__ __launch_bounds__(kBodyThreads) void k_rigid_bodies(const float *__restrict__ pairs, const int *__restrict__ list,
                                                               const int *__restrict__ off, int H, uint32_t s, double tau2, double md2,
                                                               int model, int refine, sift3d_affine_fit *__restrict__ out,
                                                               unsigned char *__restrict__ mask) {
	constexpr int NW = kBodyThreads / 64;
	__shared__ float cand[kBodyThreads][6];
	__shared__ double red[NW][16];
	__shared__ unsigned long long kred[NW];
	const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
	const int body = blockIdx.x + 1;  // the problem index p of the contract
	const int first = off[body - 1], c = off[body] - first;
	const int *__restrict__ mine = list + first;
	const double Z[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
	if (c < 3) {  // uniform: the whole workgroup leaves
		if (tid == 0) write_fit(out + blockIdx.x, Z, Z, 1, c, -1, 0, 0, 0.0);
		return;
	}
	const uint32_t sp = fmix32(s + (uint32_t)body);
	// the samples of hypothesis h, through the list
	auto triad_of = [&](uint32_t h, double P[3][3], double T[3][3]) {
		uint32_t idx[3];
		draw<3>(sp, h, (uint32_t)c, idx);
		for (int j = 0; j < 3; j++) {
			const float *p = pairs + (size_t)mine[idx[j]] * 6;
			for (int i = 0; i < 3; i++) { P[j][i] = p[i]; T[j][i] = p[3 + i]; }
		}
	};
	unsigned long long best = 0;
	for (int hb = 0; hb < H; hb += kBodyThreads) {
		const int h = hb + tid;
		double P[3][3], T[3][3], A[12];
		triad_of((uint32_t)h, P, T);
		const bool ok = solve_triad(P, T, md2, model, A) && h < H;
		const bool wave_on = hb + (tid & ~63) < H;  // a wave past H scores nothing (it still stages and meets the barriers)
		int cnt = 0;
		for (int base = 0; base < c; base += kBodyThreads) {
			__syncthreads();  // the chunk before has been read
			if (base + tid < c) {
				const float *p = pairs + (size_t)mine[base + tid] * 6;
				for (int j = 0; j < 6; j++) cand[tid][j] = p[j];
			}
			__syncthreads();
			if (wave_on) {
				const int nb = min(kBodyThreads, c - base);
				for (int j = 0; j < nb; j++) cnt += resid2(A, cand[j][0], cand[j][1], cand[j][2], cand[j][3], cand[j][4], cand[j][5]) <= tau2;
			}
		}
		if (ok) best = max(best, ((unsigned long long)(unsigned)cnt << 32) | (0xFFFFFFFFu - (unsigned)h));
	}
	for (int o = 32; o > 0; o >>= 1) best = max(best, (unsigned long long)__shfl_xor(best, o));
	if (lane == 0) kred[wv] = best;
	__syncthreads();
	best = 0;
	for (int w = 0; w < NW; w++) best = max(best, kred[w]);
	if (best == 0) {  // every hypothesis degenerate
		if (tid == 0) write_fit(out + blockIdx.x, Z, Z, 2, c, -1, 0, 0, 0.0);
		return;
	}
	const int bh = (int)(0xFFFFFFFFu - (unsigned)(best & 0xFFFFFFFFu)), bc = (int)(best >> 32);
	double A[12], A0[12];
	{
		double P[3][3], T[3][3];
		triad_of((uint32_t)bh, P, T);
		solve_triad(P, T, md2, model, A);
		for (int i = 0; i < 12; i++) A0[i] = A[i];
	}
	auto each = [&](auto &&f) {
		for (int i = tid; i < c; i += kBodyThreads) {
			const float *p = pairs + (size_t)mine[i] * 6;
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
			double x = 0.0;
#pragma unroll
			for (int w = 0; w < NW; w++) x += red[w][k];
			v[k] = x;
		}
		__syncthreads();
	};
	int status = 0, inliers = 0;
	double sumd2 = 0.0;
	refit_rigid(each, sum, A, tau2, md2, model, refine, status, inliers, sumd2);
	for (int i = tid; i < c; i += kBodyThreads) {
		const int pi = mine[i];
		const float *p = pairs + (size_t)pi * 6;
		mask[pi] = resid2(A, p[0], p[1], p[2], p[3], p[4], p[5]) <= tau2 ? 1 : 0;
	}
	if (tid == 0) write_fit(out + blockIdx.x, A, A0, status, c, bh, bc, inliers, sumd2);
}

__global__ __launch_bounds__(256) void k_labels_at_pos(const int *__restrict__ labels, int nx, int ny, int nz, const float *__restrict__ xyz,
                                                       int stride, int n, int *__restrict__ out) {
	const int i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n) return;
	const float *p = xyz + (size_t)i * stride;
	out[i] = label_at_position(labels, nx, ny, nz, p[0], p[1], p[2]);
}

}  // namespace

void launch_rigid_bodies(const float *d_pairs, const int *d_list, const int *d_off, int count, int H, uint32_t s, double tau2, double min_det,
                         int model, int refine, sift3d_affine_fit *d_out, unsigned char *d_mask, hipStream_t st) {
	hipLaunchKernelGGL(k_rigid_bodies, dim3(count), dim3(kBodyThreads), 0, st, d_pairs, d_list, d_off, H, s, tau2, min_det * min_det, model, refine,
	                   d_out, d_mask);
}

void launch_labels_at_positions(const int *d_labels, int nx, int ny, int nz, const float *d_xyz, int stride, int n, int *d_out, hipStream_t st) {
	hipLaunchKernelGGL(k_labels_at_pos, dim3((n + 255) / 256), dim3(256), 0, st, d_labels, nx, ny, nz, d_xyz, stride, n, d_out);
}

}  // namespace s3d
