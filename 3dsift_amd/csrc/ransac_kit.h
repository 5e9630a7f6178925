// ransac_kit.h -- what the RANSAC kernels of both motion models share (kernels_ransac.hip: affine; kernels_rigid.hip: rigid and
// similarity): the sampler, the scoring expression, the wave sum, the running top-k of the local fits and the record writer.
// Every fp64 expression follows the contract of include/sift3d_hip.h term by term; include after sift3d_internal.h, whose pragma
// keeps FMA contraction off.
#ifndef S3D_RANSAC_KIT_H
#define S3D_RANSAC_KIT_H

#include "sift3d_internal.h"

#include <limits.h>

namespace s3d {
namespace ransac_kit {

constexpr int kChunk = 256;  // pairs per scoring workgroup
constexpr int kRefitThreads = 256;

__host__ __device__ inline uint32_t fmix32(uint32_t x) {
	x ^= x >> 16;
	x *= 0x85ebca6bu;
	x ^= x >> 13;
	x *= 0xc2b2ae35u;
	x ^= x >> 16;
	return x;
}

// the first ND candidate positions of hypothesis h (draw j depends on the draws before it only); sp = fmix32(s + p); c >= ND
template <int ND>
__device__ inline void draw(uint32_t sp, uint32_t h, uint32_t c, uint32_t idx[ND]) {
#pragma unroll
	for (int j = 0; j < ND; j++) {
		const uint32_t u = fmix32(sp + (4u * h + (uint32_t)j));
		uint32_t i = (uint32_t)(((uint64_t)u * c) >> 32);
		for (;;) {
			bool dup = false;
			for (int q = 0; q < j; q++) dup |= (idx[q] == i);
			if (!dup) break;
			i = (i + 1 == c) ? 0u : i + 1;
		}
		idx[j] = i;
	}
}

__device__ inline double resid2(const double A[12], double rx, double ry, double rz, double tx, double ty, double tz) {
	const double e0 = (((A[0] * rx + A[1] * ry) + A[2] * rz) + A[3]) - tx;
	const double e1 = (((A[4] * rx + A[5] * ry) + A[6] * rz) + A[7]) - ty;
	const double e2 = (((A[8] * rx + A[9] * ry) + A[10] * rz) + A[11]) - tz;
	return (e0 * e0 + e1 * e1) + e2 * e2;
}

__device__ inline double wave_sum(double x) {
#pragma unroll
	for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off);
	return x;  // (a + b == b + a: every lane ends with the same bits)
}

__device__ inline float readlane_f(float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); }

__device__ inline void write_fit(sift3d_affine_fit *o, const double A[12], const double hyp[12], int status, int cand, int best_h, int best_count,
                                 int inliers, double sumd2) {
	for (int i = 0; i < 12; i++) { o->A[i] = A[i]; o->hyp[i] = hyp[i]; }
	o->status = status;
	o->candidates = cand;
	o->best_hypothesis = best_h;
	o->best_count = best_count;
	o->inliers = inliers;
	o->rms = inliers > 0 ? (float)sqrt(sumd2 / (double)inliers) : 0.f;
	o->reserved[0] = o->reserved[1] = 0;
}

// best hypothesis of a workgroup of kRefitThreads: the most inliers, ties to the smallest h; key 0 = every one degenerate
// (count < 0).  kred: one slot per wave; ends with a barrier passed.
__device__ inline unsigned long long best_key(const int *__restrict__ count, int H, unsigned long long *kred) {
	const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
	unsigned long long key = 0;
	for (int h = tid; h < H; h += kRefitThreads) {
		const int c = count[h];
		if (c >= 0) key = max(key, ((unsigned long long)(unsigned)c << 32) | (0xFFFFFFFFu - (unsigned)h));
	}
	for (int off = 32; off > 0; off >>= 1) key = max(key, (unsigned long long)__shfl_xor(key, off));
	if (lane == 0) kred[wv] = key;
	__syncthreads();
	key = 0;
	for (int w = 0; w < kRefitThreads / 64; w++) key = max(key, kred[w]);
	return key;
}

// the candidate list of query (qx, qy, qz), one wave: on return lane l < c holds entry l of the k smallest (d2, i) (empty entries are
// (+inf, INT_MAX)); chunks of 64 pairs are skipped by a ballot against the current k-th entry.  Returns c (wave-uniform).
__device__ inline int topk_neighbours(const float *__restrict__ pairs, int n, float qx, float qy, float qz, int k, float r2, int lane, float &myd,
                                      int &myi) {
	myd = __int_as_float(0x7f800000);
	myi = INT_MAX;
	int c = 0;
	for (int base = 0; base < n; base += 64) {
		const int i = base + lane;
		float d2 = 0.f;
		bool ok = false;
		if (i < n) {
			const float *pp = pairs + (size_t)i * 6;
			const float dx = pp[0] - qx, dy = pp[1] - qy, dz = pp[2] - qz;
			d2 = (dx * dx + dy * dy) + dz * dz;
			ok = (d2 == d2) && (r2 < 0.f || d2 <= r2);
		}
		const float kd = __shfl(myd, k - 1);
		const int ki = __shfl(myi, k - 1);
		unsigned long long b = __ballot(ok && (d2 < kd || (d2 == kd && i < ki)));
		while (b) {
			const int src = __ffsll((long long)b) - 1;
			b &= b - 1;
			const float nd = readlane_f(d2, src);
			const int ni = __builtin_amdgcn_readlane(i, src);
			const float cd = __shfl(myd, k - 1);
			const int ci = __shfl(myi, k - 1);
			if (!(nd < cd || (nd == cd && ni < ci))) continue;  // (the list filled up or tightened since the ballot)
			const bool less = lane < k && (myd < nd || (myd == nd && myi < ni));
			const int pos = __popcll(__ballot(less));
			const float pd = __shfl_up(myd, 1);
			const int pi = __shfl_up(myi, 1);
			if (lane > pos) { myd = pd; myi = pi; }
			else if (lane == pos) { myd = nd; myi = ni; }
			c = min(c + 1, k);
		}
	}
	return c;
}

}  // namespace ransac_kit
}  // namespace s3d

#endif
