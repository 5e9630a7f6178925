// icgn_subset.h -- what the IC-GN kernels of both orders share (kernels_icgn.hip, kernels_icgn2.hip): the walk over a subset, the
// fixed-order wave sum, the per-voxel sample of T (the clamp at T's edge, the weights of the three interpolations, the gather), the
// two pieces of the prepare kernels that do not depend on the order (the Rm pass, the LDS Cholesky) and the pick of the iterate
// kernel by interpolation.  Every function is inline, so each kernel file compiles its own copy.
#pragma once
#include "sift3d_internal.h"

namespace s3d {
namespace icgn {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kRun = -1;  // a prepare kernel's state: go on to the iteration
// how T is interpolated: the values of launch_icgn's `kind` (sift3d_internal.h)
constexpr int kKeys = 0, kLinear = 1, kBspline = 2;

typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));  // 4 x-taps of T at dword alignment
typedef float f2u __attribute__((ext_vector_type(2), aligned(4)));

__device__ inline double wave_sum(double x) {
	for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off);
	return x;
}

// the linear subset index i of offset (dx, dy, dz) advances by kThreads: 256 = sz D^2 + sy D + sx, one carry per axis at most
struct SubsetWalk {
	int r, sx, sy, sz;
	__device__ explicit SubsetWalk(int r_) : r(r_) {
		const int D = 2 * r + 1;
		sz = kThreads / (D * D);
		sy = (kThreads - sz * D * D) / D;
		sx = kThreads - sz * D * D - sy * D;
	}
	__device__ void start(int i, int &dx, int &dy, int &dz) const {
		const int D = 2 * r + 1;
		dz = i / (D * D) - r;
		dy = (i / D) % D - r;
		dx = i % D - r;
	}
	__device__ void next(int &dx, int &dy, int &dz) const {
		const int D = 2 * r + 1;
		dx += sx;
		if (dx > r) { dx -= D; dy++; }
		dy += sy;
		if (dy > r) { dy -= D; dz++; }
		dz += sz;
	}
};

__device__ inline size_t vidx(const IcgnVol &V, int x, int y, int z) { return ((size_t)z * V.ny + y) * V.nx + x; }

// T - tc at the position c + o: c = ci (integer), o in fp32; lo, hx, hy, hz: the range of admissible base taps (1 .. n - 3 cubic,
// 0 .. n - 2 linear); tsy, tsz: T's strides.
// The domain test keeps every tap inside T in fp64; fp32 rounding (a fraction within 2^-25 of 1, c + o a rounding below or onto the
// next integer) can still put the base tap one voxel outside.  The clamp moves it back and the fraction takes the difference, so the
// position is kept (t = 1 or t = -eps at the edge; + 0.f elsewhere: same bits).  The taps are shifted by tc before they are weighted.
template <int KIND>
__device__ inline float sample_shifted(const IcgnVol &T, const int ci[3], const float o[3], float tc, int lo, int hx, int hy, int hz,
                                       size_t tsy, size_t tsz) {
	constexpr bool CUBIC = KIND != kLinear;  // 64 taps
	const float flx = floorf(o[0]), fly = floorf(o[1]), flz = floorf(o[2]);
	const int ux = ci[0] + (int)flx, uy = ci[1] + (int)fly, uz = ci[2] + (int)flz;
	const int gx = min(max(ux, lo), hx), gy = min(max(uy, lo), hy), gz = min(max(uz, lo), hz);
	const float tx = (o[0] - flx) + (float)(ux - gx), ty = (o[1] - fly) + (float)(uy - gy), tz = (o[2] - flz) + (float)(uz - gz);
	float tv;
	if (CUBIC) {
		float w[3][4];
		const float t3[3] = {tx, ty, tz};
#pragma unroll
		for (int a = 0; a < 3; a++) {
			const float t = t3[a], t2 = t * t, tq = t2 * t;
			if (KIND == kBspline) {  // T holds the coefficients
				const float u = 1.f - t, sixth = 1.f / 6.f;
				w[a][0] = sixth * ((u * u) * u);
				w[a][1] = sixth * ((3.f * tq - 6.f * t2) + 4.f);
				w[a][2] = sixth * (((3.f * t2 - 3.f * tq) + 3.f * t) + 1.f);
				w[a][3] = sixth * tq;
			} else {
				w[a][0] = 0.5f * ((2.f * t2 - tq) - t);
				w[a][1] = 0.5f * ((3.f * tq - 5.f * t2) + 2.f);
				w[a][2] = 0.5f * ((4.f * t2 - 3.f * tq) + t);
				w[a][3] = 0.5f * (tq - t2);
			}
		}
		const float *b = T.d + (((size_t)(gz - 1) * T.ny + (gy - 1)) * T.nx + (gx - 1));
		tv = 0.f;
#pragma unroll
		for (int k = 0; k < 4; k++) {
			float zv = 0.f;
#pragma unroll
			for (int j = 0; j < 4; j++) {
				const f4u v = *reinterpret_cast<const f4u *>(b + (k * tsz + j * tsy)) - tc;
				const float row = fmaf(w[0][3], v.w, fmaf(w[0][2], v.z, fmaf(w[0][1], v.y, w[0][0] * v.x)));
				zv = fmaf(w[1][j], row, zv);
			}
			tv = fmaf(w[2][k], zv, tv);
		}
	} else {
		const float *b = T.d + (((size_t)gz * T.ny + gy) * T.nx + gx);
		const f2u a00 = *reinterpret_cast<const f2u *>(b) - tc, a01 = *reinterpret_cast<const f2u *>(b + tsy) - tc;
		const f2u a10 = *reinterpret_cast<const f2u *>(b + tsz) - tc, a11 = *reinterpret_cast<const f2u *>(b + tsz + tsy) - tc;
		const float r00 = fmaf(tx, a00.y - a00.x, a00.x), r01 = fmaf(tx, a01.y - a01.x, a01.x);
		const float r10 = fmaf(tx, a10.y - a10.x, a10.x), r11 = fmaf(tx, a11.y - a11.x, a11.x);
		const float z0 = fmaf(ty, r01 - r00, r00), z1 = fmaf(ty, r11 - r10, r10);
		tv = fmaf(tz, z1 - z0, z0);
	}
	return tv;
}

// ---- the prepare kernels ---------------------------------------------------------------------------------------------------------

// The two functions below hold barriers and are forced inline: left to the inliner's cost model, one of them became a call in the
// first-order kernel.  The test of the POI against R's edge stays spelled in both kernels: as a function, in any of a dozen
// spellings, it cost k_icgn2_prepare two SGPRs.

// Rm: the mean of R over the subset of radius r at q, fp64 in a fixed order through red[][0]; every thread returns the same value.
// Two barriers: red is free again on return.
// MASKED (sift3d_icgn_masked): Aq is the active byte of the voxel q (the volume k_mask_active wrote, in R's layout); an inactive voxel
// is skipped -- R is not read there -- while the walk advances as it does unmasked, and the mean is that of the *n active voxels: their
// count, an integer sum in the wave (through red[][1], exact in fp64).  n = 0 returns NaN.  The unmasked form reads neither argument.
// Labelled (sift3d_icgn_labelled): Aq points into the int volume of interior labels and a voxel is active where its entry equals
// `want`, the POI's own label (> 0, uniform over the workgroup); voxel_on states both rules.
template <class A>
__device__ __forceinline__ bool voxel_on(A a, A want) {
	if constexpr (sizeof(A) == 1) return a != 0;
	else return a == want;
}

template <int K, bool MASKED = false, class A = unsigned char>
__device__ __forceinline__ double subset_mean(const IcgnVol &R, const int q[3], int r, double (*red)[K], const A *Aq = nullptr,
                                              int *n = nullptr, A want = 0) {
	const int D = 2 * r + 1, N = D * D * D;
	const SubsetWalk W(r);
	const float *Rq = R.d + vidx(R, q[0], q[1], q[2]);
	const int sy = R.nx, sz = R.nx * R.ny;
	const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
	double s = 0.0;
	int cnt = 0;
	{
		int dx, dy, dz;
		W.start(tid, dx, dy, dz);
		for (int i = tid; i < N; i += kThreads) {
			if constexpr (MASKED) {
				if (voxel_on(Aq[dz * sz + dy * sy + dx], want)) {
					s += (double)Rq[dz * sz + dy * sy + dx];
					cnt++;
				}
			} else {
				s += (double)Rq[dz * sz + dy * sy + dx];
			}
			W.next(dx, dy, dz);
		}
	}
	s = wave_sum(s);
	if constexpr (MASKED)
		for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off);
	if (lane == 0) {
		red[wv][0] = s;
		if constexpr (MASKED) red[wv][1] = (double)cnt;
	}
	__syncthreads();
	if constexpr (MASKED) {
		*n = (int)(((red[0][1] + red[1][1]) + red[2][1]) + red[3][1]);
		const double Rm = (((red[0][0] + red[1][0]) + red[2][0]) + red[3][0]) / (double)*n;
		__syncthreads();
		return Rm;
	} else {
		const double Rm = (((red[0][0] + red[1][0]) + red[2][0]) + red[3][0]) / (double)N;
		__syncthreads();
		return Rm;
	}
}

// Cholesky H = L L^T in the lower triangle of A (LDS, filled by the caller before the call), a column per step, the trailing update
// spread over the workgroup.  Returns true (uniform) where a pivot is not positive, or where `bad` (thread 0's word: the caller's own
// reason to give up) is set.  The flag is read only between the barriers that follow its write.
template <int N>
__device__ __forceinline__ bool cholesky_lds(double (*A)[N + 1], int *s_fail, bool bad) {
	const int tid = threadIdx.x;
	if (tid == 0) *s_fail = bad;
	__syncthreads();
	bool fail = *s_fail;
	__syncthreads();  // every thread has read the flag before the first pivot may set it
	for (int k = 0; k < N && !fail; k++) {
		if (tid == 0) {
			const double d = A[k][k];
			if (!(d > 0.0)) *s_fail = 1;
			A[k][k] = sqrt(d);
		}
		__syncthreads();
		fail = *s_fail;
		if (fail) break;
		if (tid > k && tid < N) A[tid][k] = A[tid][k] / A[k][k];
		__syncthreads();
		for (int e = tid; e < N * N; e += kThreads) {
			const int i = e / N, j = e % N;
			if (j > k && i >= j) A[i][j] = A[i][j] - A[i][k] * A[j][k];
		}
		__syncthreads();
	}
	return fail;
}

// ---- the launch functions --------------------------------------------------------------------------------------------------------

// the instantiation of an iterate kernel for launch_icgn's `kind`
template <class Kernel>
inline Kernel by_kind(int kind, Kernel keys, Kernel linear, Kernel bspline) {
	return kind == kKeys ? keys : (kind == kLinear ? linear : bspline);
}

}  // namespace icgn
}  // namespace s3d
