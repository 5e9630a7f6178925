// kernels_bspline.hip -- cubic B-spline prefilter of a volume (sift3d_bspline_prefilter, include/sift3d_hip.h, which states the
// numerical contract: a truncated, differenced 33-tap FIR per axis with a mirror boundary).  No reference counterpart.
// Three axis passes, x then y then z, every intermediate volume fp32 in HBM: src -> dst, dst -> tmp, tmp -> dst.  A fused tile would
// need a 16-voxel halo on every side: (t + 32)^3 floats in 160 KiB of LDS leave t <= 2, a read amplification in the thousands;
// fusing two axes reads (t + 32)^2 / t^2 = 2.25 x at t = 64 against 2 x for two passes.  So three passes.
// One kernel for the three axes.  A workgroup of 256 threads takes a tile of 64 outputs along the axis by 64 lines (a line: a run
// along the axis; the 64 lines are consecutive x for the y and z passes, consecutive rows for the x pass).  The tile and its halo,
// 96 x 64 values mirrored into range, go to LDS once; a thread then owns 16 consecutive outputs of one line and keeps their 48
// inputs in registers: 3 LDS reads per output, not 33.  Lanes follow the lines, the LDS row stride is 65: loads, stores and LDS
// accesses of both mappings are free of bank conflicts and global accesses run along x.  The x pass stages its outputs through LDS to
// store them along x.  Products and sums are fp32, not fused (-ffp-contract=off), in the contract's order.  No atomics.
#include "sift3d_internal.h"

namespace s3d {
namespace {

constexpr int kK = 16;                      // taps on each side
constexpr int kThreads = 256;
constexpr int kLines = 64;                  // lines of a tile: the lanes of a wave
constexpr int kPer = 16;                    // outputs of a thread
constexpr int kGroups = kThreads / kLines;  // threads of a line
constexpr int kOut = kPer * kGroups;        // outputs of a tile along the axis: 64
constexpr int kIn = kOut + 2 * kK;          // with the halo: 96
constexpr int kStride = kLines + 1;         // LDS row stride in floats

// h_k = z1^k / (1 + 2 sum_{j=1..K} z1^j), z1 = sqrt(3) - 2, formed in fp64 and rounded to fp32 once
struct Taps {
	float h[kK + 1];
};
constexpr Taps make_taps() {
	const double z1 = 1.7320508075688772 - 2.0;
	double pw[kK + 1] = {1.0};
	double s = 0.0;
	for (int k = 1; k <= kK; k++) {
		pw[k] = pw[k - 1] * z1;
		s += pw[k];
	}
	Taps t{};
	for (int k = 0; k <= kK; k++) t.h[k] = (float)(pw[k] / (1.0 + 2.0 * s));
	return t;
}

// whole-sample symmetric mirror of i into [0, n): period 2n - 2, folded as often as needed; n = 1: 0
__device__ inline int mirror(int i, int n) {
	if (i >= 0 && i < n) return i;
	if (n == 1) return 0;
	const int p = 2 * n - 2;
	int j = i % p;
	if (j < 0) j += p;
	return j < n ? j : p - j;
}

// one axis pass.  An element's index is outer * so + line * sl + a * sa (a: the position along the axis, 0 <= a < n; 0 <= line < nl;
// 0 <= outer < no).  XAXIS: sa = 1, the lines are rows; otherwise sl = 1, the lines are consecutive x.
// grid.x = axis tiles * line tiles * no, axis tiles fastest
template <bool XAXIS>
__global__ __launch_bounds__(kThreads) void k_bspline_axis(const float *__restrict__ src, float *__restrict__ dst, int n, int nl, int no,
                                                          size_t sa, size_t sl, size_t so, int atiles, int ltiles) {
	__shared__ float tile[kIn * kStride];
	const int tid = threadIdx.x;
	unsigned b = blockIdx.x;
	const int a0 = (int)(b % (unsigned)atiles) * kOut;
	b /= (unsigned)atiles;
	const int l0 = (int)(b % (unsigned)ltiles) * kLines;
	const size_t base = (size_t)(b / (unsigned)ltiles) * so;
	// the tile and its halo: positions a0 - K .. a0 + kOut + K - 1, mirrored; a line past nl reads nothing
	if (XAXIS) {
		for (int i = tid; i < kIn * kLines; i += kThreads) {
			const int ai = i % kIn, li = i / kIn;
			float v = 0.f;
			if (l0 + li < nl) v = src[base + (size_t)(l0 + li) * sl + (size_t)mirror(a0 - kK + ai, n)];
			tile[ai * kStride + li] = v;
		}
	} else {
		const int li = tid & (kLines - 1);
		const bool on = l0 + li < nl;
		for (int ai = tid / kLines; ai < kIn; ai += kGroups) {
			float v = 0.f;
			if (on) v = src[base + (size_t)(l0 + li) + (size_t)mirror(a0 - kK + ai, n) * sa];
			tile[ai * kStride + li] = v;
		}
	}
	__syncthreads();
	constexpr Taps kTaps = make_taps();
	const int li = tid & (kLines - 1), g = tid / kLines;
	float w[kPer + 2 * kK];
#pragma unroll
	for (int i = 0; i < kPer + 2 * kK; i++) w[i] = tile[(g * kPer + i) * kStride + li];
	float c[kPer];
#pragma unroll
	for (int j = 0; j < kPer; j++) {
		const float s = w[j + kK];
		float acc = 0.f;
#pragma unroll
		for (int k = kK; k >= 1; k--) acc = acc + kTaps.h[k] * ((w[j + kK - k] - s) + (w[j + kK + k] - s));
		c[j] = s + acc;
	}
	if (XAXIS) {
		__syncthreads();  // every thread holds its inputs in registers: the tile's first kOut rows take the outputs
#pragma unroll
		for (int j = 0; j < kPer; j++) tile[(g * kPer + j) * kStride + li] = c[j];
		__syncthreads();
		for (int i = tid; i < kOut * kLines; i += kThreads) {
			const int ai = i % kOut, lo = i / kOut;
			if (l0 + lo < nl && a0 + ai < n) dst[base + (size_t)(l0 + lo) * sl + (size_t)(a0 + ai)] = tile[ai * kStride + lo];
		}
	} else if (l0 + li < nl) {
#pragma unroll
		for (int j = 0; j < kPer; j++) {
			const int a = a0 + g * kPer + j;
			if (a < n) dst[base + (size_t)(l0 + li) + (size_t)a * sa] = c[j];
		}
	}
}

inline size_t tiles(size_t n, int t) { return (n + (size_t)t - 1) / (size_t)t; }
constexpr size_t kMaxGroups = 0xffffff;  // workgroups of a launch: grid.x * 256 threads stays below 2^32

}  // namespace

bool bspline_prefilter_fits(int nx, int ny, int nz) {
	const size_t rows = (size_t)ny * nz;  // dimensions are ints >= 1: no product here overflows 64 bits
	const size_t gx = tiles(nx, kOut) * tiles(rows, kLines), gy = tiles(ny, kOut) * tiles(nx, kLines) * (size_t)nz;
	const size_t gz = tiles(nz, kOut) * tiles(nx, kLines) * (size_t)ny;
	return rows <= 0x7fffffffu && gx <= kMaxGroups && gy <= kMaxGroups && gz <= kMaxGroups;
}

void launch_bspline_prefilter(const float *d_src, int nx, int ny, int nz, float *d_dst, float *d_tmp, hipStream_t st) {
	const size_t sx = (size_t)nx, sxy = (size_t)nx * ny;
	const int rows = ny * nz;  // bspline_prefilter_fits: below 2^31, and every grid within kMaxGroups
	// x: src -> dst, the lines are the ny * nz rows
	hipLaunchKernelGGL(k_bspline_axis<true>, dim3((unsigned)(tiles(nx, kOut) * tiles(rows, kLines))), dim3(kThreads), 0, st, d_src, d_dst,
	                   nx, rows, 1, (size_t)1, sx, (size_t)0, (int)tiles(nx, kOut), (int)tiles(rows, kLines));
	// y: dst -> tmp, the lines are x, one plane z per outer index
	hipLaunchKernelGGL(k_bspline_axis<false>, dim3((unsigned)(tiles(ny, kOut) * tiles(nx, kLines) * nz)), dim3(kThreads), 0, st, d_dst,
	                   d_tmp, ny, nx, nz, sx, (size_t)1, sxy, (int)tiles(ny, kOut), (int)tiles(nx, kLines));
	// z: tmp -> dst, the lines are x, one row y per outer index
	hipLaunchKernelGGL(k_bspline_axis<false>, dim3((unsigned)(tiles(nz, kOut) * tiles(nx, kLines) * ny)), dim3(kThreads), 0, st, d_tmp,
	                   d_dst, nz, nx, ny, sxy, (size_t)1, sx, (int)tiles(nz, kOut), (int)tiles(nx, kLines));
}

}  // namespace s3d
