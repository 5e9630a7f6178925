// kernels_edt.hip -- the exact squared Euclidean distance transform of a byte mask and the seeded growth of labels over it
// (sift3d_mask_distance, sift3d_mask_from_distance, sift3d_mask_split, include/sift3d_hip.h, which states the contracts; DESIGN 4.14
// has the design and the measurements).  No reference counterpart.  gfx950 only.  All integer.
// The transform is separable: D(x, y, z) = min over z' of [min over y' of [min over x' of out(x', y', z') ? (x - x')^2 : none] + (y - y')^2]
// + (z - z')^2, three launches over a field of one int per voxel, `none` = kEdtNone, which no addition touches.
//   k_edt_x     a wave per row: 64 mask bytes -> one 64-bit ballot of out-voxels, the row's ballots in LDS with, per word, the last set
//               bit at or before its end and the first at or after its start (two wave scans).  A voxel finds the nearest set bit on
//               either side with count-leading / count-trailing zeros in its own word and one look into those tables.
//   k_edt_axis  the y and the z pass, one kernel with the axis' stride as an argument.  A workgroup owns 64 consecutive x, one index
//               of the third axis and kEdtRun consecutive outputs along the axis, and stages them with kEdtHalo entries on either side
//               in LDS.  A voxel starts from best = G(a) and walks outward, k = 1, 2, ..., while k^2 < best; an entry beyond the
//               staged run is read from global memory (through L2).  Exact: an entry at distance k can only lower best below k^2.
//   k_split_grow  one synchronous round of the growth: ping-pong, src -> dst, every voxel writes its own word of dst.
// Visibility: every kernel reads only what an earlier launch wrote (k_edt_axis and k_split_grow write another buffer than they read),
// so the non-coherent L2s of the XCDs do not matter here: plain loads and stores, no flags, no waiting.
#include "sift3d_internal.h"

namespace s3d {
namespace {

constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr unsigned kMaxBlocks = 1u << 20;  // larger calls loop
constexpr unsigned kCountBlocks = 2048;
constexpr int kEdtRun = 96, kEdtHalo = 16, kEdtStage = kEdtRun + 2 * kEdtHalo;  // 128 rows of 64 ints: 32 KiB of LDS
constexpr int kNoLeft = -(1 << 30), kNoRight = 1 << 30;                         // no set bit on that side of the row

__global__ __launch_bounds__(kThreads) void k_edt_x(const unsigned char *__restrict__ mask, int nx, size_t rows, int border, int nw,
                                                   int *__restrict__ out) {
	extern __shared__ unsigned long long edt_row[];  // per wave: nw ballots, then nw ints `last` and nw ints `first`
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	unsigned long long *words = edt_row + (size_t)wave * nw;
	int *last = reinterpret_cast<int *>(edt_row + (size_t)kWaves * nw) + (size_t)wave * 2 * nw, *first = last + nw;
	const int none_left = border ? -1 : kNoLeft, none_right = border ? nx : kNoRight;
	for (size_t rb = (size_t)blockIdx.x * kWaves; rb < rows; rb += (size_t)gridDim.x * kWaves) {  // the same trips for the four waves
		const size_t row = rb + wave;
		const bool live = row < rows;
		const unsigned char *m = mask + (live ? row : 0) * (size_t)nx;
		if (live)
			for (int c = 0; c < nw; c++) {
				const int x = c * 64 + lane;
				const unsigned long long b = __ballot(x < nx && m[x] == 0);  // a bit at or beyond nx is never set
				if (lane == 0) words[c] = b;
			}
		__syncthreads();
		if (live) {
			int carry = none_left;  // the last set bit in front of this group of 64 words
			for (int base = 0; base < nw; base += 64) {
				const int c = base + lane;
				const unsigned long long w = c < nw ? words[c] : 0ull;
				int v = w ? c * 64 + 63 - __builtin_clzll(w) : kNoLeft;
				for (int off = 1; off < 64; off <<= 1) {
					const int u = __shfl_up(v, off);
					if (lane >= off) v = u > v ? u : v;
				}
				v = v > carry ? v : carry;
				if (c < nw) last[c] = v;
				carry = __shfl(v, 63);
			}
			carry = none_right;
			for (int base = ((nw - 1) / 64) * 64; base >= 0; base -= 64) {
				const int c = base + lane;
				const unsigned long long w = c < nw ? words[c] : 0ull;
				int v = w ? c * 64 + __builtin_ctzll(w) : kNoRight;
				for (int off = 1; off < 64; off <<= 1) {
					const int u = __shfl_down(v, off);
					if (lane + off < 64) v = u < v ? u : v;
				}
				v = v < carry ? v : carry;
				if (c < nw) first[c] = v;
				carry = __shfl(v, 0);
			}
		}
		__syncthreads();
		if (live)
			for (int c = 0; c < nw; c++) {
				const int x = c * 64 + lane;
				if (x >= nx) break;
				const unsigned long long w = words[c];
				const unsigned long long ml = w & (~0ull >> (63 - lane)), mr = w & (~0ull << lane);
				const int left = ml ? c * 64 + 63 - __builtin_clzll(ml) : (c > 0 ? last[c - 1] : none_left);
				const int right = mr ? c * 64 + __builtin_ctzll(mr) : (c + 1 < nw ? first[c + 1] : none_right);
				int d = kEdtNone;
				if (left > kNoLeft) d = x - left;
				if (right < kNoRight && right - x < d) d = right - x;
				out[row * (size_t)nx + x] = d == kEdtNone ? kEdtNone : d * d;  // d <= nx + 1: the square fits (the entry's rule)
			}
		__syncthreads();  // the next row overwrites the tables
	}
}

// out(a) = min over a' of in(a') + (a - a')^2 along the axis of extent nA and stride sA; with border, in(-1) = in(nA) = 0.
// nO, sO: extent and stride of the third axis.  A tile: (64 x, one index of the third axis, kEdtRun outputs along the axis).
__global__ __launch_bounds__(kThreads) void k_edt_axis(const int *__restrict__ in, int *__restrict__ out, int nx, int nA, size_t sA, size_t sO,
                                                      int border, unsigned nxc, unsigned nruns, size_t ntiles) {
	__shared__ int st[kEdtStage * 64];
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	for (size_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
		const int x = (int)(t % nxc) * 64 + lane;
		const int a0 = (int)((t / nxc) % nruns) * kEdtRun, s0 = a0 - kEdtHalo;
		const size_t base = (t / ((size_t)nxc * nruns)) * sO + (size_t)(x < nx ? x : 0);
		const bool col = x < nx;
		for (int r = wave; r < kEdtStage; r += kWaves) {
			const int a = s0 + r;
			st[r * 64 + lane] = col && a >= 0 && a < nA ? in[base + (size_t)a * sA] : kEdtNone;
		}
		__syncthreads();
		for (int r = wave; r < kEdtRun && a0 + r < nA; r += kWaves) {
			if (!col) continue;
			const int a = a0 + r;
			int best = st[(r + kEdtHalo) * 64 + lane];
			if (border) {
				const int lo2 = (a + 1) * (a + 1), hi2 = (nA - a) * (nA - a);
				best = best < lo2 ? best : lo2;
				best = best < hi2 ? best : hi2;
			}
			for (int k = 1; k * k < best; k++) {  // k < nA <= 46340: the square fits
				const int lo = a - k, hi = a + k, k2 = k * k;
				if (lo < 0 && hi >= nA) break;
				if (lo >= 0) {
					const int g = lo >= s0 ? st[(lo - s0) * 64 + lane] : in[base + (size_t)lo * sA];
					if (g != kEdtNone && g + k2 < best) best = g + k2;  // none stays none; a finite sum fits (the entry's rule)
				}
				if (hi < nA) {
					const int g = hi < s0 + kEdtStage ? st[(hi - s0) * 64 + lane] : in[base + (size_t)hi * sA];
					if (g != kEdtNone && g + k2 < best) best = g + k2;
				}
			}
			out[base + (size_t)a * sA] = best;
		}
		__syncthreads();  // the next tile overwrites the stage
	}
}

__global__ __launch_bounds__(kThreads) void k_mask_from_distance(const int *__restrict__ dist2, size_t n, int level2, unsigned char *__restrict__ mask) {
	for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (size_t)gridDim.x * kThreads) mask[i] = dist2[i] >= level2 ? 1 : 0;
}

// *total += the workgroup's sum of `mine`: one atomic per workgroup that has something to add.  Every thread of the workgroup calls it.
// (One atomic per wave of a one-voxel-per-thread grid made a round of a wide front cost 16 ms at 512^3 instead of 1.2: DESIGN 4.14.)
__device__ inline void add_block_total(int mine, int *total) {
	__shared__ int part[kWaves];
	for (int off = 32; off > 0; off >>= 1) mine += __shfl_xor(mine, off);
	if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = mine;
	__syncthreads();
	if (threadIdx.x == 0) {
		int sum = 0;
		for (int w = 0; w < kWaves; w++) sum += part[w];
		if (sum > 0) atomicAdd(total, sum);
	}
}

// One round of the growth.  dst[i] = src[i], except for an in-voxel (dist2 > 0) without a label: it takes the label of the labelled
// neighbour (in src) with the largest dist2, the smallest label among equals.  *grown += the voxels labelled.
template <bool C26>
__global__ __launch_bounds__(kThreads) void k_split_grow(const int *__restrict__ dist2, const int *__restrict__ src, int *__restrict__ dst, int nx,
                                                        int ny, int nz, int *__restrict__ grown) {
	const size_t n = (size_t)nx * ny * nz, sy = (size_t)nx, sz = (size_t)nx * ny;
	int mine = 0;
	for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (size_t)gridDim.x * kThreads) {
		int l = src[i];
		if (l == 0 && dist2[i] > 0) {
			const int x = (int)(i % sy), y = (int)((i / sy) % (size_t)ny), z = (int)(i / sz);
			int bd = -1, bl = 0;
			auto look = [&](int dx, int dy, int dz) {
				if ((unsigned)(x + dx) >= (unsigned)nx || (unsigned)(y + dy) >= (unsigned)ny || (unsigned)(z + dz) >= (unsigned)nz) return;
				const size_t h = (size_t)((long long)i + dx + dy * (long long)sy + dz * (long long)sz);
				const int nl = src[h];
				if (nl <= 0) return;
				const int nd = dist2[h];
				if (nd > bd || (nd == bd && nl < bl)) {
					bd = nd;
					bl = nl;
				}
			};
			if constexpr (C26) {
#pragma unroll
				for (int dz = -1; dz <= 1; dz++)
#pragma unroll
					for (int dy = -1; dy <= 1; dy++)
#pragma unroll
						for (int dx = -1; dx <= 1; dx++)
							if (dx || dy || dz) look(dx, dy, dz);
			} else {
				look(-1, 0, 0);
				look(1, 0, 0);
				look(0, -1, 0);
				look(0, 1, 0);
				look(0, 0, -1);
				look(0, 0, 1);
			}
			l = bl;
			mine += l > 0 ? 1 : 0;
		}
		dst[i] = l;
	}
	add_block_total(mine, grown);
}

// rest[i] = 1 for an in-voxel no core reached
__global__ __launch_bounds__(kThreads) void k_split_rest(const int *__restrict__ dist2, const int *__restrict__ labels, size_t n,
                                                        unsigned char *__restrict__ rest) {
	for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (size_t)gridDim.x * kThreads)
		rest[i] = dist2[i] > 0 && labels[i] == 0 ? 1 : 0;
}

// the unreached voxels take their component's number behind the cores' (extra may be null: none is kept); *unlabelled += the in-voxels left at 0
__global__ __launch_bounds__(kThreads) void k_split_finish(const int *__restrict__ dist2, int *__restrict__ labels, const int *__restrict__ extra,
                                                          int cores, size_t n, int *__restrict__ unlabelled) {
	int mine = 0;
	for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (size_t)gridDim.x * kThreads) {
		if (labels[i] != 0 || dist2[i] <= 0) continue;
		const int e = extra ? extra[i] : 0;
		if (e > 0)
			labels[i] = cores + e;
		else
			mine++;
	}
	add_block_total(mine, unlabelled);
}

unsigned capped(size_t blocks) { return (unsigned)(blocks < kMaxBlocks ? (blocks ? blocks : 1) : kMaxBlocks); }
// the kernels that count: a resident grid (256 CUs x 8 workgroups of 256 threads) that strides over the volume, one atomic per workgroup
unsigned counted(size_t n) {
	const size_t blocks = (n + kThreads - 1) / kThreads;
	return (unsigned)(blocks < kCountBlocks ? (blocks ? blocks : 1) : kCountBlocks);
}

void edt_axis(const int *in, int *out, int nx, int nA, size_t sA, int nO, size_t sO, int border, hipStream_t st) {
	const unsigned nxc = (unsigned)((nx + 63) / 64), nruns = (unsigned)((nA + kEdtRun - 1) / kEdtRun);
	const size_t ntiles = (size_t)nxc * nruns * (size_t)nO;
	hipLaunchKernelGGL(k_edt_axis, dim3(capped(ntiles)), dim3(kThreads), 0, st, in, out, nx, nA, sA, sO, border, nxc, nruns, ntiles);
}

}  // namespace

void launch_mask_distance(const unsigned char *d_mask, int nx, int ny, int nz, int border, int *d_dist2, int *d_tmp, hipStream_t st) {
	const size_t rows = (size_t)ny * nz;
	const int nw = (nx + 63) / 64;
	const size_t lds = (size_t)kWaves * nw * (sizeof(unsigned long long) + 2 * sizeof(int));  // nx <= 46339: at most 46400 bytes
	hipLaunchKernelGGL(k_edt_x, dim3(capped((rows + kWaves - 1) / kWaves)), dim3(kThreads), lds, st, d_mask, nx, rows, border, nw, d_dist2);
	edt_axis(d_dist2, d_tmp, nx, ny, (size_t)nx, nz, (size_t)nx * ny, border, st);
	edt_axis(d_tmp, d_dist2, nx, nz, (size_t)nx * ny, ny, (size_t)nx, border, st);
}

void launch_mask_from_distance(const int *d_dist2, size_t n, int level2, unsigned char *d_mask, hipStream_t st) {
	hipLaunchKernelGGL(k_mask_from_distance, dim3(capped((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, d_dist2, n, level2, d_mask);
}

void launch_split_grow(const int *d_dist2, const int *d_src, int *d_dst, int nx, int ny, int nz, int connectivity, int *d_grown, hipStream_t st) {
	const dim3 grid(counted((size_t)nx * ny * nz)), block(kThreads);
	if (connectivity == 26)
		hipLaunchKernelGGL(k_split_grow<true>, grid, block, 0, st, d_dist2, d_src, d_dst, nx, ny, nz, d_grown);
	else
		hipLaunchKernelGGL(k_split_grow<false>, grid, block, 0, st, d_dist2, d_src, d_dst, nx, ny, nz, d_grown);
}

void launch_split_rest(const int *d_dist2, const int *d_labels, size_t n, unsigned char *d_rest, hipStream_t st) {
	hipLaunchKernelGGL(k_split_rest, dim3(capped((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, d_dist2, d_labels, n, d_rest);
}

void launch_split_finish(const int *d_dist2, int *d_labels, const int *d_extra, int cores, size_t n, int *d_unlabelled, hipStream_t st) {
	hipLaunchKernelGGL(k_split_finish, dim3(counted(n)), dim3(kThreads), 0, st, d_dist2, d_labels, d_extra, cores, n,
	                   d_unlabelled);
}

}  // namespace s3d
