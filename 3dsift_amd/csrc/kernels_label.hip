// kernels_label.hip -- connected components of a byte mask (sift3d_mask_label, sift3d_labels_at_points, include/sift3d_hip.h, which
// states the contract; DESIGN 4.13 has the design and the visibility argument).  No reference counterpart.  gfx950 only.
// A union-find over the in-voxels whose parent words live in the output itself: labels[i] is voxel i's parent (a linear voxel index,
// -1 for an out-voxel) until the last kernel turns it into the label.  A parent is never above its child, so the root of a set is its
// lowest voxel, which is also what fixes the numbering.
//   tile       one workgroup per tile of kLabelTX x kLabelTY x kLabelTZ voxels: the union-find of the tile in LDS (integer LDS
//              atomics), then every voxel stores its tile root as a global index, and a tile root the voxels of its set.
//   seams      one thread per voxel: an in-voxel is united with its preceding neighbours (3 of the 6, 13 of the 26) that lie in another
//              tile.  Lock-free: atomicMin on the parent word of the larger root, repeated from the value it returns.
//   flatten    every voxel walks to its root and lowers its own word to it; a tile root adds its count to the root's.
//   count      kept roots (a root whose set has at least min_voxels voxels) per chunk of kLabelChunk voxels; scan: their exclusive
//              sums by one workgroup; number: a kept root's number, 1 + the kept roots before it; final: labels[i] = its root's number.
// Three rules hold in every kernel.  (1) A word that another workgroup may change during the launch is read with an agent-scope
// atomic load or written with an atomic, never through a plain access: the L2s of the XCDs are not coherent inside a launch.  A
// stale parent would still be an ancestor (parents only decrease along the chain to the root), so staleness could cost hops and never
// a label.  (2) No workgroup waits for another: the only loops are the walk up a parent chain, which ends at the root, and the retry
// of a union, whose larger root strictly decreases.  (3) A parent word only decreases: atomicMin, no plain store after the tile kernel.
#include "sift3d_internal.h"

namespace s3d {
namespace {

constexpr int kThreads = 256;
constexpr int kTileVox = kLabelTX * kLabelTY * kLabelTZ;
constexpr int kPer = kTileVox / kThreads;           // voxels of a tile per thread: a thread owns the z column of (lx, ly)
constexpr unsigned kMaxBlocks = 1u << 20;           // larger calls loop (a launch of 2^32 threads is refused by the runtime)
constexpr int kChunkPer = kLabelChunk / kThreads;   // voxels of a chunk per thread
constexpr int kScanPer = 16;                        // chunk sums per thread of a scan step
static_assert(kLabelTX * kLabelTY == kThreads && kPer == kLabelTZ, "a thread per (lx, ly) column of the tile");
static_assert((kLabelTX & (kLabelTX - 1)) == 0 && (kLabelTY & (kLabelTY - 1)) == 0 && (kLabelTZ & (kLabelTZ - 1)) == 0, "tile extents are powers of two");

template <bool Lds>
__device__ inline int word(const int *p) {
	if constexpr (Lds)
		return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
	else
		return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the root of a: ends because a parent is below its child and the root is its own parent
template <bool Lds>
__device__ inline int uf_find(const int *par, int a) {
	for (;;) {
		const int p = word<Lds>(par + a);
		if (p == a) return a;
		a = p;
	}
}

// Unites the sets of a and b.  The larger root is hung under the smaller one by atomicMin; when the word was no root any more (the
// value returned is not a) its former parent `old` may have lost its link to a, so the union goes on with old and b.  The larger of
// the two roots decreases with every round.
template <bool Lds>
__device__ inline void uf_unite(int *par, int a, int b) {
	for (;;) {
		a = uf_find<Lds>(par, a);
		b = uf_find<Lds>(par, b);
		if (a == b) return;
		if (a < b) {
			const int t = a;
			a = b;
			b = t;
		}
		const int old = atomicMin(par + a, b);
		if (old == a) return;
		a = old;
	}
}

// the neighbours of a voxel that precede it in the linear order: every adjacent pair is seen once, from its later voxel
template <bool C26, class F>
__device__ inline void preceding(F f) {
	if constexpr (!C26) {
		f(-1, 0, 0);
		f(0, -1, 0);
		f(0, 0, -1);
	} else {
#pragma unroll
		for (int dz = -1; dz <= 0; dz++)
#pragma unroll
			for (int dy = -1; dy <= 1; dy++)
#pragma unroll
				for (int dx = -1; dx <= 1; dx++)
					if (dz < 0 || dy < 0 || (dy == 0 && dx < 0)) f(dx, dy, dz);
	}
}

__device__ inline bool in_tile(int lx, int ly, int lz) {
	return (unsigned)lx < (unsigned)kLabelTX && (unsigned)ly < (unsigned)kLabelTY && (unsigned)lz < (unsigned)kLabelTZ;
}

template <bool C26>
__global__ __launch_bounds__(kThreads) void k_label_tile(const unsigned char *__restrict__ mask, int nx, int ny, int nz, int tnx, int tny,
                                                        unsigned ntiles, int *__restrict__ labels, int *__restrict__ aux) {
	__shared__ int par[kTileVox];
	__shared__ int cnt[kTileVox];
	const int lx = threadIdx.x % kLabelTX, ly = threadIdx.x / kLabelTX;
	for (unsigned tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
		const int x0 = (int)(tile % (unsigned)tnx) * kLabelTX, y0 = (int)((tile / (unsigned)tnx) % (unsigned)tny) * kLabelTY;
		const int z0 = (int)(tile / ((unsigned)tnx * (unsigned)tny)) * kLabelTZ;
		const int x = x0 + lx, y = y0 + ly;
		const bool column = x < nx && y < ny;
		const size_t g0 = ((size_t)z0 * ny + y) * nx + x, sz = (size_t)nx * ny;
		bool in[kPer];
#pragma unroll
		for (int k = 0; k < kPer; k++) {
			const int l = k * kThreads + threadIdx.x;
			in[k] = column && z0 + k < nz && mask[g0 + k * sz] != 0;
			par[l] = in[k] ? l : -1;
			cnt[l] = 0;
		}
		__syncthreads();
#pragma unroll
		for (int k = 0; k < kPer; k++) {
			if (!in[k]) continue;
			const int l = k * kThreads + threadIdx.x;
			preceding<C26>([&](int dx, int dy, int dz) {
				if (!in_tile(lx + dx, ly + dy, k + dz)) return;
				const int h = l + dx + dy * kLabelTX + dz * kThreads;
				if (word<true>(par + h) >= 0) uf_unite<true>(par, l, h);  // an in-voxel's word is never negative
			});
		}
		__syncthreads();
		int root[kPer];
#pragma unroll
		for (int k = 0; k < kPer; k++) {
			root[k] = -1;
			if (!in[k]) continue;
			root[k] = uf_find<true>(par, k * kThreads + threadIdx.x);
			atomicAdd(cnt + root[k], 1);
		}
		__syncthreads();
#pragma unroll
		for (int k = 0; k < kPer; k++) {
			if (!(column && z0 + k < nz)) continue;
			const int l = k * kThreads + threadIdx.x, r = root[k];
			int p = -1;
			if (r >= 0) p = (int)(((size_t)(z0 + r / kThreads) * ny + (y0 + (r / kLabelTX) % kLabelTY)) * nx + (x0 + r % kLabelTX));
			labels[g0 + k * sz] = p;
			aux[g0 + k * sz] = r == l ? cnt[l] : 0;
		}
		__syncthreads();  // the next tile presets par and cnt
	}
}

template <bool C26>
__global__ __launch_bounds__(kThreads) void k_label_seams(const unsigned char *__restrict__ mask, int nx, int ny, int nz, int *labels) {
	const size_t n = (size_t)nx * ny * nz, sy = (size_t)nx, sz = (size_t)nx * ny;
	for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (size_t)gridDim.x * kThreads) {
		if (!mask[i]) continue;
		const int x = (int)(i % sy), y = (int)((i / sy) % (size_t)ny), z = (int)(i / sz);
		const int lx = x % kLabelTX, ly = y % kLabelTY, lz = z % kLabelTZ;
		if (lx > 0 && lx < kLabelTX - 1 && ly > 0 && ly < kLabelTY - 1 && lz > 0) continue;  // every preceding neighbour is in the tile
		preceding<C26>([&](int dx, int dy, int dz) {
			if (in_tile(lx + dx, ly + dy, lz + dz)) return;  // united by the tile kernel
			if ((unsigned)(x + dx) >= (unsigned)nx || (unsigned)(y + dy) >= (unsigned)ny || z + dz < 0) return;
			const size_t h = (size_t)((long long)i + dx + dy * (long long)sy + dz * (long long)sz);
			if (mask[h]) uf_unite<false>(labels, (int)i, (int)h);
		});
	}
}

__global__ __launch_bounds__(kThreads) void k_label_flatten(size_t n, int *labels, int *aux) {
	for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (size_t)gridDim.x * kThreads) {
		const int p = word<false>(labels + i);
		if (p < 0) continue;
		const int r = uf_find<false>(labels, p);
		if (r != p) atomicMin(labels + i, r);
		// a tile root that is no root: its voxels join the root's.  Only roots are added to, and the unions are over, so aux[i] is final.
		if ((size_t)r != i) {
			const int a = aux[i];
			if (a > 0) atomicAdd(aux + r, a);
		}
	}
}

// is voxel i a kept root?  (after flatten: a root is its own parent and aux holds the voxels of its set)
__device__ inline bool kept_root(const int *__restrict__ labels, const int *__restrict__ aux, size_t i, size_t n, int min_voxels) {
	return i < n && labels[i] == (int)i && aux[i] >= min_voxels;
}

__global__ __launch_bounds__(kThreads) void k_label_count(const int *__restrict__ labels, const int *__restrict__ aux, size_t n, int min_voxels,
                                                         int *__restrict__ sums) {
	__shared__ int total;
	if (threadIdx.x == 0) total = 0;
	__syncthreads();
	const size_t base = (size_t)blockIdx.x * kLabelChunk;
	int c = 0;
#pragma unroll
	for (int k = 0; k < kChunkPer; k++) c += kept_root(labels, aux, base + k * kThreads + threadIdx.x, n, min_voxels) ? 1 : 0;
	for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off);
	if ((threadIdx.x & 63) == 0) atomicAdd(&total, c);
	__syncthreads();
	if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// sums[0 .. nc) -> their exclusive sums, *count = the total; one workgroup, kScanPer consecutive entries per thread and step
__global__ __launch_bounds__(kThreads) void k_label_scan(int *__restrict__ sums, int nc, int *__restrict__ count) {
	__shared__ int sh[kThreads];
	int carry = 0;
	for (int base = 0; base < nc; base += kThreads * kScanPer) {
		const int first = base + threadIdx.x * kScanPer;
		int v[kScanPer], sum = 0;
#pragma unroll
		for (int k = 0; k < kScanPer; k++) {
			v[k] = first + k < nc ? sums[first + k] : 0;
			sum += v[k];
		}
		sh[threadIdx.x] = sum;
		__syncthreads();
		for (int off = 1; off < kThreads; off <<= 1) {
			const int add = (int)threadIdx.x >= off ? sh[threadIdx.x - off] : 0;
			__syncthreads();
			sh[threadIdx.x] += add;
			__syncthreads();
		}
		int run = carry + sh[threadIdx.x] - sum;
		carry += sh[kThreads - 1];
		__syncthreads();  // the next step overwrites sh
#pragma unroll
		for (int k = 0; k < kScanPer; k++) {
			if (first + k < nc) sums[first + k] = run;
			run += v[k];
		}
	}
	if (threadIdx.x == 0) *count = carry;
}

// aux[i] of a root: its number (1 + the kept roots below it), 0 for a root that is not kept
__global__ __launch_bounds__(kThreads) void k_label_number(const int *__restrict__ labels, int *__restrict__ aux, size_t n, int min_voxels,
                                                          const int *__restrict__ sums) {
	__shared__ int wave_cnt[kChunkPer][kThreads / 64];
	const size_t base = (size_t)blockIdx.x * kLabelChunk;
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	bool keep[kChunkPer];
	int before[kChunkPer];  // kept roots of the same wave and step in front of this lane
#pragma unroll
	for (int k = 0; k < kChunkPer; k++) {
		keep[k] = kept_root(labels, aux, base + k * kThreads + threadIdx.x, n, min_voxels);
		const unsigned long long b = __ballot(keep[k]);
		before[k] = __popcll(b & ((1ull << lane) - 1ull));
		if (lane == 0) wave_cnt[k][wave] = __popcll(b);
	}
	__syncthreads();
	int run = sums[blockIdx.x];
#pragma unroll
	for (int k = 0; k < kChunkPer; k++) {
		const size_t i = base + k * kThreads + threadIdx.x;
		int mine = run;
		for (int w = 0; w < kThreads / 64; w++) {
			if (w < wave) mine += wave_cnt[k][w];
			run += wave_cnt[k][w];
		}
		if (i < n && labels[i] == (int)i) aux[i] = keep[k] ? mine + before[k] + 1 : 0;
	}
}

__global__ __launch_bounds__(kThreads) void k_label_final(size_t n, int *__restrict__ labels, const int *__restrict__ aux) {
	for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (size_t)gridDim.x * kThreads) {
		const int p = labels[i];  // no thread reads another's labels word here
		labels[i] = p < 0 ? 0 : aux[p];
	}
}

__global__ __launch_bounds__(kThreads) void k_labels_at(const int *__restrict__ labels, int nx, int ny, int nz, const int *__restrict__ pts, int m,
                                                       int *__restrict__ out) {
	const int i = blockIdx.x * kThreads + threadIdx.x;
	if (i >= m) return;
	const int x = pts[3 * (size_t)i], y = pts[3 * (size_t)i + 1], z = pts[3 * (size_t)i + 2];
	const bool inside = (unsigned)x < (unsigned)nx && (unsigned)y < (unsigned)ny && (unsigned)z < (unsigned)nz;
	out[i] = inside ? labels[((size_t)z * ny + y) * nx + x] : 0;
}

unsigned capped(size_t blocks) { return (unsigned)(blocks < kMaxBlocks ? blocks : kMaxBlocks); }

}  // namespace

void launch_mask_label(const unsigned char *d_mask, int nx, int ny, int nz, int connectivity, int min_voxels, int *d_labels, int *d_aux,
                       int *d_sums, int *d_count, hipStream_t st) {
	const size_t n = (size_t)nx * ny * nz;
	const int tnx = (nx + kLabelTX - 1) / kLabelTX, tny = (ny + kLabelTY - 1) / kLabelTY, tnz = (nz + kLabelTZ - 1) / kLabelTZ;
	const unsigned ntiles = (unsigned)((size_t)tnx * tny * tnz);  // below 2^31: a tile holds a voxel
	const dim3 per_voxel(capped((n + kThreads - 1) / kThreads)), block(kThreads);
	const int nc = (int)label_chunks(n);
	if (connectivity == 26) {
		hipLaunchKernelGGL(k_label_tile<true>, dim3(capped(ntiles)), block, 0, st, d_mask, nx, ny, nz, tnx, tny, ntiles, d_labels, d_aux);
		hipLaunchKernelGGL(k_label_seams<true>, per_voxel, block, 0, st, d_mask, nx, ny, nz, d_labels);
	} else {
		hipLaunchKernelGGL(k_label_tile<false>, dim3(capped(ntiles)), block, 0, st, d_mask, nx, ny, nz, tnx, tny, ntiles, d_labels, d_aux);
		hipLaunchKernelGGL(k_label_seams<false>, per_voxel, block, 0, st, d_mask, nx, ny, nz, d_labels);
	}
	hipLaunchKernelGGL(k_label_flatten, per_voxel, block, 0, st, n, d_labels, d_aux);
	hipLaunchKernelGGL(k_label_count, dim3(nc), block, 0, st, d_labels, d_aux, n, min_voxels, d_sums);
	hipLaunchKernelGGL(k_label_scan, dim3(1), block, 0, st, d_sums, nc, d_count);
	hipLaunchKernelGGL(k_label_number, dim3(nc), block, 0, st, d_labels, d_aux, n, min_voxels, d_sums);
	hipLaunchKernelGGL(k_label_final, per_voxel, block, 0, st, n, d_labels, d_aux);
}

void launch_labels_at(const int *d_labels, int nx, int ny, int nz, const int *d_pts, int m, int *d_out, hipStream_t st) {
	hipLaunchKernelGGL(k_labels_at, dim3((m + kThreads - 1) / kThreads), dim3(kThreads), 0, st, d_labels, nx, ny, nz, d_pts, m, d_out);
}

}  // namespace s3d
