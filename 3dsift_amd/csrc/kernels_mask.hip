// kernels_mask.hip -- the per-voxel kernels in front of the masked and the labelled IC-GN (include/sift3d_hip.h: sift3d_icgn_masked,
// sift3d_icgn_labelled, sift3d_mask_from_level).  No reference counterpart.  gfx950 only.  One thread per voxel, one value stored per thread, up to
// kMaskMaxBlocks workgroups; a larger volume is walked by a grid-stride loop (a launch of 2^32 threads or more is refused by the
// runtime).  Both are a single pass over the volume in front of a call that walks it thousands of times.
//   k_mask_active     mask -> the active bytes the masked IC-GN kernels read (kernels_icgn.hip): 1 where the voxel and its six face
//                     neighbours lie in the volume and are in the mask (any non-zero byte), else 0.  A voxel on the volume's boundary
//                     is 0 without a read, so no byte outside mask[0, nx ny nz) is read.
//   k_label_interior  labels -> the int volume the labelled IC-GN kernels read: the voxel's label where the voxel and its six face
//                     neighbours lie in the volume and carry the same positive label, else 0; the boundary is 0 without a read.
//   k_mask_threshold  fp32 volume -> mask: 1 where (double)v >= level (the screening's rule for `material`; a NaN is 0), else 0.
#include "sift3d_internal.h"

namespace s3d {

namespace {

constexpr int kMaskBlock = 256;
constexpr size_t kMaskMaxBlocks = (size_t)1 << 16;  // 2^24 threads: one voxel per thread up to 256^3, a loop beyond (far more waves than are resident)

__global__ void __launch_bounds__(kMaskBlock) k_mask_active(const unsigned char *__restrict__ mask, int nx, int ny, int nz,
                                                            unsigned char *__restrict__ act) {
	const size_t n = (size_t)nx * ny * nz, sy = (size_t)nx, sz = (size_t)nx * ny;
	for (size_t i = (size_t)blockIdx.x * kMaskBlock + threadIdx.x; i < n; i += (size_t)gridDim.x * kMaskBlock) {
		const int x = (int)(i % sy), y = (int)((i / sy) % (size_t)ny), z = (int)(i / sz);
		unsigned char a = 0;
		if (x > 0 && x < nx - 1 && y > 0 && y < ny - 1 && z > 0 && z < nz - 1)
			a = mask[i] && mask[i - 1] && mask[i + 1] && mask[i - sy] && mask[i + sy] && mask[i - sz] && mask[i + sz];
		act[i] = a;
	}
}

__global__ void __launch_bounds__(kMaskBlock) k_label_interior(const int *__restrict__ labels, int nx, int ny, int nz, int *__restrict__ interior) {
	const size_t n = (size_t)nx * ny * nz, sy = (size_t)nx, sz = (size_t)nx * ny;
	for (size_t i = (size_t)blockIdx.x * kMaskBlock + threadIdx.x; i < n; i += (size_t)gridDim.x * kMaskBlock) {
		const int x = (int)(i % sy), y = (int)((i / sy) % (size_t)ny), z = (int)(i / sz);
		int a = 0;
		if (x > 0 && x < nx - 1 && y > 0 && y < ny - 1 && z > 0 && z < nz - 1) {
			const int l = labels[i];
			if (l > 0 && labels[i - 1] == l && labels[i + 1] == l && labels[i - sy] == l && labels[i + sy] == l && labels[i - sz] == l &&
			    labels[i + sz] == l)
				a = l;
		}
		interior[i] = a;
	}
}

__global__ void __launch_bounds__(kMaskBlock) k_mask_threshold(const float *__restrict__ vol, size_t n, double level,
                                                               unsigned char *__restrict__ mask) {
	for (size_t i = (size_t)blockIdx.x * kMaskBlock + threadIdx.x; i < n; i += (size_t)gridDim.x * kMaskBlock)
		mask[i] = (double)vol[i] >= level ? 1 : 0;
}

unsigned blocks_of(size_t n) {
	const size_t b = (n + kMaskBlock - 1) / kMaskBlock;
	return (unsigned)(b < kMaskMaxBlocks ? b : kMaskMaxBlocks);
}

}  // namespace

void launch_mask_active(const unsigned char *d_mask, int nx, int ny, int nz, unsigned char *d_act, hipStream_t st) {
	hipLaunchKernelGGL(k_mask_active, dim3(blocks_of((size_t)nx * ny * nz)), dim3(kMaskBlock), 0, st, d_mask, nx, ny, nz, d_act);
}

void launch_label_interior(const int *d_labels, int nx, int ny, int nz, int *d_interior, hipStream_t st) {
	hipLaunchKernelGGL(k_label_interior, dim3(blocks_of((size_t)nx * ny * nz)), dim3(kMaskBlock), 0, st, d_labels, nx, ny, nz, d_interior);
}

void launch_mask_threshold(const float *d_vol, size_t n, double level, unsigned char *d_mask, hipStream_t st) {
	hipLaunchKernelGGL(k_mask_threshold, dim3(blocks_of(n)), dim3(kMaskBlock), 0, st, d_vol, n, level, d_mask);
}

}  // namespace s3d
