// kernels_ingest.hip -- 8 / 16-bit integer voxels -> the fp32 volume every other kernel reads (include/sift3d_hip.h: sift3d_create_typed,
// sift3d_volume_to_device).  No reference counterpart: the reference widens on the host.  gfx950 only.
//
// Contract: bit for bit what the float path gives for the same voxels widened on the host.
//   * (float)v is exact for every 8 / 16-bit integer
//   * k_absmax_t forms |v| in 32-bit integers (-32768 -> 32768, -128 -> 128) and leaves the fp32 bit pattern of the maximum in the word
//     k_absmax fills: max over (float)|v| and (float) of the max over |v| are the same number
//   * k_ingest<T, true> divides by that word with __fdiv_rn, the IEEE division of k_scale (0 / 0 of an all-zero volume included)
//
// Access shape (both kernels): the source is read in 16-byte pieces (16 elements at 8 bits, 8 at 16 bits) from its first 16-byte
// boundary on; the elements in front of that boundary (head) and behind the last whole piece (tail) are scalar work of workgroup 0,
// as in k_absmax.  Any source address that is a multiple of the element size works.  k_ingest stores float4 where dst + head is
// 16-byte aligned (an instantiation of its own, chosen by the host) and narrower pieces otherwise (any 4-byte alignment of dst); no
// byte outside dst[0, n) is written.
//
// Grids (the project's rule, k_copy16 / grid_for in kernels_pyramid.hip):
//   * k_ingest is a streaming copy that widens: ONE 16-byte source piece per lane and as many workgroups as pieces, the launch form
//     k_copy16 measured 6.29 TB/s for against 4.5-5.0 TB/s as a grid-stride loop.  A workgroup stores 16 (8-bit) or 8 KiB (16-bit).
//   * k_absmax_t is a reduction that ends in one atomicMax per workgroup: at most kAbsmaxMaxBlocks workgroups and a grid-stride loop,
//     the form of k_absmax.
#include <stdint.h>

#include <algorithm>

#include "sift3d_internal.h"

namespace s3d {

namespace {

constexpr int kIngestBlock = 256;
constexpr int kAbsmaxMaxBlocks = 256 * 8;  // grid_for's cap

template <typename T> struct Piece { static constexpr int E = 16 / (int)sizeof(T); };  // elements of a 16-byte piece

// element j of a piece as a 32-bit integer (sign- or zero-extended by T)
template <typename T> __device__ __forceinline__ int piece_elem(const uint4 &v, int j) {
	constexpr int per = 4 / (int)sizeof(T);
	const unsigned w[4] = {v.x, v.y, v.z, v.w};
	return (int)(T)(w[j / per] >> (8 * (int)sizeof(T) * (j % per)));
}

// where the head ends: elements in front of the source's first 16-byte boundary (all n when the volume ends before it)
template <typename T> __host__ __device__ __forceinline__ size_t head_of(const T *src, size_t n) {
	const size_t mis = ((size_t)src & 15) / sizeof(T);
	const size_t head = mis ? (size_t)Piece<T>::E - mis : 0;
	return head < n ? head : n;
}

__device__ __forceinline__ int iabs32(int v) { return v < 0 ? -v : v; }

template <typename T>
__global__ void __launch_bounds__(kIngestBlock) k_absmax_t(const T *__restrict__ src, size_t n, unsigned *dst) {
	constexpr int E = Piece<T>::E;
	int m = 0;
	const size_t head = head_of(src, n);
	const size_t np = (n - head) / E;
	const uint4 *s16 = reinterpret_cast<const uint4 *>(src + head);
	for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < np; i += (size_t)gridDim.x * blockDim.x) {
		const uint4 v = s16[i];
#pragma unroll
		for (int j = 0; j < E; j++) m = max(m, iabs32(piece_elem<T>(v, j)));
	}
	if (blockIdx.x == 0) {
		if (threadIdx.x < head) m = max(m, iabs32((int)src[threadIdx.x]));
		const size_t tail0 = head + np * E;
		if (threadIdx.x < n - tail0) m = max(m, iabs32((int)src[tail0 + threadIdx.x]));
	}
	__shared__ int s[kIngestBlock / 64];
#pragma unroll
	for (int o = 32; o > 0; o >>= 1) m = max(m, __shfl_xor(m, o, 64));
	if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = m;
	__syncthreads();
	if (threadIdx.x == 0) {
		int r = s[0];
		for (int i = 1; i < kIngestBlock / 64; i++) r = max(r, s[i]);
		// at most 32768: exact in fp32; non-negative floats order like their bit patterns (block_max_to_global)
		if (r > 0) atomicMax(dst, __float_as_uint((float)r));
	}
}

template <bool SCALE> __device__ __forceinline__ float ingest_value(int v, float m) {
	return SCALE ? __fdiv_rn((float)v, m) : (float)v;
}

// A lane loads one 16-byte piece; the workgroup's 256 pieces then change hands through LDS, so that every store instruction of a
// wave writes 64 consecutive float4 (a lane that stored its own piece would write 64 / 32 bytes at a stride of as many: 8-bit voxels
// reached half the copy ceiling that way).  A unit = 4 elements = one float4 of output; store k of thread t is unit k * 256 + t.
// ALIGNED (the host's answer for the launch): dst + head is 16-byte aligned, the units are stored as float4.
template <typename T, bool SCALE, bool ALIGNED>
__global__ void __launch_bounds__(kIngestBlock) k_ingest(const T *__restrict__ src, size_t n, float *__restrict__ dst, const unsigned *mx) {
	constexpr int E = Piece<T>::E, U = E / 4, W = (int)sizeof(T);  // units per piece; 32-bit words per unit
	__shared__ uint4 lds[kIngestBlock];
	const float m = SCALE ? __uint_as_float(*mx) : 1.0f;
	const size_t head = head_of(src, n);
	const size_t np = (n - head) / E;
	const size_t p0 = (size_t)blockIdx.x * kIngestBlock;  // the workgroup's first piece
	if (p0 + threadIdx.x < np) lds[threadIdx.x] = reinterpret_cast<const uint4 *>(src + head)[p0 + threadIdx.x];
	__syncthreads();
#pragma unroll
	for (int k = 0; k < U; k++) {
		const unsigned u = (unsigned)k * kIngestBlock + threadIdx.x;
		if (p0 + u / U < np) {  // (a unit lies inside one piece)
			const unsigned *lw = reinterpret_cast<const unsigned *>(lds) + (size_t)u * W;
			unsigned w[W];
#pragma unroll
			for (int q = 0; q < W; q++) w[q] = lw[q];
			float f[4];
#pragma unroll
			for (int j = 0; j < 4; j++) f[j] = ingest_value<SCALE>((int)(T)(w[j * W / 4] >> (8 * W * (j % (4 / W)))), m);
			float *d = dst + head + p0 * E + (size_t)u * 4;
			if (ALIGNED) *reinterpret_cast<float4 *>(d) = make_float4(f[0], f[1], f[2], f[3]);
			else { d[0] = f[0]; d[1] = f[1]; d[2] = f[2]; d[3] = f[3]; }
		}
	}
	if (blockIdx.x == 0) {
		if (threadIdx.x < head) dst[threadIdx.x] = ingest_value<SCALE>((int)src[threadIdx.x], m);
		const size_t tail0 = head + np * E;
		if (threadIdx.x < n - tail0) dst[tail0 + threadIdx.x] = ingest_value<SCALE>((int)src[tail0 + threadIdx.x], m);
	}
}

template <typename T> void absmax_t(const void *src, size_t n, unsigned *d_max_bits, hipStream_t st) {
	const size_t blocks = std::min<size_t>(std::max<size_t>(1, (n / Piece<T>::E + kIngestBlock - 1) / kIngestBlock), kAbsmaxMaxBlocks);
	hipLaunchKernelGGL(k_absmax_t<T>, dim3((unsigned)blocks), dim3(kIngestBlock), 0, st, static_cast<const T *>(src), n, d_max_bits);
}

template <typename T, bool SCALE, bool ALIGNED> void ingest_launch(const T *src, size_t n, float *dst, const unsigned *d_max_bits, hipStream_t st) {
	// every whole piece has a lane whatever the head takes away: n / E pieces at the most
	const size_t blocks = std::max<size_t>(1, (n / Piece<T>::E + kIngestBlock - 1) / kIngestBlock);
	hipLaunchKernelGGL((k_ingest<T, SCALE, ALIGNED>), dim3((unsigned)blocks), dim3(kIngestBlock), 0, st, src, n, dst, d_max_bits);
}

template <typename T> void ingest_t(const void *src_, size_t n, float *dst, const unsigned *d_max_bits, hipStream_t st) {
	const T *src = static_cast<const T *>(src_);
	const bool aligned = (((size_t)(dst + head_of(src, n))) & 15) == 0;
	if (d_max_bits) aligned ? ingest_launch<T, true, true>(src, n, dst, d_max_bits, st) : ingest_launch<T, true, false>(src, n, dst, d_max_bits, st);
	else aligned ? ingest_launch<T, false, true>(src, n, dst, d_max_bits, st) : ingest_launch<T, false, false>(src, n, dst, d_max_bits, st);
}

}  // namespace

int dtype_bytes(int dtype) {
	switch (dtype) {
	case SIFT3D_DT_F32: return 4;
	case SIFT3D_DT_U8: case SIFT3D_DT_I8: return 1;
	case SIFT3D_DT_U16: case SIFT3D_DT_I16: return 2;
	default: return 0;
	}
}

void launch_absmax_typed(const void *src, int dtype, size_t n, unsigned *d_max_bits, hipStream_t st) {
	hipMemsetAsync(d_max_bits, 0, sizeof(unsigned), st);
	switch (dtype) {
	case SIFT3D_DT_U8: absmax_t<uint8_t>(src, n, d_max_bits, st); break;
	case SIFT3D_DT_I8: absmax_t<int8_t>(src, n, d_max_bits, st); break;
	case SIFT3D_DT_U16: absmax_t<uint16_t>(src, n, d_max_bits, st); break;
	case SIFT3D_DT_I16: absmax_t<int16_t>(src, n, d_max_bits, st); break;
	default: break;
	}
}

void launch_ingest(const void *src, int dtype, size_t n, float *dst, const unsigned *d_max_bits, hipStream_t st) {
	switch (dtype) {
	case SIFT3D_DT_U8: ingest_t<uint8_t>(src, n, dst, d_max_bits, st); break;
	case SIFT3D_DT_I8: ingest_t<int8_t>(src, n, dst, d_max_bits, st); break;
	case SIFT3D_DT_U16: ingest_t<uint16_t>(src, n, dst, d_max_bits, st); break;
	case SIFT3D_DT_I16: ingest_t<int16_t>(src, n, dst, d_max_bits, st); break;
	default: break;
	}
}

void ingest_launch_info(int dtype, int *block, int *piece_elems, int *ingest_max_blocks, int *absmax_max_blocks) {
	*block = kIngestBlock;
	*piece_elems = 16 / std::max(1, dtype_bytes(dtype));
	*ingest_max_blocks = 0;  // one piece per lane: no cap
	*absmax_max_blocks = kAbsmaxMaxBlocks;
}

void preload_ingest_kernels() { hipFuncAttributes a; (void)hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&k_ingest<uint16_t, true, true>)); }  // (see kernels_march.hip)

}  // namespace s3d
