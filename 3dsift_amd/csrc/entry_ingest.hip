// entry_ingest.hip -- C-ABI of the typed input (include/sift3d_hip.h: sift3d_dtype_bytes, sift3d_create_typed,
// sift3d_volume_to_device).  No reference counterpart.  Kernels: kernels_ingest.hip.  sift3d_volume_to_device is a one-shot entry:
// call state, timing and the order of the checks as DESIGN 4.10 (call_state.h).
#include "call_state.h"
#include "ctx_internal.h"

using namespace s3d;

namespace {
CallState g_ingest[kMaxDev];
}  // namespace

extern "C" int sift3d_dtype_bytes(int dtype, int *bytes) {
	if (!bytes || dtype_bytes(dtype) == 0) { set_last_error("sift3d_dtype_bytes: bad argument"); return SIFT3D_ERR_ARG; }
	*bytes = dtype_bytes(dtype);
	return SIFT3D_OK;
}

extern "C" int sift3d_test_ingest_launch(int dtype, int *block, int *piece_elems, int *ingest_max_blocks, int *absmax_max_blocks) {
	if (!block || !piece_elems || !ingest_max_blocks || !absmax_max_blocks || dtype_bytes(dtype) == 0 || dtype == SIFT3D_DT_F32) return SIFT3D_ERR_ARG;
	ingest_launch_info(dtype, block, piece_elems, ingest_max_blocks, absmax_max_blocks);
	return SIFT3D_OK;
}

extern "C" int sift3d_create_typed(sift3d_handle *out, const void *volume, int dtype, int nx, int ny, int nz, const sift3d_params *params,
                                   int device, int volume_on_device) {
	if (dtype == SIFT3D_DT_F32) return sift3d_create(out, static_cast<const float *>(volume), nx, ny, nz, params, device, volume_on_device);
	if (!out || !volume || nx <= 0 || ny <= 0 || nz <= 0 || dtype_bytes(dtype) == 0) { set_last_error("sift3d_create_typed: bad argument"); return SIFT3D_ERR_ARG; }
	if ((size_t)nx * ny * nz >= ((size_t)1 << 31)) { set_last_error("volume too large for int32 voxel indices"); return SIFT3D_ERR_ARG; }
	CreateCfg cfg;
	cfg.nx = nx; cfg.ny = ny; cfg.nz = nz;
	if (!volume_on_device) { cfg.host_volume = volume; cfg.host_dtype = dtype; }  // uploaded at its own width beside the allocations
	int rc = create_common(out, cfg, params, device);
	if (rc) return rc;
	sift3d_ctx *c = *out;
	// ---- constructor work proper: data_scale (Src/cSIFT3D.cc:161-162) fused with the widening ----
	const size_t V0 = (size_t)nx * ny * nz;
	const void *src = volume;
	if (!volume_on_device) {
		if ((rc = join_upload(c)) != SIFT3D_OK) { sift3d_destroy(c); *out = nullptr; return rc; }
		src = c->in_raw;
	}
	launch_absmax_typed(src, dtype, V0, c->d_inmax, c->stream);
	launch_ingest(src, dtype, V0, c->in.d, c->d_inmax, c->stream);
	// (integer voxels are finite: c->nonfinite stays false, the fused kernels are kept)
	hipError_t e = hipStreamSynchronize(c->stream);
	if (e == hipSuccess) e = hipGetLastError();
	if (e == hipSuccess && c->in_raw) { e = hipFree(c->in_raw); c->in_raw = nullptr; }
	if (e != hipSuccess) { set_last_error(hipGetErrorString(e)); sift3d_destroy(c); *out = nullptr; return SIFT3D_ERR_HIP; }
	return SIFT3D_OK;
}

extern "C" int sift3d_volume_to_device(const void *volume, int dtype, int nx, int ny, int nz, int volume_on_device, int device, float *d_dst,
                                       double *seconds) {
	const int esize = dtype_bytes(dtype);
	// (the voxel count is formed stepwise: three extents of 2^31 - 1 do not fit 64 bits)
	const bool dims_ok = nx >= 1 && ny >= 1 && nz >= 1 && (size_t)nx * ny < ((size_t)1 << 40) / (size_t)nz;
	if (!volume || !d_dst || !dims_ok || esize == 0) { set_last_error("sift3d_volume_to_device: bad argument"); return SIFT3D_ERR_ARG; }
	if (seconds) *seconds = 0;
	int rc = pick_device(device);
	if (rc) return rc;
	CallState &S = g_ingest[device];
	std::lock_guard<std::mutex> lock(S.mu);
	const size_t n = (size_t)nx * ny * nz, bytes = n * (size_t)esize;
	const bool widen = dtype != SIFT3D_DT_F32;
	// device scratch: the integer voxels of a host input
	if ((rc = S.ensure(widen && !volume_on_device ? bytes : 0, 0))) return rc;
	hipStream_t st = S.stream;
	// d_dst is the caller's: whatever the legacy default stream still does with it (or with a device input) comes first
	if ((rc = S.after_legacy_stream())) return rc;
	const void *src = volume;
	if (!volume_on_device) {
		void *land = widen ? static_cast<void *>(S.d.p) : static_cast<void *>(d_dst);
		if ((rc = staged_h2d(land, volume, bytes, device, st)) != SIFT3D_OK) { (void)hipStreamSynchronize(st); return rc; }
		src = land;
	} else if (!widen && volume != d_dst) {
		S3D_HIP_ST(st, hipMemcpyAsync(d_dst, volume, bytes, hipMemcpyDeviceToDevice, st));
	}
	S3D_HIP_ST(st, hipEventRecord(S.e0, st));
	if (widen) {
		launch_ingest(src, dtype, n, d_dst, nullptr, st);
		S3D_HIP_ST(st, hipGetLastError());
	}
	S3D_HIP_ST(st, hipEventRecord(S.e1, st));
	return S.finish(seconds);
}
