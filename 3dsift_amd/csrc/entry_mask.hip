// entry_mask.hip -- C-ABI of sift3d_mask_from_level (include/sift3d_hip.h): an fp32 volume -> the byte mask sift3d_icgn_masked takes.
// No reference counterpart.  Kernel: kernels_mask.hip.  A one-shot entry: call state, timing and the order of the checks as DESIGN
// 4.10 (call_state.h).
#include "call_state.h"

#include <math.h>

using namespace s3d;

namespace {
CallState g_mask[kMaxDev];
}  // namespace

extern "C" int sift3d_mask_from_level(const float *vol, int nx, int ny, int nz, double level, unsigned char *mask, int on_device, int device,
                                      double *seconds) {
	// (the voxel count is formed stepwise: three extents of 2^31 - 1 do not fit 64 bits; the kernel walks any count by a grid-stride loop)
	const bool dims_ok = nx >= 1 && ny >= 1 && nz >= 1 && (size_t)nx * ny < ((size_t)1 << 39) / (size_t)nz;
	if (!vol || !mask || !dims_ok || std::isnan(level)) {
		set_last_error("sift3d_mask_from_level: bad argument");
		return SIFT3D_ERR_ARG;
	}
	if (seconds) *seconds = 0;
	int rc = pick_device(device);
	if (rc) return rc;
	CallState &S = g_mask[device];
	std::lock_guard<std::mutex> lock(S.mu);
	const size_t n = (size_t)nx * ny * nz;
	// device scratch of a call on host memory: [volume | mask]
	Layout L;
	const size_t o_vol = L.take(on_device ? 0 : sizeof(float) * n), o_mask = L.take(on_device ? 0 : n);
	if ((rc = S.ensure(L.end, 0))) return rc;
	hipStream_t st = S.stream;
	const float *d_vol = vol;
	unsigned char *d_mask = mask;
	if (on_device) {
		if ((rc = S.after_legacy_stream())) return rc;
	} else {
		S3D_HIP_ST(st, upload(d_vol, S.d.p, o_vol, sizeof(float) * n, st));
		d_mask = reinterpret_cast<unsigned char *>(S.d.p + o_mask);
	}
	S3D_HIP_ST(st, hipEventRecord(S.e0, st));
	launch_mask_threshold(d_vol, n, level, d_mask, st);
	S3D_HIP_ST(st, hipGetLastError());
	S3D_HIP_ST(st, hipEventRecord(S.e1, st));
	if (!on_device) S3D_HIP_ST(st, hipMemcpyAsync(mask, d_mask, n, hipMemcpyDeviceToHost, st));
	if ((rc = S.finish(seconds))) return rc;
	if (!on_device) S3D_HIP_ST(st, hipStreamSynchronize(st));
	return SIFT3D_OK;
}
