// entry_bspline.hip -- C-ABI of the cubic B-spline prefilter (include/sift3d_hip.h: sift3d_bspline_prefilter).  No reference
// counterpart.  Call state, scratch layout, timing and the order of the checks: DESIGN 4.10 (call_state.h).
#include "call_state.h"

using namespace s3d;

namespace {
CallState g_bspline[kMaxDev];
}  // namespace

extern "C" int sift3d_bspline_prefilter(const float *src, int nx, int ny, int nz, float *dst, int on_device, int device, double *seconds) {
	if (!src || !dst || dst == src || nx < 1 || ny < 1 || nz < 1 || !bspline_prefilter_fits(nx, ny, nz)) {
		set_last_error("sift3d_bspline_prefilter: bad argument");
		return SIFT3D_ERR_ARG;
	}
	if (seconds) *seconds = 0;
	int rc = pick_device(device);
	if (rc) return rc;
	CallState &S = g_bspline[device];
	std::lock_guard<std::mutex> lock(S.mu);
	// device scratch: [the y pass's output | (host inputs) src | dst]
	const size_t bytes = sizeof(float) * (size_t)nx * ny * nz;
	Layout L;
	const size_t o_tmp = L.take(bytes), o_src = L.take(on_device ? 0 : bytes), o_dst = L.take(on_device ? 0 : bytes);
	if ((rc = S.ensure(L.end, 0))) return rc;
	hipStream_t st = S.stream;
	char *D = S.d.p;
	const float *d_src = src;
	float *d_dst = dst;
	if (on_device) {
		if ((rc = S.after_legacy_stream())) return rc;
	} else {
		d_src = reinterpret_cast<float *>(D + o_src);
		d_dst = reinterpret_cast<float *>(D + o_dst);
		S3D_HIP_ST(st, hipMemcpyAsync(D + o_src, src, bytes, hipMemcpyHostToDevice, st));
	}
	S3D_HIP_ST(st, hipEventRecord(S.e0, st));
	launch_bspline_prefilter(d_src, nx, ny, nz, d_dst, reinterpret_cast<float *>(D + o_tmp), st);
	S3D_HIP_ST(st, hipGetLastError());
	if (!on_device) S3D_HIP_ST(st, hipMemcpyAsync(dst, d_dst, bytes, hipMemcpyDeviceToHost, st));
	S3D_HIP_ST(st, hipEventRecord(S.e1, st));
	return S.finish(seconds);
}
