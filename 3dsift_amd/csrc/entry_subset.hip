// entry_subset.hip -- C-ABI of the subset screening (include/sift3d_hip.h: sift3d_subset_quality, sift3d_subset_group_by_radius,
// sift3d_default_subset_options).  No reference counterpart.  Call state, scratch layout, timing and the order of the checks: DESIGN
// 4.10 (call_state.h).
#include "call_state.h"

#include <math.h>
#include <string.h>

using namespace s3d;

namespace {
CallState g_subset[kMaxDev];

constexpr int kMinRadius = 2, kMaxRadius = 32;

// options (NULL: defaults) -> checked values
bool take_options(const sift3d_subset_options *o, SubsetParams &P) {
	sift3d_subset_options d;
	sift3d_default_subset_options(&d);
	if (!o) o = &d;
	if (o->r_min < kMinRadius || o->r_min > kMaxRadius || o->r_max < o->r_min || o->r_max > kMaxRadius) return false;
	if (o->criterion < 0 || o->criterion > 1 || o->reserved0 || o->reserved[0] || o->reserved[1]) return false;
	if (!std::isfinite(o->threshold) || o->threshold < 0.0 || std::isnan(o->level)) return false;
	if (!(o->fraction_min >= 0.0 && o->fraction_min <= 1.0)) return false;
	P.r_min = o->r_min;
	P.r_max = o->r_max;
	P.criterion = o->criterion;
	P.threshold = o->threshold;
	P.level = o->level;
	P.fraction_min = o->fraction_min;
	return true;
}
}  // namespace

extern "C" void sift3d_default_subset_options(sift3d_subset_options *o) {
	if (!o) return;
	memset(o, 0, sizeof(*o));
	o->r_min = 8;
	o->r_max = 16;
	o->level = -INFINITY;
}

extern "C" int sift3d_subset_group_by_radius(const sift3d_subset_result *res, int m, int r_min, int r_max, int *order, int *offsets,
                                             int *count) {
	const bool range = r_min >= kMinRadius && r_min <= kMaxRadius && r_max >= r_min && r_max <= kMaxRadius;
	if (m < 0 || !range || (m > 0 && (!res || !order || !offsets || !count))) {
		set_last_error("sift3d_subset_group_by_radius: bad argument");
		return SIFT3D_ERR_ARG;
	}
	const int groups = r_max - r_min + 1;
	int fill[kMaxRadius + 2] = {0};  // counts, then the next free slot of each group
	for (int i = 0; i < m; i++) {
		if (res[i].status != 0) continue;
		if (res[i].radius < r_min || res[i].radius > r_max) {
			set_last_error("sift3d_subset_group_by_radius: bad argument (a radius outside r_min..r_max)");
			return SIFT3D_ERR_ARG;
		}
		fill[res[i].radius - r_min]++;
	}
	int at = 0;
	for (int g = 0; g < groups; g++) {
		const int n = fill[g];
		if (offsets) offsets[g] = at;
		fill[g] = at;
		at += n;
	}
	if (offsets) offsets[groups] = at;
	if (count) *count = at;
	for (int i = 0; i < m; i++)
		if (res[i].status == 0) order[fill[res[i].radius - r_min]++] = i;
	return SIFT3D_OK;
}

extern "C" int sift3d_subset_quality(const float *ref, int nx, int ny, int nz, const int *points3, int m, const sift3d_subset_options *o,
                                     int on_device, int device, sift3d_subset_result *out, double *seconds) {
	SubsetParams P;
	if (m < 0 || nx < 1 || ny < 1 || nz < 1 || !ref || !out || (m > 0 && !points3) || !take_options(o, P)) {
		set_last_error("sift3d_subset_quality: bad argument");
		return SIFT3D_ERR_ARG;
	}
	if (seconds) *seconds = 0;
	int rc = pick_device(device);
	if (rc) return rc;
	if (m == 0) return SIFT3D_OK;
	CallState &S = g_subset[device];
	std::lock_guard<std::mutex> lock(S.mu);
	// device scratch: [results m | (host inputs) ref | points]; pinned host: [results]
	const size_t nr = (size_t)nx * ny * nz, res_bytes = sizeof(sift3d_subset_result) * (size_t)m;
	const size_t b_ref = on_device ? 0 : sizeof(float) * nr, b_pts = on_device ? 0 : sizeof(int) * 3 * (size_t)m;
	Layout L;
	L.take(res_bytes);
	const size_t o_ref = L.take(b_ref), o_pts = L.take(b_pts);
	if ((rc = S.ensure(L.end, res_bytes))) return rc;
	hipStream_t st = S.stream;
	char *D = S.d.p, *H = S.h.p;
	const float *d_ref = ref;
	const int *d_pts = points3;
	if (on_device && (rc = S.after_legacy_stream())) return rc;
	S3D_HIP_ST(st, upload(d_ref, D, o_ref, b_ref, st));
	S3D_HIP_ST(st, upload(d_pts, D, o_pts, b_pts, st));
	S3D_HIP_ST(st, hipEventRecord(S.e0, st));
	launch_subset_quality(IcgnVol{d_ref, nx, ny, nz}, d_pts, m, P, reinterpret_cast<sift3d_subset_result *>(D), st);
	S3D_HIP_ST(st, hipGetLastError());
	S3D_HIP_ST(st, hipMemcpyAsync(H, D, res_bytes, hipMemcpyDeviceToHost, st));
	S3D_HIP_ST(st, hipEventRecord(S.e1, st));
	if ((rc = S.finish(seconds))) return rc;
	memcpy(out, H, res_bytes);
	return SIFT3D_OK;
}
