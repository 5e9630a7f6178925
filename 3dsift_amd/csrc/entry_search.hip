// entry_search.hip -- C-ABI of the ZNCC integer search (include/sift3d_hip.h: sift3d_zncc_search, sift3d_icgn_init_from_search,
// sift3d_default_search_options).  No reference counterpart.  Call state, scratch layout, timing and the order of the checks: DESIGN
// 4.10 (call_state.h).
#include "call_state.h"

#include <math.h>
#include <string.h>

using namespace s3d;

namespace {
CallState g_search[kMaxDev];

// options (NULL: defaults) -> checked values
bool take_options(const sift3d_search_options *o, int &r, int &s) {
	sift3d_search_options d;
	sift3d_default_search_options(&d);
	if (!o) o = &d;
	if (o->subset_radius < 2 || o->subset_radius > 16 || o->search_radius < 1 || o->search_radius > 16) return false;
	for (int k = 0; k < 6; k++)
		if (o->reserved[k]) return false;
	r = o->subset_radius;
	s = o->search_radius;
	return true;
}
}  // namespace

extern "C" void sift3d_default_search_options(sift3d_search_options *o) {
	if (!o) return;
	memset(o, 0, sizeof(*o));
	o->subset_radius = 8;
	o->search_radius = 8;
}

extern "C" int sift3d_icgn_init_from_search(const sift3d_search_result *res, int m, int only_missing, double *init12) {
	if (m < 0 || (m > 0 && (!res || !init12))) {
		set_last_error("sift3d_icgn_init_from_search: bad argument");
		return SIFT3D_ERR_ARG;
	}
	for (int i = 0; i < m; i++) {
		double *p = init12 + 12 * (size_t)i;
		if (res[i].status != 0) continue;
		if (only_missing) {
			bool finite = true;
			for (int k = 0; k < 12; k++) finite = finite && std::isfinite(p[k]);
			if (finite) continue;
		}
		for (int k = 0; k < 12; k++) p[k] = 0.0;
		for (int a = 0; a < 3; a++) p[4 * a] = (double)res[i].d[a];
	}
	return SIFT3D_OK;
}

extern "C" int sift3d_zncc_search(const float *ref, int rnx, int rny, int rnz, const float *tar, int tnx, int tny, int tnz, const int *points3, int m,
                                  const int *guess3, const sift3d_search_options *o, int on_device, int device, sift3d_search_result *out,
                                  double *seconds) {
	int r, s;
	if (m < 0 || rnx < 1 || rny < 1 || rnz < 1 || tnx < 1 || tny < 1 || tnz < 1 || !ref || !tar || !out || (m > 0 && !points3) ||
	    !take_options(o, r, s)) {
		set_last_error("sift3d_zncc_search: bad argument");
		return SIFT3D_ERR_ARG;
	}
	if (seconds) *seconds = 0;
	int rc = pick_device(device);
	if (rc) return rc;
	if (m == 0) return SIFT3D_OK;
	CallState &S = g_search[device];
	std::lock_guard<std::mutex> lock(S.mu);
	// device scratch: [results m | score tables | (host inputs) ref | tar | points | guess]; pinned host: [results]
	const size_t nr = (size_t)rnx * rny * rnz, nt = (size_t)tnx * tny * tnz, res_bytes = sizeof(sift3d_search_result) * (size_t)m;
	Layout L;
	L.take(res_bytes);
	const size_t o_sc = L.take(search_score_bytes(m, s));
	PairPlan in;
	in.plan(L, on_device != 0, nr, nt, m, guess3 ? sizeof(int) * 3 : 0);
	if ((rc = S.ensure(L.end, res_bytes))) return rc;
	hipStream_t st = S.stream;
	char *D = S.d.p, *P = S.h.p;
	const float *d_ref = ref, *d_tar = tar;
	const int *d_pts = points3;
	const void *d_gs = guess3;
	if ((rc = S.stage_pair(in, on_device != 0, d_ref, d_tar, d_pts, d_gs))) return rc;
	S3D_HIP_ST(st, hipEventRecord(S.e0, st));
	launch_zncc_search(IcgnVol{d_ref, rnx, rny, rnz}, IcgnVol{d_tar, tnx, tny, tnz}, d_pts, m, static_cast<const int *>(d_gs), r, s,
	                   reinterpret_cast<double *>(D + o_sc), reinterpret_cast<sift3d_search_result *>(D), st);
	S3D_HIP_ST(st, hipGetLastError());
	S3D_HIP_ST(st, hipMemcpyAsync(P, D, res_bytes, hipMemcpyDeviceToHost, st));
	S3D_HIP_ST(st, hipEventRecord(S.e1, st));
	if ((rc = S.finish(seconds))) return rc;
	memcpy(out, P, res_bytes);
	return SIFT3D_OK;
}
