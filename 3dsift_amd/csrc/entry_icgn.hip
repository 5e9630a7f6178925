// entry_icgn.hip -- C-ABI of the IC-GN displacement refinement (include/sift3d_hip.h: sift3d_icgn, sift3d_icgn_bspline,
// sift3d_icgn_init_from_fits, sift3d_default_icgn_options).  No reference counterpart.  Call state, scratch layout, timing and the order of the checks: DESIGN 4.10
// (call_state.h).
#include "call_state.h"

#include <math.h>
#include <string.h>

using namespace s3d;

namespace {
CallState g_icgn[kMaxDev];

// options (NULL: defaults) -> checked values; kind: launch_icgn's (the interpolation option as it is)
bool take_options(const sift3d_icgn_options *o, int &r, int &max_it, double &tol, int &kind) {
	sift3d_icgn_options d;
	sift3d_default_icgn_options(&d);
	if (!o) o = &d;
	if (o->subset_radius < 2 || o->subset_radius > 32 || o->max_iterations < 1 || o->max_iterations > 100) return false;
	if (!std::isfinite(o->tolerance) || o->tolerance < 0.f || (o->interpolation != 0 && o->interpolation != 1)) return false;
	if (o->reserved[0] || o->reserved[1] || o->reserved[2] || o->reserved[3]) return false;
	r = o->subset_radius;
	max_it = o->max_iterations;
	tol = o->tolerance;
	kind = o->interpolation;
	return true;
}
}  // namespace

// the family's state, shared with the second-order entry (entry_icgn2.hip): DESIGN 4.10
CallState &s3d::icgn_call_state(int device) { return g_icgn[device]; }

extern "C" void sift3d_default_icgn_options(sift3d_icgn_options *o) {
	if (!o) return;
	memset(o, 0, sizeof(*o));
	o->subset_radius = 16;
	o->max_iterations = 20;
	o->tolerance = 1e-3f;
	o->interpolation = 0;
}

extern "C" int sift3d_icgn_init_from_fits(const sift3d_affine_fit *fits, const int *points3, int m, double *init12) {
	if (m < 0 || (m > 0 && (!fits || !points3 || !init12))) {
		set_last_error("sift3d_icgn_init_from_fits: bad argument");
		return SIFT3D_ERR_ARG;
	}
	for (int i = 0; i < m; i++) {
		double *p = init12 + 12 * (size_t)i;
		const double *A = fits[i].A;
		const double q[3] = {(double)points3[3 * i], (double)points3[3 * i + 1], (double)points3[3 * i + 2]};
		for (int a = 0; a < 3; a++) {
			// (u, v, w) = L q + b - q, F = L: ux = L00 - 1, uy = L01, ...
			p[4 * a] = fits[i].status != 0 ? NAN : (((A[4 * a] * q[0] + A[4 * a + 1] * q[1]) + A[4 * a + 2] * q[2]) + A[4 * a + 3]) - q[a];
			for (int c = 0; c < 3; c++) p[4 * a + 1 + c] = fits[i].status != 0 ? NAN : A[4 * a + c] - (a == c ? 1.0 : 0.0);
		}
	}
	return SIFT3D_OK;
}

namespace {
// the call behind sift3d_icgn (bspline 0) and sift3d_icgn_bspline (bspline 1: kind 2, T read as coefficients; coef 0: they are made
// here, in the call's scratch)
int run_icgn(const char *who, const float *ref, int rnx, int rny, int rnz, const float *tar, int tnx, int tny, int tnz, const int *points3, int m,
             const double *init12, const sift3d_icgn_options *o, int bspline, int coef, int on_device, int device, sift3d_icgn_result *out,
             double *seconds) {
	int r, max_it, kind;
	double tol;
	if (m < 0 || rnx < 1 || rny < 1 || rnz < 1 || tnx < 1 || tny < 1 || tnz < 1 || !ref || !tar || !out || (m > 0 && !points3) ||
	    !take_options(o, r, max_it, tol, kind) || (bspline && (kind != 0 || (coef != 0 && coef != 1))) ||
	    (bspline && !coef && !bspline_prefilter_fits(tnx, tny, tnz))) {
		set_last_error(std::string(who) + ": bad argument");
		return SIFT3D_ERR_ARG;
	}
	if (bspline) kind = 2;
	const bool filter = bspline && !coef;
	if (seconds) *seconds = 0;
	int rc = pick_device(device);
	if (rc) return rc;
	if (m == 0) return SIFT3D_OK;
	CallState &S = g_icgn[device];
	std::lock_guard<std::mutex> lock(S.mu);
	// device scratch: [results m | state m | (host inputs) ref | tar | points | init | (prefilter) coefficients | the y pass's output];
	// pinned host: [results]
	const size_t nr = (size_t)rnx * rny * rnz, nt = (size_t)tnx * tny * tnz, res_bytes = sizeof(sift3d_icgn_result) * (size_t)m;
	Layout L;
	L.take(res_bytes);
	const size_t o_state = L.take(icgn_state_bytes() * (size_t)m), o_ref = L.take(on_device ? 0 : sizeof(float) * nr);
	const size_t o_tar = L.take(on_device ? 0 : sizeof(float) * nt), o_pts = L.take(on_device ? 0 : sizeof(int) * 3 * (size_t)m);
	const size_t o_init = L.take(on_device || !init12 ? 0 : sizeof(double) * 12 * (size_t)m);
	const size_t o_coef = L.take(filter ? sizeof(float) * nt : 0), o_tmp = L.take(filter ? sizeof(float) * nt : 0);
	if ((rc = S.ensure(L.end, res_bytes))) return rc;
	hipStream_t st = S.stream;
	char *D = S.d.p, *P = S.h.p;
	const float *d_ref = ref, *d_tar = tar;
	const int *d_pts = points3;
	const double *d_init = init12;
	if (on_device) {
		if ((rc = S.after_legacy_stream())) return rc;
	} else {
		d_ref = reinterpret_cast<float *>(D + o_ref);
		d_tar = reinterpret_cast<float *>(D + o_tar);
		d_pts = reinterpret_cast<int *>(D + o_pts);
		S3D_HIP_ST(st, hipMemcpyAsync(D + o_ref, ref, sizeof(float) * nr, hipMemcpyHostToDevice, st));
		S3D_HIP_ST(st, hipMemcpyAsync(D + o_tar, tar, sizeof(float) * nt, hipMemcpyHostToDevice, st));
		S3D_HIP_ST(st, hipMemcpyAsync(D + o_pts, points3, sizeof(int) * 3 * (size_t)m, hipMemcpyHostToDevice, st));
		if (init12) {
			d_init = reinterpret_cast<double *>(D + o_init);
			S3D_HIP_ST(st, hipMemcpyAsync(D + o_init, init12, sizeof(double) * 12 * (size_t)m, hipMemcpyHostToDevice, st));
		}
	}
	S3D_HIP_ST(st, hipEventRecord(S.e0, st));
	if (filter) {
		float *d_coef = reinterpret_cast<float *>(D + o_coef);
		launch_bspline_prefilter(d_tar, tnx, tny, tnz, d_coef, reinterpret_cast<float *>(D + o_tmp), st);
		S3D_HIP_ST(st, hipGetLastError());
		d_tar = d_coef;
	}
	launch_icgn(IcgnVol{d_ref, rnx, rny, rnz}, IcgnVol{d_tar, tnx, tny, tnz}, d_pts, m, d_init, r, max_it, tol, kind, D + o_state,
	            reinterpret_cast<sift3d_icgn_result *>(D), st);
	S3D_HIP_ST(st, hipGetLastError());
	S3D_HIP_ST(st, hipMemcpyAsync(P, D, res_bytes, hipMemcpyDeviceToHost, st));
	S3D_HIP_ST(st, hipEventRecord(S.e1, st));
	if ((rc = S.finish(seconds))) return rc;
	memcpy(out, P, res_bytes);
	return SIFT3D_OK;
}
}  // namespace

extern "C" int sift3d_icgn(const float *ref, int rnx, int rny, int rnz, const float *tar, int tnx, int tny, int tnz, const int *points3, int m,
                           const double *init12, const sift3d_icgn_options *o, int on_device, int device, sift3d_icgn_result *out,
                           double *seconds) {
	return run_icgn("sift3d_icgn", ref, rnx, rny, rnz, tar, tnx, tny, tnz, points3, m, init12, o, 0, 0, on_device, device, out, seconds);
}

extern "C" int sift3d_icgn_bspline(const float *ref, int rnx, int rny, int rnz, const float *tar, int tnx, int tny, int tnz, const int *points3,
                                   int m, const double *init12, const sift3d_icgn_options *o, int tar_is_coefficients, int on_device,
                                   int device, sift3d_icgn_result *out, double *seconds) {
	return run_icgn("sift3d_icgn_bspline", ref, rnx, rny, rnz, tar, tnx, tny, tnz, points3, m, init12, o, 1, tar_is_coefficients, on_device,
	                device, out, seconds);
}
