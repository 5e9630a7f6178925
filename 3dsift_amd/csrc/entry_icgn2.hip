// entry_icgn2.hip -- C-ABI of the second-order IC-GN (include/sift3d_hip.h: sift3d_icgn2, sift3d_icgn2_init_from_icgn,
// sift3d_strain_input_from_icgn2).  No reference counterpart.  Call state, scratch layout, timing and the order of the checks: DESIGN
// 4.10 (call_state.h).  The call runs on the IC-GN family's state (entry_icgn.hip): the two orders are used one after the other in one
// chain, so a second mutex would never be contended, the grown scratch block is reused, and the process creates no further stream.
// The host-only logic lives in icgn2_host.h.
#include "call_state.h"
#include "icgn2_host.h"

#include <string.h>

using namespace s3d;

extern "C" int sift3d_icgn2_init_from_icgn(const sift3d_icgn_result *res, int m, double *init30) {
	if (m < 0 || (m > 0 && (!res || !init30))) {
		set_last_error("sift3d_icgn2_init_from_icgn: bad argument");
		return SIFT3D_ERR_ARG;
	}
	for (int i = 0; i < m; i++) icgn2_init_row(res[i], init30 + 30 * (size_t)i);
	return SIFT3D_OK;
}

extern "C" int sift3d_strain_input_from_icgn2(const sift3d_icgn2_result *res, int m, double zncc_min, int accept_unconverged, double *disp3,
                                              unsigned char *valid) {
	if (m < 0 || !std::isfinite(zncc_min) || (m > 0 && (!res || !disp3 || !valid))) {
		set_last_error("sift3d_strain_input_from_icgn2: bad argument");
		return SIFT3D_ERR_ARG;
	}
	for (int i = 0; i < m; i++) valid[i] = icgn2_strain_row(res[i], zncc_min, accept_unconverged, disp3 + 3 * (size_t)i);
	return SIFT3D_OK;
}

extern "C" int sift3d_icgn2(const float *ref, int rnx, int rny, int rnz, const float *tar, int tnx, int tny, int tnz, const int *points3, int m,
                            const double *init30, const sift3d_icgn_options *o, int tar_is_coefficients, int on_device, int device,
                            sift3d_icgn2_result *out, double *seconds) {
	int r, max_it, kind;
	double tol;
	if (!icgn2_args_ok(ref, rnx, rny, rnz, tar, tnx, tny, tnz, points3, m, o, tar_is_coefficients, out, r, max_it, tol, kind) ||
	    (kind == 2 && !tar_is_coefficients && !bspline_prefilter_fits(tnx, tny, tnz))) {
		set_last_error("sift3d_icgn2: bad argument");
		return SIFT3D_ERR_ARG;
	}
	const bool filter = kind == 2 && !tar_is_coefficients;
	if (seconds) *seconds = 0;
	int rc = pick_device(device);
	if (rc) return rc;
	if (m == 0) return SIFT3D_OK;
	CallState &S = icgn_call_state(device);
	std::lock_guard<std::mutex> lock(S.mu);
	const size_t nr = (size_t)rnx * rny * rnz, nt = (size_t)tnx * tny * tnz;
	const Icgn2Layout L = icgn2_layout(m, nr, nt, on_device != 0, init30 != nullptr, filter, icgn2_state_bytes());
	if ((rc = S.ensure(L.end, L.res_bytes))) return rc;
	hipStream_t st = S.stream;
	char *D = S.d.p, *P = S.h.p;
	const float *d_ref = ref, *d_tar = tar;
	const int *d_pts = points3;
	const double *d_init = init30;
	if (on_device) {
		if ((rc = S.after_legacy_stream())) return rc;
	} else {
		d_ref = reinterpret_cast<float *>(D + L.o_ref);
		d_tar = reinterpret_cast<float *>(D + L.o_tar);
		d_pts = reinterpret_cast<int *>(D + L.o_pts);
		S3D_HIP_ST(st, hipMemcpyAsync(D + L.o_ref, ref, sizeof(float) * nr, hipMemcpyHostToDevice, st));
		S3D_HIP_ST(st, hipMemcpyAsync(D + L.o_tar, tar, sizeof(float) * nt, hipMemcpyHostToDevice, st));
		S3D_HIP_ST(st, hipMemcpyAsync(D + L.o_pts, points3, sizeof(int) * 3 * (size_t)m, hipMemcpyHostToDevice, st));
		if (init30) {
			d_init = reinterpret_cast<double *>(D + L.o_init);
			S3D_HIP_ST(st, hipMemcpyAsync(D + L.o_init, init30, sizeof(double) * 30 * (size_t)m, hipMemcpyHostToDevice, st));
		}
	}
	S3D_HIP_ST(st, hipEventRecord(S.e0, st));
	if (filter) {
		float *d_coef = reinterpret_cast<float *>(D + L.o_coef);
		launch_bspline_prefilter(d_tar, tnx, tny, tnz, d_coef, reinterpret_cast<float *>(D + L.o_tmp), st);
		S3D_HIP_ST(st, hipGetLastError());
		d_tar = d_coef;
	}
	launch_icgn2(IcgnVol{d_ref, rnx, rny, rnz}, IcgnVol{d_tar, tnx, tny, tnz}, d_pts, m, d_init, r, max_it, tol, kind, D + L.o_state,
	             reinterpret_cast<sift3d_icgn2_result *>(D), st);
	S3D_HIP_ST(st, hipGetLastError());
	S3D_HIP_ST(st, hipMemcpyAsync(P, D, L.res_bytes, hipMemcpyDeviceToHost, st));
	S3D_HIP_ST(st, hipEventRecord(S.e1, st));
	if ((rc = S.finish(seconds))) return rc;
	memcpy(out, P, L.res_bytes);
	return SIFT3D_OK;
}
