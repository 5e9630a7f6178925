// entry_icgn.hip -- C-ABI of the IC-GN displacement refinement of both orders (include/sift3d_hip.h: sift3d_icgn, sift3d_icgn_bspline,
// sift3d_icgn2, sift3d_icgn_masked, sift3d_icgn_labelled, sift3d_icgn_init_from_fits, sift3d_icgn_init_from_body_fits, sift3d_icgn2_init_from_icgn, sift3d_strain_input_from_icgn2, sift3d_default_icgn_options).
// No reference counterpart.  Call state, scratch layout, timing and the order of the checks: DESIGN 4.10 (call_state.h).  The three
// calls run through one shell on one state per device: the two orders are used one after the other in one chain, so a second mutex
// would never be contended, the grown scratch block is reused, and the process creates no further stream.  The host-only logic lives
// in icgn_host.h.
#include "call_state.h"
#include "icgn_host.h"

#include <math.h>
#include <string.h>

using namespace s3d;

namespace {
CallState g_icgn[kMaxDev];
}  // namespace

extern "C" void sift3d_default_icgn_options(sift3d_icgn_options *o) {
	if (o) *o = icgn_default_options();
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

extern "C" int sift3d_icgn_init_from_body_fits(const sift3d_affine_fit *fits, int count, const int *poi_label, const int *points3, int m,
                                               double *init12) {
	if (m < 0 || count < 0 || (count > 0 && !fits) || (m > 0 && (!poi_label || !points3 || !init12))) {
		set_last_error("sift3d_icgn_init_from_body_fits: bad argument");
		return SIFT3D_ERR_ARG;
	}
	for (int i = 0; i < m; i++) {
		if (poi_label[i] >= 1 && poi_label[i] <= count) {
			sift3d_icgn_init_from_fits(fits + (poi_label[i] - 1), points3 + 3 * (size_t)i, 1, init12 + 12 * (size_t)i);
		} else {
			for (int k = 0; k < 12; k++) init12[12 * (size_t)i + k] = NAN;
		}
	}
	return SIFT3D_OK;
}

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

namespace {
// what the shell needs to know of an order: its result record, parameter count, state record and launch function
struct FirstOrder {
	typedef sift3d_icgn_result Result;
	static constexpr int kParameters = 12;
	static size_t state_bytes() { return icgn_state_bytes(); }
	static constexpr auto launch = launch_icgn;
};
struct SecondOrder {
	typedef sift3d_icgn2_result Result;
	static constexpr int kParameters = 30;
	static size_t state_bytes() { return icgn2_state_bytes(); }
	static constexpr auto launch = launch_icgn2;
};

// a masked call's own arguments (sift3d_icgn_masked): the mask lies where the volumes lie, active is host memory (may be null)
struct MaskCall {
	const unsigned char *mask;
	float min_fraction;
	int *active;
	// sift3d_icgn_labelled: the label volume takes the mask's place (mask is null then); poi_label is host memory (may be null)
	const int *labels = nullptr;
	int *poi_label = nullptr;
};
constexpr int kPlain = 0, kMasked = 1, kLabelled = 2;  // run_icgn's MODE

// the call behind sift3d_icgn, sift3d_icgn_bspline, sift3d_icgn2 and sift3d_icgn_masked (max_interpolation, bspline: icgn_args_ok's,
// which states each call's rules; MODE kMasked or kLabelled with mc: the masked and the labelled call, first order only -- the other three pass neither).  B-spline coefficients the caller did not
// bring (coef 0) are made here, in the call's scratch.
template <class Order, int MODE = kPlain>
int run_icgn(const char *who, int max_interpolation, bool bspline, const float *ref, int rnx, int rny, int rnz, const float *tar, int tnx, int tny,
             int tnz, const int *points3, int m, const double *init, const sift3d_icgn_options *o, int coef, int on_device, int device,
             typename Order::Result *out, double *seconds, const MaskCall *mc = nullptr) {
	constexpr bool MASKED = MODE == kMasked, LABELLED = MODE == kLabelled, COUNTED = MODE != kPlain;
	static_assert(!COUNTED || Order::kParameters == 12, "only the first-order kernels have masked instantiations");
	int r, max_it, kind;
	double tol;
	if (!icgn_args_ok(ref, rnx, rny, rnz, tar, tnx, tny, tnz, points3, m, o, max_interpolation, bspline, coef, out, r, max_it, tol, kind) ||
	    (MASKED && !icgn_mask_args_ok(mc->mask, mc->min_fraction)) || (LABELLED && !icgn_label_args_ok(mc->labels, mc->min_fraction, rnx, rny, rnz)) ||
	    (kind == 2 && !coef && !bspline_prefilter_fits(tnx, tny, tnz))) {
		set_last_error(std::string(who) + ": bad argument");
		return SIFT3D_ERR_ARG;
	}
	const bool filter = kind == 2 && !coef;
	if (seconds) *seconds = 0;
	int rc = pick_device(device);
	if (rc) return rc;
	if (m == 0) return SIFT3D_OK;
	CallState &S = g_icgn[device];
	std::lock_guard<std::mutex> lock(S.mu);
	const IcgnLayout L = icgn_layout(m, (size_t)rnx * rny * rnz, (size_t)tnx * tny * tnz, on_device != 0, init != nullptr, filter,
	                                 Order::state_bytes(), sizeof(typename Order::Result), Order::kParameters, MASKED, LABELLED);
	const size_t p_count = COUNTED ? al256(L.res_bytes) : L.res_bytes;  // masked: the active counts follow the results in the pinned block
	const size_t p_label = p_count + al256(L.count_bytes);              // labelled: and the POI labels follow the counts
	if ((rc = S.ensure(L.end, LABELLED ? p_label + L.count_bytes : p_count + L.count_bytes))) return rc;
	hipStream_t st = S.stream;
	char *D = S.d.p, *P = S.h.p;
	const float *d_ref = ref, *d_tar = tar;
	const int *d_pts = points3;
	const void *d_init = init;
	if ((rc = S.stage_pair(L, on_device != 0, d_ref, d_tar, d_pts, d_init))) return rc;
	const unsigned char *d_mask = nullptr;
	if constexpr (MASKED) {
		d_mask = mc->mask;
		S3D_HIP_ST(st, upload(d_mask, D, L.o_mask, L.b_mask, st));
	}
	const int *d_labels = nullptr;
	if constexpr (LABELLED) {
		d_labels = mc->labels;
		S3D_HIP_ST(st, upload(d_labels, D, L.o_labels, L.b_labels, st));
	}
	S3D_HIP_ST(st, hipEventRecord(S.e0, st));
	if (filter) {
		float *d_coef = reinterpret_cast<float *>(D + L.o_coef);
		launch_bspline_prefilter(d_tar, tnx, tny, tnz, d_coef, reinterpret_cast<float *>(D + L.o_tmp), st);
		S3D_HIP_ST(st, hipGetLastError());
		d_tar = d_coef;
	}
	const IcgnVol R{d_ref, rnx, rny, rnz}, T{d_tar, tnx, tny, tnz};
	if constexpr (MASKED) {
		unsigned char *d_act = reinterpret_cast<unsigned char *>(D + L.o_act);
		launch_mask_active(d_mask, rnx, rny, rnz, d_act, st);
		S3D_HIP_ST(st, hipGetLastError());
		launch_icgn_masked(R, T, d_pts, m, static_cast<const double *>(d_init), r, max_it, tol, kind, D + L.o_state,
		                   reinterpret_cast<sift3d_icgn_result *>(D), IcgnMask{d_act, reinterpret_cast<int *>(D + L.o_count), mc->min_fraction}, st);
	} else if constexpr (LABELLED) {
		int *d_interior = reinterpret_cast<int *>(D + L.o_interior);
		launch_label_interior(d_labels, rnx, rny, rnz, d_interior, st);
		S3D_HIP_ST(st, hipGetLastError());
		launch_icgn_labelled(R, T, d_pts, m, static_cast<const double *>(d_init), r, max_it, tol, kind, D + L.o_state,
		                     reinterpret_cast<sift3d_icgn_result *>(D),
		                     IcgnLabels{d_interior, d_labels, reinterpret_cast<int *>(D + L.o_count), reinterpret_cast<int *>(D + L.o_plabel),
		                                mc->min_fraction},
		                     st);
	} else {
		Order::launch(R, T, d_pts, m, static_cast<const double *>(d_init), r, max_it, tol, kind, D + L.o_state,
		              reinterpret_cast<typename Order::Result *>(D), st);
	}
	S3D_HIP_ST(st, hipGetLastError());
	S3D_HIP_ST(st, hipMemcpyAsync(P, D, L.res_bytes, hipMemcpyDeviceToHost, st));
	if constexpr (COUNTED) S3D_HIP_ST(st, hipMemcpyAsync(P + p_count, D + L.o_count, L.count_bytes, hipMemcpyDeviceToHost, st));
	if constexpr (LABELLED) S3D_HIP_ST(st, hipMemcpyAsync(P + p_label, D + L.o_plabel, L.count_bytes, hipMemcpyDeviceToHost, st));
	S3D_HIP_ST(st, hipEventRecord(S.e1, st));
	if ((rc = S.finish(seconds))) return rc;
	memcpy(out, P, L.res_bytes);
	if constexpr (COUNTED)
		if (mc->active) memcpy(mc->active, P + p_count, L.count_bytes);
	if constexpr (LABELLED)
		if (mc->poi_label) memcpy(mc->poi_label, P + p_label, L.count_bytes);
	return SIFT3D_OK;
}
}  // namespace

extern "C" int sift3d_icgn(const float *ref, int rnx, int rny, int rnz, const float *tar, int tnx, int tny, int tnz, const int *points3, int m,
                           const double *init12, const sift3d_icgn_options *o, int on_device, int device, sift3d_icgn_result *out,
                           double *seconds) {
	return run_icgn<FirstOrder>("sift3d_icgn", 1, false, ref, rnx, rny, rnz, tar, tnx, tny, tnz, points3, m, init12, o, 0, on_device, device, out,
	                            seconds);
}

extern "C" int sift3d_icgn_bspline(const float *ref, int rnx, int rny, int rnz, const float *tar, int tnx, int tny, int tnz, const int *points3,
                                   int m, const double *init12, const sift3d_icgn_options *o, int tar_is_coefficients, int on_device,
                                   int device, sift3d_icgn_result *out, double *seconds) {
	return run_icgn<FirstOrder>("sift3d_icgn_bspline", 0, true, ref, rnx, rny, rnz, tar, tnx, tny, tnz, points3, m, init12, o, tar_is_coefficients,
	                            on_device, device, out, seconds);
}

extern "C" int sift3d_icgn2(const float *ref, int rnx, int rny, int rnz, const float *tar, int tnx, int tny, int tnz, const int *points3, int m,
                            const double *init30, const sift3d_icgn_options *o, int tar_is_coefficients, int on_device, int device,
                            sift3d_icgn2_result *out, double *seconds) {
	return run_icgn<SecondOrder>("sift3d_icgn2", 2, false, ref, rnx, rny, rnz, tar, tnx, tny, tnz, points3, m, init30, o, tar_is_coefficients,
	                             on_device, device, out, seconds);
}

extern "C" int sift3d_icgn_masked(const float *ref, int rnx, int rny, int rnz, const float *tar, int tnx, int tny, int tnz,
                                  const unsigned char *mask, const int *points3, int m, const double *init12, const sift3d_icgn_options *o,
                                  float min_fraction, int tar_is_coefficients, int on_device, int device, sift3d_icgn_result *out, int *active,
                                  double *seconds) {
	const MaskCall mc = {mask, min_fraction, active};
	return run_icgn<FirstOrder, kMasked>("sift3d_icgn_masked", 2, false, ref, rnx, rny, rnz, tar, tnx, tny, tnz, points3, m, init12, o, tar_is_coefficients,
	                            on_device, device, out, seconds, &mc);
}

extern "C" int sift3d_icgn_labelled(const float *ref, int rnx, int rny, int rnz, const float *tar, int tnx, int tny, int tnz, const int *labels,
                                    const int *points3, int m, const double *init12, const sift3d_icgn_options *o, float min_fraction,
                                    int tar_is_coefficients, int on_device, int device, sift3d_icgn_result *out, int *active, int *poi_label,
                                    double *seconds) {
	const MaskCall mc = {nullptr, min_fraction, active, labels, poi_label};
	return run_icgn<FirstOrder, kLabelled>("sift3d_icgn_labelled", 2, false, ref, rnx, rny, rnz, tar, tnx, tny, tnz, points3, m, init12, o,
	                                       tar_is_coefficients, on_device, device, out, seconds, &mc);
}
