// entry_validate.hip -- C-ABI of the displacement validation (include/sift3d_hip.h: sift3d_validate_displacements, its host-only
// helpers and sift3d_default_validate_options; include/sift3d_hip_test.h: sift3d_validate_stage_capacity).  No reference counterpart.
// Call state, scratch layout, timing and the order of the checks: DESIGN 4.10 (call_state.h).  As in entry_strain.hip the temporaries
// depend on the input (the cell grid of the POI index on the POIs' bounding box, poi_grid.h), so they are allocated and freed inside the call.
#include "call_state.h"
#include "poi_grid.h"
#include "icgn_host.h"

#include <math.h>
#include <string.h>

#include "../../include/sift3d_hip_test.h"

using namespace s3d;

namespace {
CallState g_validate[kMaxDev];

// options (NULL: defaults) -> checked values
bool take_options(const sift3d_validate_options *o, ValidateParams &P, int &passes) {
	sift3d_validate_options d;
	sift3d_default_validate_options(&d);
	if (!o) o = &d;
	if (o->radius < 1 || o->radius > 4096 || o->min_neighbours < 3 || o->min_neighbours > 1048576 || o->passes < 1 || o->passes > 8) return false;
	if (!std::isfinite(o->threshold) || !(o->threshold > 0) || !std::isfinite(o->eps) || !(o->eps > 0) || o->reserved0) return false;
	for (int k = 0; k < 4; k++)
		if (o->reserved[k]) return false;
	P.radius = o->radius;
	P.min_nb = o->min_neighbours;
	P.threshold = o->threshold;
	P.eps = o->eps;
	passes = o->passes;
	return true;
}

bool reseeded(const sift3d_validate_result &v) { return (v.flagged && v.status == 0) || v.status == 3; }
}  // namespace

extern "C" void sift3d_default_validate_options(sift3d_validate_options *o) {
	if (!o) return;
	memset(o, 0, sizeof(*o));
	o->radius = 16;
	o->min_neighbours = 6;
	o->passes = 2;
	o->threshold = 2.0;
	o->eps = 0.1;
}

extern "C" int sift3d_validate_stage_capacity(int *n) {
	if (!n) return SIFT3D_ERR_ARG;
	*n = validate_stage_capacity();
	return SIFT3D_OK;
}

extern "C" int sift3d_validate_input_from_icgn(const sift3d_icgn_result *res, int m, double zncc_min, int accept_unconverged, double *disp3,
                                               double *grad9, unsigned char *valid) {
	const int rc = sift3d_strain_input_from_icgn(res, m, zncc_min, accept_unconverged, disp3, valid);
	if (rc || !grad9) return rc;
	for (int i = 0; i < m; i++)
		for (int c = 0; c < 3; c++)
			for (int a = 0; a < 3; a++) grad9[9 * (size_t)i + 3 * c + a] = res[i].p[4 * c + 1 + a];
	return SIFT3D_OK;
}

extern "C" int sift3d_validate_input_from_icgn2(const sift3d_icgn2_result *res, int m, double zncc_min, int accept_unconverged, double *disp3,
                                                double *grad9, unsigned char *valid) {
	const int rc = sift3d_strain_input_from_icgn2(res, m, zncc_min, accept_unconverged, disp3, valid);
	if (rc || !grad9) return rc;
	for (int i = 0; i < m; i++)
		for (int c = 0; c < 3; c++)
			for (int a = 0; a < 3; a++) grad9[9 * (size_t)i + 3 * c + a] = res[i].p[10 * c + 1 + a];
	return SIFT3D_OK;
}

extern "C" int sift3d_validate_keep(const sift3d_validate_result *val, const unsigned char *valid_in, int m, unsigned char *valid_out) {
	if (m < 0 || (m > 0 && (!val || !valid_out))) {
		set_last_error("sift3d_validate_keep: bad argument");
		return SIFT3D_ERR_ARG;
	}
	for (int i = 0; i < m; i++) valid_out[i] = (!valid_in || valid_in[i]) && val[i].status == 0 && !val[i].flagged ? 1 : 0;
	return SIFT3D_OK;
}

extern "C" int sift3d_icgn_init_from_validation(const sift3d_validate_result *val, int m, double *init12, int *count) {
	if (m < 0 || (m > 0 && (!val || !init12))) {
		set_last_error("sift3d_icgn_init_from_validation: bad argument");
		return SIFT3D_ERR_ARG;
	}
	int written = 0;
	for (int i = 0; i < m; i++) {
		if (!reseeded(val[i])) continue;
		double *p = init12 + 12 * (size_t)i;
		for (int k = 0; k < 12; k++) p[k] = 0.0;
		for (int c = 0; c < 3; c++) p[4 * c] = val[i].median[c];
		written++;
	}
	if (count) *count = written;
	return SIFT3D_OK;
}

namespace {
// both entries; labelled: label holds m labels and limits a POI's neighbours to its own body
int validate_call(const char *name, const int *points3, const double *disp3, const double *grad9, const unsigned char *valid, const int *label,
                  bool labelled, int m, const sift3d_validate_options *o, int on_device, int device, sift3d_validate_result *out,
                  double *seconds) {
	ValidateParams P;
	int passes;
	if (m < 0 || !out || (m > 0 && (!points3 || !disp3)) || (labelled && !label) || !take_options(o, P, passes)) {
		set_last_error(std::string(name) + ": bad argument");
		return SIFT3D_ERR_ARG;
	}
	if (seconds) *seconds = 0;
	int rc = pick_device(device);
	if (rc) return rc;
	if (m == 0) return SIFT3D_OK;
	CallState &D = g_validate[device];
	std::lock_guard<std::mutex> lock(D.mu);
	if ((rc = D.ensure(0, 0))) return rc;
	hipStream_t st = D.stream;
	CallTemps T;
	// block a: [results | the index's pieces | pass of a flag | folded valid bytes | flags, twice | (host inputs) points | disp | grad | valid |
	// labels]
	const size_t M = (size_t)m, wb = al256(M), res_bytes = sizeof(sift3d_validate_result) * M;
	const size_t b_pts = on_device ? 0 : sizeof(int) * 3 * M, b_disp = on_device ? 0 : sizeof(double) * 3 * M;
	const size_t b_grad = on_device || !grad9 ? 0 : sizeof(double) * 9 * M, b_valid = on_device || !valid ? 0 : M;
	const size_t b_label = on_device || !labelled ? 0 : sizeof(int) * M;
	Layout L;
	L.take(res_bytes);
	PoiGridPlan G;
	G.take(L, m);
	const size_t o_pass = L.take(sizeof(int) * M), o_fold = L.take(wb), o_flags = L.take(2 * wb);
	const size_t o_pts = L.take(b_pts), o_disp = L.take(b_disp), o_grad = L.take(b_grad), o_valid = L.take(b_valid), o_label = L.take(b_label);
	S3D_HIP(hipMalloc(&T.a, L.end));
	char *A = T.a;
	const int *d_pts = points3, *d_label = labelled ? label : nullptr;
	const double *d_disp = disp3, *d_grad = grad9;
	const unsigned char *d_valid = valid;
	if (on_device && (rc = D.after_legacy_stream())) return rc;
	S3D_HIP_ST(st, upload(d_pts, A, o_pts, b_pts, st));
	S3D_HIP_ST(st, upload(d_disp, A, o_disp, b_disp, st));
	S3D_HIP_ST(st, upload(d_grad, A, o_grad, b_grad, st));
	S3D_HIP_ST(st, upload(d_valid, A, o_valid, b_valid, st));
	S3D_HIP_ST(st, upload(d_label, A, o_label, b_label, st));
	int *d_pass = reinterpret_cast<int *>(A + o_pass);
	unsigned char *d_fold = reinterpret_cast<unsigned char *>(A + o_fold);
	unsigned char *d_flags[2] = {reinterpret_cast<unsigned char *>(A + o_flags), reinterpret_cast<unsigned char *>(A + o_flags + wb)};
	S3D_HIP_ST(st, hipEventRecord(D.e0, st));
	S3D_HIP_ST(st, hipMemsetAsync(d_pass, 0, sizeof(int) * M, st));
	S3D_HIP_ST(st, hipMemsetAsync(d_flags[0], 0, M, st));
	launch_validate_fold(d_grad, d_valid, m, d_fold, st);
	PoiIndex ix;
	if ((rc = poi_grid_build(G, A, d_pts, d_disp, d_fold, m, P.radius, T, st, ix))) return rc;
	sift3d_validate_result *d_out = reinterpret_cast<sift3d_validate_result *>(A);
	// pass p reads the flags of pass p - 1 and writes its own into the other buffer; the report reads the last pass's
	for (int p = 1; p <= passes; p++)
		launch_validate_test(d_pts, d_disp, d_grad, d_label, m, ix, P, p, d_flags[(p - 1) & 1], d_flags[p & 1], d_pass, d_out, st);
	launch_validate_test(d_pts, d_disp, d_grad, d_label, m, ix, P, 0, d_flags[passes & 1], nullptr, d_pass, d_out, st);
	S3D_HIP_ST(st, hipGetLastError());
	S3D_HIP_ST(st, hipMemcpyAsync(out, A, res_bytes, hipMemcpyDeviceToHost, st));
	S3D_HIP_ST(st, hipEventRecord(D.e1, st));
	return D.finish(seconds);
}
}  // namespace

extern "C" int sift3d_validate_displacements(const int *points3, const double *disp3, const double *grad9, const unsigned char *valid, int m,
                                             const sift3d_validate_options *o, int on_device, int device, sift3d_validate_result *out,
                                             double *seconds) {
	return validate_call("sift3d_validate_displacements", points3, disp3, grad9, valid, nullptr, false, m, o, on_device, device, out, seconds);
}

extern "C" int sift3d_validate_displacements_labelled(const int *points3, const double *disp3, const double *grad9, const unsigned char *valid,
                                                      const int *label, int m, const sift3d_validate_options *o, int on_device, int device,
                                                      sift3d_validate_result *out, double *seconds) {
	return validate_call("sift3d_validate_displacements_labelled", points3, disp3, grad9, valid, label, true, m, o, on_device, device, out,
	                     seconds);
}
