// entry_strain.hip -- C-ABI of the strain fields (include/sift3d_hip.h: sift3d_strain, sift3d_strain_input_from_icgn,
// sift3d_default_strain_options).  No reference counterpart.  Call state, scratch layout, timing and the order of the checks: DESIGN
// 4.10 (call_state.h).  The temporaries depend on the input (the cell grid of the POI index on the POIs' bounding box, poi_grid.h), so they
// are allocated and freed inside the call, and the state's grow-only blocks stay empty.
#include "call_state.h"
#include "poi_grid.h"

#include <math.h>
#include <string.h>

using namespace s3d;

namespace {
CallState g_strain[kMaxDev];

// options (NULL: defaults) -> checked values
bool take_options(const sift3d_strain_options *o, int &radius, int &min_nb, int &measure) {
	sift3d_strain_options d;
	sift3d_default_strain_options(&d);
	if (!o) o = &d;
	if (o->radius < 1 || o->radius > 4096 || o->min_neighbours < 4 || o->min_neighbours > 1048576 || o->measure < 0 || o->measure > 1) return false;
	for (int k = 0; k < 5; k++)
		if (o->reserved[k]) return false;
	radius = o->radius;
	min_nb = o->min_neighbours;
	measure = o->measure;
	return true;
}
}  // namespace

extern "C" void sift3d_default_strain_options(sift3d_strain_options *o) {
	if (!o) return;
	memset(o, 0, sizeof(*o));
	o->radius = 16;
	o->min_neighbours = 10;
	o->measure = 0;
}

extern "C" int sift3d_strain_input_from_icgn(const sift3d_icgn_result *res, int m, double zncc_min, int accept_unconverged, double *disp3,
                                             unsigned char *valid) {
	if (m < 0 || !std::isfinite(zncc_min) || (m > 0 && (!res || !disp3 || !valid))) {
		set_last_error("sift3d_strain_input_from_icgn: bad argument");
		return SIFT3D_ERR_ARG;
	}
	for (int i = 0; i < m; i++) {
		const sift3d_icgn_result &r = res[i];
		double *d = disp3 + 3 * (size_t)i;
		for (int a = 0; a < 3; a++) d[a] = r.p[4 * a];
		const bool done = r.status == 0 || (r.status == 1 && accept_unconverged);
		valid[i] = done && r.zncc >= zncc_min && std::isfinite(d[0]) && std::isfinite(d[1]) && std::isfinite(d[2]) ? 1 : 0;
	}
	return SIFT3D_OK;
}

namespace {
// both entries; labelled: label holds m labels and limits a POI's neighbours to its own body
int strain_call(const char *name, const int *points3, const double *disp3, const unsigned char *valid, const int *label, bool labelled, int m,
                const sift3d_strain_options *o, int on_device, int device, sift3d_strain_result *out, double *seconds) {
	int radius, min_nb, measure;
	if (m < 0 || !out || (m > 0 && (!points3 || !disp3)) || (labelled && !label) || !take_options(o, radius, min_nb, measure)) {
		set_last_error(std::string(name) + ": bad argument");
		return SIFT3D_ERR_ARG;
	}
	if (seconds) *seconds = 0;
	int rc = pick_device(device);
	if (rc) return rc;
	if (m == 0) return SIFT3D_OK;
	CallState &D = g_strain[device];
	std::lock_guard<std::mutex> lock(D.mu);
	if ((rc = D.ensure(0, 0))) return rc;
	hipStream_t st = D.stream;
	CallTemps T;
	// block a: [results | the index's pieces | (host inputs) points | disp | valid | labels]
	const size_t M = (size_t)m, res_bytes = sizeof(sift3d_strain_result) * M;
	const size_t b_pts = on_device ? 0 : sizeof(int) * 3 * M, b_disp = on_device ? 0 : sizeof(double) * 3 * M, b_valid = on_device || !valid ? 0 : M;
	const size_t b_label = on_device || !labelled ? 0 : sizeof(int) * M;
	Layout L;
	L.take(res_bytes);
	PoiGridPlan G;
	G.take(L, m);
	const size_t o_pts = L.take(b_pts), o_disp = L.take(b_disp), o_valid = L.take(b_valid), o_label = L.take(b_label);
	S3D_HIP(hipMalloc(&T.a, L.end));
	char *A = T.a;
	const int *d_pts = points3, *d_label = labelled ? label : nullptr;
	const double *d_disp = disp3;
	const unsigned char *d_valid = valid;
	if (on_device && (rc = D.after_legacy_stream())) return rc;
	S3D_HIP_ST(st, upload(d_pts, A, o_pts, b_pts, st));
	S3D_HIP_ST(st, upload(d_disp, A, o_disp, b_disp, st));
	S3D_HIP_ST(st, upload(d_valid, A, o_valid, b_valid, st));
	S3D_HIP_ST(st, upload(d_label, A, o_label, b_label, st));
	S3D_HIP_ST(st, hipEventRecord(D.e0, st));
	PoiIndex ix;
	if ((rc = poi_grid_build(G, A, d_pts, d_disp, d_valid, m, radius, T, st, ix))) return rc;
	launch_strain_fit(d_pts, d_disp, d_label, m, ix, radius, min_nb, measure, reinterpret_cast<sift3d_strain_result *>(A), st);
	S3D_HIP_ST(st, hipGetLastError());
	S3D_HIP_ST(st, hipMemcpyAsync(out, A, res_bytes, hipMemcpyDeviceToHost, st));
	S3D_HIP_ST(st, hipEventRecord(D.e1, st));
	return D.finish(seconds);
}
}  // namespace

extern "C" int sift3d_strain(const int *points3, const double *disp3, const unsigned char *valid, int m, const sift3d_strain_options *o,
                             int on_device, int device, sift3d_strain_result *out, double *seconds) {
	return strain_call("sift3d_strain", points3, disp3, valid, nullptr, false, m, o, on_device, device, out, seconds);
}

extern "C" int sift3d_strain_labelled(const int *points3, const double *disp3, const unsigned char *valid, const int *label, int m,
                                      const sift3d_strain_options *o, int on_device, int device, sift3d_strain_result *out, double *seconds) {
	return strain_call("sift3d_strain_labelled", points3, disp3, valid, label, true, m, o, on_device, device, out, seconds);
}
