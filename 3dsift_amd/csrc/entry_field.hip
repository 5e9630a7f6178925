// entry_field.hip -- C-ABI of the field evaluation (include/sift3d_hip.h: sift3d_field_eval, sift3d_default_field_options and the host
// helpers sift3d_field_queries_from_displacements, sift3d_field_unpack, sift3d_compose_displacements, sift3d_icgn_init_from_field).  No
// reference counterpart.  Call state, scratch layout, timing and the order of the checks: DESIGN 4.10 (call_state.h).  As in
// sift3d_strain the temporaries depend on the input (the cell grid of the POI index, poi_grid.h), so they are allocated and freed
// inside the call, and the state's grow-only blocks stay empty.
#include "call_state.h"
#include "poi_grid.h"

#include <math.h>
#include <string.h>

using namespace s3d;

namespace {
CallState g_field[kMaxDev];

// options (NULL: defaults) -> checked values
bool take_options(const sift3d_field_options *o, sift3d_field_options &v) {
	sift3d_field_options d;
	sift3d_default_field_options(&d);
	if (!o) o = &d;
	if (o->radius < 1 || o->radius > 4095 || o->min_neighbours < 4 || o->min_neighbours > 1048576 || o->weighting < 0 || o->weighting > 1 ||
	    o->require_enclosed < 0 || o->require_enclosed > 1)
		return false;
	for (int k = 0; k < 4; k++)
		if (o->reserved[k]) return false;
	v = *o;
	return true;
}
}  // namespace

extern "C" void sift3d_default_field_options(sift3d_field_options *o) {
	if (!o) return;
	memset(o, 0, sizeof(*o));
	o->radius = 16;
	o->min_neighbours = 10;
	o->weighting = 1;
	o->require_enclosed = 1;
}

extern "C" int sift3d_field_queries_from_displacements(const int *points3, const double *disp3, int m, double *queries3) {
	if (m < 0 || (m > 0 && (!points3 || !disp3 || !queries3))) {
		set_last_error("sift3d_field_queries_from_displacements: bad argument");
		return SIFT3D_ERR_ARG;
	}
	for (size_t k = 0; k < 3 * (size_t)m; k++) queries3[k] = (double)points3[k] + disp3[k];
	return SIFT3D_OK;
}

extern "C" int sift3d_field_unpack(const sift3d_field_result *res, int n, double *disp3, double *grad9, unsigned char *valid) {
	if (n < 0 || (n > 0 && (!res || !disp3))) {
		set_last_error("sift3d_field_unpack: bad argument");
		return SIFT3D_ERR_ARG;
	}
	for (int i = 0; i < n; i++) {
		for (int a = 0; a < 3; a++) disp3[3 * (size_t)i + a] = res[i].disp[a];
		if (grad9)
			for (int k = 0; k < 9; k++) grad9[9 * (size_t)i + k] = res[i].G[k];
		if (valid) valid[i] = res[i].status == 0 ? 1 : 0;
	}
	return SIFT3D_OK;
}

extern "C" int sift3d_compose_displacements(const double *dispA3, const double *gradA9, const unsigned char *validA,
                                            const sift3d_field_result *atB, int m, double *disp3, double *grad9, unsigned char *valid) {
	if (m < 0 || (grad9 && !gradA9) || (m > 0 && (!dispA3 || !atB || !disp3))) {
		set_last_error("sift3d_compose_displacements: bad argument");
		return SIFT3D_ERR_ARG;
	}
	for (int i = 0; i < m; i++) {
		const sift3d_field_result &b = atB[i];
		const bool ok = (!validA || validA[i]) && b.status == 0;
		double *d = disp3 + 3 * (size_t)i;
		for (int a = 0; a < 3; a++) d[a] = ok ? dispA3[3 * (size_t)i + a] + b.disp[a] : 0.0;
		if (grad9) {
			const double *ga = gradA9 + 9 * (size_t)i;
			double *g = grad9 + 9 * (size_t)i;
			for (int r = 0; r < 3; r++)
				for (int c = 0; c < 3; c++) {
					const double prod = (b.G[3 * r] * ga[c] + b.G[3 * r + 1] * ga[3 + c]) + b.G[3 * r + 2] * ga[6 + c];
					g[3 * r + c] = ok ? (ga[3 * r + c] + b.G[3 * r + c]) + prod : 0.0;
				}
		}
		if (valid) valid[i] = ok ? 1 : 0;
	}
	return SIFT3D_OK;
}

extern "C" int sift3d_icgn_init_from_field(const double *disp3, const double *grad9, const unsigned char *valid, int m, int only_valid,
                                           double *init12, int *count) {
	if (count) *count = 0;
	if (m < 0 || (m > 0 && (!disp3 || !init12))) {
		set_last_error("sift3d_icgn_init_from_field: bad argument");
		return SIFT3D_ERR_ARG;
	}
	int written = 0;
	for (int i = 0; i < m; i++) {
		if (only_valid && valid && !valid[i]) continue;
		double *p = init12 + 12 * (size_t)i;
		for (int c = 0; c < 3; c++) {
			p[4 * c] = disp3[3 * (size_t)i + c];
			for (int a = 0; a < 3; a++) p[4 * c + 1 + a] = grad9 ? grad9[9 * (size_t)i + 3 * c + a] : 0.0;
		}
		written++;
	}
	if (count) *count = written;
	return SIFT3D_OK;
}

namespace {
// both entries; labelled: label holds m labels, query_label nq, and a query's members are the POIs of its label
int field_call(const char *name, const int *points3, const double *disp3, const unsigned char *valid, const int *label, int m,
               const double *queries3, const int *query_label, bool labelled, int nq, const sift3d_field_options *o, int on_device, int device,
               sift3d_field_result *out, double *seconds) {
	sift3d_field_options v;
	if (m < 0 || nq < 0 || (nq > 0 && (!out || !queries3)) || (m > 0 && (!points3 || !disp3)) || (labelled && (!label || (nq > 0 && !query_label))) ||
	    !take_options(o, v)) {
		set_last_error(std::string(name) + ": bad argument");
		return SIFT3D_ERR_ARG;
	}
	if (seconds) *seconds = 0;
	int rc = pick_device(device);
	if (rc) return rc;
	if (nq == 0) return SIFT3D_OK;
	CallState &D = g_field[device];
	std::lock_guard<std::mutex> lock(D.mu);
	if ((rc = D.ensure(0, 0))) return rc;
	hipStream_t st = D.stream;
	CallTemps T;
	// block a: [results | the index's pieces (m = 0: the two cell starts of an empty one-cell index) | (host inputs) points | disp | valid |
	// queries | labels | query labels]
	const size_t M = (size_t)m, Q = (size_t)nq, res_bytes = sizeof(sift3d_field_result) * Q;
	const size_t b_pts = on_device ? 0 : sizeof(int) * 3 * M, b_disp = on_device ? 0 : sizeof(double) * 3 * M, b_valid = on_device || !valid ? 0 : M;
	const size_t b_qry = on_device ? 0 : sizeof(double) * 3 * Q;
	const size_t b_label = on_device || !labelled ? 0 : sizeof(int) * M, b_qlabel = on_device || !labelled ? 0 : sizeof(int) * Q;
	Layout L;
	L.take(res_bytes);
	PoiGridPlan G;
	size_t o_empty = 0;
	if (m > 0)
		G.take(L, m);
	else
		o_empty = L.take(sizeof(int) * 2);
	const size_t o_pts = L.take(b_pts), o_disp = L.take(b_disp), o_valid = L.take(b_valid), o_qry = L.take(b_qry);
	const size_t o_label = L.take(b_label), o_qlabel = L.take(b_qlabel);
	S3D_HIP(hipMalloc(&T.a, L.end));
	char *A = T.a;
	const int *d_pts = points3, *d_label = labelled ? label : nullptr, *d_qlabel = labelled ? query_label : nullptr;
	const double *d_disp = disp3, *d_qry = queries3;
	const unsigned char *d_valid = valid;
	if (on_device && (rc = D.after_legacy_stream())) return rc;
	S3D_HIP_ST(st, upload(d_pts, A, o_pts, b_pts, st));
	S3D_HIP_ST(st, upload(d_disp, A, o_disp, b_disp, st));
	S3D_HIP_ST(st, upload(d_valid, A, o_valid, b_valid, st));
	S3D_HIP_ST(st, upload(d_qry, A, o_qry, b_qry, st));
	S3D_HIP_ST(st, upload(d_label, A, o_label, b_label, st));
	S3D_HIP_ST(st, upload(d_qlabel, A, o_qlabel, b_qlabel, st));
	S3D_HIP_ST(st, hipEventRecord(D.e0, st));
	PoiIndex ix;
	if (m > 0) {
		// radius + 1: the integer window around floor(x) that covers the real one around x (kernels_field.hip)
		if ((rc = poi_grid_build(G, A, d_pts, d_disp, d_valid, m, v.radius + 1, T, st, ix))) return rc;
	} else {
		S3D_HIP_ST(st, hipMemsetAsync(A + o_empty, 0, sizeof(int) * 2, st));
		ix = PoiIndex{PoiGrid{0, 0, 0, v.radius + 1, 1, 1, 1}, 1, nullptr, reinterpret_cast<const int *>(A + o_empty), PoiSorted{}};
	}
	launch_field_eval(d_qry, nq, d_disp, d_label, d_qlabel, ix, v.radius, v.min_neighbours, v.weighting, v.require_enclosed,
	                  reinterpret_cast<sift3d_field_result *>(A), st);
	S3D_HIP_ST(st, hipGetLastError());
	S3D_HIP_ST(st, hipMemcpyAsync(out, A, res_bytes, hipMemcpyDeviceToHost, st));
	S3D_HIP_ST(st, hipEventRecord(D.e1, st));
	return D.finish(seconds);
}
}  // namespace

extern "C" int sift3d_field_eval(const int *points3, const double *disp3, const unsigned char *valid, int m, const double *queries3, int nq,
                                 const sift3d_field_options *o, int on_device, int device, sift3d_field_result *out, double *seconds) {
	return field_call("sift3d_field_eval", points3, disp3, valid, nullptr, m, queries3, nullptr, false, nq, o, on_device, device, out, seconds);
}

extern "C" int sift3d_field_eval_labelled(const int *points3, const double *disp3, const unsigned char *valid, const int *label, int m,
                                          const double *queries3, const int *query_label, int nq, const sift3d_field_options *o, int on_device,
                                          int device, sift3d_field_result *out, double *seconds) {
	return field_call("sift3d_field_eval_labelled", points3, disp3, valid, label, m, queries3, query_label, true, nq, o, on_device, device, out,
	                  seconds);
}
