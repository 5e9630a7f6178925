// entry_strain.hip -- C-ABI of the strain fields (include/sift3d_hip.h: sift3d_strain, sift3d_strain_input_from_icgn,
// sift3d_default_strain_options).  No reference counterpart.  Call state, scratch layout, timing and the order of the checks: DESIGN
// 4.10 (call_state.h).  The temporaries depend on the input (the cell grid on the POIs' bounding box), so they are allocated and freed
// inside the call, and the state's grow-only blocks stay empty.
#include "call_state.h"

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

extern "C" int sift3d_strain(const int *points3, const double *disp3, const unsigned char *valid, int m, const sift3d_strain_options *o,
                             int on_device, int device, sift3d_strain_result *out, double *seconds) {
	int radius, min_nb, measure;
	if (m < 0 || !out || (m > 0 && (!points3 || !disp3)) || !take_options(o, radius, min_nb, measure)) {
		set_last_error("sift3d_strain: bad argument");
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
	// block a: [results | box | cell of a POI | slots | sorted x y z idx | sorted u v w | (host inputs) points | disp | valid]
	const size_t M = (size_t)m, wi = al256(sizeof(int) * M), wd = al256(sizeof(double) * M), res_bytes = sizeof(sift3d_strain_result) * M;
	Layout L;
	L.take(res_bytes);
	const size_t o_box = L.take(sizeof(int) * 6), o_cell = L.take(wi), o_slots = L.take(wi), o_si = L.take(4 * wi), o_sd = L.take(3 * wd);
	const size_t o_pts = L.take(on_device ? 0 : sizeof(int) * 3 * M), o_disp = L.take(on_device ? 0 : sizeof(double) * 3 * M);
	const size_t o_valid = L.take(on_device || !valid ? 0 : M);
	S3D_HIP(hipMalloc(&T.a, L.end));
	char *A = T.a;
	const int *d_pts = points3;
	const double *d_disp = disp3;
	const unsigned char *d_valid = valid;
	if (on_device) {
		if ((rc = D.after_legacy_stream())) return rc;
	} else {
		d_pts = reinterpret_cast<int *>(A + o_pts);
		d_disp = reinterpret_cast<double *>(A + o_disp);
		S3D_HIP_ST(st, hipMemcpyAsync(A + o_pts, points3, sizeof(int) * 3 * M, hipMemcpyHostToDevice, st));
		S3D_HIP_ST(st, hipMemcpyAsync(A + o_disp, disp3, sizeof(double) * 3 * M, hipMemcpyHostToDevice, st));
		if (valid) {
			d_valid = reinterpret_cast<unsigned char *>(A + o_valid);
			S3D_HIP_ST(st, hipMemcpyAsync(A + o_valid, valid, M, hipMemcpyHostToDevice, st));
		}
	}
	int *d_box = reinterpret_cast<int *>(A + o_box), *d_cell = reinterpret_cast<int *>(A + o_cell), *d_slots = reinterpret_cast<int *>(A + o_slots);
	StrainSorted S;
	S.x = reinterpret_cast<int *>(A + o_si); S.y = reinterpret_cast<int *>(A + o_si + wi); S.z = reinterpret_cast<int *>(A + o_si + 2 * wi);
	S.idx = reinterpret_cast<int *>(A + o_si + 3 * wi);
	S.u = reinterpret_cast<double *>(A + o_sd); S.v = reinterpret_cast<double *>(A + o_sd + wd); S.w = reinterpret_cast<double *>(A + o_sd + 2 * wd);
	S3D_HIP_ST(st, hipEventRecord(D.e0, st));
	S3D_HIP_ST(st, hipMemsetAsync(d_box, 0x7f, sizeof(int) * 6, st));
	launch_strain_mark(d_pts, d_disp, d_valid, m, d_cell, d_box, st);
	S3D_HIP_ST(st, hipGetLastError());
	int box[6];
	S3D_HIP_ST(st, hipMemcpyAsync(box, d_box, sizeof(box), hipMemcpyDeviceToHost, st));
	S3D_HIP_ST(st, hipStreamSynchronize(st));
	const StrainGrid g = strain_choose_grid(box, radius);
	// block b: [counts per cell (then the scatter's fill marks) | cell starts | the scan's tile sums]
	const size_t cells = (size_t)g.nx * g.ny * g.nz, wc = al256(sizeof(int) * (cells + 1));
	S3D_HIP(hipMalloc(&T.b, 2 * wc + sizeof(int) * strain_scan_tiles(cells + 1)));
	int *d_cnt = reinterpret_cast<int *>(T.b), *d_start = reinterpret_cast<int *>(T.b + wc), *d_tiles = reinterpret_cast<int *>(T.b + 2 * wc);
	S3D_HIP_ST(st, hipMemsetAsync(d_cnt, 0, sizeof(int) * (cells + 1), st));
	S3D_HIP_ST(st, launch_strain_bin(d_pts, d_disp, m, g, d_cell, d_cnt, d_start, d_tiles, d_slots, S, st));
	launch_strain_fit(d_pts, d_disp, m, g, d_start, S, radius, min_nb, measure, reinterpret_cast<sift3d_strain_result *>(A), st);
	S3D_HIP_ST(st, hipGetLastError());
	S3D_HIP_ST(st, hipMemcpyAsync(out, A, res_bytes, hipMemcpyDeviceToHost, st));
	S3D_HIP_ST(st, hipEventRecord(D.e1, st));
	return D.finish(seconds);
}
