// icgn2_host.h -- the host-only logic of the second-order IC-GN entry (entry_icgn2.hip): the argument check, the scratch layout of a
// call and the two record conversions.  No HIP include: a stand-alone program can use it (tests/test_icgn2_cpu.py builds one with the
// sanitizers).
#pragma once
#include <math.h>
#include <stddef.h>

#include "../../include/sift3d_hip.h"
#include "scratch_layout.h"

namespace s3d {

// options (NULL: defaults) -> checked values; kind: launch_icgn2's (the interpolation option as it is: 0, 1 or 2)
inline bool icgn2_take_options(const sift3d_icgn_options *o, int &r, int &max_it, double &tol, int &kind) {
	const sift3d_icgn_options d = {16, 20, 1e-3f, 0, {0, 0, 0, 0}};  // sift3d_default_icgn_options
	if (!o) o = &d;
	if (o->subset_radius < 2 || o->subset_radius > 32 || o->max_iterations < 1 || o->max_iterations > 100) return false;
	if (!std::isfinite(o->tolerance) || o->tolerance < 0.f || o->interpolation < 0 || o->interpolation > 2) return false;
	if (o->reserved[0] || o->reserved[1] || o->reserved[2] || o->reserved[3]) return false;
	r = o->subset_radius;
	max_it = o->max_iterations;
	tol = o->tolerance;
	kind = o->interpolation;
	return true;
}

// everything sift3d_icgn2 refuses short of the prefilter's size limit (which needs the kernel file's word)
inline bool icgn2_args_ok(const void *ref, int rnx, int rny, int rnz, const void *tar, int tnx, int tny, int tnz, const void *points3, int m,
                          const sift3d_icgn_options *o, int coef, const void *out, int &r, int &max_it, double &tol, int &kind) {
	if (m < 0 || rnx < 1 || rny < 1 || rnz < 1 || tnx < 1 || tny < 1 || tnz < 1 || !ref || !tar || !out || (m > 0 && !points3)) return false;
	if (!icgn2_take_options(o, r, max_it, tol, kind)) return false;
	return kind == 2 ? (coef == 0 || coef == 1) : coef == 0;
}

// device scratch of a call: [results m | state m | (host inputs) ref | tar | points | init | (prefilter) coefficients | the y pass's
// output]; the pinned host block holds the results
struct Icgn2Layout {
	size_t res_bytes, o_state, o_ref, o_tar, o_pts, o_init, o_coef, o_tmp, end;
};
inline Icgn2Layout icgn2_layout(int m, size_t nr, size_t nt, bool on_device, bool has_init, bool filter, size_t state_bytes) {
	Icgn2Layout g;
	Layout L;
	g.res_bytes = sizeof(sift3d_icgn2_result) * (size_t)m;
	L.take(g.res_bytes);
	g.o_state = L.take(state_bytes * (size_t)m);
	g.o_ref = L.take(on_device ? 0 : sizeof(float) * nr);
	g.o_tar = L.take(on_device ? 0 : sizeof(float) * nt);
	g.o_pts = L.take(on_device ? 0 : sizeof(int) * 3 * (size_t)m);
	g.o_init = L.take(on_device || !has_init ? 0 : sizeof(double) * 30 * (size_t)m);
	g.o_coef = L.take(filter ? sizeof(float) * nt : 0);
	g.o_tmp = L.take(filter ? sizeof(float) * nt : 0);
	g.end = L.end;
	return g;
}

// a first-order result -> the 30 initial parameters: status 0 or 1 gives its 12 parameters and zero second derivatives, else NaN
inline void icgn2_init_row(const sift3d_icgn_result &res, double *p30) {
	const bool ok = res.status == 0 || res.status == 1;
	for (int a = 0; a < 3; a++)
		for (int k = 0; k < 10; k++) p30[10 * a + k] = !ok ? (double)NAN : (k < 4 ? res.p[4 * a + k] : 0.0);
}

// a second-order result -> its displacement and validity byte (sift3d_strain_input_from_icgn's rule)
inline unsigned char icgn2_strain_row(const sift3d_icgn2_result &res, double zncc_min, int accept_unconverged, double *d) {
	for (int a = 0; a < 3; a++) d[a] = res.p[10 * a];
	const bool done = res.status == 0 || (res.status == 1 && accept_unconverged);
	return done && res.zncc >= zncc_min && std::isfinite(d[0]) && std::isfinite(d[1]) && std::isfinite(d[2]) ? 1 : 0;
}

}  // namespace s3d
