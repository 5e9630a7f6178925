// icgn_host.h -- the host-only logic of the IC-GN entries of both orders (entry_icgn.hip): the options, the argument check of the three
// exported calls, the scratch layout of a call and the two record conversions of the second order.  No HIP include: a stand-alone
// program can use it (tests/test_icgn2_cpu.py builds one with the sanitizers).
#pragma once
#include <math.h>
#include <stddef.h>

#include "../../include/sift3d_hip.h"
#include "scratch_layout.h"

namespace s3d {

// the defaults: sift3d_default_icgn_options, and what a call with NULL options runs with
inline sift3d_icgn_options icgn_default_options() { return {16, 20, 1e-3f, 0, {0, 0, 0, 0}}; }

// options (NULL: defaults) -> checked values; kind: the interpolation option as it is, 0 .. max_interpolation
inline bool icgn_take_options(const sift3d_icgn_options *o, int max_interpolation, int &r, int &max_it, double &tol, int &kind) {
	const sift3d_icgn_options d = icgn_default_options();
	if (!o) o = &d;
	if (o->subset_radius < 2 || o->subset_radius > 32 || o->max_iterations < 1 || o->max_iterations > 100) return false;
	if (!std::isfinite(o->tolerance) || o->tolerance < 0.f || o->interpolation < 0 || o->interpolation > max_interpolation) return false;
	if (o->reserved[0] || o->reserved[1] || o->reserved[2] || o->reserved[3]) return false;
	r = o->subset_radius;
	max_it = o->max_iterations;
	tol = o->tolerance;
	kind = o->interpolation;
	return true;
}

// Everything the three calls refuse short of the prefilter's size limit (which needs the kernel file's word).  kind: the launch
// functions' (0 Keys, 1 trilinear, 2 B-spline); coef: tar_is_coefficients, which has a meaning for kind 2 only.
//   sift3d_icgn          max_interpolation 1, bspline 0, coef 0: interpolation 0 or 1
//   sift3d_icgn_bspline  max_interpolation 0, bspline 1: interpolation 0 only, run as kind 2; coef 0 or 1
//   sift3d_icgn2         max_interpolation 2, bspline 0: interpolation 0 .. 2; coef 0 or 1 with 2, else 0
inline bool icgn_args_ok(const void *ref, int rnx, int rny, int rnz, const void *tar, int tnx, int tny, int tnz, const void *points3, int m,
                         const sift3d_icgn_options *o, int max_interpolation, bool bspline, int coef, const void *out, int &r, int &max_it,
                         double &tol, int &kind) {
	if (m < 0 || rnx < 1 || rny < 1 || rnz < 1 || tnx < 1 || tny < 1 || tnz < 1 || !ref || !tar || !out || (m > 0 && !points3)) return false;
	if (!icgn_take_options(o, max_interpolation, r, max_it, tol, kind)) return false;
	if (bspline) kind = 2;
	return kind == 2 ? (coef == 0 || coef == 1) : coef == 0;
}

// sift3d_icgn_masked's own refusals, beside icgn_args_ok's with sift3d_icgn2's rules (max_interpolation 2, bspline 0)
inline bool icgn_mask_args_ok(const void *mask, float min_fraction) { return mask && min_fraction >= 0.f && min_fraction <= 1.f; }  // (a NaN fails both)

// sift3d_icgn_labelled's: the masked call's with the labels in the mask's place, and R's voxels must be counted by an int
inline bool icgn_label_args_ok(const void *labels, float min_fraction, int rnx, int rny, int rnz) {
	return icgn_mask_args_ok(labels, min_fraction) && (size_t)rnx * (size_t)rny <= (((size_t)1 << 31) - 1) / (size_t)rnz;
}

// device scratch of a call: [results m | state m | (host inputs) ref | tar | points | init | (prefilter) coefficients | the y pass's
// output | (masked) the active bytes of R's voxels | the active counts m | (masked, host inputs) mask]; the pinned host block holds
// the results and, 256-aligned behind them, the active counts.  o_opt (PairPlan) is the init table's offset.  The pieces of a masked
// call come last: an unmasked call's layout does not know of them.  A labelled call (sift3d_icgn_labelled) appends its own behind
// those: [the interior labels of R's voxels, 4 bytes each | the active counts m | the POI labels m | (host inputs) labels]; it has no
// masked piece, and neither of the other layouts moves.  Its pinned block: the results, the counts, the POI labels, each 256-aligned.
struct IcgnLayout : PairPlan {
	size_t res_bytes, o_state, o_coef, o_tmp, o_act, o_count, o_mask, b_mask, count_bytes, end;
	size_t o_interior, o_plabel, o_labels, b_labels;
};
inline IcgnLayout icgn_layout(int m, size_t nr, size_t nt, bool on_device, bool has_init, bool filter, size_t state_bytes, size_t result_bytes,
                              int parameters, bool masked = false, bool labelled = false) {
	IcgnLayout g;
	Layout L;
	g.res_bytes = result_bytes * (size_t)m;
	L.take(g.res_bytes);
	g.o_state = L.take(state_bytes * (size_t)m);
	g.plan(L, on_device, nr, nt, m, has_init ? sizeof(double) * parameters : 0);
	g.o_coef = L.take(filter ? sizeof(float) * nt : 0);
	g.o_tmp = L.take(filter ? sizeof(float) * nt : 0);
	g.count_bytes = masked ? sizeof(int) * (size_t)m : 0;
	g.b_mask = masked && !on_device ? nr : 0;
	g.o_act = L.take(masked ? nr : 0);
	g.o_count = L.take(g.count_bytes);
	g.o_mask = L.take(g.b_mask);
	g.o_interior = L.take(labelled ? sizeof(int) * nr : 0);
	if (labelled) {
		g.count_bytes = sizeof(int) * (size_t)m;
		g.o_count = L.take(g.count_bytes);
	}
	g.o_plabel = L.take(labelled ? sizeof(int) * (size_t)m : 0);
	g.b_labels = labelled && !on_device ? sizeof(int) * nr : 0;
	g.o_labels = L.take(g.b_labels);
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
