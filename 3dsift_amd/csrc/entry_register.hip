// entry_register.hip -- C-ABI of the RANSAC fits (include/sift3d_hip.h: sift3d_fit_affine[_local], sift3d_fit_rigid[_local],
// sift3d_fit_rigid_bodies, sift3d_fit_rotation).  The affine and the rigid / similarity entries share one body each: they differ in the kernels launched
// and in the candidates a fit needs (4 and 3).
// No reference counterpart.  Call state, scratch layout, timing and the order of the checks: DESIGN 4.10 (call_state.h).
#include "call_state.h"

#include <math.h>
#include <string.h>

#include <vector>

using namespace s3d;

namespace {
CallState g_ransac[kMaxDev];  // the global and the local fits of every model share it
constexpr int kAffine = -1;    // `model` of the bodies below: -1 affine, else the checked model argument of sift3d_fit_rigid (0, 1)

int min_candidates(int model) { return model == kAffine ? 4 : 3; }

// options (NULL: defaults) -> checked values; H = the hypotheses per problem
bool take_options(const sift3d_ransac_options *o, bool local, int &H, double &tau2, double &min_det, int &refine, uint32_t &s) {
	sift3d_ransac_options d;
	sift3d_default_ransac_options(&d);
	if (!o) o = &d;
	if (o->iterations < 0 || o->iterations > 65536 || o->refine < 0 || o->refine > 4) return false;
	if (!std::isfinite(o->inlier_thresh) || o->inlier_thresh < 0.f || !std::isfinite(o->min_det) || o->min_det < 0.f) return false;
	if (o->reserved[0] || o->reserved[1] || o->reserved[2]) return false;
	H = o->iterations ? o->iterations : (local ? 256 : 4096);
	tau2 = (double)o->inlier_thresh * (double)o->inlier_thresh;
	min_det = o->min_det;
	refine = o->refine;
	s = ransac_seed(o->seed);
	return true;
}

void empty_fit(sift3d_affine_fit *f, int status, int candidates) {
	memset(f, 0, sizeof(*f));
	f->status = status;
	f->candidates = candidates;
	f->best_hypothesis = -1;
}
}  // namespace

extern "C" void sift3d_default_ransac_options(sift3d_ransac_options *o) {
	if (!o) return;
	memset(o, 0, sizeof(*o));
	o->iterations = 0;
	o->inlier_thresh = 3.0f;
	o->seed = 1;
	o->refine = 1;
	o->min_det = 1.0f;
}

namespace {
int fit_global(const char *who, int model, const float *pairs6, int n, const sift3d_ransac_options *o, int on_device, int device,
               sift3d_affine_fit *out, unsigned char *inlier_mask, double *seconds) {
	int H, refine;
	double tau2, min_det;
	uint32_t s;
	if (n < 0 || !out || (n > 0 && !pairs6) || !take_options(o, false, H, tau2, min_det, refine, s)) {
		set_last_error(who);
		return SIFT3D_ERR_ARG;
	}
	if (seconds) *seconds = 0;
	int rc = pick_device(device);
	if (rc) return rc;
	if (n < min_candidates(model)) {  // status 1 is a result: nothing to run
		empty_fit(out, 1, n);
		if (inlier_mask && n) memset(inlier_mask, 0, (size_t)n);
		return SIFT3D_OK;
	}
	CallState &S = g_ransac[device];
	std::lock_guard<std::mutex> lock(S.mu);
	// device scratch: [fit | mask | hyp 12 H | count H | pairs (host inputs)]; pinned host: [fit | mask]
	Layout L;
	L.take(sizeof(sift3d_affine_fit));
	const size_t o_mask = L.take((size_t)n), o_hyp = L.take(sizeof(double) * 12 * H), o_cnt = L.take(sizeof(int) * H);
	const size_t o_pairs = L.take(on_device ? 0 : sizeof(float) * 6 * (size_t)n);
	if ((rc = S.ensure(L.end, o_hyp))) return rc;
	hipStream_t st = S.stream;
	char *D = S.d.p, *P = S.h.p;
	const float *d_pairs = pairs6;
	if (on_device) {
		if ((rc = S.after_legacy_stream())) return rc;
	} else {
		d_pairs = reinterpret_cast<float *>(D + o_pairs);
		S3D_HIP_ST(st, hipMemcpyAsync(D + o_pairs, pairs6, sizeof(float) * 6 * (size_t)n, hipMemcpyHostToDevice, st));
	}
	S3D_HIP_ST(st, hipEventRecord(S.e0, st));
	double *d_hyp = reinterpret_cast<double *>(D + o_hyp);
	int *d_cnt = reinterpret_cast<int *>(D + o_cnt);
	sift3d_affine_fit *d_fit = reinterpret_cast<sift3d_affine_fit *>(D);
	unsigned char *d_mask = reinterpret_cast<unsigned char *>(D + o_mask);
	if (model == kAffine) launch_ransac_global(d_pairs, n, H, s, tau2, min_det, refine, d_hyp, d_cnt, d_fit, d_mask, st);
	else launch_rigid_global(d_pairs, n, H, s, tau2, min_det, model, refine, d_hyp, d_cnt, d_fit, d_mask, st);
	S3D_HIP_ST(st, hipGetLastError());
	S3D_HIP_ST(st, hipMemcpyAsync(P, D, inlier_mask ? o_mask + n : sizeof(sift3d_affine_fit), hipMemcpyDeviceToHost, st));
	S3D_HIP_ST(st, hipEventRecord(S.e1, st));
	if ((rc = S.finish(seconds))) return rc;
	memcpy(out, P, sizeof(sift3d_affine_fit));
	if (inlier_mask) memcpy(inlier_mask, P + o_mask, (size_t)n);
	return SIFT3D_OK;
}

int fit_local(const char *who, int model, const float *pairs6, int n, const float *points3, int m, int k, float radius,
              const sift3d_ransac_options *o, int on_device, int device, sift3d_affine_fit *out, int *neighbours, double *seconds) {
	int H, refine;
	double tau2, min_det;
	uint32_t s;
	if (n < 0 || m < 0 || k < min_candidates(model) || k > 64 || !std::isfinite(radius) || (n > 0 && !pairs6) ||
	    (m > 0 && (!points3 || !out)) || !take_options(o, true, H, tau2, min_det, refine, s)) {
		set_last_error(who);
		return SIFT3D_ERR_ARG;
	}
	if (seconds) *seconds = 0;
	int rc = pick_device(device);
	if (rc) return rc;
	if (m == 0) return SIFT3D_OK;
	CallState &S = g_ransac[device];
	std::lock_guard<std::mutex> lock(S.mu);
	// device scratch: [fits m | neighbours m k | pairs | points (host inputs)]; pinned host: [fits | neighbours]
	const size_t fit_bytes = sizeof(sift3d_affine_fit) * (size_t)m, nb_bytes = neighbours ? sizeof(int) * (size_t)m * k : 0;
	Layout L;
	L.take(fit_bytes);
	const size_t o_nb = L.take(nb_bytes), o_pairs = L.take(on_device ? 0 : sizeof(float) * 6 * (size_t)n);
	const size_t o_pts = L.take(on_device ? 0 : sizeof(float) * 3 * (size_t)m);
	if ((rc = S.ensure(L.end, o_nb + nb_bytes))) return rc;
	hipStream_t st = S.stream;
	char *D = S.d.p, *P = S.h.p;
	const float *d_pairs = pairs6, *d_pts = points3;
	if (on_device) {
		if ((rc = S.after_legacy_stream())) return rc;
	} else {
		d_pairs = reinterpret_cast<float *>(D + o_pairs);
		d_pts = reinterpret_cast<float *>(D + o_pts);
		if (n) S3D_HIP_ST(st, hipMemcpyAsync(D + o_pairs, pairs6, sizeof(float) * 6 * (size_t)n, hipMemcpyHostToDevice, st));
		S3D_HIP_ST(st, hipMemcpyAsync(D + o_pts, points3, sizeof(float) * 3 * (size_t)m, hipMemcpyHostToDevice, st));
	}
	const float r2 = radius > 0.f ? radius * radius : -1.f;  // (-1: no limit, whatever radius^2 rounds to)
	S3D_HIP_ST(st, hipEventRecord(S.e0, st));
	sift3d_affine_fit *d_fit = reinterpret_cast<sift3d_affine_fit *>(D);
	int *d_nb = neighbours ? reinterpret_cast<int *>(D + o_nb) : nullptr;
	if (model == kAffine) launch_ransac_local(d_pairs, n, d_pts, m, k, r2, H, s, tau2, min_det, refine, d_fit, d_nb, st);
	else launch_rigid_local(d_pairs, n, d_pts, m, k, r2, H, s, tau2, min_det, model, refine, d_fit, d_nb, st);
	S3D_HIP_ST(st, hipGetLastError());
	S3D_HIP_ST(st, hipMemcpyAsync(P, D, o_nb + nb_bytes, hipMemcpyDeviceToHost, st));
	S3D_HIP_ST(st, hipEventRecord(S.e1, st));
	if ((rc = S.finish(seconds))) return rc;
	memcpy(out, P, fit_bytes);
	if (neighbours) memcpy(neighbours, P + o_nb, nb_bytes);
	return SIFT3D_OK;
}
}  // namespace

extern "C" int sift3d_fit_affine(const float *pairs6, int n, const sift3d_ransac_options *o, int on_device, int device, sift3d_affine_fit *out,
                                 unsigned char *inlier_mask, double *seconds) {
	return fit_global("sift3d_fit_affine: bad argument", kAffine, pairs6, n, o, on_device, device, out, inlier_mask, seconds);
}

extern "C" int sift3d_fit_affine_local(const float *pairs6, int n, const float *points3, int m, int k, float radius, const sift3d_ransac_options *o,
                                       int on_device, int device, sift3d_affine_fit *out, int *neighbours, double *seconds) {
	return fit_local("sift3d_fit_affine_local: bad argument", kAffine, pairs6, n, points3, m, k, radius, o, on_device, device, out, neighbours,
	                 seconds);
}

extern "C" int sift3d_fit_rigid(const float *pairs6, int n, int model, const sift3d_ransac_options *o, int on_device, int device,
                                sift3d_affine_fit *out, unsigned char *inlier_mask, double *seconds) {
	if (model != 0 && model != 1) {
		set_last_error("sift3d_fit_rigid: bad argument");
		return SIFT3D_ERR_ARG;
	}
	return fit_global("sift3d_fit_rigid: bad argument", model, pairs6, n, o, on_device, device, out, inlier_mask, seconds);
}

extern "C" int sift3d_fit_rigid_local(const float *pairs6, int n, const float *points3, int m, int k, float radius, int model,
                                      const sift3d_ransac_options *o, int on_device, int device, sift3d_affine_fit *out, int *neighbours,
                                      double *seconds) {
	if (model != 0 && model != 1) {
		set_last_error("sift3d_fit_rigid_local: bad argument");
		return SIFT3D_ERR_ARG;
	}
	return fit_local("sift3d_fit_rigid_local: bad argument", model, pairs6, n, points3, m, k, radius, o, on_device, device, out,
	                 neighbours, seconds);
}

// One fit per body.  The pairs are segmented by label on the host: a stable counting sort (two passes over the labels, which are
// copied down first when they lie on the device) gives the list of pair indices grouped by body in ascending order, whatever the
// size of a body -- one body may hold every pair -- and the list and the count + 1 segment bounds go up in one copy each.
extern "C" int sift3d_fit_rigid_bodies(const float *pairs6, int n, const int *pair_label, int count, int model, const sift3d_ransac_options *o,
                                       int on_device, int device, sift3d_affine_fit *out, unsigned char *inlier_mask, double *seconds) {
	int H, refine;
	double tau2, min_det;
	uint32_t s;
	if (n < 0 || count < 0 || (model != 0 && model != 1) || (n > 0 && (!pairs6 || !pair_label)) || (count > 0 && !out) ||
	    !take_options(o, true, H, tau2, min_det, refine, s)) {
		set_last_error("sift3d_fit_rigid_bodies: bad argument");
		return SIFT3D_ERR_ARG;
	}
	if (seconds) *seconds = 0;
	int rc = pick_device(device);
	if (rc) return rc;
	if (n == 0 || count == 0) {  // every body is empty: status 1 is a result, nothing to run
		for (int b = 0; b < count; b++) empty_fit(out + b, 1, 0);
		if (inlier_mask && n) memset(inlier_mask, 0, (size_t)n);
		return SIFT3D_OK;
	}
	CallState &S = g_ransac[device];
	std::lock_guard<std::mutex> lock(S.mu);
	// device scratch: [fits count | mask n | list n | bounds count + 1 | pairs (host inputs)]; pinned host: the first four pieces at the
	// same offsets, then the labels (device inputs)
	const size_t fit_bytes = sizeof(sift3d_affine_fit) * (size_t)count, list_bytes = sizeof(int) * (size_t)n;
	const size_t off_bytes = sizeof(int) * ((size_t)count + 1);
	Layout L;
	L.take(fit_bytes);
	const size_t o_mask = L.take((size_t)n), o_list = L.take(list_bytes), o_off = L.take(off_bytes);
	const size_t o_last = L.take(on_device ? 0 : sizeof(float) * 6 * (size_t)n);  // device: the pairs; pinned: the labels
	if ((rc = S.ensure(L.end, o_last + (on_device ? list_bytes : 0)))) return rc;
	hipStream_t st = S.stream;
	char *D = S.d.p, *P = S.h.p;
	const float *d_pairs = pairs6;
	const int *lab = pair_label;
	if (on_device) {
		if ((rc = S.after_legacy_stream())) return rc;
		S3D_HIP_ST(st, hipMemcpyAsync(P + o_last, pair_label, list_bytes, hipMemcpyDeviceToHost, st));
		S3D_HIP_ST(st, hipStreamSynchronize(st));
		lab = reinterpret_cast<const int *>(P + o_last);
	} else {
		d_pairs = reinterpret_cast<float *>(D + o_last);
		S3D_HIP_ST(st, hipMemcpyAsync(D + o_last, pairs6, sizeof(float) * 6 * (size_t)n, hipMemcpyHostToDevice, st));
	}
	int *list = reinterpret_cast<int *>(P + o_list), *off = reinterpret_cast<int *>(P + o_off);
	memset(off, 0, off_bytes);
	for (int i = 0; i < n; i++)
		if (lab[i] >= 1 && lab[i] <= count) off[lab[i]]++;
	std::vector<int> at((size_t)count);
	for (int b = 1; b <= count; b++) {
		at[b - 1] = off[b - 1];
		off[b] += off[b - 1];
	}
	for (int i = 0; i < n; i++)
		if (lab[i] >= 1 && lab[i] <= count) list[at[lab[i] - 1]++] = i;
	if (off[count]) S3D_HIP_ST(st, hipMemcpyAsync(D + o_list, list, sizeof(int) * (size_t)off[count], hipMemcpyHostToDevice, st));
	S3D_HIP_ST(st, hipMemcpyAsync(D + o_off, off, off_bytes, hipMemcpyHostToDevice, st));
	S3D_HIP_ST(st, hipEventRecord(S.e0, st));
	S3D_HIP_ST(st, hipMemsetAsync(D + o_mask, 0, (size_t)n, st));
	launch_rigid_bodies(d_pairs, reinterpret_cast<int *>(D + o_list), reinterpret_cast<int *>(D + o_off), count, H, s, tau2, min_det, model, refine,
	                    reinterpret_cast<sift3d_affine_fit *>(D), reinterpret_cast<unsigned char *>(D + o_mask), st);
	S3D_HIP_ST(st, hipGetLastError());
	S3D_HIP_ST(st, hipMemcpyAsync(P, D, inlier_mask ? o_mask + n : fit_bytes, hipMemcpyDeviceToHost, st));
	S3D_HIP_ST(st, hipEventRecord(S.e1, st));
	if ((rc = S.finish(seconds))) return rc;
	memcpy(out, P, fit_bytes);
	if (inlier_mask) memcpy(inlier_mask, P + o_mask, (size_t)n);
	return SIFT3D_OK;
}

extern "C" int sift3d_fit_rotation(const sift3d_affine_fit *fits, int m, double *quat4, double *scale, double *angle_deg) {
	if (m < 0 || (m > 0 && (!fits || !quat4 || !scale || !angle_deg))) {
		set_last_error("sift3d_fit_rotation: bad argument");
		return SIFT3D_ERR_ARG;
	}
	for (int p = 0; p < m; p++) {
		double *q = quat4 + 4 * (size_t)p;
		if (fits[p].status != 0) {
			q[0] = q[1] = q[2] = q[3] = scale[p] = angle_deg[p] = NAN;
			continue;
		}
		const double *A = fits[p].A;
		const double det = (A[0] * (A[5] * A[10] - A[6] * A[9]) - A[1] * (A[4] * A[10] - A[6] * A[8])) + A[2] * (A[4] * A[9] - A[5] * A[8]);
		const double s = cbrt(det);
		double R[3][3];
		for (int i = 0; i < 3; i++)
			for (int j = 0; j < 3; j++) R[i][j] = A[4 * i + j] / s;
		// Shepperd: the branch of the largest of (trace, R00, R11, R22) keeps the divisor away from zero
		const double tr = (R[0][0] + R[1][1]) + R[2][2];
		double w, x, y, z;
		if (tr >= R[0][0] && tr >= R[1][1] && tr >= R[2][2]) {
			w = 1.0 + tr; x = R[2][1] - R[1][2]; y = R[0][2] - R[2][0]; z = R[1][0] - R[0][1];
		} else if (R[0][0] >= R[1][1] && R[0][0] >= R[2][2]) {
			w = R[2][1] - R[1][2]; x = (1.0 + R[0][0]) - (R[1][1] + R[2][2]); y = R[0][1] + R[1][0]; z = R[0][2] + R[2][0];
		} else if (R[1][1] >= R[2][2]) {
			w = R[0][2] - R[2][0]; x = R[0][1] + R[1][0]; y = (1.0 + R[1][1]) - (R[0][0] + R[2][2]); z = R[1][2] + R[2][1];
		} else {
			w = R[1][0] - R[0][1]; x = R[0][2] + R[2][0]; y = R[1][2] + R[2][1]; z = (1.0 + R[2][2]) - (R[0][0] + R[1][1]);
		}
		const double nq = (w < 0.0 ? -1.0 : 1.0) * sqrt((w * w + x * x) + (y * y + z * z));
		q[0] = w / nq; q[1] = x / nq; q[2] = y / nq; q[3] = z / nq;
		scale[p] = s;
		angle_deg[p] = 2.0 * atan2(sqrt((q[1] * q[1] + q[2] * q[2]) + q[3] * q[3]), q[0]) * (180.0 / M_PI);
	}
	return SIFT3D_OK;
}
