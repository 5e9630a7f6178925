// entry_match_guided.hip -- C-ABI of guided matching (include/sift3d_hip.h: sift3d_match_guided, sift3d_predict_positions).  The gate
// has no reference counterpart; scoring and bookkeeping are muBruteMatcher's (reference Src/cMatcher.cc:40-144; match_host.h).  Call
// state, scratch layout, timing and the order of the checks: DESIGN 4.10 (call_state.h).  The cell grids of the two POI indexes depend
// on the positions' bounding boxes (poi_grid.h), so they are allocated and freed inside the call.
#include <float.h>
#include <math.h>
#include <string.h>

#include <algorithm>

#include "call_state.h"
#include "match_host.h"
#include "poi_grid.h"

using namespace s3d;

namespace {
struct GuidedState : CallState {
	DevBlock ab;  // device copies of host-resident descriptor matrices
};
GuidedState g_guided[kMaxDev];

constexpr float kMaxRadius = 1048576.0f;  // 2^20: with the index's coordinate bound 2^24 a window's corners stay far inside an int
}  // namespace

extern "C" int sift3d_predict_positions(const sift3d_affine_fit *fits, int nfits, const float *xyz3, int n, float *pred3) {
	if (n < 0 || (nfits != 1 && nfits != n) || (n > 0 && (!fits || !xyz3 || !pred3))) {
		set_last_error("sift3d_predict_positions: bad argument");
		return SIFT3D_ERR_ARG;
	}
	for (int i = 0; i < n; i++) {
		const sift3d_affine_fit &f = fits[nfits == 1 ? 0 : i];
		const double *A = f.A;
		const double r[3] = {(double)xyz3[3 * (size_t)i], (double)xyz3[3 * (size_t)i + 1], (double)xyz3[3 * (size_t)i + 2]};
		for (int a = 0; a < 3; a++)
			pred3[3 * (size_t)i + a] = f.status != 0 ? NAN : (float)(((A[4 * a] * r[0] + A[4 * a + 1] * r[1]) + A[4 * a + 2] * r[2]) + A[4 * a + 3]);
	}
	return SIFT3D_OK;
}

extern "C" int sift3d_match_guided(const float *ref_desc, const float *ref_xyz, int n, const float *tar_desc, const float *tar_xyz, int m,
                                   const float *pred_xyz, float radius, double thresHold, int mode, int on_device, int device, int *gIdx,
                                   int *sIdx, float *gDist, float *sDist, int *candidates, float *pairs6, int *npairs, double *seconds) {
	if (n < 0 || m < 0 || mode < 1 || mode > 3 || (n > 0 && (!ref_desc || !ref_xyz || !pred_xyz)) || (m > 0 && (!tar_desc || !tar_xyz)) ||
	    !(radius > 0.f) || !(radius <= kMaxRadius)) {  // (a NaN radius fails both comparisons)
		set_last_error("sift3d_match_guided: bad argument");
		return SIFT3D_ERR_ARG;
	}
	int rc = pick_device(device);
	if (rc) return rc;
	if (npairs) *npairs = 0;
	if (seconds) *seconds = 0;

	std::vector<float> gd(n, (float)(2 - 2 * (double)FLT_MIN)), sd(n, (float)(2 - 2 * (double)FLT_MIN)), gd2(m, 0.f), sd2(m, 0.f);
	std::vector<int> gi(n, -1), si(n, -1), gi2(m, -1), cand(n, 0);
	auto deliver = [&](const float *rx, const float *tx) {
		const int np = match_to_cvec(gi, rx, tx, pairs6);
		if (npairs) *npairs = np;
		for (int i = 0; i < n; i++) {
			if (gIdx) gIdx[i] = gi[i];
			if (sIdx) sIdx[i] = si[i];
			if (gDist) gDist[i] = gd[i];
			if (sDist) sDist[i] = sd[i];
			if (candidates) candidates[i] = cand[i];
		}
	};
	if (n == 0 || m == 0) {  // every gate is empty: index -1 and d = 2 - 2 * FLT_MIN in both places, no pair
		deliver(nullptr, nullptr);
		return SIFT3D_OK;
	}

	GuidedState &S = g_guided[device];
	std::lock_guard<std::mutex> lock(S.mu);
	const size_t nn = (size_t)n, mm = (size_t)m, big = std::max(nn, mm);
	// block d: [results gd | sd | gi | si | gate sizes (ONE D2H copy) | rows of the reverse pass | the two indexes' pieces | floors and
	// exact values of the table being indexed | (host inputs) tar_xyz | pred_xyz]; pinned host: [results | ref_xyz, tar_xyz (device inputs)]
	Layout L, H;
	const size_t res_bytes = 4 * 5 * big;
	const size_t o_res = L.take(res_bytes), o_rows = L.take(4 * big);
	PoiGridPlan Gt, Gp;
	Gt.take(L, m);
	Gp.take(L, n);
	const size_t o_pts = L.take(sizeof(int) * 3 * big), o_disp = L.take(sizeof(double) * 3 * big);
	const size_t b_txyz = on_device ? 0 : sizeof(float) * 3 * mm, b_pxyz = on_device ? 0 : sizeof(float) * 3 * nn;
	const size_t o_txyz = L.take(b_txyz), o_pxyz = L.take(b_pxyz);
	const size_t h_res = H.take(res_bytes), h_xyz = H.take(on_device ? sizeof(float) * 3 * (nn + mm) : 0);
	if ((rc = S.ensure(L.end, H.end))) return rc;
	hipStream_t st = S.stream;
	if (!on_device && (rc = S.ab.reserve(sizeof(float) * kDesc * (nn + mm), st))) return rc;

	char *D = S.d.p;
	const float *rx = ref_xyz, *tx = tar_xyz;  // host copies of the coordinates, for the pairs
	const float *d_a = ref_desc, *d_b = tar_desc, *d_txyz = tar_xyz, *d_pxyz = pred_xyz;
	if (on_device) {
		if ((rc = S.after_legacy_stream())) return rc;
		float *hx = reinterpret_cast<float *>(S.h.p + h_xyz), *hy = hx + 3 * nn;
		S3D_HIP_ST(st, hipMemcpyAsync(hx, ref_xyz, sizeof(float) * 3 * nn, hipMemcpyDeviceToHost, st));
		S3D_HIP_ST(st, hipMemcpyAsync(hy, tar_xyz, sizeof(float) * 3 * mm, hipMemcpyDeviceToHost, st));
		rx = hx; tx = hy;  // read after the first synchronisation below
	} else {
		float *da = reinterpret_cast<float *>(S.ab.p), *db = da + (size_t)kDesc * nn;
		S3D_HIP_ST(st, hipMemcpyAsync(da, ref_desc, sizeof(float) * kDesc * nn, hipMemcpyHostToDevice, st));
		S3D_HIP_ST(st, hipMemcpyAsync(db, tar_desc, sizeof(float) * kDesc * mm, hipMemcpyHostToDevice, st));
		d_a = da; d_b = db;
		S3D_HIP_ST(st, upload(d_txyz, D, o_txyz, b_txyz, st));
		S3D_HIP_ST(st, upload(d_pxyz, D, o_pxyz, b_pxyz, st));
	}
	float *d_gd = reinterpret_cast<float *>(D + o_res), *d_sd = d_gd + big;
	int *d_gi = reinterpret_cast<int *>(d_sd + big), *d_si = d_gi + big, *d_cnt = d_si + big;
	int *d_rows = reinterpret_cast<int *>(D + o_rows), *d_pts = reinterpret_cast<int *>(D + o_pts);
	double *d_disp = reinterpret_cast<double *>(D + o_disp);
	const float *h_gd = reinterpret_cast<const float *>(S.h.p + h_res), *h_sd = h_gd + big;
	const int *h_gi = reinterpret_cast<const int *>(h_sd + big), *h_si = h_gi + big, *h_cnt = h_si + big;
	// A window of half width ceil(radius) around floor(pred) is NOT a superset of the fp32 gate: pred.x = 0.99999994f, tar.x = 17.0f,
	// radius 16 -- the difference rounds to 16.0f (in the gate) while the floors differ by 17.  The rounded difference is within half an
	// ulp of the exact one, below 1 for radius <= 2^20, so |floor(tar) - floor(pred)| < radius + 2: ceil(radius) + 1 covers the gate.
	const int half_width = (int)ceilf(radius) + 1;
	CallTemps Tt, Tp;  // the cell arrays of the two indexes
	PoiIndex ix;

	S3D_HIP_ST(st, hipEventRecord(S.e0, st));
	// ---- ref -> tar: the index over the target positions, every reference row against its gate ----
	launch_gate_points(d_txyz, m, d_pts, d_disp, st);
	if ((rc = poi_grid_build(Gt, D, d_pts, d_disp, nullptr, m, half_width, Tt, st, ix))) return rc;
	launch_match_gated(d_a, d_pxyz, nullptr, n, d_b, ix, radius, half_width, d_gd, d_sd, d_gi, d_si, d_cnt, st);
	S3D_HIP_ST(st, hipGetLastError());
	S3D_HIP_ST(st, hipMemcpyAsync(S.h.p + h_res, D + o_res, res_bytes, hipMemcpyDeviceToHost, st));
	S3D_HIP_ST(st, hipEventRecord(S.e1, st));  // device time ends with the last device operation of the call (recorded again behind a reverse pass)
	S3D_HIP_ST(st, hipStreamSynchronize(st));
	memcpy(gd.data(), h_gd, sizeof(float) * nn); memcpy(sd.data(), h_sd, sizeof(float) * nn);
	memcpy(gi.data(), h_gi, sizeof(int) * nn); memcpy(si.data(), h_si, sizeof(int) * nn);
	memcpy(cand.data(), h_cnt, sizeof(int) * nn);
	match_ratio_filter(gi, gd, sd, thresHold);

	if (mode != 1) {
		std::vector<int> cnt;
		const std::vector<int> rows = match_mask_rows(gi, m, mode, cnt);
		// ---- tar -> ref over the masked targets only: the index over the predicted positions, target j against { i : j in gate(i) } ----
		if (!rows.empty()) {
			S3D_HIP_ST(st, hipMemcpyAsync(d_rows, rows.data(), sizeof(int) * rows.size(), hipMemcpyHostToDevice, st));
			launch_gate_points(d_pxyz, n, d_pts, d_disp, st);
			if ((rc = poi_grid_build(Gp, D, d_pts, d_disp, nullptr, n, half_width, Tp, st, ix))) return rc;
			launch_match_gated(d_b, d_txyz, d_rows, (int)rows.size(), d_a, ix, radius, half_width, d_gd, d_sd, d_gi, d_si, nullptr, st);
			S3D_HIP_ST(st, hipGetLastError());
			S3D_HIP_ST(st, hipMemcpyAsync(S.h.p + h_res, D + o_res, res_bytes, hipMemcpyDeviceToHost, st));
			S3D_HIP_ST(st, hipEventRecord(S.e1, st));
			S3D_HIP_ST(st, hipStreamSynchronize(st));
			for (int j : rows) { gd2[j] = h_gd[j]; sd2[j] = h_sd[j]; gi2[j] = h_gi[j]; }
		}
		match_ratio_filter(gi2, gd2, sd2, thresHold);
		match_biject(gi, cnt, gi2);
	}
	if ((rc = S.finish(seconds))) return rc;
	deliver(rx, tx);
	return SIFT3D_OK;
}
