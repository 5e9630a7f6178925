// entry_match.hip -- the brute-force matcher's C-ABI (sift3d_match*, include/sift3d_hip.h) over the kernels of kernels_match.hip.
//
// muBruteMatcher::bijectMatchBase (Src/cMatcher.cc:146-215).  The O(N*M*768) passes run on
// the device; the O(N) bookkeeping (ratio filter, countMatched, toMask, bijectFilter, toCvec) is
// replayed on the host exactly as written in the reference, including its sign-flip quirks (match_host.h).
#include <float.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <vector>

#include "sift3d_internal.h"
#include "call_state.h"
#include "match_host.h"

using namespace s3d;

// Per-device matcher state (call_state.h; r03: a call used to do 3-5 hipMalloc / hipFree and ran on the null stream).  d holds
// everything but the descriptor matrices, h the results of a pass (+ the coordinates of device-resident inputs).
namespace {
struct MatchState : CallState {
	DevBlock ab;  // device copies of host-resident descriptor matrices
};
MatchState g_match[kMaxDev];
thread_local double t_match_dev = 0.0, t_match_wall = 0.0;
thread_local int t_match_redo_rows = 0;  // rows re-scored exactly by the calling thread's last call (sift3d_debug_counters)
}  // namespace

namespace s3d { int match_redo_rows() { return t_match_redo_rows; } }

// First use of the matcher on a device, ahead of time (muBruteMatcher's constructor, sift3d_create): the kernels' code object is
// loaded (preload_match_kernels), the stream and the events exist.  Never fails loudly: a device that cannot be prepared fails in
// sift3d_match.
extern "C" int sift3d_match_warmup(int device) {
	int rc = pick_device(device);
	if (rc) return rc;
	s3d::preload_match_kernels();
	MatchState &S = g_match[device];
	std::lock_guard<std::mutex> lock(S.mu);
	return S.ensure(0, 0);  // (stream and events; the scratch is sized by the first call)
}

extern "C" int sift3d_match_times(double *device_seconds, double *wall_seconds) {
	if (device_seconds) *device_seconds = t_match_dev;
	if (wall_seconds) *wall_seconds = t_match_wall;
	return SIFT3D_OK;
}

extern "C" int sift3d_match(const float *ref_desc, const float *ref_xyz, int n, const float *tar_desc, const float *tar_xyz, int m,
                            double thresHold, int mode, int on_device, int device, int *gIdx, int *sIdx, float *gDist,
                            float *sDist, float *pairs6, int *npairs, double *seconds) {
	const auto wall0 = std::chrono::steady_clock::now();
	if (n < 0 || m < 0 || mode < 1 || mode > 3 || (n > 0 && (!ref_desc || !ref_xyz)) || (m > 0 && (!tar_desc || !tar_xyz))) {
		set_last_error("sift3d_match: bad argument");
		return SIFT3D_ERR_ARG;
	}
	int rc = pick_device(device);
	if (rc) return rc;
	if (npairs) *npairs = 0;
	if (seconds) *seconds = 0;
	t_match_dev = t_match_wall = 0.0;

	MatchState &S = g_match[device];
	std::lock_guard<std::mutex> lock(S.mu);
	const size_t nn = (size_t)std::max(n, 1), mm = (size_t)std::max(m, 1), big = std::max(nn, mm);
	// device scratch layout (256-B aligned pieces): results [gd | sd | gi | si] of a pass (ONE D2H copy), then the working arrays
	// pinned host: [results | redo count | coordinates (device inputs)]
	Layout L, H;
	const size_t o_res = L.take(4 * 4 * big), o_cand = L.take(match_cand_bytes(big)), o_rows = L.take(4 * big), o_redo = L.take(4 * (big + 1));
	const size_t o_s4 = L.take(4 * big), o_an2 = L.take(4 * nn), o_bn2 = L.take(4 * mm), o_nmax = L.take(2 * sizeof(unsigned));
	const size_t o_part = L.take(match_part_bytes(big));
	const size_t h_res = H.take(4 * 4 * big), h_redo_at = H.take(sizeof(int)), h_xyz = H.take(on_device ? 4 * 3 * (nn + mm) : 0);
	if ((rc = S.ensure(L.end, H.end))) return rc;
	hipStream_t st = S.stream;
	if (!on_device && (rc = S.ab.reserve(sizeof(float) * kDesc * (nn + mm), st))) return rc;

	std::vector<float> gd(n, 0.f), sd(n, 0.f), gd2(m, 0.f), sd2(m, 0.f);
	std::vector<int> gi(n, -1), si(n, -1), gi2(m, -1), si2(m, -1);
	const float *rx = ref_xyz, *tx = tar_xyz;
	int redo_rows = 0;
	float *d_a, *d_b;
	if (on_device) {
		if ((rc = S.after_legacy_stream())) return rc;
		d_a = const_cast<float *>(ref_desc); d_b = const_cast<float *>(tar_desc);
		float *hx = reinterpret_cast<float *>(S.h.p + h_xyz), *hy = hx + 3 * nn;
		if (n) S3D_HIP_ST(st, hipMemcpyAsync(hx, ref_xyz, sizeof(float) * 3 * n, hipMemcpyDeviceToHost, st));
		if (m) S3D_HIP_ST(st, hipMemcpyAsync(hy, tar_xyz, sizeof(float) * 3 * m, hipMemcpyDeviceToHost, st));
		rx = hx; tx = hy;  // read after the first synchronisation below
	} else {
		d_a = reinterpret_cast<float *>(S.ab.p); d_b = d_a + (size_t)kDesc * nn;
		if (n) S3D_HIP_ST(st, hipMemcpyAsync(d_a, ref_desc, sizeof(float) * kDesc * n, hipMemcpyHostToDevice, st));
		if (m) S3D_HIP_ST(st, hipMemcpyAsync(d_b, tar_desc, sizeof(float) * kDesc * m, hipMemcpyHostToDevice, st));
	}
	{
		char *D = S.d.p;
		float *d_gd = reinterpret_cast<float *>(D + o_res), *d_sd = d_gd + big;
		int *d_gi = reinterpret_cast<int *>(d_sd + big), *d_si = d_gi + big;
		int *d_cand = reinterpret_cast<int *>(D + o_cand), *d_rows = reinterpret_cast<int *>(D + o_rows), *d_redo = reinterpret_cast<int *>(D + o_redo);
		float *d_s4 = reinterpret_cast<float *>(D + o_s4), *d_an2 = reinterpret_cast<float *>(D + o_an2), *d_bn2 = reinterpret_cast<float *>(D + o_bn2);
		unsigned *d_nmax = reinterpret_cast<unsigned *>(D + o_nmax);
		void *d_part = D + o_part;
		float *h_gd = reinterpret_cast<float *>(S.h.p + h_res), *h_sd = h_gd + big;
		int *h_gi = reinterpret_cast<int *>(h_sd + big), *h_si = h_gi + big;
		int *h_redo = reinterpret_cast<int *>(S.h.p + h_redo_at);

		S3D_HIP_ST(st, hipEventRecord(S.e0, st));
		S3D_HIP_ST(st, hipMemsetAsync(d_nmax, 0, 2 * sizeof(unsigned), st));
		launch_row_norm2(d_a, n, d_an2, d_b, m, d_bn2, d_nmax, st);
		// matrices of 4 GB and more take the register-staged form (SIFT3D_HOOK_MATCH_NODMA forces it on any size, for the tests)
		const bool small = !hook(SIFT3D_HOOK_MATCH_NODMA) && (size_t)std::max(n, m) * kDesc * sizeof(float) < ((size_t)1 << 32);
		const MatchGuard g_fwd{d_s4, d_an2, d_nmax + 1, d_redo, small}, g_rev{d_s4, d_bn2, d_nmax, d_redo, small};

		// ---- ref -> tar ----
		if (n > 0 && m > 0) {
			match_rows_device(d_a, nullptr, n, d_b, m, d_cand, d_part, d_gd, d_sd, d_gi, d_si, g_fwd, st);
			S3D_HIP_ST(st, hipMemcpyAsync(h_gd, d_gd, 4 * 4 * big, hipMemcpyDeviceToHost, st));
			S3D_HIP_ST(st, hipMemcpyAsync(h_redo, d_redo, sizeof(int), hipMemcpyDeviceToHost, st));
			S3D_HIP_ST(st, hipEventRecord(S.e1, st));  // device time ends with the last device operation of the call (recorded again behind a reverse pass)
			S3D_HIP_ST(st, hipStreamSynchronize(st));
			memcpy(gd.data(), h_gd, sizeof(float) * n); memcpy(sd.data(), h_sd, sizeof(float) * n);
			memcpy(gi.data(), h_gi, sizeof(int) * n); memcpy(si.data(), h_si, sizeof(int) * n);
			redo_rows += h_redo[0];
		} else {
			S3D_HIP_ST(st, hipEventRecord(S.e1, st));
			S3D_HIP_ST(st, hipStreamSynchronize(st));
			// no targets: every dot loop is empty -> d = 2 - 2*FLT_MIN, idx -1
			for (int i = 0; i < n; i++) { gd[i] = sd[i] = (float)(2 - 2 * (double)FLT_MIN); }
		}
		match_ratio_filter(gi, gd, sd, thresHold);

		if (mode != 1) {
			std::vector<int> cnt;
			const std::vector<int> rows = match_mask_rows(gi, m, mode, cnt);
			// ---- tar -> ref over the masked targets only (masked-out rows keep gIdx2 = -1) ----
			if (!rows.empty() && n > 0) {
				S3D_HIP_ST(st, hipMemcpyAsync(d_rows, rows.data(), sizeof(int) * rows.size(), hipMemcpyHostToDevice, st));
				match_rows_device(d_b, d_rows, (int)rows.size(), d_a, n, d_cand, d_part, d_gd, d_sd, d_gi, d_si, g_rev, st);
				S3D_HIP_ST(st, hipMemcpyAsync(h_gd, d_gd, 4 * 4 * big, hipMemcpyDeviceToHost, st));
				S3D_HIP_ST(st, hipMemcpyAsync(h_redo, d_redo, sizeof(int), hipMemcpyDeviceToHost, st));
				S3D_HIP_ST(st, hipEventRecord(S.e1, st));
				S3D_HIP_ST(st, hipStreamSynchronize(st));
				for (int j : rows) { gd2[j] = h_gd[j]; sd2[j] = h_sd[j]; gi2[j] = h_gi[j]; si2[j] = h_si[j]; }
				redo_rows += h_redo[0];
			}
			match_ratio_filter(gi2, gd2, sd2, thresHold);
			match_biject(gi, cnt, gi2);
		}
		if ((rc = S.finish(&t_match_dev))) return rc;
		if (seconds) *seconds = t_match_dev;

		const int np = match_to_cvec(gi, rx, tx, pairs6);
		if (npairs) *npairs = np;
		for (int i = 0; i < n; i++) {
			if (gIdx) gIdx[i] = gi[i];
			if (sIdx) sIdx[i] = si[i];
			if (gDist) gDist[i] = gd[i];
			if (sDist) sDist[i] = sd[i];
		}
	}
	t_match_redo_rows = redo_rows;
	t_match_wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - wall0).count();
	return SIFT3D_OK;
}
