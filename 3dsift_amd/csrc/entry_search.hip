// entry_search.hip -- C-ABI of the ZNCC integer search (include/sift3d_hip.h: sift3d_zncc_search, sift3d_icgn_init_from_search,
// sift3d_default_search_options).  No reference counterpart.  Conventions of entry_icgn.hip: per-device state created on first use
// -- a non-blocking stream, timing events, a grow-only device scratch and a pinned host block for the results --, one call at a time
// per device, device time from HIP events (input uploads excluded, the result copy included), arguments checked before any device call.
#include "sift3d_internal.h"

#include <math.h>
#include <string.h>

#include <mutex>

using namespace s3d;

namespace {
struct SearchDevState {
	std::mutex mu;
	bool ready = false;
	hipStream_t stream = nullptr;
	hipEvent_t e0 = nullptr, e1 = nullptr, e_in = nullptr;
	char *d_scratch = nullptr; size_t d_bytes = 0;
	char *h_pin = nullptr; size_t h_bytes = 0;
};
constexpr int kMaxDev = 64;
SearchDevState g_search[kMaxDev];

int ensure(SearchDevState &S, size_t d_bytes, size_t h_bytes) {
	if (!S.ready) {
		if (!S.stream) S3D_HIP(hipStreamCreateWithFlags(&S.stream, hipStreamNonBlocking));
		if (!S.e0) S3D_HIP(hipEventCreate(&S.e0));
		if (!S.e1) S3D_HIP(hipEventCreate(&S.e1));
		if (!S.e_in) S3D_HIP(hipEventCreateWithFlags(&S.e_in, hipEventDisableTiming));
		S.ready = true;
	}
	auto grow = [](size_t want) { return want + want / 4 + 4096; };
	if (d_bytes > S.d_bytes) {
		S3D_HIP(hipStreamSynchronize(S.stream));
		if (S.d_scratch) (void)hipFree(S.d_scratch);
		S.d_scratch = nullptr; S.d_bytes = 0;
		S3D_HIP(hipMalloc(&S.d_scratch, grow(d_bytes)));
		S.d_bytes = grow(d_bytes);
	}
	if (h_bytes > S.h_bytes) {
		if (S.h_pin) (void)hipHostFree(S.h_pin);
		S.h_pin = nullptr; S.h_bytes = 0;
		S3D_HIP(hipHostMalloc(&S.h_pin, grow(h_bytes), hipHostMallocDefault));
		S.h_bytes = grow(h_bytes);
	}
	return SIFT3D_OK;
}
size_t al256(size_t b) { return (b + 255) & ~(size_t)255; }

// options (NULL: defaults) -> checked values
bool take_options(const sift3d_search_options *o, int &r, int &s) {
	sift3d_search_options d;
	sift3d_default_search_options(&d);
	if (!o) o = &d;
	if (o->subset_radius < 2 || o->subset_radius > 16 || o->search_radius < 1 || o->search_radius > 16) return false;
	for (int k = 0; k < 6; k++)
		if (o->reserved[k]) return false;
	r = o->subset_radius;
	s = o->search_radius;
	return true;
}

int pick_device(int device) {
	int ndev = 0;
	if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { set_last_error("no HIP device visible: no CPU fallback"); return SIFT3D_ERR_NO_DEVICE; }
	if (device < 0 || device >= ndev || device >= kMaxDev) { set_last_error("bad device index"); return SIFT3D_ERR_ARG; }
	S3D_HIP(hipSetDevice(device));
	return SIFT3D_OK;
}
}  // namespace

extern "C" void sift3d_default_search_options(sift3d_search_options *o) {
	if (!o) return;
	memset(o, 0, sizeof(*o));
	o->subset_radius = 8;
	o->search_radius = 8;
}

extern "C" int sift3d_icgn_init_from_search(const sift3d_search_result *res, int m, int only_missing, double *init12) {
	if (m < 0 || (m > 0 && (!res || !init12))) {
		set_last_error("sift3d_icgn_init_from_search: bad argument");
		return SIFT3D_ERR_ARG;
	}
	for (int i = 0; i < m; i++) {
		double *p = init12 + 12 * (size_t)i;
		if (res[i].status != 0) continue;
		if (only_missing) {
			bool finite = true;
			for (int k = 0; k < 12; k++) finite = finite && std::isfinite(p[k]);
			if (finite) continue;
		}
		for (int k = 0; k < 12; k++) p[k] = 0.0;
		for (int a = 0; a < 3; a++) p[4 * a] = (double)res[i].d[a];
	}
	return SIFT3D_OK;
}

#define SCHK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { set_last_error(std::string(#call) + ": " + hipGetErrorString(e_)); (void)hipStreamSynchronize(st); return SIFT3D_ERR_HIP; } } while (0)

extern "C" int sift3d_zncc_search(const float *ref, int rnx, int rny, int rnz, const float *tar, int tnx, int tny, int tnz, const int *points3, int m,
                                  const int *guess3, const sift3d_search_options *o, int on_device, int device, sift3d_search_result *out,
                                  double *seconds) {
	int r, s;
	if (m < 0 || rnx < 1 || rny < 1 || rnz < 1 || tnx < 1 || tny < 1 || tnz < 1 || !ref || !tar || !out || (m > 0 && !points3) ||
	    !take_options(o, r, s)) {
		set_last_error("sift3d_zncc_search: bad argument");
		return SIFT3D_ERR_ARG;
	}
	if (seconds) *seconds = 0;
	int rc = pick_device(device);
	if (rc) return rc;
	if (m == 0) return SIFT3D_OK;
	SearchDevState &S = g_search[device];
	std::lock_guard<std::mutex> lock(S.mu);
	// device scratch: [results m | score tables | (host inputs) ref | tar | points | guess]; pinned host: [results]
	const size_t nr = (size_t)rnx * rny * rnz, nt = (size_t)tnx * tny * tnz, res_bytes = sizeof(sift3d_search_result) * (size_t)m;
	const size_t o_sc = al256(res_bytes), o_ref = o_sc + al256(search_score_bytes(m, s));
	const size_t o_tar = o_ref + (on_device ? 0 : al256(sizeof(float) * nr)), o_pts = o_tar + (on_device ? 0 : al256(sizeof(float) * nt));
	const size_t o_gs = o_pts + (on_device ? 0 : al256(sizeof(int) * 3 * (size_t)m));
	const size_t d_bytes = o_gs + (on_device || !guess3 ? 0 : sizeof(int) * 3 * (size_t)m);
	if ((rc = ensure(S, d_bytes, res_bytes))) return rc;
	hipStream_t st = S.stream;
	char *D = S.d_scratch;
	const float *d_ref = ref, *d_tar = tar;
	const int *d_pts = points3, *d_gs = guess3;
	if (on_device) {
		// device inputs: work the caller queued on the legacy default stream is ordered in front (as in sift3d_icgn)
		SCHK(hipEventRecord(S.e_in, nullptr));
		SCHK(hipStreamWaitEvent(st, S.e_in, 0));
	} else {
		d_ref = reinterpret_cast<float *>(D + o_ref);
		d_tar = reinterpret_cast<float *>(D + o_tar);
		d_pts = reinterpret_cast<int *>(D + o_pts);
		SCHK(hipMemcpyAsync(D + o_ref, ref, sizeof(float) * nr, hipMemcpyHostToDevice, st));
		SCHK(hipMemcpyAsync(D + o_tar, tar, sizeof(float) * nt, hipMemcpyHostToDevice, st));
		SCHK(hipMemcpyAsync(D + o_pts, points3, sizeof(int) * 3 * (size_t)m, hipMemcpyHostToDevice, st));
		if (guess3) {
			d_gs = reinterpret_cast<int *>(D + o_gs);
			SCHK(hipMemcpyAsync(D + o_gs, guess3, sizeof(int) * 3 * (size_t)m, hipMemcpyHostToDevice, st));
		}
	}
	SCHK(hipEventRecord(S.e0, st));
	launch_zncc_search(IcgnVol{d_ref, rnx, rny, rnz}, IcgnVol{d_tar, tnx, tny, tnz}, d_pts, m, d_gs, r, s, reinterpret_cast<double *>(D + o_sc),
	                   reinterpret_cast<sift3d_search_result *>(D), st);
	SCHK(hipGetLastError());
	SCHK(hipMemcpyAsync(S.h_pin, D, res_bytes, hipMemcpyDeviceToHost, st));
	SCHK(hipEventRecord(S.e1, st));
	SCHK(hipEventSynchronize(S.e1));
	float ms = 0;
	SCHK(hipEventElapsedTime(&ms, S.e0, S.e1));
	if (seconds) *seconds = (double)ms * 1e-3;
	memcpy(out, S.h_pin, res_bytes);
	return SIFT3D_OK;
}
#undef SCHK
