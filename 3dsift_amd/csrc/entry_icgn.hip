// entry_icgn.hip -- C-ABI of the IC-GN displacement refinement (include/sift3d_hip.h: sift3d_icgn, sift3d_icgn_init_from_fits,
// sift3d_default_icgn_options).  No reference counterpart.  Conventions of entry_register.hip: per-device state created on first use
// -- a non-blocking stream, timing events, a grow-only device scratch and a pinned host block for the results --, one call at a time
// per device, device time from HIP events (input uploads excluded, the result copy included), arguments checked before any device call.
#include "sift3d_internal.h"

#include <math.h>
#include <string.h>

#include <mutex>

using namespace s3d;

namespace {
struct IcgnDevState {
	std::mutex mu;
	bool ready = false;
	hipStream_t stream = nullptr;
	hipEvent_t e0 = nullptr, e1 = nullptr, e_in = nullptr;
	char *d_scratch = nullptr; size_t d_bytes = 0;
	char *h_pin = nullptr; size_t h_bytes = 0;
};
constexpr int kMaxDev = 64;
IcgnDevState g_icgn[kMaxDev];

int ensure(IcgnDevState &S, size_t d_bytes, size_t h_bytes) {
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
bool take_options(const sift3d_icgn_options *o, int &r, int &max_it, double &tol, int &cubic) {
	sift3d_icgn_options d;
	sift3d_default_icgn_options(&d);
	if (!o) o = &d;
	if (o->subset_radius < 2 || o->subset_radius > 32 || o->max_iterations < 1 || o->max_iterations > 100) return false;
	if (!std::isfinite(o->tolerance) || o->tolerance < 0.f || (o->interpolation != 0 && o->interpolation != 1)) return false;
	if (o->reserved[0] || o->reserved[1] || o->reserved[2] || o->reserved[3]) return false;
	r = o->subset_radius;
	max_it = o->max_iterations;
	tol = o->tolerance;
	cubic = o->interpolation == 0;
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

extern "C" void sift3d_default_icgn_options(sift3d_icgn_options *o) {
	if (!o) return;
	memset(o, 0, sizeof(*o));
	o->subset_radius = 16;
	o->max_iterations = 20;
	o->tolerance = 1e-3f;
	o->interpolation = 0;
}

extern "C" int sift3d_icgn_init_from_fits(const sift3d_affine_fit *fits, const int *points3, int m, double *init12) {
	if (m < 0 || (m > 0 && (!fits || !points3 || !init12))) {
		set_last_error("sift3d_icgn_init_from_fits: bad argument");
		return SIFT3D_ERR_ARG;
	}
	for (int i = 0; i < m; i++) {
		double *p = init12 + 12 * (size_t)i;
		const double *A = fits[i].A;
		const double q[3] = {(double)points3[3 * i], (double)points3[3 * i + 1], (double)points3[3 * i + 2]};
		for (int a = 0; a < 3; a++) {
			// (u, v, w) = L q + b - q, F = L: ux = L00 - 1, uy = L01, ...
			p[4 * a] = fits[i].status != 0 ? NAN : (((A[4 * a] * q[0] + A[4 * a + 1] * q[1]) + A[4 * a + 2] * q[2]) + A[4 * a + 3]) - q[a];
			for (int c = 0; c < 3; c++) p[4 * a + 1 + c] = fits[i].status != 0 ? NAN : A[4 * a + c] - (a == c ? 1.0 : 0.0);
		}
	}
	return SIFT3D_OK;
}

#define ICHK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { set_last_error(std::string(#call) + ": " + hipGetErrorString(e_)); (void)hipStreamSynchronize(st); return SIFT3D_ERR_HIP; } } while (0)

extern "C" int sift3d_icgn(const float *ref, int rnx, int rny, int rnz, const float *tar, int tnx, int tny, int tnz, const int *points3, int m,
                           const double *init12, const sift3d_icgn_options *o, int on_device, int device, sift3d_icgn_result *out,
                           double *seconds) {
	int r, max_it, cubic;
	double tol;
	if (m < 0 || rnx < 1 || rny < 1 || rnz < 1 || tnx < 1 || tny < 1 || tnz < 1 || !ref || !tar || !out || (m > 0 && !points3) ||
	    !take_options(o, r, max_it, tol, cubic)) {
		set_last_error("sift3d_icgn: bad argument");
		return SIFT3D_ERR_ARG;
	}
	if (seconds) *seconds = 0;
	int rc = pick_device(device);
	if (rc) return rc;
	if (m == 0) return SIFT3D_OK;
	IcgnDevState &S = g_icgn[device];
	std::lock_guard<std::mutex> lock(S.mu);
	// device scratch: [results m | state m | (host inputs) ref | tar | points | init]; pinned host: [results]
	const size_t nr = (size_t)rnx * rny * rnz, nt = (size_t)tnx * tny * tnz, res_bytes = sizeof(sift3d_icgn_result) * (size_t)m;
	const size_t o_state = al256(res_bytes), o_ref = o_state + al256(icgn_state_bytes() * (size_t)m);
	const size_t o_tar = o_ref + (on_device ? 0 : al256(sizeof(float) * nr)), o_pts = o_tar + (on_device ? 0 : al256(sizeof(float) * nt));
	const size_t o_init = o_pts + (on_device ? 0 : al256(sizeof(int) * 3 * (size_t)m));
	const size_t d_bytes = o_init + (on_device || !init12 ? 0 : sizeof(double) * 12 * (size_t)m);
	if ((rc = ensure(S, d_bytes, res_bytes))) return rc;
	hipStream_t st = S.stream;
	char *D = S.d_scratch;
	const float *d_ref = ref, *d_tar = tar;
	const int *d_pts = points3;
	const double *d_init = init12;
	if (on_device) {
		// device inputs: work the caller queued on the legacy default stream is ordered in front (as in sift3d_match)
		ICHK(hipEventRecord(S.e_in, nullptr));
		ICHK(hipStreamWaitEvent(st, S.e_in, 0));
	} else {
		d_ref = reinterpret_cast<float *>(D + o_ref);
		d_tar = reinterpret_cast<float *>(D + o_tar);
		d_pts = reinterpret_cast<int *>(D + o_pts);
		ICHK(hipMemcpyAsync(D + o_ref, ref, sizeof(float) * nr, hipMemcpyHostToDevice, st));
		ICHK(hipMemcpyAsync(D + o_tar, tar, sizeof(float) * nt, hipMemcpyHostToDevice, st));
		ICHK(hipMemcpyAsync(D + o_pts, points3, sizeof(int) * 3 * (size_t)m, hipMemcpyHostToDevice, st));
		if (init12) {
			d_init = reinterpret_cast<double *>(D + o_init);
			ICHK(hipMemcpyAsync(D + o_init, init12, sizeof(double) * 12 * (size_t)m, hipMemcpyHostToDevice, st));
		}
	}
	ICHK(hipEventRecord(S.e0, st));
	launch_icgn(IcgnVol{d_ref, rnx, rny, rnz}, IcgnVol{d_tar, tnx, tny, tnz}, d_pts, m, d_init, r, max_it, tol, cubic, D + o_state,
	            reinterpret_cast<sift3d_icgn_result *>(D), st);
	ICHK(hipGetLastError());
	ICHK(hipMemcpyAsync(S.h_pin, D, res_bytes, hipMemcpyDeviceToHost, st));
	ICHK(hipEventRecord(S.e1, st));
	ICHK(hipEventSynchronize(S.e1));
	float ms = 0;
	ICHK(hipEventElapsedTime(&ms, S.e0, S.e1));
	if (seconds) *seconds = (double)ms * 1e-3;
	memcpy(out, S.h_pin, res_bytes);
	return SIFT3D_OK;
}
#undef ICHK
