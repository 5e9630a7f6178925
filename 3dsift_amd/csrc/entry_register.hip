// entry_register.hip -- C-ABI of the RANSAC affine fits (include/sift3d_hip.h: sift3d_fit_affine, sift3d_fit_affine_local).
// No reference counterpart.  Conventions of the matcher (kernels_match.hip): per-device state created on first use -- a non-blocking
// stream, timing events, a grow-only device scratch and a pinned host block for the results --, one call at a time per device, device
// time from HIP events (input uploads excluded, the result copy included), arguments checked before any device call.
#include "sift3d_internal.h"

#include <math.h>
#include <string.h>

#include <mutex>

using namespace s3d;

namespace {
struct RansacState {
	std::mutex mu;
	bool ready = false;
	hipStream_t stream = nullptr;
	hipEvent_t e0 = nullptr, e1 = nullptr, e_in = nullptr;
	char *d_scratch = nullptr; size_t d_bytes = 0;
	char *h_pin = nullptr; size_t h_bytes = 0;
};
constexpr int kMaxDev = 64;
RansacState g_ransac[kMaxDev];

int ensure(RansacState &S, size_t d_bytes, size_t h_bytes) {
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

int pick_device(int device) {
	int ndev = 0;
	if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { set_last_error("no HIP device visible: no CPU fallback"); return SIFT3D_ERR_NO_DEVICE; }
	if (device < 0 || device >= ndev || device >= kMaxDev) { set_last_error("bad device index"); return SIFT3D_ERR_ARG; }
	S3D_HIP(hipSetDevice(device));
	return SIFT3D_OK;
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

#define RCHK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { set_last_error(std::string(#call) + ": " + hipGetErrorString(e_)); (void)hipStreamSynchronize(st); return SIFT3D_ERR_HIP; } } while (0)

extern "C" int sift3d_fit_affine(const float *pairs6, int n, const sift3d_ransac_options *o, int on_device, int device, sift3d_affine_fit *out,
                                 unsigned char *inlier_mask, double *seconds) {
	int H, refine;
	double tau2, min_det;
	uint32_t s;
	if (n < 0 || !out || (n > 0 && !pairs6) || !take_options(o, false, H, tau2, min_det, refine, s)) {
		set_last_error("sift3d_fit_affine: bad argument");
		return SIFT3D_ERR_ARG;
	}
	if (seconds) *seconds = 0;
	int rc = pick_device(device);
	if (rc) return rc;
	if (n < 4) {  // status 1 is a result: nothing to run
		empty_fit(out, 1, n);
		if (inlier_mask && n) memset(inlier_mask, 0, (size_t)n);
		return SIFT3D_OK;
	}
	RansacState &S = g_ransac[device];
	std::lock_guard<std::mutex> lock(S.mu);
	// device scratch: [fit | mask | hyp 12 H | count H | pairs (host inputs)]; pinned host: [fit | mask]
	const size_t o_mask = al256(sizeof(sift3d_affine_fit)), o_hyp = o_mask + al256((size_t)n), o_cnt = o_hyp + al256(sizeof(double) * 12 * H);
	const size_t o_pairs = o_cnt + al256(sizeof(int) * H), d_bytes = o_pairs + (on_device ? 0 : sizeof(float) * 6 * (size_t)n);
	if ((rc = ensure(S, d_bytes, o_hyp))) return rc;
	hipStream_t st = S.stream;
	char *D = S.d_scratch;
	const float *d_pairs = pairs6;
	if (on_device) {
		// device inputs: work the caller queued on the legacy default stream is ordered in front (as in sift3d_match)
		RCHK(hipEventRecord(S.e_in, nullptr));
		RCHK(hipStreamWaitEvent(st, S.e_in, 0));
	} else {
		d_pairs = reinterpret_cast<float *>(D + o_pairs);
		RCHK(hipMemcpyAsync(D + o_pairs, pairs6, sizeof(float) * 6 * (size_t)n, hipMemcpyHostToDevice, st));
	}
	RCHK(hipEventRecord(S.e0, st));
	launch_ransac_global(d_pairs, n, H, s, tau2, min_det, refine, reinterpret_cast<double *>(D + o_hyp), reinterpret_cast<int *>(D + o_cnt),
	                     reinterpret_cast<sift3d_affine_fit *>(D), reinterpret_cast<unsigned char *>(D + o_mask), st);
	RCHK(hipGetLastError());
	RCHK(hipMemcpyAsync(S.h_pin, D, inlier_mask ? o_mask + n : sizeof(sift3d_affine_fit), hipMemcpyDeviceToHost, st));
	RCHK(hipEventRecord(S.e1, st));
	RCHK(hipEventSynchronize(S.e1));
	float ms = 0;
	RCHK(hipEventElapsedTime(&ms, S.e0, S.e1));
	if (seconds) *seconds = (double)ms * 1e-3;
	memcpy(out, S.h_pin, sizeof(sift3d_affine_fit));
	if (inlier_mask) memcpy(inlier_mask, S.h_pin + o_mask, (size_t)n);
	return SIFT3D_OK;
}

extern "C" int sift3d_fit_affine_local(const float *pairs6, int n, const float *points3, int m, int k, float radius, const sift3d_ransac_options *o,
                                       int on_device, int device, sift3d_affine_fit *out, int *neighbours, double *seconds) {
	int H, refine;
	double tau2, min_det;
	uint32_t s;
	if (n < 0 || m < 0 || k < 4 || k > 64 || !std::isfinite(radius) || (n > 0 && !pairs6) || (m > 0 && (!points3 || !out)) ||
	    !take_options(o, true, H, tau2, min_det, refine, s)) {
		set_last_error("sift3d_fit_affine_local: bad argument");
		return SIFT3D_ERR_ARG;
	}
	if (seconds) *seconds = 0;
	int rc = pick_device(device);
	if (rc) return rc;
	if (m == 0) return SIFT3D_OK;
	RansacState &S = g_ransac[device];
	std::lock_guard<std::mutex> lock(S.mu);
	// device scratch: [fits m | neighbours m k | pairs | points (host inputs)]; pinned host: [fits | neighbours]
	const size_t fit_bytes = sizeof(sift3d_affine_fit) * (size_t)m, nb_bytes = neighbours ? sizeof(int) * (size_t)m * k : 0;
	const size_t o_nb = al256(fit_bytes), o_pairs = o_nb + al256(nb_bytes), o_pts = o_pairs + (on_device ? 0 : al256(sizeof(float) * 6 * (size_t)n));
	const size_t d_bytes = o_pts + (on_device ? 0 : sizeof(float) * 3 * (size_t)m);
	if ((rc = ensure(S, d_bytes, o_nb + nb_bytes))) return rc;
	hipStream_t st = S.stream;
	char *D = S.d_scratch;
	const float *d_pairs = pairs6, *d_pts = points3;
	if (on_device) {
		RCHK(hipEventRecord(S.e_in, nullptr));
		RCHK(hipStreamWaitEvent(st, S.e_in, 0));
	} else {
		d_pairs = reinterpret_cast<float *>(D + o_pairs);
		d_pts = reinterpret_cast<float *>(D + o_pts);
		if (n) RCHK(hipMemcpyAsync(D + o_pairs, pairs6, sizeof(float) * 6 * (size_t)n, hipMemcpyHostToDevice, st));
		RCHK(hipMemcpyAsync(D + o_pts, points3, sizeof(float) * 3 * (size_t)m, hipMemcpyHostToDevice, st));
	}
	const float r2 = radius > 0.f ? radius * radius : -1.f;  // (-1: no limit, whatever radius^2 rounds to)
	RCHK(hipEventRecord(S.e0, st));
	launch_ransac_local(d_pairs, n, d_pts, m, k, r2, H, s, tau2, min_det, refine, reinterpret_cast<sift3d_affine_fit *>(D),
	                    neighbours ? reinterpret_cast<int *>(D + o_nb) : nullptr, st);
	RCHK(hipGetLastError());
	RCHK(hipMemcpyAsync(S.h_pin, D, o_nb + nb_bytes, hipMemcpyDeviceToHost, st));
	RCHK(hipEventRecord(S.e1, st));
	RCHK(hipEventSynchronize(S.e1));
	float ms = 0;
	RCHK(hipEventElapsedTime(&ms, S.e0, S.e1));
	if (seconds) *seconds = (double)ms * 1e-3;
	memcpy(out, S.h_pin, fit_bytes);
	if (neighbours) memcpy(neighbours, S.h_pin + o_nb, nb_bytes);
	return SIFT3D_OK;
}
#undef RCHK
