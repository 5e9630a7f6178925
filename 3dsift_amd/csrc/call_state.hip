// call_state.hip -- the shared part of the one-shot entry points (call_state.h).  Host only, no kernels.
#include "call_state.h"

namespace s3d {

static size_t grow(size_t want) { return want + want / 4 + 4096; }  // head room: calls of similar size do not reallocate

int DevBlock::reserve(size_t want, hipStream_t st) {
	if (want <= bytes) return SIFT3D_OK;
	S3D_HIP(hipStreamSynchronize(st));
	if (p) (void)hipFree(p);
	p = nullptr; bytes = 0;
	S3D_HIP(hipMalloc(&p, grow(want)));
	bytes = grow(want);
	return SIFT3D_OK;
}

int PinBlock::reserve(size_t want) {
	if (want <= bytes) return SIFT3D_OK;
	if (p) (void)hipHostFree(p);
	p = nullptr; bytes = 0;
	S3D_HIP(hipHostMalloc(&p, grow(want), hipHostMallocDefault));
	bytes = grow(want);
	return SIFT3D_OK;
}

int CallState::ensure(size_t d_bytes, size_t h_bytes) {
	if (!ready) {  // (a failed creation leaves the objects made so far in place: the next call goes on from there)
		if (!stream) S3D_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
		if (!e0) S3D_HIP(hipEventCreate(&e0));
		if (!e1) S3D_HIP(hipEventCreate(&e1));
		if (!e_in) S3D_HIP(hipEventCreateWithFlags(&e_in, hipEventDisableTiming));
		ready = true;
	}
	int rc = d.reserve(d_bytes, stream);
	return rc ? rc : h.reserve(h_bytes);
}

// Device-resident inputs: work the caller queued on the legacy default stream (torch's default stream is that one) is ordered in front of
// the call; inputs produced on other streams must be complete when the call is made (sift3d_run's are).
int CallState::after_legacy_stream() {
	S3D_HIP_ST(stream, hipEventRecord(e_in, nullptr));
	S3D_HIP_ST(stream, hipStreamWaitEvent(stream, e_in, 0));
	return SIFT3D_OK;
}

int CallState::stage_pair(const PairPlan &P, bool on_device, const float *&ref, const float *&tar, const int *&pts, const void *&opt) {
	if (on_device) return after_legacy_stream();
	S3D_HIP_ST(stream, hipMemcpyAsync(d.p + P.o_ref, ref, P.b_ref, hipMemcpyHostToDevice, stream));
	S3D_HIP_ST(stream, hipMemcpyAsync(d.p + P.o_tar, tar, P.b_tar, hipMemcpyHostToDevice, stream));
	S3D_HIP_ST(stream, hipMemcpyAsync(d.p + P.o_pts, pts, P.b_pts, hipMemcpyHostToDevice, stream));
	if (opt) S3D_HIP_ST(stream, hipMemcpyAsync(d.p + P.o_opt, opt, P.b_opt, hipMemcpyHostToDevice, stream));
	ref = reinterpret_cast<const float *>(d.p + P.o_ref);
	tar = reinterpret_cast<const float *>(d.p + P.o_tar);
	pts = reinterpret_cast<const int *>(d.p + P.o_pts);
	if (opt) opt = d.p + P.o_opt;
	return SIFT3D_OK;
}

int CallState::finish(double *seconds) {
	S3D_HIP_ST(stream, hipEventSynchronize(e1));
	float ms = 0;
	S3D_HIP_ST(stream, hipEventElapsedTime(&ms, e0, e1));
	if (seconds) *seconds = (double)ms * 1e-3;
	return SIFT3D_OK;
}

int pick_device(int device) {
	int ndev = 0;
	if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { set_last_error("no HIP device visible: no CPU fallback"); return SIFT3D_ERR_NO_DEVICE; }
	if (device < 0 || device >= ndev || device >= kMaxDev) { set_last_error("bad device index"); return SIFT3D_ERR_ARG; }
	S3D_HIP(hipSetDevice(device));
	return SIFT3D_OK;
}

}  // namespace s3d
