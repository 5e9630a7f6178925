// call_state.h -- what the one-shot entry points share (sift3d_match, sift3d_match_guided, sift3d_fit_affine[_local], sift3d_icgn[_bspline],
// sift3d_icgn2, sift3d_icgn_masked, sift3d_icgn_labelled, sift3d_fit_rigid[_local], sift3d_fit_rigid_bodies, sift3d_mask_from_level, sift3d_zncc_search, sift3d_strain, sift3d_validate_displacements, sift3d_field_eval, sift3d_bspline_prefilter, sift3d_subset_quality): the per-device call state, its grow-only blocks, the
// scratch layout, the staging of a volume pair, the device pick and the stream-aware check macro.  Every family keeps an array of
// states of its own (its own stream and mutex per device).
#pragma once
#include <mutex>

#include "scratch_layout.h"
#include "sift3d_internal.h"

namespace s3d {

constexpr int kMaxDev = 64;  // devices with a state (and a staging pool) of their own

// Grow-only allocations, reused by every later call.  After a failed allocation p is null and bytes is zero.
struct DevBlock {
	char *p = nullptr;
	size_t bytes = 0;
	int reserve(size_t want, hipStream_t st);  // st is synchronised before a block it may still use is freed
};
struct PinBlock {
	char *p = nullptr;
	size_t bytes = 0;
	int reserve(size_t want);
};

// Per-device state of one family, created on first use and never destroyed: a non-blocking stream, the timing events, the device scratch
// and the pinned host block for the results.  One call at a time per device: the caller holds mu from ensure() to the end of the call.
struct CallState {
	std::mutex mu;
	bool ready = false;
	hipStream_t stream = nullptr;
	hipEvent_t e0 = nullptr, e1 = nullptr, e_in = nullptr;
	DevBlock d;
	PinBlock h;
	int ensure(size_t d_bytes, size_t h_bytes);  // stream and events on first use; d and h hold at least that much
	int after_legacy_stream();                   // device inputs: the call runs behind the legacy default stream
	// a volume pair's inputs (scratch_layout.h, PairPlan) -> where the kernels read them: device inputs stay where they are and the call
	// runs behind the legacy default stream; host inputs are uploaded to their pieces of d, in the plan's order (opt may be null)
	int stage_pair(const PairPlan &P, bool on_device, const float *&ref, const float *&tar, const int *&pts, const void *&opt);
	int finish(double *seconds);                 // waits for e1; *seconds (may be NULL) = e0 -> e1
};

int pick_device(int device);  // checks the index, makes the device current

// an input table p of a call -> where the kernels read it.  Its piece of the scratch block at base + off: bytes > 0, the host table
// is uploaded there and p moves to it; no bytes (a device input, an optional table that is absent), p stays as it is
template <class T>
hipError_t upload(const T *&p, char *base, size_t off, size_t bytes, hipStream_t st) {
	if (!bytes) return hipSuccess;
	const T *host = p;
	p = reinterpret_cast<const T *>(base + off);
	return hipMemcpyAsync(base + off, host, bytes, hipMemcpyHostToDevice, st);
}

// a HIP call of an entry that has work on stream st: the stream is drained before the error is returned
#define S3D_HIP_ST(st, call)                                                                            \
	do {                                                                                                \
		hipError_t e_ = (call);                                                                         \
		if (e_ != hipSuccess) {                                                                         \
			s3d::set_last_error(std::string(#call) + ": " + hipGetErrorString(e_));                     \
			(void)hipStreamSynchronize(st);                                                             \
			return SIFT3D_ERR_HIP;                                                                      \
		}                                                                                               \
	} while (0)

}  // namespace s3d
