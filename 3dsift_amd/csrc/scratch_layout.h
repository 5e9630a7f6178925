// scratch_layout.h -- the bump layout of a call's scratch block.  Host only, no HIP include: a stand-alone program can
// use it (tests/test_call_state_cpu.py).
#pragma once
#include <stddef.h>

namespace s3d {

inline size_t al256(size_t b) { return (b + 255) & ~(size_t)255; }

// Pieces at 256-byte aligned offsets, in the order they are taken: take() returns the piece's offset, end is the block's size.  A piece
// of no bytes (an input that is already on the device, an output nobody asked for) takes no room.
struct Layout {
	size_t end = 0;
	size_t take(size_t bytes) {
		const size_t at = end;
		end += al256(bytes);
		return at;
	}
};

// The inputs of a call on a volume pair: ref, tar, m integer points and an optional fourth table of m rows.  Already on the device
// they take no room; from the host they are pieces of the scratch block, in that order, which CallState::stage_pair (call_state.h)
// fills.  b_*: the bytes to upload.
struct PairPlan {
	size_t o_ref = 0, o_tar = 0, o_pts = 0, o_opt = 0, b_ref = 0, b_tar = 0, b_pts = 0, b_opt = 0;
	void plan(Layout &L, bool on_device, size_t nr, size_t nt, int m, size_t opt_row_bytes) {  // opt_row_bytes 0: no fourth table
		b_ref = on_device ? 0 : sizeof(float) * nr;
		b_tar = on_device ? 0 : sizeof(float) * nt;
		b_pts = on_device ? 0 : sizeof(int) * 3 * (size_t)m;
		b_opt = on_device ? 0 : opt_row_bytes * (size_t)m;
		o_ref = L.take(b_ref);
		o_tar = L.take(b_tar);
		o_pts = L.take(b_pts);
		o_opt = L.take(b_opt);
	}
};

}  // namespace s3d
