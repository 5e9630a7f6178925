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

}  // namespace s3d
