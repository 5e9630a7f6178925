// poi_window.h -- device code of the POI index (poi_grid.h): the coordinate bound, and the window of a POI as the kernels walk it.
// The side of a cell is at least the window's half width, so a window touches at most 3 x 3 x 3 cells; cells consecutive in x are
// consecutive in memory, so these are 9 contiguous runs of the sorted arrays, walked as one sequence.
#pragma once
#include "poi_grid.h"

namespace s3d {

constexpr int kCoordMax = 1 << 24;  // a POI with a coordinate beyond +-2^24 neither contributes nor gets a window

__device__ inline bool coord_ok(int v) { return v <= kCoordMax && v >= -kCoordMax; }
// floor(a / s), s > 0
__device__ inline int floor_div(int a, int s) { return a >= 0 ? a / s : -((-a + s - 1) / s); }
__device__ inline int wave_isum(int x) {
	for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off);
	return x;
}

// The window of half width radius around (x, y, z), the same in every lane of the wave: rb[k] the first entry of run k, cum[k] the
// entries of the runs before it, total those of all nine.  Pinned: the tables are stated wave-uniform (readfirstlane), which keeps
// them in scalar registers.
template <bool Pinned>
struct PoiWindow {
	int rb[9], cum[10], total;

	__device__ PoiWindow(const PoiGrid &g, const int *__restrict__ start, int ncells, int x, int y, int z, int radius) {
		// the cells the window touches, per axis (none where the window misses the grid)
		const int lox = max(floor_div(x - radius - g.x0, g.side), 0), hix = min(floor_div(x + radius - g.x0, g.side), g.nx - 1);
		const int loy = max(floor_div(y - radius - g.y0, g.side), 0), hiy = min(floor_div(y + radius - g.y0, g.side), g.ny - 1);
		const int loz = max(floor_div(z - radius - g.z0, g.side), 0), hiz = min(floor_div(z + radius - g.z0, g.side), g.nz - 1);
		const int nc = start[ncells];
		cum[0] = 0;
#pragma unroll
		for (int k = 0; k < 9; k++) {
			const int zz = loz + k / 3, yy = loy + k % 3;
			int b = 0, e = 0;
			if (zz <= hiz && yy <= hiy && lox <= hix) {
				const int row = (zz * g.ny + yy) * g.nx;
				b = min(max(start[row + lox], 0), nc);
				e = min(max(start[row + hix + 1], b), nc);
			}
			rb[k] = pin(b);
			cum[k + 1] = pin(cum[k] + (e - b));
		}
		total = cum[9];
	}

	// sequence position t in [0, total) -> its entry of the sorted arrays
	__device__ int entry(int t) const {
		int j = rb[0] + t;
#pragma unroll
		for (int k = 1; k < 9; k++)
			if (t >= cum[k]) j = rb[k] + (t - cum[k]);
		return j;
	}

private:
	__device__ static int pin(int v) {
		if constexpr (Pinned) v = __builtin_amdgcn_readfirstlane(v);
		return v;
	}
};

// the lane that holds the k-th set bit of b (k from 0; k below the number of set bits)
__device__ inline int kth_set_bit(unsigned long long b, int k) {
	int pos = 0;
#pragma unroll
	for (int w = 32; w > 0; w >>= 1) {
		const int c = __popcll((b >> pos) & ((1ull << w) - 1ull));
		if (k >= c) {
			k -= c;
			pos += w;
		}
	}
	return pos;
}

// The walk of the labelled kernels: f(j) for the entries j of the window that match (the centre's label), lane l taking the l-th,
// (l + 64)-th, ... of the MATCHING entries in the window's order -- the share it has in the plain walk (t = lane, lane + 64, ...)
// when every entry matches, and one that the entries of other labels, present or not, do not move: a lane's partial sums, and so the
// bytes of a record, depend on the POIs of its own label only.  Matches are drawn from each 64 entries by ballot and handed to the
// lanes by shuffle; up to 63 wait in `hold` (lane l: the l-th waiting one) for the next batch.  Called by all 64 lanes.
template <bool Pinned, class Match, class F>
__device__ inline void walk_matching(const PoiWindow<Pinned> &W, int lane, Match match, F f) {
	const int total = W.total;
	int hold = 0, nhold = 0;
	for (int t0 = 0; t0 < total; t0 += 64) {
		const int t = t0 + lane;
		int j = 0;
		bool m = false;
		if (t < total) {
			j = W.entry(t);
			m = match(j);
		}
		const unsigned long long b = __ballot(m);
		if (nhold == 0 && b == ~0ull) {  // 64 matches and nobody waits: the batch is what the lanes hold
			f(j);
			continue;
		}
		const int cnt = __popcll(b);
		const int want = lane - nhold;  // the new match that completes a batch in this lane
		const int j1 = __shfl(j, kth_set_bit(b, want > 0 ? want : 0));
		if (nhold + cnt >= 64) {
			const int j2 = __shfl(j, kth_set_bit(b, min(64 - nhold + lane, 63)));  // the matches behind the batch wait
			f(lane < nhold ? hold : j1);
			hold = j2;
			nhold += cnt - 64;
		} else {
			if (want >= 0 && want < cnt) hold = j1;
			nhold += cnt;
		}
	}
	if (lane < nhold) f(hold);
}

}  // namespace s3d
