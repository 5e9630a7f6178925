// poi_grid.h -- the spatial index over a call's POIs: a uniform cell grid over the bounding box of the contributing POIs
// and the POIs sorted by cell, which sift3d_strain, sift3d_validate_displacements, sift3d_field_eval (around real-valued centres) and
// sift3d_match_guided (its POIs are keypoint positions) walk window by window (poi_window.h).  Built by
// poi_grid_build (kernels_poigrid.hip).  Host-compilable: a stand-alone program can use the grid rule (tests/test_strain_cases_cpu.py).
#pragma once
#include "scratch_layout.h"
#include "sift3d_internal.h"

namespace s3d {

// the cell grid over the bounding box of the contributing POIs: cell (cx, cy, cz) = (q - origin) / side per axis, cx fastest
struct PoiGrid {
	int x0, y0, z0, side, nx, ny, nz;
};
// the contributing POIs in cell order, a cell's POIs in ascending index
struct PoiSorted {
	int *x, *y, *z, *idx;
	double *u, *v, *w;
};

constexpr int kPoiBoxEmpty = 0x7f7f7f7f;  // the preset of the box, every byte alike: above any coordinate that contributes
constexpr int kPoiScanTile = 4096;  // cells of a tile of the exclusive scan over the cell counts
inline size_t poi_scan_tiles(size_t n) { return (n + kPoiScanTile - 1) / kPoiScanTile; }  // entries of the tile scratch for n scanned values

// the grid over the box the mark kernel left (min x, y, z, min -x, -y, -z; kPoiBoxEmpty where no POI contributes): the side is the
// radius, enlarged until the grid has at most 2^24 cells.  The extents reach 2^25 + 1, so the products are formed in 64 bits and
// stepwise.
inline PoiGrid poi_choose_grid(const int *box, int radius) {
	constexpr long long kMaxCells = 1 << 24;
	PoiGrid g = {0, 0, 0, radius, 1, 1, 1};
	if (box[0] == kPoiBoxEmpty) return g;
	g.x0 = box[0]; g.y0 = box[1]; g.z0 = box[2];
	const long long ex = (long long)-box[3] - box[0], ey = (long long)-box[4] - box[1], ez = (long long)-box[5] - box[2];
	long long side = radius;
	for (;;) {
		const long long nx = ex / side + 1, ny = ey / side + 1, nz = ez / side + 1;
		if (nx * ny <= kMaxCells && nx * ny * nz <= kMaxCells) {
			g.side = (int)side; g.nx = (int)nx; g.ny = (int)ny; g.nz = (int)nz;
			return g;
		}
		side += (side + 3) / 4;
	}
}

// the index's pieces of a call's block a, between the entry's results and its own pieces:
// [box | cell of a POI | slots | sorted x y z idx | sorted u v w]
struct PoiGridPlan {
	size_t o_box = 0, o_cell = 0, o_slots = 0, o_si = 0, o_sd = 0, wi = 0, wd = 0;  // wi, wd: the stride of a sorted int / double array
	void take(Layout &L, int m) {
		wi = al256(sizeof(int) * (size_t)m);
		wd = al256(sizeof(double) * (size_t)m);
		o_box = L.take(sizeof(int) * 6);
		o_cell = L.take(wi);
		o_slots = L.take(wi);
		o_si = L.take(4 * wi);
		o_sd = L.take(3 * wd);
	}
};

// what a kernel that walks windows reads: cell[i] is POI i's cell (negative: it does not contribute), start[c] .. start[c + 1] are the
// entries of cell c in the sorted arrays, start[ncells] their number
struct PoiIndex {
	PoiGrid g;
	int ncells;
	const int *cell, *start;
	PoiSorted S;
};

// the temporaries of one call whose sizes depend on the input (sift3d_strain, sift3d_validate_displacements): freed when the call
// returns, however it returns
struct CallTemps {
	char *a = nullptr, *b = nullptr;
	~CallTemps() {
		if (a) (void)hipFree(a);
		if (b) (void)hipFree(b);
	}
};

// Builds the index of m POIs on stream st: presets the box, marks the contributors (d_valid null: every POI may), reads the box back
// (the stream is synchronised), chooses the grid for the radius, allocates block b into T.b, bins and fills ix.  A: the call's block a, which holds the plan's pieces.  Returns a
// SIFT3D_ code; a failure after work was queued drains the stream.
int poi_grid_build(const PoiGridPlan &P, char *A, const int *d_pts, const double *d_disp, const unsigned char *d_valid, int m, int radius,
                   CallTemps &T, hipStream_t st, PoiIndex &ix);

}  // namespace s3d
