// kernels_field.hip -- the displacement field at real-valued positions (sift3d_field_eval, include/sift3d_hip.h, which states the
// numerical contract).  No reference counterpart.  A query's members come from the POI index (kernels_poigrid.hip), built with
// radius + 1: the integer window of that half width around floor(x) covers the real window of half width radius around x (and a
// member that only the rounding of q - x admits), and still touches at most 3 x 3 x 3 cells: 9 contiguous runs (poi_window.h).
//   eval       one wave per query, four queries per workgroup, the grid capped and looped over.  The 9 runs are walked as one
//              sequence, lane l taking entries l, l + 64, ...  Three walks: count, lowest index (u0) and sides; the 22 sums; the
//              residual.  Sums are fp64, reduced by an xor butterfly: a fixed order, the same value in every lane.  Every lane
//              solves the 3 x 3 system (Cholesky: the weighted twin of k_strain_fit's), lane 0 writes the record.
//              No float atomics.
#include "poi_window.h"

#include <math.h>

namespace s3d {
namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxBlocks = 16384;  // larger calls loop
constexpr double kPivotRel = 1e-9;

__device__ inline int wave_min(int x) {
	for (int off = 32; off > 0; off >>= 1) x = min(x, __shfl_xor(x, off));
	return x;
}
__device__ inline int wave_or(int x) {
	for (int off = 32; off > 0; off >>= 1) x |= __shfl_xor(x, off);
	return x;
}
__device__ inline double wave_sum(double x) {
	for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off);
	return x;
}

__device__ inline bool query_ok(double v) { return fabs(v) <= (double)kCoordMax; }  // false for NaN and inf

__device__ inline void write_failed(sift3d_field_result *o, int n, int sides, int status) {
	for (int k = 0; k < 3; k++) o->disp[k] = 0.0;
	for (int k = 0; k < 9; k++) o->G[k] = 0.0;
	o->rms = 0.0;
	o->wsum = 0.0;
	o->neighbours = n;
	o->sides = sides;
	o->status = status;
	o->reserved = 0;
}

// Labelled (sift3d_field_eval_labelled): a member also has the query's label, which is positive, and the lanes share out the entries of
// that label (walk_matching, poi_window.h); the plain instantiations read no label and walk as they always did
template <bool Weighted, bool Labelled>
__global__ __launch_bounds__(kThreads) void k_field_eval(const double *__restrict__ queries, int nq, const double *__restrict__ disp,
                                                        const int *__restrict__ label, const int *__restrict__ qlabel, PoiGrid g,
                                                        const int *__restrict__ start, int ncells, PoiSorted S, int radius, int min_nb,
                                                        int enclosed, sift3d_field_result *__restrict__ out) {
	const int lane = threadIdx.x & 63;
	const double rad = (double)radius;
	for (size_t i = (size_t)blockIdx.x * kWaves + (threadIdx.x >> 6); i < (size_t)nq; i += (size_t)gridDim.x * kWaves) {
		const double x = queries[3 * i], y = queries[3 * i + 1], z = queries[3 * i + 2];
		if (!(query_ok(x) && query_ok(y) && query_ok(z))) {
			if (lane == 0) write_failed(out + i, 0, 0, 2);
			continue;
		}
		int own = 0;
		if constexpr (Labelled) {
			own = qlabel[i];
			if (own <= 0) {
				if (lane == 0) write_failed(out + i, 0, 0, 1);
				continue;
			}
		}
		const PoiWindow<true> W(g, start, ncells, (int)floor(x), (int)floor(y), (int)floor(z), radius + 1);
		const int total = W.total;
		// entry j -> its offsets; the weight, 0 where it is no member or lies on a face of the weighted window
		auto weigh = [&](int j, double d[3]) -> double {
			d[0] = (double)S.x[j] - x;
			d[1] = (double)S.y[j] - y;
			d[2] = (double)S.z[j] - z;
			if (!(fabs(d[0]) <= rad && fabs(d[1]) <= rad && fabs(d[2]) <= rad)) return 0.0;
			if constexpr (Weighted) {
				const double t0 = d[0] / rad, t1 = d[1] / rad, t2 = d[2] / rad;
				const double f0 = 1.0 - t0 * t0, f1 = 1.0 - t1 * t1, f2 = 1.0 - t2 * t2;
				return ((f0 * f0) * (f1 * f1)) * (f2 * f2);
			} else {
				return 1.0;
			}
		};

		// f(j) for the lane's share of the window's entries: every 64th of them, or (labelled) every 64th of those of the query's label
		auto walk = [&](auto f) {
			if constexpr (Labelled)
				walk_matching(W, lane, [&](int j) { return label[S.idx[j]] == own; }, f);
			else
				for (int t = lane; t < total; t += 64) f(W.entry(t));
		};

		// walk 1: the count, the lowest index and the sides among the counted members
		int n = 0, first = 0x7fffffff, sides = 0;
		walk([&](int j) {
			double d[3];
			if (weigh(j, d) > 0.0) {
				n++;
				first = min(first, S.idx[j]);
#pragma unroll
				for (int a = 0; a < 3; a++) sides |= (d[a] <= 0.0 ? 1 << (2 * a) : 0) | (d[a] >= 0.0 ? 2 << (2 * a) : 0);
			}
		});
		n = wave_isum(n);
		first = wave_min(first);
		sides = wave_or(sides);
		if (n < min_nb) {
			if (lane == 0) write_failed(out + i, n, sides, 1);
			continue;
		}
		if (enclosed && sides != 63) {
			if (lane == 0) write_failed(out + i, n, sides, 5);
			continue;
		}
		const double u0[3] = {disp[3 * (size_t)first], disp[3 * (size_t)first + 1], disp[3 * (size_t)first + 2]};

		// walk 2: W = sum w, S1 = sum w d, S2 = sum w d d^T, U = sum w (u - u0), P[c][a] = sum w (u_c - u0_c) d_a
		double sw = 0, s1[3] = {0, 0, 0}, s2[6] = {0, 0, 0, 0, 0, 0}, U[3] = {0, 0, 0}, P[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
		walk([&](int j) {
			double d[3];
			const double w = weigh(j, d);
			if (!(w > 0.0)) return;
			const double wd[3] = {w * d[0], w * d[1], w * d[2]};
			const double wa[3] = {w * (S.u[j] - u0[0]), w * (S.v[j] - u0[1]), w * (S.w[j] - u0[2])};
			sw += w;
#pragma unroll
			for (int c = 0; c < 3; c++) {
				s1[c] += wd[c];
				U[c] += wa[c];
#pragma unroll
				for (int b = 0; b < 3; b++) P[c][b] += wa[c] * d[b];
			}
			s2[0] += wd[0] * d[0]; s2[1] += wd[0] * d[1]; s2[2] += wd[0] * d[2];
			s2[3] += wd[1] * d[1]; s2[4] += wd[1] * d[2]; s2[5] += wd[2] * d[2];
		});
		sw = wave_sum(sw);
#pragma unroll
		for (int c = 0; c < 3; c++) {
			s1[c] = wave_sum(s1[c]);
			U[c] = wave_sum(U[c]);
#pragma unroll
			for (int b = 0; b < 3; b++) P[c][b] = wave_sum(P[c][b]);
		}
#pragma unroll
		for (int k = 0; k < 6; k++) s2[k] = wave_sum(s2[k]);

		// C = S2 - S1 S1^T / W and its Cholesky factor; a pivot at or under 1e-9 of C's largest diagonal entry (or NaN): degenerate window
		const double c00 = s2[0] - s1[0] * s1[0] / sw, c01 = s2[1] - s1[0] * s1[1] / sw, c02 = s2[2] - s1[0] * s1[2] / sw;
		const double c11 = s2[3] - s1[1] * s1[1] / sw, c12 = s2[4] - s1[1] * s1[2] / sw, c22 = s2[5] - s1[2] * s1[2] / sw;
		const double floor_p = kPivotRel * fmax(c00, fmax(c11, c22));
		bool ok = c00 > floor_p;
		const double l00 = sqrt(c00), l10 = c01 / l00, l20 = c02 / l00;
		const double p1 = c11 - l10 * l10;
		ok = ok && p1 > floor_p;
		const double l11 = sqrt(p1), l21 = (c12 - l20 * l10) / l11;
		const double p2 = (c22 - l20 * l20) - l21 * l21;
		ok = ok && p2 > floor_p;
		if (!ok) {
			if (lane == 0) write_failed(out + i, n, sides, 4);
			continue;
		}
		const double l22 = sqrt(p2);
		double G[3][3], dsp[3];
#pragma unroll
		for (int c = 0; c < 3; c++) {
			const double b0 = P[c][0] - s1[0] * U[c] / sw, b1 = P[c][1] - s1[1] * U[c] / sw, b2 = P[c][2] - s1[2] * U[c] / sw;
			const double y0 = b0 / l00, y1 = (b1 - l10 * y0) / l11, y2 = ((b2 - l20 * y0) - l21 * y1) / l22;
			G[c][2] = y2 / l22;
			G[c][1] = (y1 - l21 * G[c][2]) / l11;
			G[c][0] = ((y0 - l10 * G[c][1]) - l20 * G[c][2]) / l00;
			dsp[c] = (u0[c] + U[c] / sw) - ((G[c][0] * s1[0] + G[c][1] * s1[1]) + G[c][2] * s1[2]) / sw;
		}

		// walk 3: the weighted residual of the fitted plane
		double rs = 0;
		walk([&](int j) {
			double d[3];
			const double w = weigh(j, d);
			if (!(w > 0.0)) return;
			const double uj[3] = {S.u[j], S.v[j], S.w[j]};
			double ee = 0;
#pragma unroll
			for (int c = 0; c < 3; c++) {
				const double e = (uj[c] - dsp[c]) - ((G[c][0] * d[0] + G[c][1] * d[1]) + G[c][2] * d[2]);
				ee += e * e;
			}
			rs += w * ee;
		});
		rs = wave_sum(rs);

		if (lane == 0) {
			sift3d_field_result *o = out + i;
#pragma unroll
			for (int c = 0; c < 3; c++) {
				o->disp[c] = dsp[c];
#pragma unroll
				for (int b = 0; b < 3; b++) o->G[3 * c + b] = G[c][b];
			}
			o->rms = sqrt(rs / (3.0 * sw));
			o->wsum = sw;
			o->neighbours = n;
			o->sides = sides;
			o->status = 0;
			o->reserved = 0;
		}
	}
}

template <bool Weighted, bool Labelled>
void launch_one(dim3 grid, const double *d_queries, int nq, const double *d_disp, const int *d_label, const int *d_qlabel, const PoiIndex &ix,
                int radius, int min_nb, int enclosed, sift3d_field_result *d_out, hipStream_t st) {
	hipLaunchKernelGGL((k_field_eval<Weighted, Labelled>), grid, dim3(kThreads), 0, st, d_queries, nq, d_disp, d_label, d_qlabel, ix.g, ix.start,
	                   ix.ncells, ix.S, radius, min_nb, enclosed, d_out);
}
}  // namespace

void launch_field_eval(const double *d_queries, int nq, const double *d_disp, const int *d_label, const int *d_qlabel, const PoiIndex &ix,
                       int radius, int min_nb, int weighting, int enclosed, sift3d_field_result *d_out, hipStream_t st) {
	const size_t want = ((size_t)nq + kWaves - 1) / kWaves;
	const dim3 grid((unsigned)(want < (size_t)kMaxBlocks ? want : (size_t)kMaxBlocks));
	const bool labelled = d_qlabel != nullptr;
	if (weighting && labelled)
		launch_one<true, true>(grid, d_queries, nq, d_disp, d_label, d_qlabel, ix, radius, min_nb, enclosed, d_out, st);
	else if (weighting)
		launch_one<true, false>(grid, d_queries, nq, d_disp, d_label, d_qlabel, ix, radius, min_nb, enclosed, d_out, st);
	else if (labelled)
		launch_one<false, true>(grid, d_queries, nq, d_disp, d_label, d_qlabel, ix, radius, min_nb, enclosed, d_out, st);
	else
		launch_one<false, false>(grid, d_queries, nq, d_disp, d_label, d_qlabel, ix, radius, min_nb, enclosed, d_out, st);
}

}  // namespace s3d
