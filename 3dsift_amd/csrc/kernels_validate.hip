// kernels_validate.hip -- the normalised median test of the POIs' displacements (sift3d_validate_displacements, include/sift3d_hip.h,
// which states the numerical contract).  No reference counterpart.  The neighbours come from the POI index
// (kernels_poigrid.hip), so a window is 9 contiguous runs of the sorted arrays (poi_window.h).
//   fold       per POI: the valid byte and the finiteness of its nine gradients in one byte, which mark then takes as the valid byte.
//   test       one wave per POI (one wave per workgroup: the wave's LDS is its own and a barrier costs nothing).  The runs are walked
//              as in k_strain_fit, lane l taking entries l, l + 64, ...; S.idx[j] skips the POI itself, reads the flag of the pass before
//              and gathers the neighbour's gradient.  Launched once per pass over ping-pong flag bytes and once more for the report.
// Exact medians by radix selection on the order-preserving 64-bit key of a double (-0 folded into +0), 8 bits per round, the digit
// counts of a round in a 256-bin LDS histogram by integer LDS atomics.  The rounds start below the bits that the smallest and the
// largest key share -- a smooth field's values share sign, exponent and leading mantissa bits, and a round in which every key has the
// same digit would serialise all 64 lanes on one bin.  Two sources of keys, one selection:
//   staged     n <= kCap neighbours: a component's estimates are written to LDS once (compacted by ballot) and the rounds read them
//              there; the absolute deviations replace them in place for the MAD.
//   walked     n > kCap: every round walks the runs again and forms the estimate anew; nothing is stored, so n has no bound.
// For even n the upper middle value is the lower one if enough keys are <= it, else the smallest key above it: one more read.
#include "poi_window.h"

#include <math.h>

namespace s3d {
namespace {

typedef unsigned long long u64;

constexpr int kFoldThreads = 256;
constexpr int kCap = 1024;  // staged keys of a wave: 8 KB of LDS beside the 1 KB histogram

__device__ inline u64 wave_min64(u64 x) {
	for (int off = 32; off > 0; off >>= 1) {
		const u64 y = __shfl_xor(x, off);
		x = y < x ? y : x;
	}
	return x;
}
__device__ inline u64 wave_max64(u64 x) {
	for (int off = 32; off > 0; off >>= 1) {
		const u64 y = __shfl_xor(x, off);
		x = y > x ? y : x;
	}
	return x;
}
// a value every lane holds alike, as the compiler may know it
__device__ inline int uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ inline u64 uniform64(u64 v) {
	return ((u64)(unsigned)__builtin_amdgcn_readfirstlane((int)(v >> 32)) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((int)v);
}

// finite doubles -> keys in the same order; -0 and +0 share a key
__device__ inline u64 key_of(double v) {
	if (v == 0.0) v = 0.0;
	const u64 b = (u64)__double_as_longlong(v);
	return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ inline double value_of(u64 k) {
	const u64 b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
	return __longlong_as_double((long long)b);
}

__global__ __launch_bounds__(kFoldThreads) void k_validate_fold(const double *__restrict__ grad, const unsigned char *__restrict__ valid, int m,
                                                               unsigned char *__restrict__ fold) {
	const int i = blockIdx.x * kFoldThreads + threadIdx.x;
	if (i >= m) return;
	bool on = !valid || valid[i];
	if (grad)
		for (int k = 0; k < 9; k++) on = on && isfinite(grad[9 * (size_t)i + k]);
	fold[i] = on ? 1 : 0;
}

// The key of rank k (0-based, ascending) among the n >= 1 keys that each(f) hands to f, every lane its share; lo and hi are the
// smallest and the largest of them.  hist: 256 ints of the wave's LDS.  Every lane returns the same key.
template <class Each>
__device__ inline u64 radix_select(Each each, int k, u64 lo, u64 hi, int *hist, int lane) {
	if (lo == hi) return lo;
	int shift = uniform((63 - __clzll((long long)(lo ^ hi))) & ~7);
	u64 mask = shift >= 56 ? 0ull : ~0ull << (shift + 8);
	u64 prefix = lo & mask;
	int4 *hist4 = reinterpret_cast<int4 *>(hist);
	for (; shift >= 0; shift -= 8) {
		hist4[lane] = make_int4(0, 0, 0, 0);
		__syncthreads();
		each([&](u64 key) {
			if ((key & mask) == prefix) atomicAdd(&hist[(int)(key >> shift) & 255], 1);
		});
		__syncthreads();
		const int4 h = hist4[lane];  // the lane's four bins; no other lane reads or clears them
		const int s = (h.x + h.y) + (h.z + h.w);
		int incl = s;
		for (int off = 1; off < 64; off <<= 1) {
			const int v = __shfl_up(incl, off);
			if (lane >= off) incl += v;
		}
		const int excl = incl - s;
		const bool here = excl <= k && k < incl;  // true in exactly one lane
		int digit = 0, nk = 0;
		if (here) {
			int r = k - excl;
			digit = 4 * lane;
			if (r >= h.x) {
				r -= h.x;
				digit++;
				if (r >= h.y) {
					r -= h.y;
					digit++;
					if (r >= h.z) {
						r -= h.z;
						digit++;
					}
				}
			}
			nk = r;
		}
		const int src = __ffsll((long long)__ballot(here)) - 1;
		digit = uniform(__shfl(digit, src));
		k = uniform(__shfl(nk, src));
		prefix |= (u64)digit << shift;
		mask |= 0xffull << shift;
	}
	return prefix;
}

// the median of the n >= 1 values whose keys each(f) hands out: the middle one, or 0.5 * (lo + hi) of the two middle ones
template <class Each>
__device__ inline double median_of(Each each, int n, int *hist, int lane) {
	u64 lo = ~0ull, hi = 0ull;
	each([&](u64 key) {
		lo = key < lo ? key : lo;
		hi = key > hi ? key : hi;
	});
	lo = uniform64(wave_min64(lo));
	hi = uniform64(wave_max64(hi));
	const u64 a = radix_select(each, (n - 1) / 2, lo, hi, hist, lane);
	if (n & 1) return value_of(a);
	int le = 0;
	u64 above = ~0ull;
	each([&](u64 key) {
		if (key <= a)
			le++;
		else
			above = key < above ? key : above;
	});
	le = wave_isum(le);
	above = wave_min64(above);
	const u64 b = le > n / 2 ? a : above;
	return 0.5 * (value_of(a) + value_of(b));
}

__device__ inline void write_record(sift3d_validate_result *o, const double *med, const double *mad, double score, int n, int status,
                                    int flagged, int pass) {
	for (int c = 0; c < 3; c++) {
		o->median[c] = med ? med[c] : 0.0;
		o->mad[c] = mad ? mad[c] : 0.0;
	}
	o->score = score;
	o->neighbours = n;
	o->status = status;
	o->flagged = flagged;
	o->pass = pass;
}

// Labelled (the labelled test): a neighbour also has the POI's own label, which is positive; the plain instantiation reads no label
template <bool Labelled>
__global__ __launch_bounds__(64) void k_validate_test(const int *__restrict__ pts, const double *__restrict__ disp, const double *__restrict__ grad,
                                                      const int *__restrict__ label, const int *__restrict__ cell, int m, PoiGrid g,
                                                      const int *__restrict__ start, int ncells, PoiSorted S, ValidateParams P, int pass,
                                                      const unsigned char *__restrict__ fin,
                                                      unsigned char *__restrict__ fout, int *__restrict__ pass_of,
                                                      sift3d_validate_result *__restrict__ out) {
	__shared__ u64 keys[kCap];
	__shared__ int4 hist4[64];
	int *hist = reinterpret_cast<int *>(hist4);
	const int lane = threadIdx.x;
	const int i = blockIdx.x;
	if (i >= m) return;
	const int x = pts[3 * (size_t)i], y = pts[3 * (size_t)i + 1], z = pts[3 * (size_t)i + 2];
	const bool in_range = coord_ok(x) && coord_ok(y) && coord_ok(z);
	const bool contributes = in_range && cell[i] >= 0;
	const int prev = fin[i];
	if (pass > 0) {
		if (!contributes || prev) {  // not tested in this pass: the flag is carried over
			if (lane == 0) fout[i] = (unsigned char)prev;
			return;
		}
	} else if (!in_range) {
		if (lane == 0) write_record(out + i, nullptr, nullptr, 0.0, 0, 2, 0, 0);
		return;
	}
	const int radius = P.radius;
	const PoiWindow<true> W(g, start, ncells, x, y, z, radius);
	const int total = W.total;
	int own = 0;
	if constexpr (Labelled) own = label[i];
	// a neighbour of this launch: inside the window, not the POI itself, not flagged by the pass before (and of the POI's body)
	auto keep = [&](int j) {
		if (!(abs(S.x[j] - x) <= radius && abs(S.y[j] - y) <= radius && abs(S.z[j] - z) <= radius)) return false;
		const int id = S.idx[j];
		if constexpr (Labelled)
			if (own <= 0 || label[id] != own) return false;
		return id != i && !fin[id];
	};
	// neighbour j's estimate of component c at the POI
	auto estimate = [&](int j, int c) {
		double u = (c == 0 ? S.u : c == 1 ? S.v : S.w)[j];
		if (grad) {
			const double *G = grad + 9 * (size_t)S.idx[j] + 3 * c;
			const double dx = (double)(x - S.x[j]), dy = (double)(y - S.y[j]), dz = (double)(z - S.z[j]);
			u = u + ((G[0] * dx + G[1] * dy) + G[2] * dz);
		}
		return u;
	};

	int n = 0;
	for (int t = lane; t < total; t += 64) n += keep(W.entry(t)) ? 1 : 0;
	n = uniform(wave_isum(n));
	if (n < P.min_nb) {
		if (lane == 0) {
			if (pass > 0)
				fout[i] = 0;
			else
				write_record(out + i, nullptr, nullptr, 0.0, n, 1, prev, pass_of[i]);
		}
		return;
	}

	double med[3], mad[3];
#pragma unroll 1
	for (int c = 0; c < 3; c++) {
		if (n <= kCap) {
			int base = 0;
			for (int t0 = 0; t0 < total; t0 += 64) {
				const int t = t0 + lane;
				bool k = false;
				u64 key = 0;
				if (t < total) {
					const int j = W.entry(t);
					if (keep(j)) {
						k = true;
						key = key_of(estimate(j, c));
					}
				}
				const u64 b = __ballot(k);
				if (k) keys[base + __popcll(b & ((1ull << lane) - 1ull))] = key;
				base += __popcll(b);
			}
			__syncthreads();
			auto staged = [&](auto f) {
				for (int t = lane; t < n; t += 64) f(keys[t]);
			};
			const double mc = median_of(staged, n, hist, lane);
			__syncthreads();
			for (int t = lane; t < n; t += 64) keys[t] = key_of(fabs(value_of(keys[t]) - mc));
			__syncthreads();
			med[c] = mc;
			mad[c] = median_of(staged, n, hist, lane);
			__syncthreads();  // the next component's staging overwrites the keys
		} else {
			auto walked = [&](auto f) {
				for (int t = lane; t < total; t += 64) {
					const int j = W.entry(t);
					if (keep(j)) f(key_of(estimate(j, c)));
				}
			};
			const double mc = median_of(walked, n, hist, lane);
			auto deviations = [&](auto f) {
				for (int t = lane; t < total; t += 64) {
					const int j = W.entry(t);
					if (keep(j)) f(key_of(fabs(estimate(j, c) - mc)));
				}
			};
			med[c] = mc;
			mad[c] = median_of(deviations, n, hist, lane);
		}
	}

	double score = 0.0;
	if (contributes) {
#pragma unroll
		for (int c = 0; c < 3; c++) {
			const double s = fabs(disp[3 * (size_t)i + c] - med[c]) / (mad[c] + P.eps);
			if (c == 0 || s > score) score = s;
		}
	}
	if (lane != 0) return;
	if (pass > 0) {
		const bool flag = score > P.threshold;
		fout[i] = flag ? 1 : 0;
		if (flag) pass_of[i] = pass;
	} else {
		write_record(out + i, med, mad, score, n, contributes ? 0 : 3, prev, pass_of[i]);
	}
}

int blocks_for(size_t n, int per) { return (int)((n + per - 1) / per); }
}  // namespace

int validate_stage_capacity() { return kCap; }

void launch_validate_fold(const double *d_grad, const unsigned char *d_valid, int m, unsigned char *d_fold, hipStream_t st) {
	hipLaunchKernelGGL(k_validate_fold, dim3(blocks_for(m, kFoldThreads)), dim3(kFoldThreads), 0, st, d_grad, d_valid, m, d_fold);
}

void launch_validate_test(const int *d_pts, const double *d_disp, const double *d_grad, const int *d_label, int m, const PoiIndex &ix,
                          ValidateParams P, int pass, const unsigned char *d_fin, unsigned char *d_fout, int *d_pass,
                          sift3d_validate_result *d_out, hipStream_t st) {
	if (d_label)
		hipLaunchKernelGGL(k_validate_test<true>, dim3(m), dim3(64), 0, st, d_pts, d_disp, d_grad, d_label, ix.cell, m, ix.g, ix.start, ix.ncells,
		                   ix.S, P, pass, d_fin, d_fout, d_pass, d_out);
	else
		hipLaunchKernelGGL(k_validate_test<false>, dim3(m), dim3(64), 0, st, d_pts, d_disp, d_grad, d_label, ix.cell, m, ix.g, ix.start, ix.ncells,
		                   ix.S, P, pass, d_fin, d_fout, d_pass, d_out);
}

}  // namespace s3d
