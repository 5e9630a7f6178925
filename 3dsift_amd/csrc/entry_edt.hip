// entry_edt.hip -- C-ABI of the distance transform and of the labels of touching bodies (include/sift3d_hip.h: sift3d_mask_distance,
// sift3d_mask_from_distance, sift3d_distance_at_points, sift3d_default_split_options, sift3d_mask_split).  No reference counterpart.
// Kernels: kernels_edt.hip, and kernels_label.hip for the components of the cores and of what they do not reach.  One-shot entries:
// call state, timing and the order of the checks as DESIGN 4.10 (call_state.h).
#include "call_state.h"

using namespace s3d;

namespace {
CallState g_dist[kMaxDev], g_erode[kMaxDev], g_dist_at[kMaxDev], g_split[kMaxDev];

constexpr int kRoundBatch = 8;  // growth rounds per read-back of their counters (even: a batch ends in the buffer it began in)

// extents >= 1 whose product fits an int (formed stepwise: three extents of 2^31 - 1 do not fit 64 bits)
bool dims_fit_int(int nx, int ny, int nz) {
	return nx >= 1 && ny >= 1 && nz >= 1 && (size_t)nx * ny <= (((size_t)1 << 31) - 1) / (size_t)nz;
}
// ... and whose largest squared distance, border included, fits an int
bool dims_fit_distance(int nx, int ny, int nz) {
	if (!dims_fit_int(nx, ny, nz) || nx > 46340 || ny > 46340 || nz > 46340) return false;
	const long long a = nx + 1, b = ny + 1, c = nz + 1;
	return a * a + b * b + c * c < (1ll << 31);
}
bool split_options_ok(const sift3d_split_options *o) {
	return o && (o->connectivity == 6 || o->connectivity == 26) && o->core_dist2 >= 1 && o->min_core_voxels >= 1 && o->border >= 0 && o->border <= 1 &&
	       o->max_rounds >= 0 && o->keep_unreached >= 0 && o->keep_unreached <= 1 && o->min_voxels >= 1;
}
}  // namespace

extern "C" void sift3d_default_split_options(sift3d_split_options *o) {
	if (!o) return;
	o->connectivity = 6;
	o->core_dist2 = 16;
	o->min_core_voxels = 1;
	o->border = 1;
	o->max_rounds = 0;
	o->keep_unreached = 1;
	o->min_voxels = 1;
}

extern "C" int sift3d_mask_distance(const unsigned char *mask, int nx, int ny, int nz, int border, int *dist2, int on_device, int device,
                                    double *seconds) {
	if (!mask || !dist2 || !dims_fit_distance(nx, ny, nz) || border < 0 || border > 1) {
		set_last_error("sift3d_mask_distance: bad argument");
		return SIFT3D_ERR_ARG;
	}
	if (seconds) *seconds = 0;
	int rc = pick_device(device);
	if (rc) return rc;
	CallState &S = g_dist[device];
	std::lock_guard<std::mutex> lock(S.mu);
	const size_t n = (size_t)nx * ny * nz;
	// device scratch: [the field between the y and the z pass | (host memory) mask | dist2]
	Layout L;
	const size_t o_tmp = L.take(sizeof(int) * n), o_mask = L.take(on_device ? 0 : n), o_dist = L.take(on_device ? 0 : sizeof(int) * n);
	if ((rc = S.ensure(L.end, 0))) return rc;
	hipStream_t st = S.stream;
	const unsigned char *d_mask = mask;
	int *d_dist = dist2;
	if (on_device) {
		if ((rc = S.after_legacy_stream())) return rc;
	} else {
		S3D_HIP_ST(st, upload(d_mask, S.d.p, o_mask, n, st));
		d_dist = reinterpret_cast<int *>(S.d.p + o_dist);
	}
	S3D_HIP_ST(st, hipEventRecord(S.e0, st));
	launch_mask_distance(d_mask, nx, ny, nz, border, d_dist, reinterpret_cast<int *>(S.d.p + o_tmp), st);
	S3D_HIP_ST(st, hipGetLastError());
	S3D_HIP_ST(st, hipEventRecord(S.e1, st));
	if (!on_device) S3D_HIP_ST(st, hipMemcpyAsync(dist2, d_dist, sizeof(int) * n, hipMemcpyDeviceToHost, st));
	if ((rc = S.finish(seconds))) return rc;
	if (!on_device) S3D_HIP_ST(st, hipStreamSynchronize(st));
	return SIFT3D_OK;
}

extern "C" int sift3d_mask_from_distance(const int *dist2, int nx, int ny, int nz, int level2, unsigned char *mask, int on_device, int device,
                                         double *seconds) {
	// (the voxel count is formed stepwise, as in sift3d_mask_from_level; the kernel walks any count by a grid-stride loop)
	const bool dims_ok = nx >= 1 && ny >= 1 && nz >= 1 && (size_t)nx * ny < ((size_t)1 << 39) / (size_t)nz;
	if (!dist2 || !mask || !dims_ok) {
		set_last_error("sift3d_mask_from_distance: bad argument");
		return SIFT3D_ERR_ARG;
	}
	if (seconds) *seconds = 0;
	int rc = pick_device(device);
	if (rc) return rc;
	CallState &S = g_erode[device];
	std::lock_guard<std::mutex> lock(S.mu);
	const size_t n = (size_t)nx * ny * nz;
	// device scratch of a call on host memory: [dist2 | mask]
	Layout L;
	const size_t o_dist = L.take(on_device ? 0 : sizeof(int) * n), o_mask = L.take(on_device ? 0 : n);
	if ((rc = S.ensure(L.end, 0))) return rc;
	hipStream_t st = S.stream;
	const int *d_dist = dist2;
	unsigned char *d_mask = mask;
	if (on_device) {
		if ((rc = S.after_legacy_stream())) return rc;
	} else {
		S3D_HIP_ST(st, upload(d_dist, S.d.p, o_dist, sizeof(int) * n, st));
		d_mask = reinterpret_cast<unsigned char *>(S.d.p + o_mask);
	}
	S3D_HIP_ST(st, hipEventRecord(S.e0, st));
	launch_mask_from_distance(d_dist, n, level2, d_mask, st);
	S3D_HIP_ST(st, hipGetLastError());
	S3D_HIP_ST(st, hipEventRecord(S.e1, st));
	if (!on_device) S3D_HIP_ST(st, hipMemcpyAsync(mask, d_mask, n, hipMemcpyDeviceToHost, st));
	if ((rc = S.finish(seconds))) return rc;
	if (!on_device) S3D_HIP_ST(st, hipStreamSynchronize(st));
	return SIFT3D_OK;
}

extern "C" int sift3d_distance_at_points(const int *dist2, int nx, int ny, int nz, const int *points3, int m, int *poi_dist2, int on_device,
                                         int device) {
	if (!dist2 || !dims_fit_int(nx, ny, nz) || m < 0 || (m > 0 && (!points3 || !poi_dist2))) {
		set_last_error("sift3d_distance_at_points: bad argument");
		return SIFT3D_ERR_ARG;
	}
	if (!on_device) {
		for (int i = 0; i < m; i++) {
			const int x = points3[3 * (size_t)i], y = points3[3 * (size_t)i + 1], z = points3[3 * (size_t)i + 2];
			const bool inside = x >= 0 && x < nx && y >= 0 && y < ny && z >= 0 && z < nz;
			poi_dist2[i] = inside ? dist2[((size_t)z * ny + y) * nx + x] : 0;
		}
		return SIFT3D_OK;
	}
	int rc = pick_device(device);
	if (rc) return rc;
	if (m == 0) return SIFT3D_OK;
	CallState &S = g_dist_at[device];
	std::lock_guard<std::mutex> lock(S.mu);
	if ((rc = S.ensure(sizeof(int) * (size_t)m, 0))) return rc;
	hipStream_t st = S.stream;
	if ((rc = S.after_legacy_stream())) return rc;
	int *d_out = reinterpret_cast<int *>(S.d.p);
	S3D_HIP_ST(st, hipEventRecord(S.e0, st));
	launch_labels_at(dist2, nx, ny, nz, points3, m, d_out, st);  // the look-up of an int volume at integer points, 0 outside
	S3D_HIP_ST(st, hipGetLastError());
	S3D_HIP_ST(st, hipMemcpyAsync(poi_dist2, d_out, sizeof(int) * (size_t)m, hipMemcpyDeviceToHost, st));
	S3D_HIP_ST(st, hipEventRecord(S.e1, st));
	return S.finish(nullptr);
}

extern "C" int sift3d_mask_split(const unsigned char *mask, int nx, int ny, int nz, const sift3d_split_options *o, int *labels, int *count,
                                 int *dist2, sift3d_split_info *info, int on_device, int device, double *seconds) {
	if (!mask || !labels || !count || !dims_fit_distance(nx, ny, nz) || !split_options_ok(o)) {
		set_last_error("sift3d_mask_split: bad argument");
		return SIFT3D_ERR_ARG;
	}
	if (seconds) *seconds = 0;
	int rc = pick_device(device);
	if (rc) return rc;
	CallState &S = g_split[device];
	std::lock_guard<std::mutex> lock(S.mu);
	const size_t n = (size_t)nx * ny * nz;
	const bool own_dist = !(on_device && dist2);
	// device scratch: [aux: the transform's middle field, the labelling's root words, the growth's second volume | the labels of the
	// unreached components | sums of the chunks | cores, unreached, unlabelled and the round counters | the core / unreached bytes |
	// dist2 unless the caller's is on the device | (host memory) mask | labels]
	Layout L;
	const size_t o_aux = L.take(sizeof(int) * n), o_extra = L.take(o->keep_unreached ? sizeof(int) * n : 0);
	const size_t o_sums = L.take(sizeof(int) * label_chunks(n)), o_cnt = L.take(sizeof(int) * (3 + kRoundBatch)), o_bytes = L.take(n);
	const size_t o_dist = L.take(own_dist ? sizeof(int) * n : 0), o_mask = L.take(on_device ? 0 : n);
	const size_t o_labels = L.take(on_device ? 0 : sizeof(int) * n);
	if ((rc = S.ensure(L.end, 0))) return rc;
	hipStream_t st = S.stream;
	const unsigned char *d_mask = mask;
	int *d_labels = labels;
	if (on_device) {
		if ((rc = S.after_legacy_stream())) return rc;
	} else {
		S3D_HIP_ST(st, upload(d_mask, S.d.p, o_mask, n, st));
		d_labels = reinterpret_cast<int *>(S.d.p + o_labels);
	}
	int *d_dist = own_dist ? reinterpret_cast<int *>(S.d.p + o_dist) : dist2;
	int *d_aux = reinterpret_cast<int *>(S.d.p + o_aux), *d_extra = o->keep_unreached ? reinterpret_cast<int *>(S.d.p + o_extra) : nullptr;
	int *d_sums = reinterpret_cast<int *>(S.d.p + o_sums), *d_cnt = reinterpret_cast<int *>(S.d.p + o_cnt), *d_grown = d_cnt + 3;
	unsigned char *d_bytes = reinterpret_cast<unsigned char *>(S.d.p + o_bytes);
	int tail[3] = {0, 0, 0};  // cores, unreached bodies, unlabelled
	S3D_HIP_ST(st, hipMemsetAsync(d_cnt, 0, sizeof(int) * 3, st));
	S3D_HIP_ST(st, hipEventRecord(S.e0, st));
	// 1, 2: the transform and the cores
	launch_mask_distance(d_mask, nx, ny, nz, o->border, d_dist, d_aux, st);
	launch_mask_from_distance(d_dist, n, o->core_dist2, d_bytes, st);
	launch_mask_label(d_bytes, nx, ny, nz, o->connectivity, o->min_core_voxels, d_labels, d_aux, d_sums, d_cnt, st);
	S3D_HIP_ST(st, hipGetLastError());
	S3D_HIP_ST(st, hipMemcpyAsync(tail, d_cnt, sizeof(int), hipMemcpyDeviceToHost, st));
	S3D_HIP_ST(st, hipStreamSynchronize(st));
	const int cores = tail[0];
	// 3: the growth, kRoundBatch rounds per read-back.  A round after the last one that labelled something is the identity, so the
	// batch size does not show in the result.
	int rounds = 0, done = 0;
	int *cur = d_labels, *other = d_aux;
	for (bool more = cores > 0; more;) {
		const int batch = o->max_rounds > 0 && o->max_rounds - done < kRoundBatch ? o->max_rounds - done : kRoundBatch;
		if (batch <= 0) break;
		int grown[kRoundBatch];
		S3D_HIP_ST(st, hipMemsetAsync(d_grown, 0, sizeof(int) * kRoundBatch, st));
		for (int r = 0; r < batch; r++) {
			launch_split_grow(d_dist, cur, other, nx, ny, nz, o->connectivity, d_grown + r, st);
			int *t = cur;
			cur = other;
			other = t;
		}
		S3D_HIP_ST(st, hipGetLastError());
		S3D_HIP_ST(st, hipMemcpyAsync(grown, d_grown, sizeof(int) * batch, hipMemcpyDeviceToHost, st));
		S3D_HIP_ST(st, hipStreamSynchronize(st));
		for (int r = 0; r < batch; r++) {
			if (grown[r] > 0)
				rounds++;
			else
				more = false;
		}
		done += batch;
	}
	if (cur != d_labels) S3D_HIP_ST(st, hipMemcpyAsync(d_labels, cur, sizeof(int) * n, hipMemcpyDeviceToDevice, st));  // an odd last batch
	// 4, 5: the components of what no core reached, behind the cores' numbers
	if (o->keep_unreached) {
		launch_split_rest(d_dist, d_labels, n, d_bytes, st);
		launch_mask_label(d_bytes, nx, ny, nz, o->connectivity, o->min_voxels, d_extra, d_aux, d_sums, d_cnt + 1, st);
	}
	launch_split_finish(d_dist, d_labels, d_extra, cores, n, d_cnt + 2, st);
	S3D_HIP_ST(st, hipGetLastError());
	S3D_HIP_ST(st, hipEventRecord(S.e1, st));
	S3D_HIP_ST(st, hipMemcpyAsync(tail + 1, d_cnt + 1, sizeof(int) * 2, hipMemcpyDeviceToHost, st));
	if (!on_device) S3D_HIP_ST(st, hipMemcpyAsync(labels, d_labels, sizeof(int) * n, hipMemcpyDeviceToHost, st));
	if (dist2 && own_dist) S3D_HIP_ST(st, hipMemcpyAsync(dist2, d_dist, sizeof(int) * n, hipMemcpyDeviceToHost, st));
	if ((rc = S.finish(seconds))) return rc;
	S3D_HIP_ST(st, hipStreamSynchronize(st));
	*count = cores + tail[1];
	if (info) {
		info->cores = cores;
		info->unreached_bodies = tail[1];
		info->rounds = rounds;
		info->unlabelled = tail[2];
	}
	return SIFT3D_OK;
}
