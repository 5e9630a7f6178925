// entry_label.hip -- C-ABI of the connected-component labels (include/sift3d_hip.h: sift3d_mask_label, sift3d_labels_at_points, sift3d_labels_at_positions;
// include/sift3d_hip_test.h: sift3d_test_label_tile).  No reference counterpart.  Kernels: kernels_label.hip.  One-shot entries: call
// state, timing and the order of the checks as DESIGN 4.10 (call_state.h).
#include "call_state.h"

#include "../../include/sift3d_hip_test.h"

using namespace s3d;

namespace {
CallState g_label[kMaxDev], g_labels_at[kMaxDev];

// extents >= 1 whose product fits an int (formed stepwise: three extents of 2^31 - 1 do not fit 64 bits)
bool dims_fit_int(int nx, int ny, int nz) {
	return nx >= 1 && ny >= 1 && nz >= 1 && (size_t)nx * ny <= (((size_t)1 << 31) - 1) / (size_t)nz;
}
}  // namespace

extern "C" int sift3d_test_label_tile(int t[3]) {
	if (!t) return SIFT3D_ERR_ARG;
	t[0] = kLabelTX;
	t[1] = kLabelTY;
	t[2] = kLabelTZ;
	return SIFT3D_OK;
}

extern "C" int sift3d_mask_label(const unsigned char *mask, int nx, int ny, int nz, int connectivity, int min_voxels, int *labels, int *count,
                                 int on_device, int device, double *seconds) {
	if (!mask || !labels || !count || !dims_fit_int(nx, ny, nz) || (connectivity != 6 && connectivity != 26) || min_voxels < 1) {
		set_last_error("sift3d_mask_label: bad argument");
		return SIFT3D_ERR_ARG;
	}
	if (seconds) *seconds = 0;
	int rc = pick_device(device);
	if (rc) return rc;
	CallState &S = g_label[device];
	std::lock_guard<std::mutex> lock(S.mu);
	const size_t n = (size_t)nx * ny * nz;
	// device scratch: [voxel counts, then numbers, of the roots | sums of the chunks | count | (host memory) mask | labels]
	Layout L;
	const size_t o_aux = L.take(sizeof(int) * n), o_sums = L.take(sizeof(int) * label_chunks(n)), o_count = L.take(sizeof(int));
	const size_t o_mask = L.take(on_device ? 0 : n), o_labels = L.take(on_device ? 0 : sizeof(int) * n);
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
	int *d_count = reinterpret_cast<int *>(S.d.p + o_count);
	S3D_HIP_ST(st, hipEventRecord(S.e0, st));
	launch_mask_label(d_mask, nx, ny, nz, connectivity, min_voxels, d_labels, reinterpret_cast<int *>(S.d.p + o_aux),
	                  reinterpret_cast<int *>(S.d.p + o_sums), d_count, st);
	S3D_HIP_ST(st, hipGetLastError());
	S3D_HIP_ST(st, hipEventRecord(S.e1, st));
	S3D_HIP_ST(st, hipMemcpyAsync(count, d_count, sizeof(int), hipMemcpyDeviceToHost, st));
	if (!on_device) S3D_HIP_ST(st, hipMemcpyAsync(labels, d_labels, sizeof(int) * n, hipMemcpyDeviceToHost, st));
	if ((rc = S.finish(seconds))) return rc;
	S3D_HIP_ST(st, hipStreamSynchronize(st));
	return SIFT3D_OK;
}

extern "C" int sift3d_labels_at_points(const int *labels, int nx, int ny, int nz, const int *points3, int m, int *poi_label, int on_device,
                                       int device) {
	if (!labels || !dims_fit_int(nx, ny, nz) || m < 0 || (m > 0 && (!points3 || !poi_label))) {
		set_last_error("sift3d_labels_at_points: bad argument");
		return SIFT3D_ERR_ARG;
	}
	if (!on_device) {
		for (int i = 0; i < m; i++) {
			const int x = points3[3 * (size_t)i], y = points3[3 * (size_t)i + 1], z = points3[3 * (size_t)i + 2];
			const bool inside = x >= 0 && x < nx && y >= 0 && y < ny && z >= 0 && z < nz;
			poi_label[i] = inside ? labels[((size_t)z * ny + y) * nx + x] : 0;
		}
		return SIFT3D_OK;
	}
	int rc = pick_device(device);
	if (rc) return rc;
	if (m == 0) return SIFT3D_OK;
	CallState &S = g_labels_at[device];
	std::lock_guard<std::mutex> lock(S.mu);
	if ((rc = S.ensure(sizeof(int) * (size_t)m, 0))) return rc;
	hipStream_t st = S.stream;
	if ((rc = S.after_legacy_stream())) return rc;
	int *d_out = reinterpret_cast<int *>(S.d.p);
	S3D_HIP_ST(st, hipEventRecord(S.e0, st));
	launch_labels_at(labels, nx, ny, nz, points3, m, d_out, st);
	S3D_HIP_ST(st, hipGetLastError());
	S3D_HIP_ST(st, hipMemcpyAsync(poi_label, d_out, sizeof(int) * (size_t)m, hipMemcpyDeviceToHost, st));
	S3D_HIP_ST(st, hipEventRecord(S.e1, st));
	return S.finish(nullptr);
}

extern "C" int sift3d_labels_at_positions(const int *labels, int nx, int ny, int nz, const float *xyz, int stride, int n, int *out_label,
                                          int on_device, int device) {
	if (!labels || !dims_fit_int(nx, ny, nz) || n < 0 || stride < 3 || (n > 0 && (!xyz || !out_label))) {
		set_last_error("sift3d_labels_at_positions: bad argument");
		return SIFT3D_ERR_ARG;
	}
	if (!on_device) {
		for (int i = 0; i < n; i++) {
			const float *p = xyz + (size_t)i * stride;
			out_label[i] = label_at_position(labels, nx, ny, nz, p[0], p[1], p[2]);
		}
		return SIFT3D_OK;
	}
	int rc = pick_device(device);
	if (rc) return rc;
	if (n == 0) return SIFT3D_OK;
	CallState &S = g_labels_at[device];
	std::lock_guard<std::mutex> lock(S.mu);
	if ((rc = S.ensure(sizeof(int) * (size_t)n, 0))) return rc;
	hipStream_t st = S.stream;
	if ((rc = S.after_legacy_stream())) return rc;
	int *d_out = reinterpret_cast<int *>(S.d.p);
	S3D_HIP_ST(st, hipEventRecord(S.e0, st));
	launch_labels_at_positions(labels, nx, ny, nz, xyz, stride, n, d_out, st);
	S3D_HIP_ST(st, hipGetLastError());
	S3D_HIP_ST(st, hipMemcpyAsync(out_label, d_out, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost, st));
	S3D_HIP_ST(st, hipEventRecord(S.e1, st));
	return S.finish(nullptr);
}
