"""CPU restatement of the per-body calls of include/sift3d_hip.h (sift3d_fit_rigid_bodies, sift3d_labels_at_positions,
sift3d_icgn_init_from_body_fits, sift3d_icgn_labelled): test infrastructure only.  Each is one sentence on a restatement that exists:
a body's fit is rigid_ref.fit on the body's pairs in ascending index with the problem index p = L; a POI of the labelled IC-GN is
icgn_mask_ref's POI under the mask labels == L."""
import numpy as np

import icgn_mask_ref
import rigid_ref

FIT_KEYS = ("status", "candidates", "best_hypothesis", "best_count", "inliers", "hyp", "A", "rms")


def fit_bodies(pairs, pair_label, count, iterations=256, **opts):
    """the list of rigid_ref.fit's dicts, body L at index L - 1 (each with `rows`, the body's pair indices, ascending), and the mask
    (n,) bool scattered back: a pair of no body and a body of status 1 or 2 have 0"""
    pairs = np.asarray(pairs, np.float32).reshape(-1, 6)
    lab = np.asarray(pair_label, np.int64).reshape(-1)
    mask = np.zeros(len(pairs), bool)
    fits = []
    for L in range(1, int(count) + 1):
        rows = np.flatnonzero(lab == L)
        with np.errstate(all="ignore"):
            f = rigid_ref.fit(pairs[rows], p=L, iterations=iterations, **opts)
        f["rows"] = rows
        if f["status"] in (0, 3):
            mask[rows] = f["mask"]
        fits.append(f)
    return fits, mask


def labels_at_positions(labels, xyz):
    """the label at the voxel nearest to each fp32 position (the first three columns of xyz), 0 outside: per axis inside iff
    -0.5 <= float64(x) < n - 0.5, then i = floor(float64(x) + 0.5)"""
    labels = np.asarray(labels)
    pos = np.asarray(xyz, np.float32)[:, :3].astype(np.float64)
    nz, ny, nx = labels.shape
    out = np.zeros(len(pos), np.int32)
    with np.errstate(invalid="ignore"):
        for i, p in enumerate(pos):
            if all(-0.5 <= p[a] and p[a] < n - 0.5 for a, n in enumerate((nx, ny, nz))):
                x, y, z = (int(np.floor(v + 0.5)) for v in p)
                out[i] = labels[z, y, x]
    return out


def labels_at(labels, points):
    labels = np.asarray(labels)
    nz, ny, nx = labels.shape
    q = np.asarray(points, np.int64).reshape(-1, 3)
    inside = (q >= 0).all(1) & (q[:, 0] < nx) & (q[:, 1] < ny) & (q[:, 2] < nz)
    out = np.zeros(len(q), np.int32)
    out[inside] = labels[q[inside, 2], q[inside, 1], q[inside, 0]]
    return out


def icgn_labelled(R, T, labels, points, init=None, min_fraction=0.0, tar_is_coefficients=False, **opts):
    """arrays like capi.icgn_labelled's: per distinct POI label L one icgn_mask_ref.icgn_masked over the POIs of L with the mask
    labels == L; a POI whose label is <= 0 is run under the empty mask (status 5 and 2 first, else n = 0 and status 7)"""
    pts = np.asarray(points, np.int64).reshape(-1, 3)
    lab = labels_at(labels, pts)
    m = len(pts)
    out = {"p": np.zeros((m, 12)), "zncc": np.zeros(m), "last_step": np.zeros(m), "iterations": np.zeros(m, np.int64),
           "status": np.zeros(m, np.int64), "active": np.zeros(m, np.int64), "label": lab}
    for L in np.unique(lab):
        rows = np.flatnonzero(lab == L)
        mask = (np.asarray(labels) == L).astype(np.uint8) if L > 0 else np.zeros(np.asarray(labels).shape, np.uint8)
        w = icgn_mask_ref.icgn_masked(R, T, mask, pts[rows], None if init is None else np.asarray(init)[rows], min_fraction,
                                      tar_is_coefficients, **opts)
        for k in ("p", "zncc", "last_step", "iterations", "status", "active"):
            out[k][rows] = w[k]
    out["displacement"] = out["p"][:, [0, 4, 8]]
    out["gradient"] = out["p"].reshape(-1, 3, 4)[:, :, 1:]
    return out
