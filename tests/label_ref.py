"""NumPy restatement of the label contracts of include/sift3d_hip.h.  sift3d_mask_label: the minimum of the linear voxel index over
the neighbourhood, iterated until nothing changes (roots(), which also counts the sweeps), then the numbering of the kept
components in ascending order of their lowest voxel (number()).  The labelled window calls (sift3d_strain_labelled,
sift3d_validate_displacements_labelled, sift3d_field_eval_labelled): per label L > 0 the EXISTING restatements (tests/strain_ref.py,
tests/validate_ref.py, tests/field_ref.py) are called with valid & (label == L) and the rows (queries) of label L are kept
(literal=True), or, which gives the same arrays faster, on the POIs of label L alone; the rows of a label <= 0 are built by the rule:
status 2 where a coordinate is out of range, else status 1 with no neighbours."""
import numpy as np

import field_ref
import strain_ref
import validate_ref

BIG = np.iinfo(np.int64).max


def _shifted(a, dz, dy, dx, fill):
    """b[z, y, x] = a[z + dz, y + dy, x + dx], fill outside"""
    out = np.full_like(a, fill)
    nz, ny, nx = a.shape
    src = tuple(slice(max(d, 0), n + min(d, 0)) for d, n in ((dz, nz), (dy, ny), (dx, nx)))
    dst = tuple(slice(max(-d, 0), n + min(-d, 0)) for d, n in ((dz, nz), (dy, ny), (dx, nx)))
    out[dst] = a[src]
    return out


def offsets(connectivity):
    assert connectivity in (6, 26)
    o = [(dz, dy, dx) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dz, dy, dx) != (0, 0, 0)]
    return [d for d in o if connectivity == 26 or sum(abs(v) for v in d) == 1]


def roots(mask, connectivity=6):
    """(per voxel the lowest linear index of its component, BIG outside the mask; the sweeps it took, the last one changing nothing)"""
    m = np.asarray(mask) != 0
    lab = np.where(m, np.arange(m.size, dtype=np.int64).reshape(m.shape), BIG)
    offs = offsets(connectivity)
    sweeps = 0
    while True:
        sweeps += 1
        new = lab
        for d in offs:
            new = np.minimum(new, _shifted(lab, *d, BIG))
        new = np.where(m, new, BIG)
        if np.array_equal(new, lab):
            return lab, sweeps
        lab = new


def number(root, min_voxels=1):
    """the labels (int32) and the count from roots()'s first result"""
    inside = root != BIG
    vals, inverse, sizes = np.unique(root[inside], return_inverse=True, return_counts=True)
    kept = sizes >= min_voxels
    numbers = np.where(kept, np.cumsum(kept), 0).astype(np.int32)   # np.unique sorts: ascending lowest voxel
    out = np.zeros(root.shape, np.int32)
    out[inside] = numbers[inverse]
    return out, int(kept.sum())


def label(mask, connectivity=6, min_voxels=1):
    """labels (nz, ny, nx) int32 and count of sift3d_mask_label"""
    return number(roots(mask, connectivity)[0], min_voxels)


def labels_at(labels, points):
    """sift3d_labels_at_points"""
    lab = np.asarray(labels)
    q = np.asarray(points, np.int64).reshape(-1, 3)
    nz, ny, nx = lab.shape
    inside = (q >= 0).all(1) & (q[:, 0] < nx) & (q[:, 1] < ny) & (q[:, 2] < nz)
    out = np.zeros(len(q), np.int32)
    out[inside] = lab[q[inside, 2], q[inside, 1], q[inside, 0]]
    return out


def _valid_of(valid, lab, L):
    on = np.asarray(lab).reshape(-1) == L
    if valid is not None:
        on = on & (np.asarray(valid).reshape(-1) != 0)
    return on.astype(np.uint8)


def _rows(a, rows):
    return None if a is None else np.asarray(a)[rows]


def strain(points, disp, valid, lab, literal=False, **opts):
    """sift3d_strain_labelled: arrays like strain_ref.strain's.  literal: the restatement sees every POI, with valid & (label == L);
    otherwise it sees the POIs of label L alone, which is the same thing (the others neither contribute nor are kept, and the order of
    the rest stands) in time m_L^2 instead of m m_L"""
    q = np.asarray(points, np.int64).reshape(-1, 3)
    u = np.asarray(disp, np.float64).reshape(-1, 3)
    lab = np.asarray(lab).reshape(-1)
    out = strain_ref.strain(q[:0], u[:0], None, **opts)
    out = {k: np.zeros((len(q),) + v.shape[1:], v.dtype) for k, v in out.items()}
    low = lab <= 0
    out["status"][low] = np.where((np.abs(q[low]) > strain_ref.COORD_MAX).any(1), 2, 1)
    for L in np.unique(lab[~low]):
        rows = lab == L
        if literal:
            part = strain_ref.strain(q, u, _valid_of(valid, lab, L), **opts)
            part = {k: v[rows] for k, v in part.items()}
        else:
            part = strain_ref.strain(q[rows], u[rows], _rows(valid, rows), **opts)
        for k in out:
            out[k][rows] = part[k]
    return out


def validate(points, disp, grad, valid, lab, literal=False, **opts):
    """sift3d_validate_displacements_labelled: records like validate_ref.validate's; literal as for strain()"""
    q = np.asarray(points, np.int64).reshape(-1, 3)
    u = np.asarray(disp, np.float64).reshape(-1, 3)
    g = None if grad is None else np.asarray(grad, np.float64).reshape(-1, 9)
    lab = np.asarray(lab).reshape(-1)
    out = np.zeros(len(q), validate_ref.RESULT_DTYPE)
    low = lab <= 0
    out["status"][low] = np.where((np.abs(q[low]) > validate_ref.COORD_MAX).any(1), 2, 1)
    for L in np.unique(lab[~low]):
        rows = lab == L
        if literal:
            out[rows] = validate_ref.validate(q, u, g, _valid_of(valid, lab, L), **opts)[rows]
        else:
            out[rows] = validate_ref.validate(q[rows], u[rows], _rows(g, rows), _rows(valid, rows), **opts)
    return out


def evaluate(points, disp, valid, lab, queries, query_lab, literal=False, **opts):
    """sift3d_field_eval_labelled: arrays like field_ref.evaluate's; literal as for strain()"""
    q = np.asarray(points, np.int64).reshape(-1, 3)
    u = np.asarray(disp, np.float64).reshape(-1, 3)
    xs = np.asarray(queries, np.float64).reshape(-1, 3)
    lab, qlab = np.asarray(lab).reshape(-1), np.asarray(query_lab).reshape(-1)
    out = field_ref.evaluate(q, u, valid, xs[:0], **opts)
    out = {k: np.zeros((len(xs),) + v.shape[1:], v.dtype) for k, v in out.items()}
    low = qlab <= 0
    with np.errstate(invalid="ignore"):
        out["status"][low] = np.where((np.abs(xs[low]) <= field_ref.COORD_MAX).all(1), 1, 2)
    for L in np.unique(qlab[~low]):
        rows, mine = qlab == L, lab == L
        if literal:
            part = field_ref.evaluate(q, u, _valid_of(valid, lab, L), xs[rows], **opts)
        else:
            part = field_ref.evaluate(q[mine], u[mine], _rows(valid, mine), xs[rows], **opts)
        for k in out:
            out[k][rows] = part[k]
    return out
