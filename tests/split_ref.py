"""NumPy restatement of the contracts of sift3d_mask_distance, sift3d_mask_from_distance, sift3d_distance_at_points and
sift3d_mask_split (include/sift3d_hip.h).  The transform is, axis by axis, D(a) = min over a' of G(a') + (a - a')^2 in int64 with
NONE (no out-voxel) kept through every addition; with border the two voxels just outside the axis hold G = 0.  The split is the header's
rule word for word: the cores' components by tests/label_ref.py, the growth in synchronous rounds with shifted arrays, the components
of what no core reached behind the cores' numbers."""
import numpy as np

import label_ref

NONE = 2 ** 31 - 1   # SIFT3D_DIST2_NONE
DEFAULTS = {"connectivity": 6, "core_dist2": 16, "min_core_voxels": 1, "border": 1, "max_rounds": 0, "keep_unreached": 1, "min_voxels": 1}


def _shift_axis(a, axis, k, fill):
    """b[.., i, ..] = a[.., i + k, ..] along axis, fill outside"""
    out = np.full_like(a, fill)
    n = a.shape[axis]
    if abs(k) >= n:
        return out
    src, dst = [slice(None)] * a.ndim, [slice(None)] * a.ndim
    src[axis] = slice(max(k, 0), n + min(k, 0))
    dst[axis] = slice(max(-k, 0), n + min(-k, 0))
    out[tuple(dst)] = a[tuple(src)]
    return out


def _axis_pass(G, axis, border):
    n = G.shape[axis]
    best = G.copy()
    if border:
        shape = [1] * G.ndim
        shape[axis] = n
        i = np.arange(n, dtype=np.int64).reshape(shape)
        best = np.minimum(best, np.minimum((i + 1) ** 2, (n - i) ** 2))
    for k in range(1, n):
        if k * k >= best.max():   # no voxel can still gain from an entry k or more away
            break
        for s in (k, -k):
            g = _shift_axis(G, axis, s, NONE)
            best = np.minimum(best, np.where(g >= NONE, NONE, g + k * k))
    return best


def distance(mask, border=1):
    """dist2 (nz, ny, nx) int32 of sift3d_mask_distance"""
    m = np.asarray(mask) != 0
    assert m.ndim == 3 and border in (0, 1)
    G = np.where(m, NONE, 0).astype(np.int64)
    for axis in (2, 1, 0):   # x, y, z
        G = _axis_pass(G, axis, border)
    return G.astype(np.int32)


def mask_from_distance(dist2, level2):
    return (np.asarray(dist2) >= level2).astype(np.uint8)


def distance_at(dist2, points):
    return label_ref.labels_at(dist2, points)


def grow(labels, dist2, inside, connectivity, max_rounds=0):
    """(labels after the growth, the rounds that labelled at least one voxel)"""
    lab = np.array(labels, np.int32)
    d = np.asarray(dist2, np.int64)
    offs = label_ref.offsets(connectivity)
    rounds = 0
    while max_rounds == 0 or rounds < max_rounds:
        best_d = np.full(lab.shape, -1, np.int64)
        best_l = np.zeros(lab.shape, np.int32)
        for off in offs:
            nl = label_ref._shifted(lab, *off, 0)    # the labels at the start of the round
            nd = label_ref._shifted(d, *off, 0)
            better = (nl > 0) & ((nd > best_d) | ((nd == best_d) & (nl < best_l)))
            best_d = np.where(better, nd, best_d)
            best_l = np.where(better, nl, best_l)
        new = inside & (lab == 0) & (best_l > 0)
        if not new.any():
            break
        lab[new] = best_l[new]
        rounds += 1
    return lab, rounds


def split(mask, **opts):
    """labels (int32), count, info (dict), dist2 of sift3d_mask_split"""
    o = dict(DEFAULTS)
    assert set(opts) <= set(o), opts
    o.update(opts)
    inside = np.asarray(mask) != 0
    d = distance(inside, o["border"])
    lab, cores = label_ref.label(d >= o["core_dist2"], o["connectivity"], o["min_core_voxels"])
    rounds = 0
    if cores:
        lab, rounds = grow(lab, d, inside, o["connectivity"], o["max_rounds"])
    unreached = 0
    if o["keep_unreached"]:
        extra, unreached = label_ref.label(inside & (lab == 0), o["connectivity"], o["min_voxels"])
        lab = np.where(extra > 0, extra + cores, lab).astype(np.int32)
    info = {"cores": cores, "unreached_bodies": unreached, "rounds": rounds, "unlabelled": int((inside & (lab == 0)).sum())}
    return lab, cores + unreached, info, d
