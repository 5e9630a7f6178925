"""The cases of the per-body tests, shared by tests/test_body_cpu.py (which checks their claims on the restatement, tests/body_ref.py)
and tests/test_gpu_body_fits.py / tests/test_gpu_icgn_labelled.py (which run them on the GPU).  Everything is computed once per process
and read-only."""
import functools

import numpy as np

import body_ref
import icgn_mask_cases as mcases
import label_cases
import rigid_ref

# ---- the spheres scene as a set of matched keypoints -------------------------------------------------------------------------------
# label_cases.spheres(): 12 spheres of radius 11, each with a rotation of 2..4 degrees and a translation of its own.
TAU, NOISE, OUTLIERS, H = 1.0, 0.2, 0.3, 256
ROT_BOUND = 5e-3  # max abs element of (fitted - planted) rotation, for a body with at least MIN_PAIRS pairs
MIN_PAIRS = 17
KEY_RADIUS = 10.0  # keypoints lie within this of a centre: the nearest voxel is then within 10 + sqrt(3) / 2 < 11, inside the sphere
# How many pairs a body needs for ROT_BOUND at this noise.  An inlier set of n_in points spread uniformly in a ball of radius
# a = KEY_RADIUS has sum (x^2 + y^2) = n_in * 2 a^2 / 5 about each axis, so the least-squares rotation about an axis has the standard
# deviation NOISE / sqrt(n_in * 2 a^2 / 5), and the elements of R - R_planted are those angles to first order.  ROT_BOUND at four
# standard deviations (36 elements are judged) needs n_in >= (4 * 0.2 / 5e-3)^2 / 40 = 640 inliers, that is 915 pairs at 30 % outliers.
# The large bodies hold 1000 pairs; two bodies hold fewer than MIN_PAIRS and are only required to be fitted (or refused) as the
# restatement does.
BODY_PAIRS = (1000, 5, 1000, 1000, 12, 1000, 1000, 1000, 1000, 1000, 1000, 1000)
AIR_PAIRS = 300  # keypoints anywhere in the volume: most lie in air (label 0), some in a sphere, whose outliers they are


@functools.lru_cache(maxsize=None)
def sphere_labels():
    """the (64, 80, 96) int32 label volume of label_cases.spheres(), numbered as its POI labels are (mask_label's order)"""
    vol, centres, q, u, body = label_cases.spheres()
    z, y, x = np.indices(vol.shape)
    p = np.stack([x, y, z], -1).astype(np.float64)
    lab = np.zeros(vol.shape, np.int32)
    for c in centres:
        inside = ((p - c) ** 2).sum(-1) <= label_cases.SPHERE_RADIUS ** 2
        rows = inside[q[:, 2], q[:, 1], q[:, 0]]
        number = np.unique(body[rows])
        assert len(number) == 1 and number[0] > 0
        lab[inside] = number[0]
    lab.setflags(write=False)
    return lab


@functools.lru_cache(maxsize=None)
def planted():
    """A (12, 3, 4): the motion [R | b] of body L at index L - 1, and the centre of body L: recovered from the scene's POIs, whose
    displacement is exactly affine in the position"""
    vol, centres, q, u, body = label_cases.spheres()
    lab = sphere_labels()
    A = np.zeros((12, 3, 4))
    cen = np.zeros((12, 3))
    for L in range(1, 13):
        rows = body == L
        X = np.concatenate([q[rows].astype(np.float64), np.ones((int(rows.sum()), 1))], 1)
        A[L - 1] = np.linalg.lstsq(X, q[rows] + u[rows], rcond=None)[0].T
        c = centres[[lab[int(round(c[2])), int(round(c[1])), int(round(c[0]))] == L for c in centres]]
        assert len(c) == 1
        cen[L - 1] = c[0]
    A.setflags(write=False)
    cen.setflags(write=False)
    return A, cen


@functools.lru_cache(maxsize=None)
def grains():
    """pairs (n, 6) float32 (shuffled over the index range), pair_label (n,) int32 by the nearest voxel, count = 12"""
    rng = np.random.default_rng(2026)
    A, cen = planted()
    lab = sphere_labels()
    ref, tar = [], []
    for L, n in enumerate(BODY_PAIRS, 1):
        d = rng.normal(size=(n, 3))
        d *= (KEY_RADIUS * rng.random(n) ** (1 / 3) / np.linalg.norm(d, axis=1))[:, None]
        r = (cen[L - 1] + d).astype(np.float32).astype(np.float64)
        t = r @ A[L - 1][:, :3].T + A[L - 1][:, 3] + rng.normal(0, NOISE, (n, 3))
        bad = rng.random(n) < OUTLIERS
        t[bad] = r[bad] + rng.uniform(-8, 8, (int(bad.sum()), 3))
        ref.append(r)
        tar.append(t)
    r = rng.uniform(-0.5, np.array(lab.shape[::-1]) - 0.5, (AIR_PAIRS, 3))
    ref.append(r)
    tar.append(r + rng.uniform(-8, 8, (AIR_PAIRS, 3)))
    pairs = np.concatenate([np.concatenate(ref), np.concatenate(tar)], 1).astype(np.float32)
    pairs = np.ascontiguousarray(pairs[rng.permutation(len(pairs))])
    label = body_ref.labels_at_positions(lab, pairs)
    pairs.setflags(write=False)
    label.setflags(write=False)
    return pairs, label, 12


@functools.lru_cache(maxsize=None)
def grains_reference():
    pairs, label, count = grains()
    return body_ref.fit_bodies(pairs, label, count, iterations=H, inlier_thresh=TAU)


def rotation_error(A, L):
    return float(np.abs(np.asarray(A, np.float64).reshape(3, 4)[:, :3] - planted()[0][L - 1][:, :3]).max())


CONTACT_REACH = 5.0


def contact_pois(reach=CONTACT_REACH):
    """the lattice POIs of the scene that lie in a sphere and within `reach` voxels of another sphere's surface: points, planted
    displacement, label.  The spheres stand 3.3 voxels apart at the closest and the step-4 lattice puts no POI within 3 voxels of a
    neighbour: the nearest 36 lie 4.26 .. 4.37 voxels from it, which is what reach = 5 selects (test_body_cpu.py checks both)."""
    vol, centres, q, u, body = label_cases.spheres()
    A, cen = planted()
    d = np.linalg.norm(q[:, None, :].astype(np.float64) - cen[None], axis=2) - label_cases.SPHERE_RADIUS  # distance to each surface
    d[np.arange(len(q)), np.maximum(body, 1) - 1] = np.inf
    rows = (body > 0) & (d.min(1) <= reach)
    return q[rows], u[rows], body[rows]


# ---- the seams of k_rigid_bodies -----------------------------------------------------------------------------------------------------
SEAM_SIZES = (0, 2, 3, 4, 63, 64, 65, 255, 256, 257, 1000)  # body L holds SEAM_SIZES[L - 1] pairs
SEAM_H = (1, 255, 256, 257, 1024)


def bodies_of(sizes, seed, extra=(0, -1, None), extra_each=7, noise=0.3, outliers=0.3):
    """pairs, pair_label, count: body L holds sizes[L - 1] pairs of a motion of its own, shuffled over the index range together with
    extra_each pairs of each label of `extra` (None: count + 1), which belong to no body"""
    rng = np.random.default_rng(seed)
    count = len(sizes)
    rows, labels = [], []
    for L, n in enumerate(sizes, 1):
        R = rigid_ref.rotation(rng.normal(size=3), rng.uniform(2, 12))
        p, _, _, _ = rigid_ref.synth_pairs(n, rng, R=R, b=rng.uniform(-10, 10, 3), noise=noise, outliers=outliers, extent=100.0)
        rows.append(p)
        labels.append(np.full(n, L))
    for e in extra:
        p, _, _, _ = rigid_ref.synth_pairs(extra_each, rng, extent=100.0)
        rows.append(p)
        labels.append(np.full(extra_each, count + 1 if e is None else e))
    pairs, labels = np.concatenate(rows).astype(np.float32), np.concatenate(labels).astype(np.int32)
    order = rng.permutation(len(pairs))
    return np.ascontiguousarray(pairs[order]), np.ascontiguousarray(labels[order]), count


@functools.lru_cache(maxsize=None)
def seams():
    pairs, labels, count = bodies_of(SEAM_SIZES, 77)
    pairs.setflags(write=False)
    labels.setflags(write=False)
    return pairs, labels, count


# ---- labels_at_positions: the battery ---------------------------------------------------------------------------------------------------
def position_battery(shape=(5, 6, 7)):
    """labels (nz, ny, nx) int32, all different and positive, and (n, 3) float32 positions: per axis k - 0.5 and k + 0.5 exactly, -0.5 and
    n - 0.5, their float neighbours on both sides, NaN, +-Inf, +-1e30, with the other two coordinates inside"""
    nz, ny, nx = shape
    labels = (1 + np.arange(nz * ny * nx, dtype=np.int32)).reshape(shape)
    rows = []
    for axis, n in enumerate((nx, ny, nz)):
        vals = []
        for k in range(n + 1):
            for v in (np.float32(k - 0.5), np.float32(k + 0.5), np.float32(k)):
                vals += [v, np.nextafter(v, np.float32(-np.inf)), np.nextafter(v, np.float32(np.inf))]
        vals += [np.float32(np.nan), np.float32(np.inf), np.float32(-np.inf), np.float32(1e30), np.float32(-1e30), np.float32(-0.0)]
        for v in vals:
            p = [1.25, 2.5, 3.75]
            p[axis] = v
            rows.append(p)
    return labels, np.array(rows, np.float32)


# ---- the labelled IC-GN scene ---------------------------------------------------------------------------------------------------------
X_CUT, DIAG = 18, 52          # slabs 5 (x < X_CUT) and 2 (x >= X_CUT); body 900 where y + z >= DIAG: a staircase in the y-z plane
STRIP_Z, STRIP_Y = (8, 11), (8, 11)  # label 0 at z in [8, 11), label -4 at y in [8, 11)
LABELS = (5, 2, 900)
# rows of labelled_pois: the two POIs where the three bodies meet.  At r = 2 the second keeps 20 active voxels for 12 parameters; H is
# then so badly conditioned that the kernels' fp32 per-voxel arithmetic shows through the restatement's bars (measured on an MI355X:
# 1.5e-4 voxel, 5.8e-5 in the gradient, every other POI within them), so these two rows are judged by the bit-for-bit comparison with
# icgn_masked only.
JUNCTION_ROWS = (18, 19)
LABELLED_R = (2, 3, 6)


@functools.lru_cache(maxsize=None)
def labelled_volume():
    """the int32 labels of icgn_mask_cases.volumes()' R"""
    z, y, x = np.indices((mcases.NZ, mcases.NY, mcases.NX))
    lab = np.where(x < X_CUT, 5, 2).astype(np.int32)
    lab[y + z >= DIAG] = 900
    lab[(z >= STRIP_Z[0]) & (z < STRIP_Z[1])] = 0
    lab[(y >= STRIP_Y[0]) & (y < STRIP_Y[1])] = -4
    lab.setflags(write=False)
    return lab


@functools.lru_cache(maxsize=None)
def labelled_pois(r):
    """POIs on, 1 voxel off and r off each contact, on R's faces, in the 0 and -4 strips and outside R; and their perturbed truth"""
    lo, hi = r + 1, np.array([mcases.NX, mcases.NY, mcases.NZ]) - 2 - r
    q = []
    for x in (X_CUT, X_CUT - 1, X_CUT + 1, X_CUT - 2, X_CUT + r, X_CUT - 1 - r):   # the plane between 5 and 2
        q.append((x, 20, 20))
    for s in (DIAG, DIAG - 1, DIAG + 1, DIAG - 2, DIAG + r, DIAG - 1 - r):           # the staircase, on both slabs
        q.append((12, 24, s - 24))
        q.append((25, s - 27, 27))
    q += [(X_CUT, 25, DIAG - 25), (X_CUT - 1, 25, DIAG - 26)]                        # where the three meet
    for a in range(3):                                                                # R's faces
        for v in (lo, hi[a]):
            p = [20, 20, 20]
            p[a] = v
            q.append(tuple(p))
    q += [(14, 20, 9), (22, 20, STRIP_Z[0] - 1), (14, 9, 20), (22, STRIP_Y[1], 20)]   # in and beside the strips
    q += [(0, 20, 20), (-3, 5, 5), (mcases.NX + 4, 20, 20), (20, 20, mcases.NZ - 1), (lo - 1, 20, 20)]  # status 2
    q = np.array(q, np.int32)
    truth = mcases.volumes()[3]
    init = mcases.perturbed(truth(q), np.random.default_rng(70 + r))
    q.setflags(write=False)
    init.setflags(write=False)
    return q, init
