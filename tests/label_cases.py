"""Inputs of the label tests (tests/test_label_cpu.py, tests/test_gpu_labels.py, tests/test_gpu_labelled_windows.py): the masks of
sift3d_mask_label, placed by the extents T of the tile whose union-find the kernel runs in LDS (a second kernel merges the seams
between tiles), and the scenes of several bodies.  A mask is an (nz, ny, nx) uint8 array.  reference(name, connectivity, min_voxels)
is the restatement's answer (tests/label_ref.py), computed once per process and never modified."""
import functools
import importlib

import numpy as np

import label_ref as ref

DEFAULT_TILE = (32, 8, 8)   # include/sift3d_hip_test.h, sift3d_test_label_tile


@functools.lru_cache(maxsize=None)
def tile():
    """(tx, ty, tz) from the library's hook, the documented extents where no library is built"""
    try:
        return tuple(importlib.import_module("3dsift_amd.capi").label_tile())
    except Exception:
        return DEFAULT_TILE


def _vol(nx, ny, nz):
    return np.zeros((nz, ny, nx), np.uint8)


def _set(m, *voxels):
    for x, y, z in voxels:
        m[z, y, x] = 1
    return m


# ---- plain shapes ------------------------------------------------------------------------------------------------------------------
def zero():
    return _vol(7, 6, 5)


def full():
    """every voxel in, the bytes 1, 128 and 255 mixed; several tiles along every axis"""
    tx, ty, tz = tile()
    rng = np.random.default_rng(11)
    return rng.choice(np.array([1, 128, 255], np.uint8), (tz + 2, ty + 3, tx + 5))


def line(axis):
    shape = [1, 1, 1]
    shape[2 - axis] = 300
    return np.ones(shape, np.uint8)


def checkerboard():
    tx, ty, tz = tile()
    z, y, x = np.indices((tz + 1, ty + 2, tx + 3))
    return ((x + y + z) % 2 == 0).astype(np.uint8)


def extent(axis, n):
    """a random half-full mask whose extent on `axis` (0 x, 1 y, 2 z) is n, the other two small and no multiples of T"""
    dims = [5, 5, 3]
    dims[axis] = n
    rng = np.random.default_rng(100 + 10 * axis + n % 7)
    return (rng.random((dims[2], dims[1], dims[0])) < 0.5).astype(np.uint8)


def extents():
    """name -> (axis, n) for n = 1, T - 1, T, T + 1, 2 T + 1 on every axis"""
    out = {}
    for axis, t in enumerate(tile()):
        for tag, n in (("1", 1), ("T-1", t - 1), ("T", t), ("T+1", t + 1), ("2T+1", 2 * t + 1)):
            out[f"extent-{'xyz'[axis]}-{tag}"] = (axis, n)
    return out


# ---- contacts across the seams between tiles: every pair is one component under 26; a face pair also under 6 ------------------------
def seam_face(axis):
    """two voxels that share a face across the first tile boundary of `axis`"""
    t = tile()
    a = [3, 2, 1]
    b = list(a)
    a[axis], b[axis] = t[axis] - 1, t[axis]
    return _set(_vol(t[0] + 3, t[1] + 3, t[2] + 3), a, b)


def seam_edge(direction):
    """pairs that share only an edge parallel to `direction`, across the tile boundaries of the other two axes: both diagonals, two
    planes apart along the edge"""
    t = tile()
    p, q = [a for a in range(3) if a != direction]
    pairs = []
    for k, (sp, sq) in enumerate(((0, 0), (0, 1))):
        a, b = [0, 0, 0], [0, 0, 0]
        a[direction] = b[direction] = 1 + 3 * k
        a[p], b[p] = t[p] - 1, t[p]
        a[q], b[q] = (t[q] - 1, t[q]) if sq == 0 else (t[q], t[q] - 1)
        pairs += [a, b]
    return _set(_vol(t[0] + 3, t[1] + 3, t[2] + 3), *pairs)


def seam_corner():
    """pairs that share only a corner where eight tiles meet: the four body diagonals, each at a corner of its own of a 3 x 3 x 3
    arrangement of tiles, so that the pairs do not touch one another"""
    tx, ty, tz = tile()
    m = _vol(2 * tx + 2, 2 * ty + 2, 2 * tz + 2)
    corners = ((tx, ty, tz), (2 * tx, ty, tz), (tx, 2 * ty, tz), (tx, ty, 2 * tz))
    for (cx, cy, cz), (sx, sy) in zip(corners, ((0, 0), (1, 0), (0, 1), (1, 1))):
        a = (cx - 1 + sx, cy - 1 + sy, cz - 1)
        b = (cx - sx, cy - sy, cz)
        _set(m, a, b)
    return m


SEAM_PAIRS = {"seam-face-x": 1, "seam-face-y": 1, "seam-face-z": 1, "seam-edge-x": 2, "seam-edge-y": 2, "seam-edge-z": 2, "seam-corner": 4}


# ---- long and ramified components ----------------------------------------------------------------------------------------------------
def serpentine():
    """one path through every second row of every second plane of a 33 x 17 x 9 volume: the rows of a plane joined at alternating
    ends, the planes at alternating corners"""
    m = _vol(33, 17, 9)
    for z in range(0, 9, 2):
        for y in range(0, 17, 2):
            m[z, y, :] = 1
            if y + 2 < 17:
                m[z, y + 1, 32 if (y // 2) % 2 == 0 else 0] = 1
        if z + 2 < 9:   # a plane's path runs from (0, 0) to (32, 16); the next plane is walked backwards
            if (z // 2) % 2 == 0:
                m[z + 1, 16, 32] = 1
            else:
                m[z + 1, 0, 0] = 1
    return m


RANDOM_DENSITIES = {"random-0.10": 0.10, "random-0.25": 0.25, "random-0.3116": 0.3116, "random-0.6": 0.6}


def random_mask(name):
    """70 x 45 x 37 voxels; 0.10 is just above the percolation threshold of 26-connectivity, 0.3116 that of 6-connectivity"""
    rng = np.random.default_rng(int(round(RANDOM_DENSITIES[name] * 10000)))
    return (rng.random((37, 45, 70)) < RANDOM_DENSITIES[name]).astype(np.uint8)


def u_shape():
    """component A is a U whose arms stand in two different tiles along x, and its lowest voxel is the top of the far arm; component
    B, a single voxel, lies between the two tops in the linear order.  A is number 1 by its lowest voxel; numbering by the voxel at
    which the near tile first saw A would put B first."""
    tx = tile()[0]
    m = _vol(tx + 8, 7, 1)
    far, near = tx + 4, 2
    m[0, 0:6, far] = 1      # lowest voxel: (far, 0)
    m[0, 2:6, near] = 1     # top of the near arm: (near, 2)
    m[0, 5, near:far + 1] = 1
    m[0, 1, 20] = 1         # B
    return m


MASKS = {"zero": zero, "full": full, "line-x": functools.partial(line, 0), "line-z": functools.partial(line, 2), "checkerboard": checkerboard,
         "seam-face-x": functools.partial(seam_face, 0), "seam-face-y": functools.partial(seam_face, 1),
         "seam-face-z": functools.partial(seam_face, 2), "seam-edge-x": functools.partial(seam_edge, 0),
         "seam-edge-y": functools.partial(seam_edge, 1), "seam-edge-z": functools.partial(seam_edge, 2), "seam-corner": seam_corner,
         "serpentine": serpentine, "u-shape": u_shape}
MASKS.update({name: functools.partial(extent, *args) for name, args in extents().items()})
MASKS.update({name: functools.partial(random_mask, name) for name in RANDOM_DENSITIES})


@functools.lru_cache(maxsize=None)
def get(name):
    m = np.ascontiguousarray(MASKS[name](), np.uint8)
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def reference_roots(name, connectivity):
    root, sweeps = ref.roots(get(name), connectivity)
    root.setflags(write=False)
    return root, sweeps


@functools.lru_cache(maxsize=None)
def reference(name, connectivity, min_voxels=1):
    lab, count = ref.number(reference_roots(name, connectivity)[0], min_voxels)
    lab.setflags(write=False)
    return lab, count


@functools.lru_cache(maxsize=None)
def size_cuts():
    """(name, connectivity, min_voxels): 3 on the 0.25 mask, and the size of its second largest component and one more"""
    lab, count = reference("random-0.25", 6)
    sizes = np.sort(np.bincount(lab.reshape(-1))[1:])
    s = int(sizes[-2])
    return (("random-0.25", 6, 3), ("random-0.25", 6, s), ("random-0.25", 6, s + 1), ("random-0.25", 26, 3))


# ---- scenes of several bodies --------------------------------------------------------------------------------------------------------
SCENE_RADIUS = 8


def lattice(counts=(10, 10, 10), step=4, origin=2):
    g = [origin + step * np.arange(n) for n in counts]
    z, y, x = np.meshgrid(g[2], g[1], g[0], indexing="ij")
    return np.stack([x, y, z], -1).reshape(-1, 3).astype(np.int32)


@functools.lru_cache(maxsize=None)
def two_bodies():
    """two bodies, each translated rigidly, that meet at the plane z = 19.5: points, disp, label"""
    q = lattice()
    low = q[:, 2] < 20
    u = np.where(low[:, None], np.array([0.5, -0.25, 0.125]), np.array([-1.5, 0.75, 0.125]))
    return q, np.ascontiguousarray(u), np.where(low, 1, 2).astype(np.int32)


@functools.lru_cache(maxsize=None)
def grain():
    """a grain of 27 POIs (all coordinates in 14..22) translated in a matrix that follows 0.01 (y, z, x): points, disp, label (matrix
    1, grain 2) and the query between them"""
    q = lattice()
    inside = ((q >= 14) & (q <= 22)).all(1)
    smooth = 0.01 * q[:, [1, 2, 0]].astype(np.float64)
    u = np.where(inside[:, None], np.array([1.5, -0.75, 0.5]), smooth)
    return q, np.ascontiguousarray(u), np.where(inside, 2, 1).astype(np.int32), np.array([[13.0, 18.0, 18.0]])


SPHERE_RADIUS = 11.0
SPHERE_LEVEL = 0.5


def _rotation(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


@functools.lru_cache(maxsize=None)
def spheres():
    """a 96 x 80 x 64 volume of 12 textured spheres (grey values 1..2 in air of 0) at least two voxels apart, each with a rotation of
    a few degrees and a translation of its own; POIs on the step-4 lattice.  Returns vol (float32), centres (12, 3), points, disp (the
    rigid motion of the sphere that holds the POI, 0 in air), body (12 numbered 1..12 in the order of mask_label, 0 in air)."""
    rng = np.random.default_rng(96)
    centres = np.array([[12 + 24 * i, 13 + 27 * j, 32 + 4 * (-1) ** (i + j)] for j in range(3) for i in range(4)], np.float64)
    z, y, x = np.indices((64, 80, 96))
    p = np.stack([x, y, z], -1).astype(np.float64)
    vol = np.zeros((64, 80, 96), np.float32)
    body_of = np.zeros((64, 80, 96), np.int32)
    for k, c in enumerate(centres):
        inside = ((p - c) ** 2).sum(-1) <= SPHERE_RADIUS ** 2
        vol[inside] = (1.0 + rng.random(int(inside.sum()))).astype(np.float32)
        body_of[inside] = k + 1
    # mask_label's numbers: ascending lowest voxel
    first = [int(np.flatnonzero(body_of.reshape(-1) == k + 1)[0]) for k in range(len(centres))]
    rank = np.argsort(np.argsort(first)) + 1
    q = lattice((24, 20, 16))
    body = body_of[q[:, 2], q[:, 1], q[:, 0]]
    u = np.zeros((len(q), 3))
    for k, c in enumerate(centres):
        R = _rotation(rng.normal(size=3), 0.03 + 0.04 * rng.random())
        t = rng.uniform(-1.5, 1.5, 3)
        rows = body == k + 1
        d = q[rows].astype(np.float64) - c
        u[rows] = d @ R.T - d + t
    numbered = np.where(body > 0, rank[np.maximum(body, 1) - 1], 0).astype(np.int32)
    return vol, centres, q, u, numbered
