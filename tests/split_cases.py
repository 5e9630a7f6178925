"""The cases of the distance-transform and split tests (tests/test_split_cpu.py checks their claims on the restatement,
tests/split_ref.py; tests/test_gpu_edt.py and tests/test_gpu_split.py run them on the GPU).  A mask is an (nz, ny, nx) uint8 array;
ball centres are (x, y, z).  Everything is computed once per process and read-only."""
import functools

import numpy as np

import body_cases
import body_ref
import label_cases
import rigid_ref
import split_ref as ref


def balls(shape, spheres):
    """the mask of the union of the balls (cx, cy, cz, r): (x - cx)^2 + (y - cy)^2 + (z - cz)^2 <= r^2"""
    z, y, x = np.indices(shape)
    m = np.zeros(shape, bool)
    for cx, cy, cz, r in spheres:
        m |= (x - cx) ** 2 + (y - cy) ** 2 + (z - cz) ** 2 <= r * r
    return m.astype(np.uint8)


# scene A: two balls of radius 9 whose centres are 14 apart: one component, a neck at x = 21
A_BALLS = ((14, 16, 16, 9), (28, 16, 16, 9))
A_OPTS = {"border": 1, "core_dist2": 49}
# scene B: a ball of radius 10 and one of radius 7 that overlap
B_BALLS = ((14, 14, 13, 10), (27, 20, 17, 7))
B_CORE_DIST2 = (16, 25, 30, 36)
# scene C: scene A widened, with a third ball too small to hold a core
C_BALLS = A_BALLS + ((50, 16, 16, 4),)


def _packing():
    """about 12 overlapping balls of radius 6..9 in 48 x 56 x 64 (nz, ny, nx), some cut by the volume's faces"""
    rng = np.random.default_rng(412)
    spheres = [(int(rng.integers(4, 60)), int(rng.integers(4, 52)), int(rng.integers(4, 44)), int(rng.integers(6, 10))) for _ in range(12)]
    return balls((48, 56, 64), spheres)


SCENES = {"A": lambda: balls((32, 32, 44), A_BALLS), "B": lambda: balls((32, 36, 44), B_BALLS), "C": lambda: balls((32, 32, 60), C_BALLS),
          "packing": _packing}


@functools.lru_cache(maxsize=None)
def scene(name):
    m = np.ascontiguousarray(SCENES[name]() if name in SCENES else label_cases.get(name))
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def distance(name, border):
    d = ref.distance(scene(name), border)
    d.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def _split(name, opts):
    lab, count, info, d = ref.split(scene(name), **dict(opts))
    lab.setflags(write=False)
    d.setflags(write=False)
    return lab, count, info, d


def split(name, **opts):
    """the restatement's labels, count, info, dist2 of a scene (or of a mask of label_cases)"""
    return _split(name, tuple(sorted(opts.items())))


# what the GPU split test runs, beside the scenes at both connectivities: (mask, options)
SPLIT_RUNS = (
    ("packing", {"core_dist2": 16}), ("packing", {"core_dist2": 25, "connectivity": 26}), ("packing", {"core_dist2": 16, "border": 0}),
    ("random-0.3116", {"core_dist2": 2}), ("random-0.10", {"core_dist2": 2, "connectivity": 26}), ("random-0.6", {"core_dist2": 3}),
    ("random-0.6", {"core_dist2": 2, "connectivity": 26, "border": 0}),
    ("A", dict(A_OPTS, max_rounds=1)), ("A", dict(A_OPTS, max_rounds=3)), ("packing", {"core_dist2": 16, "max_rounds": 3, "connectivity": 26}),
    ("packing", {"core_dist2": 30, "min_core_voxels": 40}), ("random-0.6", {"core_dist2": 3, "min_core_voxels": 2, "min_voxels": 3}),
    ("C", dict(A_OPTS, min_voxels=257)), ("C", dict(A_OPTS, min_voxels=258)), ("random-0.6", {"core_dist2": 3, "keep_unreached": 0}),
)

# ---- the transform's battery -----------------------------------------------------------------------------------------------------------


def _random(shape, density, seed):
    return (np.random.default_rng(seed).random(shape) < density).astype(np.uint8)


def _single(shape, at, value):
    m = np.full(shape, 1 - value, np.uint8)
    m[at] = value
    return m


EDT_MASKS = {
    "all-out": lambda: np.zeros((5, 6, 7), np.uint8), "all-in": lambda: np.ones((9, 20, 70), np.uint8),
    "one-out-corner": lambda: _single((40, 37, 70), (0, 0, 0), 0), "one-out-far-corner": lambda: _single((40, 37, 70), (39, 36, 69), 0),
    "one-in": lambda: _single((6, 7, 9), (3, 2, 5), 1),
    # a long axis exceeds what a workgroup stages, on each axis in turn (shapes are (nz, ny, nx))
    "long-x": lambda: _random((3, 3, 5000), 0.98, 1), "long-y": lambda: _random((3, 5000, 3), 0.98, 2),
    "long-z": lambda: _random((5000, 3, 2), 0.98, 3), "two-runs": lambda: _random((2, 70, 130), 0.98, 4),
    "long-y-one-out": lambda: _single((2, 700, 3), (1, 650, 2), 0),
    # the ballot words along x
    "x-63": lambda: _random((3, 4, 63), 0.9, 5), "x-64": lambda: _random((3, 4, 64), 0.9, 6), "x-65": lambda: _random((3, 4, 65), 0.9, 7),
    "x-129": lambda: _random((3, 4, 129), 0.97, 8), "x-1": lambda: _random((30, 20, 1), 0.8, 9),
}


@functools.lru_cache(maxsize=None)
def edt_mask(name):
    m = np.ascontiguousarray(EDT_MASKS[name]() if name in EDT_MASKS else scene(name))
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def edt_reference(name, border):
    d = ref.distance(edt_mask(name), border)
    d.setflags(write=False)
    return d


def edt_names():
    return sorted(EDT_MASKS) + sorted(label_cases.MASKS) + ["A", "packing"]


# ---- end to end: scene A as two grains that move differently ---------------------------------------------------------------------------
PAIRS_PER_BALL = 300
KEY_RADIUS = 8.0   # keypoints lie within this of a centre: the nearest voxel is then within 8 + sqrt(3) / 2 < 9, inside the ball


@functools.lru_cache(maxsize=None)
def motions():
    """A (2, 3, 4): the rigid motion [R | b] of each ball of scene A about its centre: 6 degrees about one axis, 5 about another"""
    out = np.zeros((2, 3, 4))
    for k, (axis, deg, t) in enumerate((((1.0, 2.0, 0.5), 6.0, (0.8, -0.4, 0.3)), ((-1.0, 0.5, 2.0), -5.0, (-0.6, 0.7, -0.2)))):
        R = rigid_ref.rotation(np.array(axis), deg)
        c = np.array(A_BALLS[k][:3], np.float64)
        out[k, :, :3] = R
        out[k, :, 3] = c + np.array(t) - R @ c
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def grain_pairs():
    """pairs (600, 6) float32, shuffled: PAIRS_PER_BALL keypoints in each ball of scene A, moved by the ball's motion, with the noise and
    the outliers of body_cases.grains()"""
    rng = np.random.default_rng(2026)
    A = motions()
    refs, tars = [], []
    for k in range(2):
        n = PAIRS_PER_BALL
        d = rng.normal(size=(n, 3))
        d *= (KEY_RADIUS * rng.random(n) ** (1 / 3) / np.linalg.norm(d, axis=1))[:, None]
        r = (np.array(A_BALLS[k][:3], np.float64) + d).astype(np.float32).astype(np.float64)
        t = r @ A[k][:, :3].T + A[k][:, 3] + rng.normal(0, body_cases.NOISE, (n, 3))
        bad = rng.random(n) < body_cases.OUTLIERS
        t[bad] = r[bad] + rng.uniform(-8, 8, (int(bad.sum()), 3))
        refs.append(r)
        tars.append(t)
    pairs = np.concatenate([np.concatenate(refs), np.concatenate(tars)], 1).astype(np.float32)
    pairs = np.ascontiguousarray(pairs[rng.permutation(len(pairs))])
    pairs.setflags(write=False)
    return pairs


def rotation_error(A, k):
    """max abs element of (fitted - planted) rotation of ball k"""
    return float(np.abs(np.asarray(A, np.float64).reshape(3, 4)[:, :3] - motions()[k][:, :3]).max())


def fit_errors(labels, count):
    """the restatement's fits of grain_pairs() under `labels`: per body the rotation error against each of the two planted motions"""
    pairs = grain_pairs()
    fits, _ = body_ref.fit_bodies(pairs, body_ref.labels_at_positions(labels, pairs), count, iterations=body_cases.H, inlier_thresh=body_cases.TAU)
    return [(f["status"], rotation_error(f["A"], 0), rotation_error(f["A"], 1)) for f in fits]
