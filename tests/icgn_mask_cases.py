"""The cases of the masked IC-GN tests, shared by tests/test_icgn_mask_cpu.py (which checks their preconditions on the restatement,
tests/icgn_mask_ref.py) and tests/test_gpu_icgn_mask.py (which runs them on the GPU).

The volumes: R is 40 x 36 x 44 voxels (x, y, z all different, so a transposed or mis-strided mask index cannot pass), cut out of a
48 x 44 x 52 scene at the offset (4, 4, 4); T is the whole deformed scene, so a subset of any radius up to 16 stays inside T's tap
domain wherever it lies in R.  A POI q of R sits at q + 4 in the scene: its true displacement into T is the scene's plus 4."""
import functools

import numpy as np

import bspline_ref as bref
import icgn_ref as ref

NX, NY, NZ = 40, 36, 44
OFF = 4
BIG = (NZ + 2 * OFF, NY + 2 * OFF, NX + 2 * OFF)
GRAD = [k for k in range(12) if k % 4]
# the project's bars of a fixed-length run against the restatement (tests/test_gpu_icgn.py): displacement, gradient, zncc
BARS = (1e-4, 1e-5, 1e-5)


@functools.lru_cache(maxsize=None)
def volumes():
    """R (NZ, NY, NX), T (BIG), T's float32 B-spline coefficients and truth(points of R) -> (m, 12)"""
    Rb, Tb, truth_big = ref.scene(BIG, ref.rot(1.5, -1.0, 2.0), (0.4, 0.3, 0.25), seed=7)
    R = np.ascontiguousarray(Rb[OFF:OFF + NZ, OFF:OFF + NY, OFF:OFF + NX])

    def truth(points):
        p = truth_big(np.asarray(points, np.float64).reshape(-1, 3) + OFF)
        p[:, [0, 4, 8]] += OFF
        return p

    for a in (R, Tb):
        a.setflags(write=False)
    C = bref.prefilter(Tb, f32=True)
    C.setflags(write=False)
    return R, Tb, C, truth


def perturbed(truth, rng, du=0.25, dg=0.005):
    return truth + np.where(np.arange(12) % 4 == 0, rng.uniform(-du, du, truth.shape), rng.uniform(-dg, dg, truth.shape))


def pois(r, m=12, seed=0):
    """m POIs of R whose subset of radius r plus its margin lies in R: the six with q = r + 1 (or n - 2 - r) on a face first"""
    lo, hi = r + 1, np.array([NX, NY, NZ]) - 2 - r
    rng = np.random.default_rng(500 + 10 * r + seed)
    q = np.stack([rng.integers(lo, hi[a] + 1, m) for a in range(3)], 1)
    for a in range(3):
        q[2 * a, a] = lo
        q[2 * a + 1, a] = hi[a]
    return q.astype(np.int32)


# ---- the agreement cases: six half-spaces through the POIs' subsets, r = 3 and 6 ---------------------------------------------

HALF_SPACES = [(r, axis, side) for r in (3, 6) for axis in (0, 1, 2) for side in ("<", ">")]
HALF_IDS = [f"r{r}-{'xyz'[a]}{s}" for r, a, s in HALF_SPACES]
RUNS = [(max_it, interp) for max_it in (1, 5) for interp in (0, 1, 2)]  # tolerance 0: exactly max_it updates


def axis_mask(axis, side, c):
    """coordinate `axis` (0 x, 1 y, 2 z) < c or > c"""
    g = np.arange((NX, NY, NZ)[axis])
    keep = g < c if side == "<" else g > c
    shape = [1, 1, 1]
    shape[2 - axis] = len(g)
    return np.ascontiguousarray(np.broadcast_to(keep.reshape(shape), (NZ, NY, NX))).astype(np.uint8)


def half_space(r, axis, side):
    """mask, POIs (3, sharing their coordinate c0 along `axis`), init, and the active count every POI has.  The mask ends two voxels
    beyond c0: the in-mask offsets along the axis are -r .. 1 (or -1 .. r), the active ones -r .. 0 (0 .. r): (r + 1) of (2r + 1)
    planes, more than half the subset."""
    _, _, _, truth = volumes()
    rng = np.random.default_rng(900 + 100 * r + 10 * axis + (side == ">"))
    q = np.array([(18, 16, 20), (23, 20, 25), (15, 21, 17)])
    c0 = int(q[0, axis])
    q[:, axis] = c0
    mask = axis_mask(axis, side, c0 + 2 if side == "<" else c0 - 2)
    D = 2 * r + 1
    return mask, q.astype(np.int32), perturbed(truth(q), rng), (r + 1) * D * D


def run_options(r, max_it, interp):
    return dict(subset_radius=r, max_iterations=max_it, tolerance=0.0, interpolation=interp)


# ---- status 7 and 4 -------------------------------------------------------------------------------------------------------------

STATUS_R, STATUS_Q = 6, np.array([[20, 18, 22]], np.int32)


def status_masks():
    """r = 6 at one POI: the half-space mask x < qx + 2 (n = 7 * 169 = 1183 active voxels); the same with the margin voxel
    (qx - r - 1, qy, qz) masked out, which costs the cube exactly its voxel (qx - r, qy, qz); a float min_fraction with
    n - 1 < min_fraction * N <= n; a box with 11 active voxels in the plane dx = 0 (H[1][1] = 0 exactly: status 4); a box with one
    (dR = 0: status 4); the empty mask (status 7)"""
    r, (qx, qy, qz) = STATUS_R, STATUS_Q[0]
    N = (2 * r + 1) ** 3
    full = axis_mask(0, "<", qx + 2)
    n = (r + 1) * (2 * r + 1) ** 2
    less = full.copy()
    less[qz, qy, qx - r - 1] = 0
    mf = np.float32((n - 0.5) / N)
    assert not float(n) < float(mf) * float(N) and float(n - 1) < float(mf) * float(N)
    eleven = np.zeros((NZ, NY, NX), np.uint8)
    eleven[qz - 1:qz + 2, qy - 6:qy + 7, qx - 1:qx + 2] = 1
    one = np.zeros((NZ, NY, NX), np.uint8)
    one[qz, qy, qx] = 1
    one[qz, qy, [qx - 1, qx + 1]] = 1
    one[qz, [qy - 1, qy + 1], qx] = 1
    one[[qz - 1, qz + 1], qy, qx] = 1
    return dict(full=full, less=less, n=n, min_fraction=float(mf), eleven=eleven, one=one, empty=np.zeros((NZ, NY, NX), np.uint8))


# ---- one masked-out voxel per sentinel of the walk --------------------------------------------------------------------------------

SENTINEL_R = (2, 3, 6)
SENTINEL_Q = np.array([[19, 17, 23]], np.int32)


def sentinel_case(r, i):
    """the mask that is 1 but at the subset voxel of linear index i (x fastest) of SENTINEL_Q, and R with a NaN there"""
    R = volumes()[0].copy()
    D = 2 * r + 1
    dx, dy, dz = i % D - r, (i // D) % D - r, i // (D * D) - r
    x, y, z = SENTINEL_Q[0] + (dx, dy, dz)
    mask = np.ones((NZ, NY, NX), np.uint8)
    mask[z, y, x] = 0
    R[z, y, x] = np.nan
    return R, mask
