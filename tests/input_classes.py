"""Deterministic volumes of the value classes real CT / MR data carries and the synthetic blob volumes do not: signed
intensities, exactly-zero and constant backgrounds (subnormal Gaussian tails, plateau ties under the strict extremum
comparisons), integer-quantised data, hot voxels, subnormal and near-overflow input, NaN / Inf background.

TEST INFRASTRUCTURE ONLY.  3dsift_amd/synth.py stays untouched (bench and the goldens depend on its stream); everything here is
derived from its volumes or from numpy's PCG64 in a fixed order.  tests/test_input_classes_cpu.py proves on the oracle alone
that every class really contains what it is named for; tests/test_gpu_input_classes.py runs them through the HIP path.
"""
import importlib

import numpy as np

synth = importlib.import_module("3dsift_amd.synth")

SHAPES = {"a": (64, 72, 80),   # four octaves: 80x72x64, 40x36x32 and the two one-workgroup octaves 20x18x16, 10x9x8
          "b": (45, 51, 70)}   # non-cubic, odd, not tile aligned; three octaves
SEED = 5


def base(shape):
    """today's kind: blobs that blanket the volume plus U[0, 0.01)"""
    return synth.blobs(shape, seed=SEED, noise=0.01)


def _centre(shape):
    return tuple(n // 2 for n in shape)


def negated(shape):
    return -base(shape)


def offset(shape):
    return base(shape) - np.float32(0.7)


def negdom(shape):
    """negative-dominant: max|v| is taken from a negative voxel"""
    return base(shape) - np.float32(3.0)


def sparse(shape):
    """three blobs on exact zero: the Gaussian tails of the pyramid run down through the subnormals to zero"""
    return synth.blobs(shape, seed=SEED, nblobs=3)


def box(shape):
    v = np.zeros(shape, np.float32)
    cz, cy, cx = _centre(shape)
    v[cz:cz + 3, cy:cy + 5, cx:cx + 4] = 1.0
    return v


def _hot(shape, value):
    v = base(shape)
    cz, cy, cx = _centre(shape)
    v[cz + 3, cy - 5, cx + 7] = value
    return v


def hot1e30(shape):
    return _hot(shape, np.float32(1e30))


def hot3e38(shape):
    """everything else is divided down to ~1e-38: a pyramid of subnormals around one spike"""
    return _hot(shape, np.float32(3e38))


def masked(shape):
    """blobs + noise with the background (values below 0.25) set to exact zero: plateau ties next to real structure"""
    v = synth.blobs(shape, seed=SEED, noise=0.05)
    v[v < 0.25] = 0.0
    return v


def steps(shape):
    """piecewise constant, plateaus wider than the widest Gaussian kernel: a staircase along x, one along y, one step in z"""
    nz, ny, nx = shape
    z, y, x = np.ogrid[0:nz, 0:ny, 0:nx]
    return ((x // 27) % 3 + 2 * ((y // 24) % 2) + 3 * (z >= nz // 2)).astype(np.float32)


def quantised(shape):
    return np.round(np.float32(40.0) * base(shape)).astype(np.float32)


def tiny(shape):
    """subnormal and barely normal INPUT through data_scale's division"""
    return base(shape) * np.float32(1e-38)


def huge(shape):
    return base(shape) * np.float32(1e38)


def mixed(shape):
    """the subnormal class that also has keypoints: 60 small, sharp, anisotropic blobs on exact zero, their tails NOT cut (the
    volume of test_descriptor_sparse_volume_coarse_estimate without its 1e-3 threshold)"""
    nz, ny, nx = shape
    rng = np.random.Generator(np.random.PCG64(SEED))
    vol = np.zeros(shape, np.float32)
    zz, yy, xx = np.mgrid[0:nz, 0:ny, 0:nx].astype(np.float32)
    for _ in range(60):
        c = rng.uniform(0.15, 0.85, 3) * np.array(shape); s = rng.uniform(1.0, 3.0, 3); a = rng.uniform(0.4, 1.0)
        vol += (a * np.exp(-0.5 * (((zz - c[0]) / s[0]) ** 2 + ((yy - c[1]) / s[1]) ** 2 + ((xx - c[2]) / s[2]) ** 2))).astype(np.float32)
    return vol


# The non-finite classes sit on the masked volume: it keeps tens of keypoints outside the region a NaN poisons (every level
# spreads it by the kernel's half width; the two smallest octaves are NaN throughout), some with a NaN inside their descriptor
# window and some without.
def nan_voxel(shape):
    v = masked(shape)
    cz, cy, cx = _centre(shape)
    v[cz, cy, cx] = np.nan
    return v


def nan_slab(shape):
    """NaN background in the leading planes (0..7 of 64)"""
    v = masked(shape)
    v[:shape[0] // 8] = np.nan
    return v


def nan_block(shape):
    """an interior block of NaN"""
    v = masked(shape)
    cz, cy, cx = _centre(shape)
    v[cz - 2:cz + 2, cy - 4:cy, cx + 2:cx + 6] = np.nan
    return v


def nan_corner(shape):
    v = masked(shape)
    v[-1, -1, -1] = np.nan
    v[0, 0, 0] = np.nan
    return v


def pos_inf(shape):
    """Inf / Inf = NaN at the voxel, every other voxel becomes +-0"""
    v = masked(shape)
    cz, cy, cx = _centre(shape)
    v[cz, cy, cx] = np.inf
    return v


def neg_inf(shape):
    v = masked(shape)
    cz, cy, cx = _centre(shape)
    v[cz - 2, cy + 3, cx - 4] = -np.inf
    return v


SIGNED = ("negated", "offset", "negdom")
SUBNORMAL = ("sparse", "box", "hot3e38", "mixed")
TIES = ("masked", "steps")
NAN = ("nan_voxel", "nan_slab", "nan_block", "nan_corner")
INF = ("pos_inf", "neg_inf")
NONFINITE = NAN + INF
FINITE = SIGNED + ("sparse", "box", "hot1e30", "hot3e38", "masked", "steps", "quantised", "tiny", "huge", "mixed")
ALL = FINITE + NONFINITE

# every class at the four-octave shape; the odd three-octave shape for one class of each kind
CASES = [(name, "a") for name in ALL] + [(name, "b") for name in ("negdom", "mixed", "masked", "quantised", "nan_slab", "nan_block", "pos_inf")]
CASE_IDS = [f"{name}-{s}" for name, s in CASES]


def make(name, shape_key="a"):
    v = globals()[name](SHAPES[shape_key])
    assert v.dtype == np.float32 and v.shape == SHAPES[shape_key]
    return v
