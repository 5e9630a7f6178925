"""Deterministic 8 / 16-bit integer volumes for the typed-input tests (sift3d_create_typed, sift3d_volume_to_device).

TEST INFRASTRUCTURE ONLY.  The parity volumes are the blob / quantised generators of tests/input_classes.py (3dsift_amd/synth.py
underneath), scaled to each dtype's range, with the values the kernels can get wrong planted: the most negative value of a signed
type, whose |v| does not exist in the type itself, as the ONLY voxel that attains max|v|, and the largest value of an unsigned type.
tests/test_ingest_cpu.py proves on the oracle alone that each volume holds what it is named for and yields keypoints, so that
tests/test_gpu_ingest.py cannot pass vacuously.
"""
import importlib

import numpy as np

import input_classes as ic

synth = importlib.import_module("3dsift_amd.synth")

DTYPES = ("uint8", "int8", "uint16", "int16")
EXTREMES = {"uint8": (0, 255), "int8": (-128, 127), "uint16": (0, 65535), "int16": (-32768, 32767)}
CODES = {"float32": 0, "uint8": 1, "int8": 2, "uint16": 3, "int16": 4}  # SIFT3D_DT_ of include/sift3d_hip.h

# (nz, ny, nx).  "odd": an odd voxel count, no extent a multiple of anything the kernels tile by; "fused": every x / y extent of
# octave 0 is >= 33, the smallest a level may have to take the fused level kernels (S3D_FUSED_MIN_DEFAULT)
SHAPES = {"odd": (45, 51, 71), "fused": (40, 48, 64)}
MIN_KEYPOINTS = 20
SEED = 5


def _unit(shape):
    """blobs + noise in [0, 1], the quantised class's base (tests/input_classes.py) before its rounding"""
    v = ic.base(shape).astype(np.float64)
    return v / v.max()


def parity(dtype, shape_key):
    """the parity volume of a dtype: the blob volume over the dtype's whole range, rounded; signed types are centred, so that both
    signs occur, and their most negative value is planted at one voxel after everything else has been kept above it"""
    shape = SHAPES[shape_key]
    lo, hi = EXTREMES[dtype]
    u = _unit(shape)
    if lo == 0:
        v = np.round(u * hi)  # the brightest voxel is exactly `hi`
    else:
        v = np.clip(np.round(u * (hi - lo) + lo), lo + 1, hi)  # lo + 1 = -hi: |v| <= hi everywhere ...
        v[shape[0] // 3, shape[1] // 2, shape[2] // 5] = lo       # ... but here: max|v| = -lo = hi + 1, from this voxel alone
    return v.astype(dtype)


def degenerate(which):
    """volumes without any structure: data_scale's 0 / 0 and a constant"""
    if which == "zeros_u8":
        return np.zeros((9, 11, 13), np.uint8)
    if which == "const_i16":
        return np.full((9, 11, 13), -7, np.int16)
    raise KeyError(which)


def conversion_values(dtype, n, marks):
    """n values drawn over the full range of dtype (seeded), the type's two extremes written alternately to the first and last element
    and to the elements at and beside every index of `marks` (the head and tail boundaries of the kernel's access shape)"""
    lo, hi = EXTREMES[dtype]
    rng = np.random.Generator(np.random.PCG64(SEED + n))
    v = rng.integers(lo, hi + 1, size=n, dtype=np.int64)
    spots = {0, n - 1}
    for m in marks:
        spots.update((m - 1, m))
    for k, i in enumerate(sorted(s for s in spots if 0 <= s < n)):
        v[i] = (lo, hi)[k % 2]
    return v.astype(dtype)


def dvc_pair(dtype="uint16", shape=(48, 48, 48), shift=(0.4, -0.3, 0.25)):
    """reference and target of the upload-once test: the same blobs, the target shifted by a sub-voxel amount, as integers"""
    lo, hi = EXTREMES[dtype]
    ref = synth.blobs(shape, seed=SEED, noise=0.01)
    tar = synth.blobs(shape, seed=SEED, noise=0.01, shift=shift)
    top = max(ref.max(), tar.max())
    return tuple(np.round(v.astype(np.float64) / top * hi).astype(dtype) for v in (ref, tar))
