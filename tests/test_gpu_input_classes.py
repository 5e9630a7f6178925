"""-m gpu: the HIP path on the value classes of tests/input_classes.py (signed, sparse / box on exact zero, hot voxel, masked
background, steps, quantised, subnormal and near-overflow input, NaN voxel / slab / block / corner, +-Inf voxel) against the CPU oracle.
tests/test_input_classes_cpu.py proves, on the oracle alone, that each class holds the subnormals, ties or NaNs it is named for.

Finite classes: input, every Gaussian / DoG level, level_info and the extrema bit for bit, keypoints under hipcheck.compare_keypoints'
bars.  Non-finite classes: NaN positions as a mask and the bits of everything else (hipcheck.nan_equal_bits), the same extrema and
keypoints in the same order, descriptor rows under the usual bars wherever the oracle's row is finite -- which includes the constant
row the reference's truncation makes of a NaN histogram (tests/test_input_classes_cpu.py)."""
import contextlib
import hashlib
import importlib

import numpy as np
import pytest

import detect_full_ref as dref
import input_classes as ic
from hipcheck import (bits, compare_keypoints, compare_keypoints_nonfinite, compare_pyramids, compare_pyramids_nan, extrema_table,
                      nan_equal_bits)

pytestmark = pytest.mark.gpu

capi = importlib.import_module("3dsift_amd.capi")

_oracle = {}


def oracle_run(orc, name, key):
    if (name, key) not in _oracle:
        o = orc.extractor(ic.make(name, key)).run(5)
        _oracle[(name, key)] = (o, o.extrema(), o.keypoints())
    return _oracle[(name, key)]


def check_against_oracle(g, name, orc_run):
    o, oext, (okp, odesc) = orc_run
    finite = name in ic.FINITE
    if finite:
        assert np.array_equal(bits(g.input()), bits(o.input()))
        compare_pyramids(g, o)
    else:
        assert nan_equal_bits(g.input(), o.input()) == 0
        compare_pyramids_nan(g, o)
    assert np.array_equal(extrema_table(g.extrema()), extrema_table(oext)), (len(g.extrema()), len(oext))
    kp, desc = g.GetKeypoints()
    if finite:
        compare_keypoints(kp, desc, okp, odesc)
    else:
        compare_keypoints_nonfinite(kp, desc, okp, odesc)
    return kp, desc


def full_hash(g):
    """extrema, keypoints, descriptors and every DoG level of a run (NaN payloads included: one device, one arithmetic)"""
    h = hashlib.sha1()
    kp, d = g.GetKeypoints()
    h.update(np.ascontiguousarray(g.extrema()).tobytes()); h.update(kp.tobytes()); h.update(d.tobytes())
    for o in range(g.num_octaves):
        for i in range(5):
            h.update(np.isnan(g.dog(o, i)).tobytes()); h.update(np.nan_to_num(g.dog(o, i), nan=0.0).tobytes())
    return h.hexdigest()


@pytest.mark.parametrize("name,key", ic.CASES, ids=ic.CASE_IDS)
def test_pipeline_vs_oracle(orc, name, key):
    g = capi.CreateCSIFT3D(ic.make(name, key)).KpSiftAlgorithm()
    kp, _ = check_against_oracle(g, name, oracle_run(orc, name, key))
    o = oracle_run(orc, name, key)[0]
    for idx in range(g.num_octaves * 5):
        assert g.level_info(1, idx) == o.level_info(1, idx), idx
    if name in ("mixed", "masked") + ic.NAN and key == "a":
        assert len(kp) >= 20   # (the CPU test's conditions: these classes are compared on real keypoints)


FORMS = {
    "eager": dict(dog_eager=1, glast_eager=1),       # every DoG and Gaussian level written: no lazily formed values in the extremum test
    "separable": dict(separable=1),                  # the generic three-pass kernels for every level
    "wide_tiles": dict(march_tiles=1),               # 64 x 32 tiles wherever the geometry allows
    "narrow_tiles_eager": dict(march_tiles=2, dog_eager=1, glast_eager=1),
}


# A volume with a non-finite voxel takes the generic kernels for every level whatever the hooks say (sift3d_create): the tile and
# separable hooks select nothing there, only the eager DoG levels are a path of their own.
FORM_CASES = [(name, form) for name in ic.ALL for form in FORMS if name in ic.FINITE or form == "eager"]


@pytest.mark.parametrize("name,form", FORM_CASES, ids=[f"{n}-{f}" for n, f in FORM_CASES])
def test_forms_vs_oracle(orc, name, form):
    """the forms with arithmetic paths of their own: each against the oracle, and bit for bit the plain run"""
    vol = ic.make(name, "a")
    plain = full_hash(capi.CreateCSIFT3D(vol).KpSiftAlgorithm())
    with contextlib.ExitStack() as st:
        for h, v in FORMS[form].items():
            st.enter_context(capi.hook(h, v))
        g = capi.CreateCSIFT3D(vol).KpSiftAlgorithm()
        check_against_oracle(g, name, oracle_run(orc, name, "a"))
        assert full_hash(g) == plain


def _table64(e):
    return np.stack([e["octave"], e["level"], e["x"].astype(np.int64), e["y"].astype(np.int64), e["z"].astype(np.int64)], 1).astype(np.int64)


@pytest.mark.parametrize("neighbours,refine", [(80, False), (8, True), (80, True)])
@pytest.mark.parametrize("name", ["masked", "steps", "mixed", "sparse", "hot3e38", "nan_voxel", "nan_block", "nan_slab"])
def test_detect_options_vs_restatement_on_the_oracle_dog(orc, name, neighbours, refine):
    """the opt-in 80-neighbour scan and the sub-voxel refinement (kernels_detect_full.hip) on ties, subnormals and NaN: the CPU
    restatement tests/detect_full_ref.py applied to the ORACLE's DoG levels"""
    vol = ic.make(name, "a")
    o = oracle_run(orc, name, "a")[0]
    dogs = [[o.dog(oc, i) for i in range(5)] for oc in range(o.num_octaves)]
    g = capi.CSIFT3D(vol).set_detect_options(neighbours=neighbours, refine=refine).KpSiftAlgorithm()
    rows = dref.extrema_table(dogs, 0.1, neighbours)
    want = dref.refined_table(dogs, rows, 0.1, neighbours, dict(max_offset=0.5)) if refine else rows
    got = _table64(g.extrema())
    assert np.array_equal(got, np.asarray(want).reshape(-1, 5)), (len(got), len(want))


SHARDED = ["mixed", "negdom", "nan_slab"]


def _single(vol):
    g = capi.CreateCSIFT3D(vol).KpSiftAlgorithm()
    return g.GetKeypoints()


@pytest.mark.parametrize("partial", [False, True], ids=["whole_windows", "partial_windows"])
@pytest.mark.parametrize("name", SHARDED)
def test_native_sharded_equals_single_volume(name, partial):
    """two simulated ranks: the slabs' abs-max merge and scale, the dogmax exchange, the partial integer histograms"""
    vol = ic.make(name, "a")
    kp, ds = _single(vol)
    assert len(kp) >= 20
    sh = capi.ShardedCSIFT3D(vol, devices=(0,), sim_ranks=2, sharded_octaves=1, partial_windows=partial)
    assert sh.info()["partial_windows"] == partial
    k2, d2 = sh.KpSiftAlgorithm().GetKeypoints()
    sh.close()
    assert np.array_equal(k2.view(np.uint8), kp.view(np.uint8)) and np.array_equal(bits(d2), bits(ds))


@pytest.mark.parametrize("name", SHARDED)
def test_python_slab_driver_equals_single_volume(name):
    slab = importlib.import_module("3dsift_amd.slab")
    vol = ic.make(name, "a")
    nz, ny, nx = vol.shape
    kp, ds = _single(vol)
    ex = slab.SlabExtractor((nx, ny, nz), slab.SimComm(2), sharded_octaves=1)
    ex.load(volume=vol)
    ex.KpSiftAlgorithm()
    k2, d2 = ex.GetKeypoints()
    ex.close()
    assert len(k2) == len(kp)
    for f in kp.dtype.names:
        assert np.array_equal(bits(k2[f]) if k2[f].dtype == np.float32 else k2[f], bits(kp[f]) if kp[f].dtype == np.float32 else kp[f]), f
    assert np.array_equal(bits(d2), bits(ds))


def _arrays(orc):
    """a subnormal-rich and a NaN-bearing array: a Gaussian level of the sparse volume, and a block with NaN, Inf and -0"""
    o = orc.extractor(ic.make("sparse", "b")).run(2)
    sub = o.gss(0, 4)
    assert int(((np.abs(sub) < np.float32(1.17549435e-38)) & (sub != 0)).sum()) > 500
    rng = np.random.default_rng(17)
    nan = rng.standard_normal((21, 26, 37)).astype(np.float32)
    nan[10, 13, 18] = np.nan; nan[3, 3, 30] = np.inf; nan[17, 20, 5] = -np.inf; nan[0, 0, 0] = np.nan; nan[5, 5, 5] = -0.0
    return {"subnormal": sub, "nan": nan}


@pytest.mark.parametrize("which", ["subnormal", "nan"])
def test_free_functions(orc, which):
    from test_gpu_free_functions import _line_rule

    v = _arrays(orc)[which]
    for sigma in (0.9733, 2.452547):
        assert nan_equal_bits(capi.gaussian_smooth(v, sigma), orc.gaussian_smooth(v, sigma)) == 0, sigma
    small = np.ascontiguousarray(v[:9, :12, :20])
    w = np.random.default_rng(3).uniform(-0.5, 1.0, 5).astype(np.float32)
    for dim in range(3):
        with np.errstate(all="ignore"):
            want = np.apply_along_axis(_line_rule, 2 - dim, small, w)
        assert nan_equal_bits(capi.conv_axis(small, dim, w), want) == 0, dim
    other = np.roll(v, 3, axis=2) * np.float32(0.75)
    with np.errstate(all="ignore"):
        assert nan_equal_bits(capi.dog_sub(v, other), (other - v) * np.float32(-1.0)) == 0
    half = tuple(s // 2 for s in v.shape)
    assert nan_equal_bits(capi.downsample(v), v[::2, ::2, ::2][:half[0], :half[1], :half[2]]) == 0


@pytest.mark.parametrize("name", ["nan_slab", "nan_block"])
def test_matcher_on_descriptors_of_a_nan_volume(orc, name):
    """descriptors of a NaN volume and of its copy shifted by one voxel in x (constant rows of NaN windows among them): modes 1-3"""
    va = ic.make(name, "a")
    vb = np.roll(va, 1, axis=2)
    out = []
    for v in (va, vb):
        kp, desc = capi.CreateCSIFT3D(v).KpSiftAlgorithm().GetKeypoints()
        assert len(kp) >= 20 and np.isfinite(desc).all()
        out.append((desc, np.stack([kp["rx"], kp["ry"], kp["rz"]], 1)))
    (da, xa), (db, xb) = out
    assert (da == da[:, :1]).all(axis=1).any(), "no constant row: the NaN windows are not exercised"
    m = capi.muBruteMatcher()
    for mode, fn in ((1, m.injectMatch), (2, m.bijectMatch), (3, m.enhancedMatch)):
        got = fn(da, xa, db, xb, 0.85)
        want = orc.match(da, xa, db, xb, 0.85, mode)
        for k in want:
            assert np.array_equal(got[k], want[k]), (mode, k)
