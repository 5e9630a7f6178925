"""CPU tests: our restatement against what the untouched reference produced on fresh seeded inputs (beyond the other goldens).
The reference's results are stored in tests/golden/g11_vs_ref.npz (tests/golden/make_golden.py g11): level hashes, extrema,
keypoints, descriptors and matcher outputs, compared bit for bit."""
import hashlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from make_golden import G11_MATCH, G11_PIPELINE, G11_WIDE, g11_level_hashes  # noqa: E402

from conftest import golden  # noqa: E402


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


@pytest.fixture(scope="module")
def g11():
    return golden("g11_vs_ref.npz")


def check_hashes(got, want):
    assert len(got) == len(want)
    for h, w in zip(got, want):
        assert h == w, h.split(":")[0]


@pytest.mark.parametrize("shape,seed,noise", G11_PIPELINE)
def test_full_pipeline_matches_reference(orc, synth, g11, shape, seed, noise):
    p = f"p{G11_PIPELINE.index((shape, seed, noise))}_"
    vol = synth.blobs(shape, seed=seed, noise=noise)
    assert sha(vol) == str(g11[p + "vol_sha"])
    b = orc.extractor(vol).run(5)
    assert b.num_octaves == int(g11[p + "noct"])
    # every Gaussian / DoG level (the [1:-1]^3 interior of the last level of an octave of <= 9 voxels: the reference reads out of
    # bounds there)
    check_hashes(g11_level_hashes(b, b.num_octaves, 6, 5, crop=True), g11[p + "hashes"])
    ea, eb = g11[p + "extrema"], b.extrema()
    assert len(ea) == len(eb)
    for f in ("x", "y", "z", "scale", "octave", "level"):
        assert np.array_equal(ea[f], eb[f]), f
    ka, da_ = g11[p + "kp"], g11[p + "desc"]
    kb, db_ = b.keypoints()
    assert len(ka) == len(kb)
    for f in ("x", "y", "z", "scale", "octave", "level", "rx", "ry", "rz", "win", "eigvalue", "Rotation", "str_tensor"):
        assert np.array_equal(ka[f], kb[f]), f
    assert np.array_equal(bits(da_), bits(db_))


def test_wide_kernels_match_reference(orc, synth, g11):
    """num_kp_levels = 1 with a wide sigma: Gaussian kernels of up to 89 taps (the product accepts up to 129 since late r04; the
    restatement had a 64-tap buffer).  Octaves 0 and 1 (lines of at least 48 voxels): pyramid, extrema and keypoints of the restatement
    against the untouched reference.  From octave 2 on the kernel (hw 44) is wider than the line and the reference reads out of bounds
    -- undefined there, like its 8^3 octaves with the default parameters -- so those octaves are not compared."""
    w = G11_WIDE
    vol = synth.blobs(w["shape"], seed=w["seed"], noise=w["noise"])
    assert sha(vol) == str(g11["w_vol_sha"])
    b = orc.extractor(vol, **w["params"]).run(5)
    assert b.num_octaves == int(g11["w_noct"]) and b.num_octaves >= 2
    check_hashes(g11_level_hashes(b, 2, 4, 3, crop=False), g11["w_hashes"])
    ea, eb = g11["w_extrema"], b.extrema()
    eb = eb[eb["octave"] < 2]
    assert len(ea) == len(eb) and len(ea) > 0
    for f in ("x", "y", "z", "scale", "octave", "level"):
        assert np.array_equal(ea[f], eb[f]), f
    ka, da_ = g11["w_kp"], g11["w_desc"]
    kb, db_ = b.keypoints()
    mb = kb["octave"] < 2
    kb, db_ = kb[mb], db_[mb]
    assert len(ka) == len(kb)
    for f in ("x", "y", "z", "scale", "octave", "level", "rx", "ry", "rz", "win", "eigvalue", "Rotation", "str_tensor"):
        assert np.array_equal(ka[f], kb[f]), f
    assert np.array_equal(bits(da_), bits(db_))


def test_matcher_matches_reference(orc, synth, g11):
    m = G11_MATCH
    va = synth.blobs(m["shape"], seed=m["seed"])
    vb = synth.blobs(m["shape"], seed=m["seed"], shift=m["shift"])
    ka, da = orc.extractor(va).run(5).keypoints()
    kb, db = orc.extractor(vb).run(5).keypoints()
    xa = np.stack([ka["rx"], ka["ry"], ka["rz"]], 1)
    xb = np.stack([kb["rx"], kb["ry"], kb["rz"]], 1)
    assert len(ka) > 5 and len(kb) > 5
    # the descriptor sets the reference matched are the restatement's of these volumes
    for got, key in ((da, "m_da"), (xa, "m_xa"), (db, "m_db"), (xb, "m_xb")):
        assert np.array_equal(bits(got), bits(g11[key])), key
    for mode in m["modes"]:
        for thr in m["thresholds"]:
            o = orc.match(da, xa, db, xb, thr, mode)
            pre = f"m_m{mode}_t{int(round(thr * 100))}_"
            keys = [k[len(pre):] for k in g11.files if k.startswith(pre)]
            assert keys
            for k in keys:
                assert np.array_equal(g11[pre + k], o[k]), (mode, thr, k)


# ---- the value classes of tests/input_classes.py on the reference itself, where oracle/_ref/libref3dsift.so was built -------------
import input_classes as ic  # noqa: E402
import oracle_lib as ol  # noqa: E402
from hipcheck import nan_equal_bits  # noqa: E402

needs_ref = pytest.mark.skipif(not ol.available("ref"), reason="oracle/_ref/libref3dsift.so is built only where the reference tree exists")


@needs_ref
@pytest.mark.parametrize("name", ["mixed", "masked", "steps", "negdom", "hot3e38", "nan_slab", "nan_voxel", "nan_block", "nan_corner", "pos_inf", "neg_inf"])
def test_input_classes_match_the_reference(orc, name):
    """One subnormal class with keypoints (mixed) and one without (hot3e38), the tie-heavy ones, a signed one and EVERY non-finite class
    through the untouched reference and the restatement: every level (NaN positions as a mask, everything else by bits; the shell of the
    last level of an octave of <= 9 voxels is cropped as in g11), extrema, keypoint records and descriptors bit for bit.

    The reference survives NaN and Inf input and its result does not depend on the thread count (run here on 1 and 7 threads).  Two
    things it does there, both restated:
      * its interior convolution term is tap * (1 * src[p - d] + 0 * src[p - d + 1]) (Src/cSIFT3D.cc:701-708): a non-finite voxel
        spreads one voxel further towards the low end of every axis than the taps reach.  The restatement used tap * src[p - d],
        which is the same bits on finite data only, and disagreed on nan_voxel / nan_block / nan_corner / the Inf classes (91 voxels
        of level 0 on nan_voxel, 275 instead of 312 extrema) until it took the reference's form for volumes that hold a non-finite voxel.
      * a descriptor window with a NaN sample ends as the CONSTANT row, never a NaN row: the truncation at Src/cSIFT3D.cc:1355
        replaces NaN by the threshold."""
    vol = ic.make(name)
    ref = ol.load("ref")
    b = orc.extractor(vol).run(5)
    eb = b.extrema()
    kb, db_ = b.keypoints()
    try:
        for threads in (1, 7):
            ref.set_threads(threads)
            a = ref.extractor(vol).run(5)
            assert a.num_octaves == b.num_octaves
            assert nan_equal_bits(a.input(), b.input()) == 0
            for o in range(a.num_octaves):
                for kind, n, ga, gb in (("gss", 6, a.gss, b.gss), ("dog", 5, a.dog, b.dog)):
                    for i in range(n):
                        x, y = ga(o, i), gb(o, i)
                        if min(x.shape) <= 9 and i == n - 1:
                            x, y = x[1:-1, 1:-1, 1:-1], y[1:-1, 1:-1, 1:-1]
                        assert nan_equal_bits(x, y) == 0, (kind, o, i, threads)
            ea = a.extrema()
            assert len(ea) == len(eb)
            for f in ("x", "y", "z", "scale", "octave", "level"):
                assert np.array_equal(ea[f], eb[f]), f
            ka, da_ = a.keypoints()
            assert len(ka) == len(kb)
            for f in ("x", "y", "z", "scale", "octave", "level", "rx", "ry", "rz", "win", "eigvalue", "Rotation", "str_tensor"):
                assert np.array_equal(bits(ka[f]) if ka[f].dtype == np.float32 else ka[f], bits(kb[f]) if kb[f].dtype == np.float32 else kb[f]), f
            assert np.array_equal(bits(da_), bits(db_))
            if name in ic.NAN:
                assert (da_ == da_[:, :1]).all(axis=1).any() and not np.isnan(da_).any()
    finally:
        ref.set_threads(0)
