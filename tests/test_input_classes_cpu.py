"""CPU test: every generator of tests/input_classes.py proves its class ON THE ORACLE ALONE.  A GPU parity test can only catch a
subnormal, tie or NaN bug if the oracle's own result contains subnormals, ties or NaNs; the conditions below are what
tests/test_gpu_input_classes.py relies on.  Counts at (64, 72, 80), measured on the oracle (docs/experiments.md has the table):

  class       extrema / keypoints   subnormal pyramid values   exact-zero DoG voxels   NaN pyramid values
  sparse           3 / 0                   15 036                   740 051
  box              0 / 0                    3 790                 1 545 923
  hot3e38          0 / 0                3 664 768                       118
  mixed          181 / 30                   5 638                       318
  masked         629 / 81                       0                   106 578
  steps           27 / 0                        0                   127 509
  nan_voxel      275 / 40 (16)                                      106 098               1 226 687
  nan_slab       268 / 39 (29)                                       87 426               1 813 680
  nan_block      245 / 40 (25)                                      105 626               1 347 031
  nan_corner     448 / 56 (11)                                      104 028                 521 938
  (in brackets: keypoints whose descriptor window holds a NaN)

WHAT THE REFERENCE DOES WITH A NaN IN A DESCRIPTOR WINDOW.  A NaN gradient sample passes every rejection of the face lookup (all its
comparisons are false) and lands in the histogram, the first normalisation spreads it over the row -- and the truncation
`desc[i] = desc[i] < trunc_thresh ? desc[i] : trunc_thresh` (reference Src/cSIFT3D.cc:1355) then replaces every NaN by the
threshold.  The final row is the CONSTANT row (fl(1 / sqrt(768)) everywhere): finite, identical for every such keypoint, and never
NaN.  So no volume can give "a keypoint whose descriptor row has a NaN"; the condition that can be asserted, and is, is a
keypoint with the constant row beside keypoints with ordinary rows.  tests/test_oracle_vs_ref.py pins the same rows on the
untouched reference."""
import numpy as np
import pytest

import input_classes as ic

FLT_MIN = np.float32(1.17549435e-38)


def levels(o):
    for oc in range(o.num_octaves):
        for i in range(6):
            yield oc, "gss", i, o.gss(oc, i)
        for i in range(5):
            yield oc, "dog", i, o.dog(oc, i)


def pyramid_stats(o):
    sub = zero = 0
    nan = [0] * o.num_octaves
    for oc, kind, _, a in levels(o):
        sub += int(((np.abs(a) < FLT_MIN) & (a != 0)).sum())
        nan[oc] += int(np.isnan(a).sum())
        if kind == "dog":
            zero += int((a == 0).sum())
    return sub, zero, nan


def constant_rows(desc):
    """rows the reference's truncation made out of a NaN histogram: every element the same value"""
    return (desc == desc[:, :1]).all(axis=1) if len(desc) else np.zeros(0, bool)


def run(orc, name, key="a"):
    o = orc.extractor(ic.make(name, key)).run(5)
    kp, desc = o.keypoints()
    return o, o.extrema(), kp, desc


def test_generators_are_deterministic_and_cover_every_class():
    assert set(n for n, _ in ic.CASES) == set(ic.ALL) and len(set(ic.CASE_IDS)) == len(ic.CASES)
    assert any(k == "b" for _, k in ic.CASES)
    for name, key in ic.CASES:
        a, b = ic.make(name, key), ic.make(name, key)
        assert a.tobytes() == b.tobytes(), name
        assert np.isfinite(a).all() == (name in ic.FINITE), name
    assert (ic.make("negdom") < 0).all() and ic.make("offset").min() < 0 < ic.make("offset").max()
    q = ic.make("quantised")
    assert np.array_equal(q, np.round(q)) and len(np.unique(q)) > 20
    t = ic.make("tiny")
    assert int(((np.abs(t) < FLT_MIN) & (t != 0)).sum()) > 1000, "subnormal INPUT voxels"
    assert np.isfinite(ic.make("huge")).all() and ic.make("huge").max() > 1e38
    assert int(np.isnan(ic.make("nan_voxel")).sum()) == 1 and np.isnan(ic.make("nan_slab")[:8]).all()
    c = ic.make("nan_corner")
    assert np.isnan(c[0, 0, 0]) and np.isnan(c[-1, -1, -1]) and int(np.isnan(c).sum()) == 2
    assert ic.make("pos_inf").max() == np.inf and ic.make("neg_inf").min() == -np.inf


def test_shapes_reach_the_small_octave_launch(orc):
    """(64, 72, 80): four octaves, the last two of 20x18x16 and 10x9x8 voxels (kernels_small.hip takes octaves of <= 32^3)"""
    o = orc.extractor(ic.make("masked")).run(2)
    assert o.num_octaves == 4
    assert o.level_info(0, 2 * 6)[0] == (20, 18, 16) and o.level_info(0, 3 * 6)[0] == (10, 9, 8)
    assert orc.extractor(ic.make("masked", "b")).run(2).num_octaves == 3


@pytest.mark.parametrize("name", ic.SUBNORMAL)
def test_subnormal_classes_have_subnormals(orc, name):
    o, ext, kp, _ = run(orc, name)
    sub, zero, _ = pyramid_stats(o)
    print(name, "extrema", len(ext), "keypoints", len(kp), "subnormal", sub, "zero DoG", zero)
    assert sub >= 1000, sub


def test_a_subnormal_volume_has_keypoints(orc):
    """`mixed` is the one: subnormal pyramid values AND >= 100 extrema AND >= 20 keypoints"""
    o, ext, kp, desc = run(orc, "mixed")
    sub, _, _ = pyramid_stats(o)
    assert sub >= 1000 and len(ext) >= 100 and len(kp) >= 20, (sub, len(ext), len(kp))
    assert np.isfinite(desc).all()


@pytest.mark.parametrize("name", ic.TIES)
def test_tie_classes_have_exact_zero_dog_voxels(orc, name):
    o, ext, kp, _ = run(orc, name)
    _, zero, _ = pyramid_stats(o)
    print(name, "extrema", len(ext), "keypoints", len(kp), "zero DoG", zero)
    assert zero >= 100_000, zero
    if name == "masked":
        assert len(kp) >= 50, len(kp)


@pytest.mark.parametrize("name", ic.NAN)
def test_nan_classes(orc, name):
    o, ext, kp, desc = run(orc, name)
    _, _, nan = pyramid_stats(o)
    touched = constant_rows(desc)
    print(name, "extrema", len(ext), "keypoints", len(kp), "NaN per octave", nan, "constant rows", int(touched.sum()))
    assert len(ext) >= 50 and len(kp) >= 5, (len(ext), len(kp))
    assert all(n > 0 for n in nan), nan
    # the module docstring: the reference's truncation turns a NaN histogram into the constant row, never into a NaN row
    assert not np.isnan(desc).any()
    assert touched.any() and (~touched).any(), (int(touched.sum()), len(kp))
    assert np.array_equal(desc[touched], np.full((int(touched.sum()), 768), desc[touched][0, 0]))
    # 1 / sqrt(768) up to the rounding of a sequential fp32 sum of 768 equal squares (relative 768 * 2^-24 at the very most)
    assert abs(float(desc[touched][0, 0]) * 768 ** 0.5 - 1.0) < 768 * 2.0 ** -24
    for f in ("rx", "ry", "rz", "win", "eigvalue", "Rotation", "str_tensor"):
        assert np.isfinite(kp[f]).all(), f
    # a pure function of the input: the same bytes on 1, 7 and 16 threads
    want = [ext.tobytes(), kp.tobytes(), desc.tobytes()] + [a.tobytes() for _, _, _, a in levels(o)]
    try:
        for t in (1, 7, 16):
            orc.set_threads(t)
            o2, e2, k2, d2 = run(orc, name)
            got = [e2.tobytes(), k2.tobytes(), d2.tobytes()] + [a.tobytes() for _, _, _, a in levels(o2)]
            assert got == want, t
    finally:
        orc.set_threads(0)


@pytest.mark.parametrize("name", ic.INF)
def test_inf_classes(orc, name):
    """x / Inf = +-0 everywhere, Inf / Inf = NaN at the voxel: NaN around it, exact zeros beyond, nothing detected"""
    o, ext, kp, _ = run(orc, name)
    inp = o.input()
    assert int(np.isnan(inp).sum()) == 1 and (inp[~np.isnan(inp)] == 0).all()
    _, zero, nan = pyramid_stats(o)
    assert all(n > 0 for n in nan) and zero >= 100_000 and len(ext) == 0 and len(kp) == 0


def _table(e):
    return np.stack([e["octave"], e["level"], e["x"].astype(np.int32), e["y"].astype(np.int32), e["z"].astype(np.int32)], 1)


def test_signed_classes_keep_the_extrema_of_the_unsigned_source(orc):
    """Negation flips every DoG value exactly: the same extrema.  The offsets are NOT exact in fp32 (v - 0.7 rounds, the scale
    factor changes), but on this volume the extrema table is unchanged for both; verified here, on the CPU."""
    src = _table(orc.extractor(ic.base(ic.SHAPES["a"])).run(3).extrema())
    assert len(src) >= 100
    for name in ic.SIGNED:
        got = _table(orc.extractor(ic.make(name)).run(3).extrema())
        assert np.array_equal(got, src), name
    # negdom: max|v| comes from a negative voxel
    v = ic.make("negdom")
    assert np.abs(v).max() == -v.min() and orc.extractor(v).run(1).input().min() == -1.0
