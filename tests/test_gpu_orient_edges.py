"""-m gpu: sift3d_orient_keypoint on the planted keypoints of tests/kp_cases.py -- every border position, every window size and path of
k_orient, every code, every threshold from both sides, hostile voxel values in and around the window, 32 amplitudes -- one call each against
the oracle's orient_one (tests/test_kp_cases_cpu.py asserts on the oracle that the cases do what they claim).

The code always equals the oracle's.  Accepted keypoints: str_tensor, win, eigvalue and Rotation bit for bit (the r03 contract).  Rejected
keypoints keep the parallel (FMA, butterfly) sums of the screening pass: every component of str_tensor and win is compared with the fp64
sum of the same fp32 terms (kp_cases.orient_sums) as |got - f64| / sum |term|.  The oracle's own sequential fp32 sums measure 4.162e-5 in
that quantity (largest over the 1937 orientation cases of the module, at the radius-20 window: 33 000 terms added one after the other;
tests/test_kp_cases_cpu.py::test_fp64_bar_of_the_sequential_sums prints and asserts it); both are orderings of the same terms under one
n eps sum |term| bound, the bar here is 4x that: 1.668e-4 (kp_cases.FP64_BAR).  Records poisoned by NaN / Inf are compared by pattern."""
import importlib

import numpy as np
import pytest

import kp_cases as K
from hipcheck import bits, nan_equal_bits

pytestmark = pytest.mark.gpu

FIELDS = ("str_tensor", "win", "eigvalue", "Rotation")


@pytest.fixture(scope="module")
def capi():
    m = importlib.import_module("3dsift_amd.capi")
    assert m.device_count() >= 1, "GPU tests need a visible MI355X (no CPU fallback exists)"
    return m


def _call(capi, c):
    sigma, mer, ct = c.args
    rec = np.array([c.rec], dtype=capi.KP_DTYPE)
    code = capi.orient_keypoint(c.level, c.unit, rec, sigma, mer, ct)
    return code, rec[0]


def _pattern(a):
    a = np.asarray(a, np.float32)
    return np.isnan(a), np.isposinf(a), np.isneginf(a)


def _mismatch(orc, c, got, rec):
    """None, or what is wrong with the call's result"""
    want, ko = K.oracle_orient(orc, c)
    if got != want:
        return "code %d, oracle %d" % (got, want)
    st = rec["str_tensor"]
    if not (bits(st[3]) == bits(st[1]) and bits(st[6]) == bits(st[2]) and bits(st[7]) == bits(st[5])):
        return "str_tensor is not symmetric"
    if want == 1:
        for f in FIELDS:
            if nan_equal_bits(rec[f], ko[f]):
                return "%s differs from the oracle's in %d elements" % (f, nan_equal_bits(rec[f], ko[f]))
        return None
    q = K.sum_ratio(rec, *K.orient_sums(c.level, c.unit, c.rec, c.args[0]))
    if q is None:
        for a, b in zip(_pattern(K.record_sums(rec)), _pattern(K.record_sums(ko))):
            if not np.array_equal(a, b):
                return "non-finite pattern %s, oracle %s" % (K.record_sums(rec), K.record_sums(ko))
        return None
    return None if q <= K.FP64_BAR else "window sums off the fp64 sums by %.3g of sum |term| (bar %.3g)" % (q, K.FP64_BAR)


def _run(capi, orc, cases):
    bad, results, worst = [], {}, 0.0
    for c in K.by_tables(cases):
        got, rec = _call(capi, c)
        results[c.name] = (got, rec)
        m = _mismatch(orc, c, got, rec)
        if m:
            bad.append((c.name, m))
        if got != 1:
            worst = max(worst, K.sum_ratio(rec, *K.orient_sums(c.level, c.unit, c.rec, c.args[0])) or 0.0)
    print("%d cases, %d wrong; rejected keypoints: window sums within %.3g of the fp64 sums (bar %.3g)" % (len(cases), len(bad), worst, K.FP64_BAR))
    for b in bad:
        print("  ", *b)
    assert not bad, (len(bad), len(cases), bad[:12])
    return results


@pytest.mark.parametrize("unit", K.UNITS)
def test_border_positions(capi, orc, unit):
    """distance 0 .. R + 1 from each face, corners and edge midpoints, on a 52 x 44 x 48 and a 45 x 37 x 41 level (no row a multiple of
    four; on the device the tile pieces start at the alignment of the box the entry cuts out: widths 11 .. 21, every residue modulo 4),
    the level taken as octave log2(unit)'s"""
    _run(capi, orc, K.orient_border(orc, unit))


@pytest.mark.parametrize("unit", K.UNITS)
def test_window_sizes(capi, orc, unit):
    """3 sigma just under and just over every integer radius 1 .. 20, central and two voxels from the x, y and z face"""
    _run(capi, orc, K.orient_sizes(orc, unit))


def test_tile_limits_and_paths(capi, orc):
    """clipped footprints of exactly 28 x 27 (the LDS tile: list and box scan), 29 x 27, 28 x 28, 27 x 28 (global loads), and a small
    footprint whose weight table is too long for its LDS copy"""
    _run(capi, orc, K.orient_tiles(orc))


def test_every_code(capi, orc):
    """constant level, pure ramps (rank-one tensor: the two small eigenvalues are rounding noise of either sign), near-isotropic blobs,
    and a grid over L0"""
    res = _run(capi, orc, K.orient_codes(orc))
    assert {r[0] for r in res.values()} == {-1, -2, -3, 1}


def test_thresholds_from_both_sides(capi, orc):
    """max_eig_ratio at the fp32 float below, at and above max(r01, r12); corner_thresh likewise around the corner cosine; the level scaled
    by two adjacent floats between which |mean gradient|^2 crosses 1e-10.  Twice: identical bytes."""
    ratio, corner = K.orient_straddles(orc)
    cases = ratio + corner
    for weak, strong, _, _ in K.orient_gg_straddles(orc):
        cases += [weak, strong]
    first = _run(capi, orc, cases)
    second = _run(capi, orc, cases)
    for n in first:
        assert first[n][0] == second[n][0] and first[n][1].tobytes() == second[n][1].tobytes(), n
    assert [first[c.name][0] for c in ratio] == [-2, 1, 1] * (len(ratio) // 3)
    assert [first[c.name][0] for c in corner] == [1, 1, -3] * (len(corner) // 3)


def test_voxel_values_in_and_around_the_window(capi, orc):
    """NaN, +Inf and 3e38 at (a) the corner of the window's box, (b) the voxel behind the sphere's pole, (c) the centre, (d) the three floats
    the last 16-byte piece of a tile row reads behind column tw - 1 -- in the box the entry copies to the device these are columns 0 .. 2
    of the next box row, or of the next plane's first row (kp_cases.orient_plants): (a) and (d) leave the result bit-identical to the
    unplanted call"""
    plants = K.orient_plants(orc)
    res = _run(capi, orc, [c for _, c, _ in plants] + list({b.name: b for _, _, b in plants}.values()))
    for kind, c, base in plants:
        same = res[c.name][0] == res[base.name][0] and res[c.name][1].tobytes() == res[base.name][1].tobytes()
        assert same == (kind in "ad"), (c.name, res[c.name][0], res[base.name][0])


def test_amplitude(capi, orc):
    """L0 2^e, e = -24 .. -1 and -126, -60, -40, 4, 10, 20, 40, 60: the oracle runs on every scaled level"""
    _run(capi, orc, K.orient_amplitude(orc))
