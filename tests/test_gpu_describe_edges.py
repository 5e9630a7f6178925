"""-m gpu: sift3d_describe_keypoint on the planted keypoints of tests/kp_cases.py -- every border position, rotations that put voxels
exactly on cell faces, gradients on the vertices, edges and face centres of the icosahedron, any first guess of the fixed-point unit, window
radii from a handful of voxels to 55, 32 amplitudes, hostile voxel values -- one call each against the oracle's describe_one, the rotation
passed as the orientation stage leaves it.

Bars: the project's own (hipcheck.compare_keypoints): RMS of the row <= 2e-5, every element within 1e-4; the returned rotation bit-identical
to the oracle's; rows the oracle makes constant or zero (poisoned, flat or sub-threshold windows) bit-identical.  Every case runs again under
the hooks desc_nosplit and desc_nocache (bit-identical to the default form's row: integer histograms, "bitwise reproducible whatever the
schedule") and desc_exact_cells (within the bars of the oracle; tests/test_gpu_parity.py grants that form 2e-6 to the default, not equality)."""
import importlib

import numpy as np
import pytest

import kp_cases as K
from hipcheck import bits, descriptor_errors, nan_equal_bits

pytestmark = pytest.mark.gpu

RMS_TOL, ABS_TOL = 2e-5, 1e-4


@pytest.fixture(scope="module")
def capi():
    m = importlib.import_module("3dsift_amd.capi")
    assert m.device_count() >= 1, "GPU tests need a visible MI355X (no CPU fallback exists)"
    return m


def _call(capi, c):
    rec = np.array([c.rec], dtype=capi.KP_DTYPE)
    row = capi.describe_keypoint(c.level, c.unit, rec)
    return rec[0], row


def _row_mismatch(row, want):
    if np.isnan(want).any() or (want == want[0]).all():   # poisoned, constant or zero: bit for bit (a NaN by position)
        n = nan_equal_bits(row, want)
        return "differs in %d elements from the oracle's constant / zero / NaN row (%r ..., oracle %r ...)" % (n, row[:2], want[:2]) if n else None
    if not np.isfinite(row).all():
        return "non-finite row"
    _, rms, worst = descriptor_errors(row[None], want[None])
    return None if rms <= RMS_TOL and worst <= ABS_TOL else "rms %.3g (bar %.0e), worst element %.3g (bar %.0e)" % (rms, RMS_TOL, worst, ABS_TOL)


def _mismatch(capi, orc, c, hooks=True):
    ko, want = K.oracle_describe(orc, c)
    kg, row = _call(capi, c)
    if nan_equal_bits(kg["Rotation"], ko["Rotation"]):
        return "rotation", row
    m = _row_mismatch(row, want)
    if m:
        return m, row
    if hooks:
        for h in ("desc_nosplit", "desc_nocache"):
            with capi.hook(h, 1):
                _, r2 = _call(capi, c)
            if nan_equal_bits(r2, row):
                return "%s: %d elements differ from the default form's row" % (h, nan_equal_bits(r2, row)), row
        with capi.hook("desc_exact_cells", 1):
            _, r2 = _call(capi, c)
        m = _row_mismatch(r2, want)
        if m:
            return "desc_exact_cells: " + m, row
    return None, row


def _run(capi, orc, cases, hooks=True):
    bad, rows = [], {}
    for c in K.by_tables(cases):
        m, rows[c.name] = _mismatch(capi, orc, c, hooks)
        if m:
            bad.append((c.name, m))
    print("%d cases, %d wrong" % (len(cases), len(bad)))
    for b in bad:
        print("  ", *b)
    assert not bad, (len(bad), len(cases), bad[:12])
    return rows


@pytest.mark.parametrize("unit", K.UNITS)
def test_border_positions(capi, orc, unit):
    """scale 1 (radius 14.14): distance 0 .. R + 1 from each face, corners and edge midpoints of both levels; the rotation of the oracle's
    orientation of that voxel where it accepts it, else the identity"""
    _run(capi, orc, K.describe_border(orc, unit))


def test_rotations(capi, orc):
    """the 24 proper signed permutations (offsets exactly on cell faces and centres: the kCellBand exact path, the kClipMargin cube clip),
    45 degrees about each axis, 8 random rotations; one central voxel and one three voxels from a corner"""
    _run(capi, orc, K.describe_rotations(orc))


def test_gradients_on_the_icosahedron(capi, orc):
    """ramps along the 12 vertices, 30 edge midpoints and 20 face centres (turned by the rotation) plus 1e-3 of a smooth perturbation: the
    symmetry lookup, its 6e-6 margin and the ordered scan, through the march"""
    _run(capi, orc, K.describe_icosahedron(orc))


def test_first_guess_of_the_unit_does_not_matter(capi, orc):
    """str_tensor zero, true x 2^-40, true, true x 2^40, +Inf, NaN, each with the estimate divided by 2^0, 2^20, 2^40: all 18 rows of a
    keypoint within the bars of the ONE oracle row, each again under desc_nosplit / desc_nocache (bit-identical: on the second pass the
    split form's finisher repeats the window alone) and desc_exact_cells, and the second pass ran"""
    bad, redone = [], 0
    for c, shift in K.describe_first_guess(orc):
        with capi.hook("desc_mass_shift", shift):
            _call(capi, c)
            redone += capi.describe_keypoint_second_passes()
            m, _ = _mismatch(capi, orc, c)
        if m:
            bad.append((c.name, m))
    assert not bad, bad[:12]
    assert redone >= 1


def test_window_sizes(capi, orc):
    """scale 0.3 (a handful of voxels), 1.0, 2.7 / 2.8 (either side of the table's LDS copy: the 2.8 table stays in global memory), 3.9
    (radius 55: the `share` branch of unit_fails), central in a 120^3 level and five voxels from its corner; flat windows: the zero row"""
    rows = _run(capi, orc, K.describe_sizes(orc))
    assert not rows["dsize_flat_s1"].any() and not rows["dsize_flat_s0.3"].any()


def _overflows(c):
    return c.name.endswith("3e38") and ("_b_" in c.name or "_c_" in c.name)


def test_voxel_values_in_and_around_the_window(capi, orc):
    """NaN, +Inf and 3e38 at (a) the corner of the window's box, NaN and +Inf at (b) the voxel behind the sphere's pole and (c) the centre:
    (a) leaves the row bit-identical to the unplanted call, (b) and (c) give the reference's constant row bit for bit"""
    plants = [p for p in K.describe_plants(orc) if not _overflows(p[1])]
    rows = _run(capi, orc, [c for _, c, _ in plants] + list({b.name: b for _, _, b in plants}.values()))
    for kind, c, base in plants:
        assert (rows[c.name].tobytes() == rows[base.name].tobytes()) == (kind == "a"), c.name


def test_voxel_values_that_overflow_the_gradient(capi, orc):
    """3e38 at (b) and (c): the central differences stay finite (1.5e38), |g|^2 overflows.  The reference's float histogram then holds
    +Inf in the bins the voxel reaches, its first normalisation turns those into NaN and every other bin into 0, the clamp the NaN into the
    threshold: a row with 3 (b) or 96 (c) equal elements, zero elsewhere.  k_describe's integer histogram cannot hold an Inf (its row is the
    constant row, as for a NaN: rms 0.0494 / 0.0410 off); the entry's k_describe_overflow marks the bins such voxels reach and writes the
    reference's row."""
    _run(capi, orc, [p[1] for p in K.describe_plants(orc) if _overflows(p[1])])


@pytest.mark.parametrize("half", (0, 1))
def test_amplitude(capi, orc, half):
    """L0 2^e on four keypoints, the record (rotation, first guess) the unscaled level's: the oracle is not amplitude invariant (its
    |g|^2 >= eps and fabs(det) < eps tests are absolute) and runs on every scaled level"""
    cases = K.describe_amplitude(orc)
    _run(capi, orc, cases[half::2])


def test_call_history(capi, orc):
    """orient_keypoint with sigma = 2.2 scale immediately before describe_keypoint (another orientation table in the one-keypoint
    context): the row is bit-identical"""
    for c in K.describe_border(orc, 1.0)[::20]:
        _, plain = _call(capi, c)
        rec = np.array([c.rec], dtype=capi.KP_DTYPE)
        capi.orient_keypoint(c.level, c.unit, rec, 2.2 * float(c.rec["scale"]))
        _, after = _call(capi, c)
        assert np.array_equal(bits(plain), bits(after)), c.name
