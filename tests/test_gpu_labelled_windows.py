"""GPU tests of the labelled window calls (sift3d_strain_labelled, sift3d_validate_displacements_labelled, sift3d_field_eval_labelled)
and of the chain mask_from_level -> mask_label -> labels_at -> strain.  With all labels 1 a call returns the unlabelled call's record
byte for byte.  With 2, 7 and about 300 random labels, some 0 or negative, on the parity inputs of tests/strain_ref.py and
tests/field_ref.py and on a planted case of tests/validate_cases.py, the records equal the per-label wrappers of tests/label_ref.py
over the existing restatements: validation exactly (its contract is bit for bit), strain and field within the existing bars
strain_ref.bar(e, max |u|) and field_ref.bar(e, max |u|) with the integers exact.  The scenes of several bodies give what the CPU
tests computed for them: no strain and no flag within a body.  A POI's record keeps its bytes when the displacements of the POIs of
other labels change (a NaN among them, at POIs that do not span the bounding box of the contributing ones: that box places the cell
grid, which fixes the order of a window's fp64 sums)."""
import importlib

import numpy as np
import pytest

import field_ref
import label_cases as cases
import label_ref as ref
import strain_ref
import validate_cases
import validate_ref

pytestmark = pytest.mark.gpu

capi = importlib.import_module("3dsift_amd.capi")
STRAIN_FIELDS = ("disp", "G", "E", "principal", "equivalent", "rms", "neighbours", "status")
FIELD_FIELDS = ("disp", "G", "rms", "wsum", "neighbours", "sides", "status")
STRAIN_RADII, FIELD_RADII = (7, 20), (5, 16)
VALIDATE_CASE = "planted-k0.002-n0.02-grad"
LABEL_COUNTS = (2, 7, 300)


def same_bytes(a, b, fields):
    return [k for k in fields if np.asarray(a[k]).tobytes() != np.asarray(b[k]).tobytes()]


def random_labels(m, count, seed):
    """labels 1..count, 5 % of them 0 and 3 % negative"""
    rng = np.random.default_rng(seed)
    lab = rng.integers(1, count + 1, m).astype(np.int32)
    r = rng.random(m)
    lab[r < 0.05] = 0
    lab[(r >= 0.05) & (r < 0.08)] = -rng.integers(1, 5, int(((r >= 0.05) & (r < 0.08)).sum()))
    return lab


def agree(got, want, bar, floats, ints, what):
    for k in ints:
        assert np.array_equal(got[k], want[k]), (what, k, np.flatnonzero(got[k] != want[k])[:8].tolist())
    worst = 0.0
    for k in floats:
        assert np.isfinite(got[k]).all(), (what, k)
        worst = max(worst, float(np.abs(got[k].reshape(len(want[k]), -1) - want[k].reshape(len(want[k]), -1)).max()))
    print(f"{what}: largest difference {worst:.3e}, bar {bar:.3e}, status counts {np.bincount(want['status']).tolist()}")
    assert worst <= bar, (what, worst, bar)


@pytest.fixture(scope="module")
def strain_e():
    return strain_ref.parity_error()


@pytest.fixture(scope="module")
def field_e():
    return field_ref.parity_error()


# ---- all labels equal: the unlabelled call's bytes ------------------------------------------------------------------------------------

def test_all_labels_one_is_the_plain_call_byte_for_byte():
    q, u, valid = strain_ref.parity_inputs()
    one = np.ones(len(q), np.int32)
    for radius in strain_ref.PARITY_RADII:
        for measure in strain_ref.MEASURES:
            o = dict(radius=radius, min_neighbours=strain_ref.PARITY_MIN_NEIGHBOURS, measure=measure)
            assert not same_bytes(capi.strain(q, u, valid, label=one, **o), capi.strain(q, u, valid, **o), STRAIN_FIELDS), o
    for c, grad in ((validate_cases.get(VALIDATE_CASE), True), (dict(points=q, disp=u, grad=None, valid=valid, opts=dict(radius=7)), False)):
        plain = capi.validate(c["points"], c["disp"], c["grad"], c["valid"], **c["opts"])
        own = capi.validate(c["points"], c["disp"], c["grad"], c["valid"], label=np.full(len(c["points"]), 9, np.int32), **c["opts"])
        assert plain["records"].tobytes() == own["records"].tobytes() and plain["flagged"].sum() > 0
    q, u, valid, xs = field_ref.parity_inputs()
    for radius in field_ref.PARITY_RADII:
        for weighting in field_ref.WEIGHTINGS:
            for enclosed in (0, 1):
                o = dict(radius=radius, min_neighbours=field_ref.PARITY_MIN_NEIGHBOURS, weighting=weighting, require_enclosed=enclosed)
                own = capi.field_eval(q, u, valid, xs, label=np.ones(len(q), np.int32), query_label=np.ones(len(xs), np.int32), **o)
                assert own["records"].tobytes() == capi.field_eval(q, u, valid, xs, **o)["records"].tobytes(), o


# ---- random labels against the per-label wrappers ------------------------------------------------------------------------------------

@pytest.mark.parametrize("count", LABEL_COUNTS)
def test_strain_equals_the_per_label_restatement(count, strain_e):
    q, u, valid = strain_ref.parity_inputs()
    lab = random_labels(len(q), count, 10 + count)
    bar = strain_ref.bar(strain_e, strain_ref.largest_u(u))
    for radius in STRAIN_RADII:
        for measure in strain_ref.MEASURES:
            o = dict(radius=radius, min_neighbours=strain_ref.PARITY_MIN_NEIGHBOURS, measure=measure)
            got = capi.strain(q, u, valid, label=lab, **o)
            want = ref.strain(q, u, valid, lab, **o)
            assert len(got["status"]) == len(q)   # no POI is left out
            agree(got, want, bar, strain_ref.FLOATS, ("neighbours", "status"), f"strain, {count} labels, r{radius}, measure {measure}")
            low = lab <= 0
            assert (got["status"][low] == 1).all() and not got["neighbours"][low].any()
            assert all(not got[k][low].any() for k in strain_ref.FLOATS)


@pytest.mark.parametrize("count", LABEL_COUNTS)
def test_validation_equals_the_per_label_restatement(count):
    for c in (validate_cases.get(VALIDATE_CASE), validate_cases.get("block-p2"),
              dict(zip(("points", "disp", "valid"), strain_ref.parity_inputs()), grad=None, opts=dict(radius=9, min_neighbours=4))):
        lab = random_labels(len(c["points"]), count, 20 + count)
        got = capi.validate(c["points"], c["disp"], c["grad"], c["valid"], label=lab, **c["opts"])["records"]
        want = ref.validate(c["points"], c["disp"], c["grad"], c["valid"], lab, **c["opts"])
        assert len(got) == len(lab)
        bad = validate_ref.same(got, want)
        assert not bad, (count, bad)
        low = lab <= 0
        assert (got["status"][low] == 1).all() and not got["neighbours"][low].any() and not got["flagged"][low].any()


@pytest.mark.parametrize("count", LABEL_COUNTS)
def test_field_equals_the_per_label_restatement(count, field_e):
    q, u, valid, xs = field_ref.parity_inputs()
    lab, qlab = random_labels(len(q), count, 30 + count), random_labels(len(xs), count, 40 + count)
    bar = field_ref.bar(field_e, field_ref.largest_u(u))
    for radius in FIELD_RADII:
        for weighting in field_ref.WEIGHTINGS:
            o = dict(radius=radius, min_neighbours=field_ref.PARITY_MIN_NEIGHBOURS, weighting=weighting, require_enclosed=0)
            got = capi.field_eval(q, u, valid, xs, label=lab, query_label=qlab, **o)
            want = ref.evaluate(q, u, valid, lab, xs, qlab, **o)
            assert len(got["status"]) == len(xs)
            agree(got, want, bar, field_ref.FLOATS, field_ref.INTS, f"field, {count} labels, r{radius}, weighting {weighting}")
            low = qlab <= 0
            assert (got["status"][low] == 1).all() and not got["neighbours"][low].any() and not got["sides"][low].any()
    # require_enclosed on top: field_ref.enclosed() of the wrapper's answer
    o = dict(radius=16, min_neighbours=field_ref.PARITY_MIN_NEIGHBOURS, weighting=1)
    got = capi.field_eval(q, u, valid, xs, label=lab, query_label=qlab, require_enclosed=1, **o)
    want = field_ref.enclosed(ref.evaluate(q, u, valid, lab, xs, qlab, require_enclosed=0, **o))
    agree(got, want, bar, field_ref.FLOATS, field_ref.INTS, f"field, {count} labels, enclosed")


def test_out_of_range_comes_before_the_label():
    q, u, lab = (a.copy() for a in cases.two_bodies())
    q[5] = (2 ** 24 + 1, 2, 2)
    q[6] = (2, -2 ** 24 - 1, 2)
    lab[5], lab[7] = 0, -3
    s = capi.strain(q, u, None, label=lab, radius=8)
    v = capi.validate(q, u, None, None, label=lab, radius=8)
    x = q.astype(np.float64)
    x[8] = np.nan
    qlab = lab.copy()
    qlab[8] = 0
    f = capi.field_eval(q, u, None, x, label=lab, query_label=qlab, radius=8)
    for r in (s, v, f):
        assert r["status"][[5, 6, 7]].tolist() == [2, 2, 1] and not r["neighbours"][[5, 6, 7]].any()
    assert f["status"][8] == 2 and not f["sides"][[5, 6, 7, 8]].any()


# ---- the scenes --------------------------------------------------------------------------------------------------------------------------

def test_two_bodies_have_no_strain_within_a_body():
    q, u, lab = cases.two_bodies()
    plain = capi.strain(q, u, None, radius=cases.SCENE_RADIUS)
    assert abs(np.abs(plain["E"]).max() - 0.075) < 5e-4
    own = capi.strain(q, u, None, label=lab, radius=cases.SCENE_RADIUS)
    assert not own["status"].any() and own["neighbours"].min() == 27
    assert all(not own[k].any() for k in ("E", "G", "rms"))   # exactly 0
    assert np.array_equal(own["disp"], u)


def test_the_grain_is_not_flagged_within_its_body():
    q, u, lab, x = cases.grain()
    plain = capi.validate(q, u, None, None, radius=cases.SCENE_RADIUS)
    assert plain["flagged"][lab == 2].all() and not plain["flagged"][lab == 1].any()
    own = capi.validate(q, u, None, None, label=lab, radius=cases.SCENE_RADIUS)
    assert not own["flagged"].any() and not own["status"].any() and own["neighbours"].min() == 26
    blend = capi.field_eval(q, u, None, x, radius=cases.SCENE_RADIUS)
    assert np.allclose(blend["disp"][0], (0.99, -0.39, 0.34), atol=5e-3)
    for L, want in ((1, 0.01 * x[0, [1, 2, 0]]), (2, np.array([1.5, -0.75, 0.5]))):
        part = capi.field_eval(q, u, None, x, label=lab, query_label=np.array([L], np.int32), radius=cases.SCENE_RADIUS, require_enclosed=0)
        assert part["status"][0] == 0 and np.allclose(part["disp"][0], want, atol=1e-12)


# ---- independence of the other bodies ------------------------------------------------------------------------------------------------------

def test_a_record_does_not_depend_on_the_pois_of_other_labels():
    q, u, valid = strain_ref.parity_inputs()
    lab = random_labels(len(q), 3, 77)
    mine = lab == 2
    on = strain_ref.contributes(q, u, valid)
    inner = ((q > q[on].min(0)) & (q < q[on].max(0))).all(1)   # not on the bounding box of the contributing POIs
    rng = np.random.default_rng(78)
    u2 = u.copy()
    u2[~mine] = rng.normal(0.0, 50.0, (int((~mine).sum()), 3))
    nan_rows = np.flatnonzero(~mine & inner)[::5]
    u2[nan_rows, rng.integers(0, 3, len(nan_rows))] = np.nan
    assert len(nan_rows) > 100 and (lab[nan_rows] == 1).any() and (lab[nan_rows] <= 0).any()
    o = dict(radius=20, min_neighbours=strain_ref.PARITY_MIN_NEIGHBOURS)
    a, b = capi.strain(q, u, valid, label=lab, **o), capi.strain(q, u2, valid, label=lab, **o)
    assert (a["status"][mine] == 0).sum() > 200
    assert not same_bytes({k: a[k][mine] for k in STRAIN_FIELDS}, {k: b[k][mine] for k in STRAIN_FIELDS}, STRAIN_FIELDS)
    assert same_bytes({k: a[k][lab == 1] for k in STRAIN_FIELDS}, {k: b[k][lab == 1] for k in STRAIN_FIELDS}, STRAIN_FIELDS)   # the others moved
    a, b = (capi.validate(q, d, None, valid, label=lab, radius=9, min_neighbours=4)["records"] for d in (u, u2))
    assert a[mine].tobytes() == b[mine].tobytes() and (a["status"][mine] == 0).sum() > 200
    xs = q[mine].astype(np.float64) + 0.25
    qlab = np.full(len(xs), 2, np.int32)
    a, b = (capi.field_eval(q, d, valid, xs, label=lab, query_label=qlab, radius=16, min_neighbours=6, require_enclosed=0)["records"] for d in (u, u2))
    assert a.tobytes() == b.tobytes() and (a["status"] == 0).sum() > 200


# ---- the chain on a granular volume ----------------------------------------------------------------------------------------------------------

def test_spheres_chain(strain_e):
    vol, centres, q, u, body = cases.spheres()
    mask = capi.mask_from_level(vol, cases.SPHERE_LEVEL)
    labels, count = capi.mask_label(mask, 26, min_voxels=100)
    assert count == len(centres) == 12
    lab = capi.labels_at(labels, q)
    assert np.array_equal(lab, body)
    valid = (lab > 0).astype(np.uint8)
    bar = strain_ref.bar(strain_e, strain_ref.largest_u(u))
    o = dict(radius=cases.SCENE_RADIUS, min_neighbours=10, measure=0)
    own = capi.strain(q, u, valid, label=lab, **o)
    grains = (lab > 0) & (own["status"] == 0)
    assert grains.sum() > 900 and (own["status"][lab == 0] == 1).all()
    worst = float(np.abs(own["E"][grains]).max())
    plain = capi.strain(q, u, valid, **o)
    near = (lab > 0) & (plain["status"] == 0) & (plain["neighbours"] > own["neighbours"])   # a window that reaches into another sphere
    worst_plain = float(np.abs(plain["E"][near]).max())
    print(f"rigid spheres: |E| <= {worst:.3e} within a body (bar {bar:.3e}), up to {worst_plain:.3e} across contacts at {int(near.sum())} POIs")
    assert worst <= bar
    assert near.sum() > 100 and (np.abs(plain["E"][near]).max(1) > bar).all()
    # the same through device pointers
    import torch
    dl, dcount = capi.mask_label(capi.mask_from_level(torch.from_numpy(vol).cuda(), cases.SPHERE_LEVEL), 26, min_voxels=100)
    assert dcount == count and np.array_equal(dl.cpu().numpy(), labels)
    assert np.array_equal(capi.labels_at(dl, torch.from_numpy(q).cuda()), lab)
