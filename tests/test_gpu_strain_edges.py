"""GPU tests of the strain fields (sift3d_strain) on the cases of tests/strain_cases.py, which tests/test_strain_cases_cpu.py checks on
the CPU: windows on both sides of the degeneracy rule's floor with each of c00, p1 and p2 deciding, exactly degenerate windows (c00 = 0
among them), a constant of 2^20 added to every displacement, boxes whose extents are one under, at and one over a multiple of the cell
side, stars at radius 1, 2 and 4096, grids the cell cap coarsens (cube, needles, sheets), POIs outside the box of the contributing ones,
the invariances of the parity inputs (translation to the ends of the coordinate range, POI order, signed axis permutations, valid
bytes other than 1) and affine fields with known strains.  The grid cases also go through sift3d_validate_displacements, whose contract
is exact (tests/validate_ref.py): a wrong neighbour set shows there as a wrong median.

The bar of every fp64 field is test_gpu_strain.py's, ref.bar(e, max |u|), except on the tilted windows near the floor, whose fit is
ill-conditioned in itself: there the bar is ref.bar(2 e_case, max |u|), e_case measured on the CPU per case (strain_cases.e_case; the
restatement's two solves and 16 POI orders).  status and neighbours are compared exactly everywhere."""
import ctypes as C
import importlib

import numpy as np
import pytest

import strain_cases as cases
import strain_ref as ref
import validate_cases
import validate_ref

pytestmark = pytest.mark.gpu

capi = importlib.import_module("3dsift_amd.capi")
FIELDS = ref.FLOATS + ("neighbours", "status")


@pytest.fixture(scope="module")
def e():
    return ref.parity_error()


def same_bytes(a, b):
    return [k for k in FIELDS if np.ascontiguousarray(a[k]).tobytes() != np.ascontiguousarray(b[k]).tobytes()]


def agree(got, want, bar, what=""):
    assert np.array_equal(got["status"], want["status"]), (got["status"], want["status"])
    assert np.array_equal(got["neighbours"], want["neighbours"]), (got["neighbours"], want["neighbours"])
    worst = {k: float(np.abs(got[k] - want[k]).max()) if len(want[k]) else 0.0 for k in ref.FLOATS}
    print(f"{what}: max |got - ref| = {max(worst.values()):.2e} ({max(worst, key=worst.get)}); bar {bar:.2e}")
    assert all(np.isfinite(got[k]).all() for k in ref.FLOATS)
    assert max(worst.values()) <= bar, (worst, bar)
    failed = got["status"] != 0
    assert not any(got[k][failed].any() for k in ref.FLOATS)


def run(c, **more):
    return capi.strain(c["points"], c["disp"], c["valid"], **dict(c["opts"], **more))


def check(e, c, what, **more):
    """the call against the restatement on the same input, within the ordinary bar"""
    got = run(c, **more)
    agree(got, cases.reference(c, **more), ref.bar(e, cases.umax(c)), what)
    return got


def check_validate(c, what):
    """the same points, displacements and valid bytes through the median test, no gradients, the smallest min_neighbours: exact"""
    v = validate_cases.case(c["points"], c["disp"], None, c["valid"], radius=c["opts"]["radius"], min_neighbours=3)
    got = capi.validate(v["points"], v["disp"], v["grad"], v["valid"], **v["opts"])["records"]
    want = validate_ref.validate(v["points"], v["disp"], v["grad"], v["valid"], **v["opts"])
    bad = validate_ref.same(got, want)
    assert not bad, (what, bad)
    assert all(np.isfinite(got[k]).all() for k in ("median", "mad", "score"))
    return got


# ---- the degeneracy rule ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cases.THIN))
def test_thin_windows_at_the_pivot_floor(e, name):
    c = cases.pivot_case(name)
    got = check(e, c, f"{name} (rho = {c['rho']:.3e})")
    assert (got["status"][0], got["neighbours"][0]) == (c["status"], c["n"])
    check(e, c, f"{name}, infinitesimal", measure=1)


@pytest.mark.parametrize("name", list(cases.TILTED))
def test_tilted_windows_at_the_pivot_floor(name):
    c = cases.pivot_case(name)
    bar = cases.tilted_bar(name)
    for measure in ref.MEASURES:
        got = run(c, measure=measure)
        agree(got, cases.reference(c, measure=measure), bar, f"{name} measure {measure} (rho = {c['rho']:.3e}, e_case = {cases.e_case(name):.3e})")
        assert (got["status"][0], got["neighbours"][0]) == (c["status"], c["n"])


@pytest.mark.parametrize("name", list(cases.DEGENERATE))
def test_exactly_degenerate_windows(e, name):
    c = cases.DEGENERATE[name]()
    got = check(e, c, name)
    assert (got["status"] == 4).all() and (got["neighbours"] == len(c["points"])).all()


# ---- sums on u - u0 --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", cases.SHIFT_RADII)
def test_constant_shift(e, radius):
    q, u, valid = cases.dyadic_parity_inputs()
    for measure in ref.MEASURES:
        opts = dict(radius=radius, min_neighbours=ref.PARITY_MIN_NEIGHBOURS, measure=measure)
        a, b = capi.strain(q, u, valid, **opts), capi.strain(q, u + cases.SHIFT, valid, **opts)
        agree(a, ref.strain(q, u, valid, **opts), ref.bar(e, ref.largest_u(u)), f"dyadic parity inputs r{radius} measure {measure}")
        assert (a["status"] == 0).sum() > 1000
        bad = cases.shift_disagreement(a, b, e)
        assert not bad, bad


# ---- the cell grid's seams -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r,axis,delta", cases.EXTENT_CASES, ids=[f"r{r}-{'xyz'[a]}{d:+d}" for r, a, d in cases.EXTENT_CASES])
def test_extents_at_multiples_of_the_side(e, r, axis, delta):
    c = cases.extents(r, axis, delta)
    what = f"extent {'xyz'[axis]} = 5 x {r} {delta:+d}"
    check(e, c, what)
    check_validate(c, what)


@pytest.mark.parametrize("r", cases.STAR_RADII)
def test_stars_at_the_extremes_of_the_radius(e, r):
    for contribute, n in ((True, 7), (False, 6)):
        c = cases.stars(r, contribute)
        got = check(e, c, f"stars r{r}, centres {'in' if contribute else 'out'}")
        assert (got["neighbours"][c["centres"]] == n).all() and (got["status"][c["centres"]] == 0).all()
        assert (got["neighbours"][c["corners"]] == 1).all() and (got["status"][c["corners"]] == 1).all()


@pytest.mark.parametrize("box,r", cases.COARSE_CASES, ids=[f"{b}-r{r}" for b, r in cases.COARSE_CASES])
def test_coarsened_grids(e, box, r):
    c = cases.coarsened(box, r)
    side, n = c["grid"]
    what = f"{box} r{r} (side {side}, {n[0]} x {n[1]} x {n[2]} cells)"
    got = check(e, c, what)
    assert (got["status"][:-2] == 0).all() and (got["neighbours"][-2:] == 1).all()
    check_validate(c, what)


@pytest.mark.parametrize("r", cases.OUTSIDE_RADII)
def test_poi_outside_the_box(e, r):
    c = cases.outside(r)
    got = check(e, c, f"outside r{r}")
    rows = c["outsiders"]
    assert set(np.unique(got["status"][rows])) == {0, 1, 4} and (got["status"][rows[-6:]] == 1).all() and not got["neighbours"][rows[-6:]].any()
    check_validate(c, f"outside r{r}")


# ---- invariances of the parity inputs --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def unmoved(e):
    out = {}
    for r in cases.INVARIANCE_RADII:
        c = cases.translated("none", r)
        out[r] = check(e, c, f"parity inputs with two outsiders r{r}")
        assert out[r]["neighbours"][-2:].min() > 0
    return out


@pytest.mark.parametrize("name", list(cases.translations()))
@pytest.mark.parametrize("r", cases.INVARIANCE_RADII)
def test_translation(unmoved, r, name):
    c = cases.translated(name, r)
    got = run(c)
    bad = cases.translation_disagreement(unmoved[r], got, c["out_of_range"])
    assert not bad, bad
    check_validate(c, f"translation {name} r{r}")


@pytest.mark.parametrize("r", cases.INVARIANCE_RADII)
def test_permutation_of_the_pois(e, r):
    q, u, valid = ref.parity_inputs()
    want = ref.parity_reference(r, 0)
    p = np.random.default_rng(r).permutation(len(q))
    got = capi.strain(q[p], u[p], valid[p], radius=r, min_neighbours=ref.PARITY_MIN_NEIGHBOURS)
    agree(got, {k: want[k][p] for k in FIELDS}, ref.bar(e, ref.largest_u(u)), f"permuted parity inputs r{r}")


@pytest.mark.parametrize("r", cases.INVARIANCE_RADII)
def test_signed_axis_permutations(e, r):
    q, u, valid = ref.parity_inputs()
    bar = ref.bar(e, ref.largest_u(u))
    for measure in ref.MEASURES:
        base = ref.parity_reference(r, measure)
        for perm, signs in cases.AXIS_MAPS:
            Q = cases.axis_matrix(perm, signs)
            got = capi.strain((q @ Q.T).astype(np.int32), u @ Q.T, valid, radius=r, min_neighbours=ref.PARITY_MIN_NEIGHBOURS, measure=measure)
            agree(got, cases.mapped_result(base, Q), bar, f"axes {perm} signs {signs} r{r} measure {measure}")


def raw_strain(q, u, valid, **opts):
    """sift3d_strain with the valid bytes as they are (capi.strain hands the library 0 and 1 only)"""
    o = capi.StrainOptions()
    capi.lib().sift3d_default_strain_options(C.byref(o))
    for k, v in opts.items():
        setattr(o, k, v)
    q, u, valid = np.ascontiguousarray(q, np.int32), np.ascontiguousarray(u, np.float64), np.ascontiguousarray(valid, np.uint8)
    out = np.zeros(len(q), capi.STRAIN_DTYPE)
    rc = capi.lib().sift3d_strain(q.ctypes.data, u.ctypes.data, valid.ctypes.data, len(q), C.byref(o), 0, 0, out.ctypes.data, None)
    assert rc == 0, capi.lib().sift3d_last_error()
    return out


def test_valid_bytes_other_than_one():
    q, u, valid = ref.parity_inputs()
    for r in cases.INVARIANCE_RADII:
        opts = dict(radius=r, min_neighbours=ref.PARITY_MIN_NEIGHBOURS)
        want = raw_strain(q, u, valid, **opts)
        via = capi.strain(q, u, valid, **opts)
        assert all(want[k].tobytes() == np.ascontiguousarray(via[k]).tobytes() for k in FIELDS)
        for byte in (2, 128, 255):
            assert raw_strain(q, u, valid * np.uint8(byte), **opts).tobytes() == want.tobytes(), byte
            assert not same_bytes(capi.strain(q, u, valid * np.uint8(byte), **opts), via), byte
        mixed = np.where(np.arange(len(q)) % 3 == 0, 255, np.where(np.arange(len(q)) % 3 == 1, 2, 128)).astype(np.uint8) * valid
        assert raw_strain(q, u, mixed, **opts).tobytes() == want.tobytes()
    v0 = check_validate(dict(points=q, disp=u, valid=valid, opts=dict(radius=7)), "valid bytes 0 / 1")
    v255 = check_validate(dict(points=q, disp=u, valid=valid * np.uint8(255), opts=dict(radius=7)), "valid bytes 0 / 255")
    assert v0.tobytes() == v255.tobytes()


# ---- fields with known answers ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cases.known_fields()))
def test_known_fields(e, name):
    c = cases.known(name)
    G, b = c["G"], c["b"]
    bar = ref.bar(e, cases.umax(c))
    for measure in ref.MEASURES:
        got = check(e, c, f"{name} measure {measure}", measure=measure)
        E, pr, eq = ref.strain_of(G, measure)
        assert (got["status"] == 0).all() and got["neighbours"].min() == 27 and got["neighbours"].max() == 125
        worst = {"G": np.abs(got["G"] - G).max(), "disp": np.abs(got["disp"] - c["disp"]).max(), "E": np.abs(got["E"] - E).max(),
                 "principal": np.abs(got["principal"] - pr).max(), "equivalent": np.abs(got["equivalent"] - eq).max(), "rms": got["rms"].max()}
        print(f"{name} measure {measure}: max |got - closed form| = {max(worst.values()):.2e} ({max(worst, key=worst.get)}); bar {bar:.2e}")
        assert max(worst.values()) <= bar, worst
        # the eigenvalues of the E the call reports, by eigvalsh: descending up to the bar (e_mid is formed by subtraction)
        own = np.linalg.eigvalsh(cases.sym_of(got["E"]))[:, ::-1]
        assert np.abs(got["principal"] - own).max() <= bar
        assert (got["principal"][:, :-1] - got["principal"][:, 1:]).min() >= -bar
    if name == "constant":
        got = run(c)
        assert not got["G"].any() and not got["E"].any() and not got["principal"].any() and not got["rms"].any() and (got["disp"] == b).all()
