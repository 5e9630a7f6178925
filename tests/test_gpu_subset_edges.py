"""GPU tests of the subset screening (sift3d_subset_quality) at the smallest shapes at which the kernel can go wrong, on a
72 x 70 x 68 volume of integer-valued noise (every sum is exact: every field but eig is compared bit for bit with
tests/subset_ref.py): every radius 2 .. 32 forced with the cube + margin on either side of each face; the device form inside a
NaN-filled buffer; the selection stopping at every radius under both criteria and `feasible` cut by each face; spikes on the seams of
the kernel's walk (tests/subset_cases.py lists them for the walk built: the block, then shell by shell); constant, NaN, Inf, 3e38
and -0.0 voxels; and the material screen on both sides of material / N.

eig is compared within 4 x the measured distance of the restatement's Jacobi solve from numpy.linalg.eigvalsh (relative to the
trace; the sums under it are exact here).  Every threshold lies 1e-6 (relative) away from every c(rho) it is compared with, every
fraction_min as far from material / N (tests/test_subset_cpu.py checks both)."""
import importlib

import numpy as np
import pytest

import subset_cases as cs
import subset_ref as ref

pytestmark = pytest.mark.gpu

capi = importlib.import_module("3dsift_amd.capi")
EXACT = ("mean", "dR", "G", "radius", "status", "feasible", "material")
HUGE = 1e300  # a threshold no sum reaches


def exact(got, want, what=""):
    """every field but eig: NaN where the restatement has NaN (the contract does not say which NaN: sign and payload are free) and
    the same bytes everywhere else (so the same infinities and zeros' signs)"""
    for k in EXACT:
        g, w = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k], np.asarray(got[k]).dtype)
        if g.dtype.kind == "f":
            assert np.array_equal(np.isnan(g), np.isnan(w)), (what, k, g, w)
            g, w = np.where(np.isnan(g), 0.0, g), np.where(np.isnan(w), 0.0, w)
        assert g.tobytes() == w.tobytes(), (what, k, got[k], want[k])


@pytest.fixture(scope="module")
def jac():
    recs = ref.profile(cs.edge_volume(), cs.EDGE_CENTRE, 2, 32)
    e = ref.jacobi_error([w["G"] for w in recs])
    print(f"Jacobi vs eigvalsh over the centre's 31 radii: {e:.3e} x trace")
    return e


def eig_close(got, want, jac):
    tr = want["G"][..., :3].sum(axis=-1)
    bar = 4 * jac * tr + 4 * np.spacing(np.abs(tr))
    fin = np.isfinite(want["eig"])
    assert np.array_equal(got["eig"][~fin], want["eig"][~fin], equal_nan=True)
    d = np.abs(got["eig"] - want["eig"])
    assert (~fin | (d <= np.broadcast_to(np.atleast_1d(bar)[..., None], d.shape))).all(), (d, bar)


def stack(recs):
    """restatement records (dicts) -> arrays like capi.subset_quality's"""
    out = {k: np.array([w[k] for w in recs]) for k in ref.FIELDS}
    for k in ("radius", "status", "feasible", "material"):
        out[k] = out[k].astype(np.int32)
    return out


def select(recs, criterion, threshold, fraction_min=0.0):
    """the record a walk over the cached profile `recs` (radius r_min .. feasible) reports"""
    for w in recs:
        c = ref.criterion_value(w["G"], w["eig"], criterion)
        if np.isfinite(c) and c >= threshold:
            N = float((2 * w["radius"] + 1) ** 3)
            return dict(w, status=3 if float(w["material"]) < fraction_min * N else 0, feasible=recs[-1]["radius"])
    return dict(recs[-1], status=1, feasible=recs[-1]["radius"])


@pytest.mark.parametrize("rho", range(2, 33))
def test_every_radius_forced(jac, rho):
    R = cs.edge_volume()
    pts, ok = cs.face_pois(rho)
    got = capi.subset_quality(R, pts, r_min=rho, r_max=rho)
    want = ref.quality(R, pts, r_min=rho, r_max=rho)
    assert np.array_equal(want["status"], np.where(ok, 0, 2)) and (want["radius"][ok] == rho).all()
    exact(got, want, rho)
    eig_close(got, want, jac)
    assert (got["feasible"] == np.where(ok, rho, 0)).all() and (got["material"] == np.where(ok, (2 * rho + 1) ** 3, 0)).all()


def test_device_volume_inside_a_nan_buffer():
    """the volume sits inside a larger allocated buffer of NaN: a read past either end of R would show in the sums"""
    import torch

    R = cs.edge_volume()
    nz, ny, nx = R.shape
    pad = nx * ny + nx + 1
    buf = torch.full((pad + R.size + pad,), float("nan"), dtype=torch.float32, device="cuda")
    buf[pad:pad + R.size] = torch.from_numpy(R.ravel().copy()).cuda()
    vol = buf[pad:pad + R.size].view(nz, ny, nx)
    assert vol.is_contiguous() and vol.data_ptr() == buf.data_ptr() + 4 * pad
    lo32, hi32 = [33, 33, 33], [nx - 34, ny - 34, nz - 34]
    for r_min, r_max, pts in ((32, 32, [lo32, hi32]), (2, 32, [lo32, hi32, [3, 3, 3], [nx - 4, ny - 4, nz - 4], [1, 1, 1], [nx - 2, ny - 2, nz - 2]]),
                              (2, 2, [[3, 3, 3], [nx - 4, ny - 4, nz - 4], [3, ny - 4, 3], [nx - 4, 3, nz - 4]])):
        pts = np.array(pts, np.int32)
        a = capi.subset_quality(R, pts, r_min=r_min, r_max=r_max, threshold=HUGE)
        b = capi.subset_quality(vol, pts, r_min=r_min, r_max=r_max, threshold=HUGE)
        assert a["records"].tobytes() == b["records"].tobytes()
        walked = a["status"] != 2
        assert walked.sum() >= 2 and (a["status"][walked] == 1).all() and np.isfinite(a["G"]).all() and np.isfinite(a["dR"]).all()
        exact(b, ref.quality(R, pts, r_min=r_min, r_max=r_max, threshold=HUGE))


@pytest.mark.parametrize("criterion", [0, 1])
def test_selection_stops_at_every_radius(jac, criterion):
    R = cs.edge_volume()
    cut, feas = cs.cut_pois()
    pts = np.concatenate([np.array([cs.EDGE_CENTRE], np.int32), cut])
    profiles = [ref.profile(R, q, 2, int(f)) for q, f in zip(pts, [32] + feas.tolist())]
    for rho, t in cs.selection_plan(criterion):
        got = capi.subset_quality(R, pts, r_min=2, r_max=32, criterion=criterion, threshold=t)
        want = stack([select(p, criterion, t) for p in profiles])
        assert (want["radius"][0], want["status"][0]) == (rho, 0)
        exact(got, want, (criterion, rho))
        eig_close(got, want, jac)
    assert np.array_equal(got["feasible"], [32] + feas.tolist())      # each of the six faces cuts it
    assert (got["status"][1:] == 1).all() and np.array_equal(got["radius"][1:], feas)  # the last threshold: c(31) < t <= c(32)


@pytest.mark.parametrize("r_min,r_max", [(2, 32), (4, 6)])
def test_walk_seams(jac, r_min, r_max):
    """a spike on the first and the last voxel of the block and of every shell, and on the last voxel of the workgroup's first round
    and the first of its second: a voxel the walk skips, repeats or puts into the wrong shell changes a record"""
    R = cs.edge_volume().copy()
    c = np.array(cs.EDGE_CENTRE)
    tags = cs.seams(r_min, r_max)
    for i, (dx, dy, dz) in enumerate(tags.values()):
        R[c[2] + dz, c[1] + dy, c[0] + dx] = np.float32(100000 + 37 * i)  # integer-valued: the sums stay exact
    recs = ref.profile(R, c, r_min, r_max)
    assert all(float(w["dR"]) ** 2 < 2 ** 53 for w in recs)
    pts = c[None].astype(np.int32)
    got = capi.subset_quality(R, pts, r_min=r_min, r_max=r_max, threshold=HUGE)
    want = stack([select(recs, 0, HUGE)])
    exact(got, want, "all shells")
    eig_close(got, want, jac)
    cc = [float(ref.criterion_value(w["G"], w["eig"], 0)) for w in recs]
    for k in range(1, len(recs)):  # stop at every radius above r_min: the running totals after each shell
        t = float(np.sqrt(cc[k - 1] * cc[k]))
        assert cs.clear_of(t, cc) and cc[k - 1] < t < cc[k]
        got = capi.subset_quality(R, pts, r_min=r_min, r_max=r_max, threshold=t)
        want = stack([select(recs, 0, t)])
        assert want["radius"][0] == r_min + k
        exact(got, want, ("stop", r_min + k))
    # the forced block of every radius sees the same voxels
    for rho in (r_max, (r_min + r_max) // 2):
        exact(capi.subset_quality(R, pts, r_min=rho, r_max=rho), stack([dict(ref.direct(R, c, rho), status=0, feasible=rho)]), ("block", rho))


def test_constant_and_negative_zero_volumes():
    pts = np.array([cs.EDGE_CENTRE, [5, 5, 5], [2, 40, 40]], np.int32)
    for value in (7.25, -0.0, 0.0):
        R = np.full(cs.EDGE_SHAPE, value, np.float32)
        got = capi.subset_quality(R, pts, r_min=3, r_max=12)
        exact(got, ref.quality(R, pts, r_min=3, r_max=12), value)
        ok = got["status"] != 2
        assert (got["status"] == [0, 0, 2]).all() and (got["radius"][ok] == 3).all()
        assert not got["dR"].any() and not got["G"].any() and not got["eig"].any() and (got["mean"][ok] == value).all()
        assert np.array_equal(np.signbit(got["mean"][ok]), [False, False])  # -0.0 + 0 / N = +0.0; 7.25 stays positive
        got = capi.subset_quality(R, pts, r_min=3, r_max=12, threshold=1e-300)
        exact(got, ref.quality(R, pts, r_min=3, r_max=12, threshold=1e-300), value)
        assert (got["status"] == [1, 1, 2]).all() and (got["radius"] == [12, 4, 0]).all() and not got["G"].any()


@pytest.mark.parametrize("where,offset", [("cube", (6, 0, 0)), ("cube_z", (2, -3, -6)), ("margin_edge", (6, 6, 0)), ("margin_corner", (-6, 6, 6))])
def test_nan_at_chebyshev_distance(jac, where, offset):
    """a NaN at Chebyshev distance 6: radii <= 4 are unchanged; radius 5 reads it only when it lies on a face of the margin (one
    coordinate at distance 6), not on the margin's edges and corners; radii >= 6 hold it"""
    clean = cs.edge_volume()
    R = clean.copy()
    c = np.array(cs.EDGE_CENTRE)
    R[c[2] + offset[2], c[1] + offset[1], c[0] + offset[0]] = np.nan
    pts = c[None].astype(np.int32)
    on_face = sum(abs(v) == 6 for v in offset) == 1
    for rho in (3, 4, 5, 6, 7):
        got = capi.subset_quality(R, pts, r_min=rho, r_max=rho)
        exact(got, ref.quality(R, pts, r_min=rho, r_max=rho), (where, rho))
        N = (2 * rho + 1) ** 3
        if rho <= 4 or (rho == 5 and not on_face):
            assert got["records"].tobytes() == capi.subset_quality(clean, pts, r_min=rho, r_max=rho)["records"].tobytes()
            assert got["status"][0] == 0 and got["material"][0] == N
        else:
            assert got["status"][0] == 1 and np.isnan(got["G"]).any() and np.isnan(got["eig"]).all()
            assert got["material"][0] == (N - 1 if rho >= 6 else N)  # the NaN voxel is no material; in the margin it is not counted at all
            assert np.isnan(got["dR"][0]) == (rho >= 6)
    # one walk: a threshold met before the NaN is reached reports that radius; one met only behind it reports the NaN record of r_max
    cc = cs.centre_criteria(0)
    got = capi.subset_quality(R, pts, r_min=2, r_max=10, threshold=float(np.sqrt(cc[1] * cc[2])))
    exact(got, ref.quality(clean, pts, r_min=2, r_max=10, threshold=float(np.sqrt(cc[1] * cc[2]))), "stop at 4")
    assert (got["radius"][0], got["status"][0]) == (4, 0)
    got = capi.subset_quality(R, pts, r_min=2, r_max=10, threshold=float(np.sqrt(cc[5] * cc[6])))
    exact(got, ref.quality(R, pts, r_min=2, r_max=10, threshold=float(np.sqrt(cc[5] * cc[6]))), "behind the NaN")
    assert (got["radius"][0], got["status"][0]) == (10, 1) and np.isnan(got["G"]).any()


@pytest.mark.parametrize("what", ["+inf", "-inf", "3e38"])
def test_infinite_and_overflowing_voxels_never_qualify(what):
    R = cs.edge_volume().copy()
    c = np.array(cs.EDGE_CENTRE)
    if what == "3e38":  # the fp32 difference across the voxel between them overflows; every voxel is finite
        R[c[2], c[1] + 1, c[0] + 3] = 3e38
        R[c[2], c[1] + 1, c[0] + 1] = -3e38
    else:
        R[c[2] + 1, c[1], c[0] - 2] = np.inf if what == "+inf" else -np.inf
    pts = c[None].astype(np.int32)
    for criterion in (0, 1):
        got = capi.subset_quality(R, pts, r_min=2, r_max=9, criterion=criterion)
        want = ref.quality(R, pts, r_min=2, r_max=9, criterion=criterion)
        exact(got, want, (what, criterion))
        assert (got["radius"][0], got["status"][0]) == (9, 1) and not np.isfinite(got["G"]).all() and np.isnan(got["eig"]).all()
    far = np.array([[c[0] + 20, c[1], c[2]]], np.int32)  # a cube that does not hold them is not touched
    got = capi.subset_quality(R, far, r_min=2, r_max=9, threshold=HUGE)
    assert got["records"].tobytes() == capi.subset_quality(cs.edge_volume(), far, r_min=2, r_max=9, threshold=HUGE)["records"].tobytes()


@pytest.mark.parametrize("case", range(3), ids=["level-at-a-voxel", "one-float-below", "one-float-above"])
def test_material_screen(case):
    R = cs.edge_volume()
    level, m, below, above = cs.material_cases()[case]
    pts = np.array([cs.EDGE_CENTRE], np.int32)
    r = cs.MATERIAL_RADIUS
    for f, status in ((below, 0), (above, 3), (0.0, 0), (1.0, 3)):
        got = capi.subset_quality(R, pts, r_min=r, r_max=r, level=level, fraction_min=f)
        want = ref.quality(R, pts, r_min=r, r_max=r, level=level, fraction_min=f)
        exact(got, want, (case, f))
        assert (got["status"][0], got["material"][0], got["radius"][0]) == (status, m, r)
    # status 1 comes before status 3: no radius qualifies, the material is not asked
    got = capi.subset_quality(R, pts, r_min=r, r_max=r, level=level, fraction_min=1.0, threshold=HUGE)
    assert (got["status"][0], got["material"][0]) == (1, m)
    assert capi.subset_quality(R, pts, r_min=r, r_max=r, level=np.inf)["material"][0] == 0
