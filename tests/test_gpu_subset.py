"""GPU tests of the subset screening (sift3d_subset_quality) against its NumPy restatement (tests/subset_ref.py): parity on a blob
scene, the same with an "air" half, a layered and two diagonal volumes under both criteria; integer-valued volumes bit for bit;
scaling by powers of two; reproducibility, independence of the POIs' order, host against device input; m = 0, m = 1 and one long
call; and the chain subset_quality -> subset_groups -> one icgn call per radius.

status, radius, feasible and material are compared with ==.  The doubles are compared within the bar subset_ref.field_bars forms
from e, the largest |plain fp64 sum - exact sum| / sum |term| of the restatement over the parity inputs (16 seeded permutations of
the order; tests/test_subset_cpu.py measures and prints the same): the GPU bar is max(4 e, 1e-13) x sum |term|, eig adds 4 x the
measured distance of the restatement's Jacobi solve from numpy.linalg.eigvalsh.  Measured: e = 5.1e-13, bar 2.0e-12; Jacobi 3.5e-16
of the trace.  Every threshold lies 1e-6 (relative) away from every c(rho) it is compared with (tests/test_subset_cpu.py checks it),
which is why radius and status are compared exactly and no POI is excluded."""
import importlib

import numpy as np
import pytest

import subset_cases as cs
import subset_ref as ref

pytestmark = pytest.mark.gpu

capi = importlib.import_module("3dsift_amd.capi")
INTS = ("radius", "status", "feasible", "material")
WORST = {}  # field -> largest |GPU - restatement| / bar seen, printed by the tests


@pytest.fixture(scope="module")
def bars():
    e = 0.0
    for name in cs.FLOAT:
        for k, q in enumerate(cs.pois()[[0, 13, 26]]):
            e = max(e, ref.summation_error(cs.volumes()[name], q, cs.R_MAX, seed=k))
    w = np.concatenate([cs.parity_reference(n, 0)["G"][cs.parity_reference(n, 0)["status"] != 2] for n in cs.FLOAT])
    ej = ref.jacobi_error(w)
    print(f"e = {e:.3e}, bar = {ref.bar_rel(e):.3e} x sum |term|, Jacobi = {ej:.3e} x trace")
    return ref.bar_rel(e), ej


def same_bytes(a, b, fields=ref.FIELDS):
    return all(np.ascontiguousarray(a[k]).tobytes() == np.ascontiguousarray(b[k]).tobytes() for k in fields)


def agree(got, want, R, pts, bars, what):
    """the integers with ==; the doubles within the bar of each record (the same NaNs and infinities where the restatement has them)"""
    for k in INTS:
        assert np.array_equal(got[k], want[k]), (what, k, got[k], want[k])
    worst = {"mean": 0.0, "dR2": 0.0, "G": 0.0, "eig": 0.0}
    diff = dict(worst)
    for i, q in enumerate(np.asarray(pts).reshape(-1, 3)):
        if want["status"][i] == 2:
            assert got["mean"][i] == 0 and got["dR"][i] == 0 and not got["G"][i].any() and not got["eig"][i].any()
            continue
        b = ref.field_bars(R, q, int(want["radius"][i]), *bars)
        pairs = {"mean": (got["mean"][i], want["mean"][i]), "dR2": (got["dR"][i] ** 2, want["dR"][i] ** 2), "G": (got["G"][i], want["G"][i]),
                 "eig": (got["eig"][i], want["eig"][i])}
        for k, (g, w) in pairs.items():
            g, w = np.atleast_1d(g), np.atleast_1d(w)
            fin = np.isfinite(w)
            assert np.array_equal(g[~fin], w[~fin], equal_nan=True), (what, k, i, g, w)
            if fin.any():
                d = np.abs(g - w)[fin]
                bk = np.broadcast_to(b[k], w.shape)[fin]
                assert (d <= bk).all(), (what, k, i, g, w, b[k])
                diff[k] = max(diff[k], float(d.max()))
                worst[k] = max(worst[k], float((d / np.maximum(bk, 1e-300)).max()))
    for k in worst:
        WORST[k] = max(WORST.get(k, 0.0), worst[k])
    print(f"{what}: largest |GPU - restatement| " + ", ".join(f"{k} {diff[k]:.3e} ({worst[k]:.2e} of its bar)" for k in worst))


@pytest.mark.parametrize("criterion", [0, 1])
@pytest.mark.parametrize("name", cs.FLOAT)
def test_parity_with_restatement(bars, name, criterion):
    R, pts = cs.volumes()[name], cs.pois()
    want = cs.parity_reference(name, criterion)
    got = capi.subset_quality(R, pts, r_min=cs.R_MIN, r_max=cs.R_MAX, criterion=criterion, threshold=cs.threshold(name, criterion))
    agree(got, want, R, pts, bars, f"{name}/criterion {criterion}")
    assert got["seconds"] > 0
    if name == "diagonal_z":  # texture along (1, 1, 0) and z: the per-axis sums accept r_min, the smallest eigenvalue refuses
        ok = want["status"] != 2
        assert (got["status"][ok] == (0 if criterion == 0 else 1)).all()
    if name in ("layered", "diagonal"):
        assert (got["status"][want["status"] != 2] == 1).all()


def test_diagonal_volume_threshold_zero(bars):
    """R = f(x + y): criterion 0 with the default threshold accepts r_min; criterion 1 with a threshold gives status 1"""
    R, pts = cs.volumes()["diagonal"], cs.pois()
    got = capi.subset_quality(R, pts, r_min=cs.R_MIN, r_max=cs.R_MAX)
    agree(got, ref.quality(R, pts, r_min=cs.R_MIN, r_max=cs.R_MAX), R, pts, bars, "diagonal/threshold 0")
    ok = got["status"] != 2
    assert (got["status"][ok] == 0).all() and (got["radius"][ok] == cs.R_MIN).all()
    got = capi.subset_quality(R, pts, r_min=cs.R_MIN, r_max=cs.R_MAX, criterion=1, threshold=cs.threshold("diagonal", 1))
    assert (got["status"][ok] == 1).all() and (got["radius"][ok] == got["feasible"][ok]).all()


@pytest.mark.parametrize("criterion", [0, 1])
@pytest.mark.parametrize("name", cs.INTEGER)
def test_integer_volumes_bit_for_bit(bars, name, criterion):
    R, pts = cs.volumes()[name], cs.pois()
    want = cs.parity_reference(name, criterion)
    got = capi.subset_quality(R, pts, r_min=cs.R_MIN, r_max=cs.R_MAX, criterion=criterion, threshold=cs.threshold(name, criterion))
    assert same_bytes(got, want, ("mean", "dR", "G", "radius", "status", "feasible", "material"))
    agree(got, want, R, pts, bars, f"{name}/criterion {criterion}")


@pytest.mark.parametrize("e", [20, -20])
def test_power_of_two_scaling(e):
    R, pts = cs.volumes()["scene"], cs.pois()
    t = cs.threshold("scene", 0)
    a = capi.subset_quality(R, pts, r_min=cs.R_MIN, r_max=cs.R_MAX, threshold=t)
    s = np.float32(2.0 ** e)
    b = capi.subset_quality(R * s, pts, r_min=cs.R_MIN, r_max=cs.R_MAX, threshold=t * 4.0 ** e)
    assert same_bytes(a, b, INTS)
    assert (a["G"] * 4.0 ** e).tobytes() == b["G"].tobytes()
    assert (a["eig"] * 4.0 ** e).tobytes() == b["eig"].tobytes()
    assert (a["mean"] * 2.0 ** e).tobytes() == b["mean"].tobytes() and (a["dR"] * 2.0 ** e).tobytes() == b["dR"].tobytes()


def test_reproducible_and_independent_of_the_other_pois():
    R, pts = cs.volumes()["half_flat"], cs.pois()
    kw = dict(r_min=cs.R_MIN, r_max=cs.R_MAX, criterion=1, threshold=cs.threshold("half_flat", 1))
    a = capi.subset_quality(R, pts, **kw)
    b = capi.subset_quality(R, pts, **kw)
    assert same_bytes(a, b) and a["records"].tobytes() == b["records"].tobytes()
    rng = np.random.default_rng(9)
    idx = np.concatenate([rng.permutation(len(pts)), rng.integers(0, len(pts), 50)])  # a permutation, then duplicates
    c = capi.subset_quality(R, pts[idx], **kw)
    assert c["records"].tobytes() == a["records"][idx].tobytes()


def test_host_and_device_input_agree():
    import torch

    R, pts = cs.volumes()["scene"], cs.pois()
    kw = dict(r_min=cs.R_MIN, r_max=cs.R_MAX, threshold=cs.threshold("scene", 0))
    a = capi.subset_quality(R, pts, **kw)
    b = capi.subset_quality(torch.from_numpy(R.copy()).cuda(), pts, **kw)
    c = capi.subset_quality(torch.from_numpy(R.copy()).cuda(), torch.from_numpy(pts).cuda(), **kw)
    assert a["records"].tobytes() == b["records"].tobytes() == c["records"].tobytes()


def test_empty_single_and_long_calls():
    R = cs.volumes()["uint8"]
    got = capi.subset_quality(R, np.zeros((0, 3), np.int32))
    assert all(len(got[k]) == 0 for k in ref.FIELDS) and got["seconds"] == 0
    q = np.array([[24, 23, 22]], np.int32)
    got = capi.subset_quality(R, q, r_min=5, r_max=9, threshold=cs.threshold("uint8", 0))
    want = ref.quality(R, q, r_min=5, r_max=9, threshold=cs.threshold("uint8", 0))
    assert same_bytes(got, want, ("mean", "dR", "G", "radius", "status", "feasible", "material")) and got["status"][0] == 0
    # 10^5 POIs at r 2..3 in a 20^3 volume: a few hundred distinct positions (some outside the volume), each restated once
    V = np.ascontiguousarray(R[:20, :20, :20])
    rng = np.random.default_rng(10)
    pts = np.stack([rng.integers(-1, 21, 100000), rng.integers(2, 8, 100000), rng.integers(3, 7, 100000)], 1).astype(np.int32)
    c3 = [ref.criteria(V, (10, 5, 5), 2, 3, 0)[1][k] for k in (0, 1)]
    t = cs.pick_threshold([v for q in np.unique(pts, axis=0) for v in ref.criteria(V, q, 2, 3, 0)[1]], float(np.sqrt(c3[0] * c3[1])))
    got = capi.subset_quality(V, pts, r_min=2, r_max=3, threshold=t)
    uniq, inv = np.unique(pts, axis=0, return_inverse=True)
    want = ref.quality(V, uniq, r_min=2, r_max=3, threshold=t)
    assert {0, 1, 2} <= set(want["status"].tolist()) and {2, 3} <= set(want["radius"].tolist())
    for k in ("mean", "dR", "G", "radius", "status", "feasible", "material"):
        assert np.ascontiguousarray(want[k][inv.ravel()]).tobytes() == np.ascontiguousarray(got[k]).tobytes(), k


def test_chain_screen_group_refine():
    """subset_quality (4 .. 16) -> subset_groups -> one icgn call per radius: the POIs of the flat half are not refined, every
    status-0 POI converges (icgn_ref converges on them at these radii: tests/test_subset_cpu.py)"""
    R, T, pts, u = cs.chain_case()
    want = cs.chain_reference()
    got = capi.subset_quality(R, pts, r_min=cs.CHAIN_R_MIN, r_max=cs.CHAIN_R_MAX, threshold=cs.chain_threshold())
    for k in INTS:
        assert np.array_equal(got[k], want[k]), k
    flat = pts[:, 0] + cs.CHAIN_R_MAX + 1 < cs.CHAIN_SHAPE[2] // 2
    assert flat.any() and (got["status"][flat] == 1).all() and not got["G"][flat].any()
    groups = capi.subset_groups(got, cs.CHAIN_R_MIN, cs.CHAIN_R_MAX)
    theirs = ref.group_by_radius(got["radius"], got["status"], cs.CHAIN_R_MIN, cs.CHAIN_R_MAX)
    assert len(groups) == len(theirs) >= 3 and all(a[0] == b[0] and np.array_equal(a[1], b[1]) for a, b in zip(groups, theirs))
    refined = np.zeros(len(pts), bool)
    err = 0.0
    for radius, idx in groups:
        res = capi.icgn(R, T, pts[idx], subset_radius=radius)
        assert (res["status"] == 0).all(), (radius, idx, res["status"])
        refined[idx] = True
        err = max(err, float(np.abs(res["displacement"] - u[idx]).max()))
    assert np.array_equal(refined, got["status"] == 0) and not refined[flat].any()
    print(f"chain: {refined.sum()} of {len(pts)} POIs refined in {len(groups)} groups, largest displacement error {err:.4f} voxels")
