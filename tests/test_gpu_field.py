"""GPU tests of the field evaluation (sift3d_field_eval) against its NumPy restatement (tests/field_ref.py): parity on scattered POIs
from windows of 3^3 voxels to one that holds every POI under both weightings, the tie to sift3d_strain, a known affine field and a
constant one, the window's faces, every status, the continuity of the weighted fit, device pointers, a call long enough for the capped
grid to loop, repeatability, the C++ shell, and the chain the feature is for: two load steps composed into one field that starts
IC-GN where a zero start fails, and a coarse grid that seeds a denser one.

The bar of every fp64 field: max(4 e, 1e-12) x max(1, the largest |u| of the case), e = the largest absolute difference between the
restatement's two solves (normal equations as the header writes them / numpy.linalg.lstsq on the rows sqrt(w) [1, d]) over every
field of every status-0 query of the parity inputs, computed on the CPU (field_ref.parity_error; tests/test_field_cpu.py prints it).
Measured: e = 1.09e-11 (the window of radius 40 over some 500 POIs), so the bar is 4.4e-11 x max(1, max |u|): 3.1e-10 on the parity
inputs.  status, neighbours and sides are compared exactly and no query is excluded."""
import importlib

import numpy as np
import pytest

import field_ref as ref
import field_shell
import icgn_ref

pytestmark = pytest.mark.gpu

capi = importlib.import_module("3dsift_amd.capi")
FIELDS = ref.FLOATS + ref.INTS
G0 = np.array([[0.010, -0.004, 0.002], [0.003, -0.020, 0.001], [-0.002, 0.005, 0.015]])
B0 = np.array([1.25, -2.5, 0.75])


@pytest.fixture(scope="module")
def e():
    v = ref.parity_error()
    print(f"e = {v:.3e}")
    return v


def same_bytes(a, b):
    return all(np.ascontiguousarray(a[k]).tobytes() == np.ascontiguousarray(b[k]).tobytes() for k in FIELDS + ("records",))


def agree(got, want, bar):
    for k in ref.INTS:
        assert np.array_equal(got[k], want[k]), (k, got[k], want[k])
    worst = {k: float(np.abs(got[k] - want[k]).max()) if len(want[k]) else 0.0 for k in ref.FLOATS}
    print("max |got - ref|: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()) + f"; bar {bar:.2e}")
    assert all(np.isfinite(got[k]).all() for k in ref.FLOATS)
    assert max(worst.values()) <= bar, (worst, bar)
    failed = got["status"] != 0
    assert not any(got[k][failed].any() for k in ref.FLOATS) and not got["records"]["reserved"].any()


def check(e, q, u, valid, xs, **opts):
    """the call against the restatement on the same input, within the case's bar"""
    got = capi.field_eval(q, u, valid, xs, **opts)
    want = ref.evaluate(q, u, valid, xs, **opts)
    agree(got, want, ref.bar(e, ref.largest_u(u)))
    return got


CASES = [(r, wt) for r in ref.PARITY_RADII for wt in ref.WEIGHTINGS]


@pytest.mark.parametrize("radius,weighting", CASES, ids=[f"r{r}-{('uniform', 'biweight')[wt]}" for r, wt in CASES])
def test_parity_with_restatement(e, radius, weighting):
    q, u, valid, xs = ref.parity_inputs()
    bar = ref.bar(e, ref.largest_u(u))
    opts = dict(radius=radius, min_neighbours=ref.PARITY_MIN_NEIGHBOURS, weighting=weighting)
    got = capi.field_eval(q, u, valid, xs, require_enclosed=0, **opts)
    agree(got, ref.parity_reference(radius, weighting), bar)
    assert got["seconds"] > 0
    agree(capi.field_eval(q, u, valid, xs, **opts), ref.enclosed(ref.parity_reference(radius, weighting)), bar)


@pytest.mark.parametrize("radius", [5, 16])
def test_tie_to_strain(e, radius):
    """uniform weights, no enclosure asked, the queries on the POIs: sift3d_strain's fit"""
    q, u, valid, _ = ref.parity_inputs()
    bar = ref.bar(e, ref.largest_u(u))
    want = capi.strain(q, u, valid, radius=radius, min_neighbours=ref.PARITY_MIN_NEIGHBOURS)
    got = capi.field_eval(q, u, valid, q.astype(np.float64), radius=radius, min_neighbours=ref.PARITY_MIN_NEIGHBOURS, weighting=0, require_enclosed=0)
    assert np.array_equal(got["status"], want["status"]) and np.array_equal(got["neighbours"], want["neighbours"])
    assert set(got["status"]) <= {0, 1, 4} and (got["status"] == 0).sum() > 1000
    worst = {k: float(np.abs(got[k] - want[k]).max()) for k in ("disp", "G", "rms")}
    print("max |field - strain|: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()) + f"; bar {bar:.2e}")
    assert max(worst.values()) <= bar
    ok = got["status"] == 0
    assert np.array_equal(got["wsum"][ok], got["neighbours"][ok].astype(np.float64))


def test_affine_and_constant_field(e):
    rng = np.random.default_rng(6)
    q = ref.jittered_lattice(rng, (9, 8, 7))
    xs = rng.random((400, 3)) * np.array([40.0, 36.0, 32.0]) - 2.0
    u = q @ G0.T + B0
    bar = ref.bar(e, ref.largest_u(u))
    for weighting in ref.WEIGHTINGS:
        got = check(e, q, u, None, xs, radius=7, weighting=weighting, require_enclosed=0)
        ok = got["status"] == 0
        assert ok.sum() > 350 and (got["sides"][ok] != 63).any()
        assert np.abs(got["G"][ok] - G0).max() <= bar and np.abs(got["disp"][ok] - (xs[ok] @ G0.T + B0)).max() <= bar and got["rms"].max() <= bar
        const = capi.field_eval(q, np.tile(B0, (len(q), 1)), None, xs, radius=7, weighting=weighting, require_enclosed=0)
        assert np.array_equal(const["status"], got["status"])
        assert not const["G"].any() and not const["rms"].any() and (const["disp"][ok] == B0).all() and not const["disp"][~ok].any()


def test_window_faces(e):
    g = 3 * np.arange(5)
    q = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(np.int32)
    u = q @ G0.T + B0 + np.random.default_rng(3).normal(0, 0.01, (len(q), 3))
    # a POI at |d_a| = radius exactly: counted with uniform weights, weight 0 under the biweight
    xs = np.array([[6.0, 6.0, 6.0], [6.0, 7.5, 6.0], [3.0, 9.0, 12.0]])
    a = check(e, q, u, None, xs, radius=3, min_neighbours=4, weighting=0, require_enclosed=0)
    b = check(e, q, u, None, xs, radius=3, min_neighbours=4, weighting=1, require_enclosed=0)
    assert list(a["neighbours"]) == [27, 18, 18] and list(b["neighbours"]) == [1, 2, 1]
    # 2^-40 past the face: no member; on it: a member; 2^-40 inside: a member of either weighting
    blk = np.stack(np.meshgrid(*[np.arange(10, 13)] * 3, indexing="ij"), -1).reshape(-1, 3)
    q = np.concatenate([[[0, 11, 11]], blk]).astype(np.int32)
    u = q @ G0.T + B0
    eps = 2.0 ** -40
    xs = np.array([[5.0 + eps, 11, 11], [5.0, 11, 11], [5.0 - eps, 11, 11]])
    assert xs[0, 0] > 5.0 > xs[2, 0]
    a = check(e, q, u, None, xs, radius=5, min_neighbours=4, weighting=0, require_enclosed=0)
    b = check(e, q, u, None, xs, radius=5, min_neighbours=4, weighting=1, require_enclosed=0)
    assert list(a["neighbours"]) == [9, 10, 1] and list(b["neighbours"]) == [9, 0, 1]
    # queries whose floor lies in another cell than their members (cells of side radius + 1 from the box's corner), negative coordinates
    q, u, xs = ref.cell_inputs()
    for weighting in ref.WEIGHTINGS:
        for enclosed in (0, 1):
            got = check(e, q, u, None, xs, weighting=weighting, require_enclosed=enclosed, **ref.CELL_OPTIONS)
            assert (got["status"] == 0).sum() > 1700 and (got["status"] == 1).sum() > 20 and (got["status"] == (5 if enclosed else 4)).sum() > 5
    rng = np.random.default_rng(8)
    # two clusters 3000 voxels apart at radius 1: 1501^3 cells of side 2 are over the cap, the cells grow
    blk = np.stack(np.meshgrid(*[np.arange(3)] * 3, indexing="ij"), -1).reshape(-1, 3)
    q = np.concatenate([blk, blk + 3000]).astype(np.int32)
    u = q @ G0.T + rng.normal(0, 0.05, (len(q), 3))
    xs = np.array([[1.0, 1.0, 1.0], [1.5, 1.25, 0.75], [3001.5, 3001.25, 3000.75], [3001, 3001, 3001], [1500, 1500, 1500], [-0.5, 1, 1], [3002.5, 3001, 3001],
                   [2.0, 2.0, 3.0], [2999.0, 3000.0, 3000.0]])
    for weighting in ref.WEIGHTINGS:
        got = check(e, q, u, None, xs, radius=1, min_neighbours=4, weighting=weighting, require_enclosed=0)
        assert list(got["neighbours"][:5]) == ([27, 8, 8, 27, 0] if weighting == 0 else [1, 8, 8, 1, 0])
    # the same at the ends of the coordinate range: the box spans 2^25 + 1 voxels on every axis
    q = np.concatenate([blk - 2 ** 24, blk + 2 ** 24 - 2]).astype(np.int32)
    u = (q / 2.0 ** 24) @ G0.T + rng.normal(0, 0.05, (len(q), 3))
    xs = np.array([[-2.0 ** 24 + 1.5] * 3, [2.0 ** 24 - 1.25] * 3, [2.0 ** 24] * 3, [-2.0 ** 24] * 3, [0.5, 0.5, 0.5]])
    got = check(e, q, u, None, xs, radius=1, min_neighbours=4, weighting=0, require_enclosed=0)
    assert list(got["neighbours"]) == [8, 8, 8, 8, 0] and list(got["status"]) == [0, 0, 0, 0, 1]


def test_statuses(e):
    g = 3 * np.arange(5)
    q = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(np.int32)
    u = q @ G0.T + B0 + np.random.default_rng(9).normal(0, 0.01, (len(q), 3))
    mid = np.array([6.4, 5.7, 6.2])
    # 2: a query that is not finite or out of range; an out-of-range POI contributes nothing
    far = np.concatenate([q, [[2 ** 24 + 1, 6, 6], [6, -2 ** 24 - 1, 6], [6, 6, 2 ** 31 - 1]]]).astype(np.int32)
    ufar = np.concatenate([u, np.full((3, 3), 50.0)])
    xs = np.array([mid, [np.nan, 6, 6], [6, np.inf, 6], [6, 6, -np.inf], [2.0 ** 24 + 1, 6, 6], [6, -2.0 ** 24 - 1, 6], [2.0 ** 24, 6, 6]])
    got = check(e, far, ufar, None, xs, radius=4095, min_neighbours=4)
    assert list(got["status"]) == [0, 2, 2, 2, 2, 2, 1] and list(got["neighbours"]) == [125, 0, 0, 0, 0, 0, 0] and not got["sides"][1:].any()
    # 1: n = min_neighbours - 1 and n = min_neighbours (the window of radius 4 around mid holds 27 POIs)
    for mn, st in ((27, 0), (28, 1)):
        got = check(e, q, u, None, mid[None], radius=4, min_neighbours=mn)
        assert (got["status"][0], got["neighbours"][0], got["sides"][0]) == (st, 27, 63)
    # 5: one case per missing bit of sides; the same query is fitted when enclosure is not asked for
    out = []
    for axis in range(3):
        for value in (-0.5, 12.5):
            x = mid.copy()
            x[axis] = value
            out.append(x)
    for weighting in ref.WEIGHTINGS:
        got = check(e, q, u, None, np.array(out), radius=7, weighting=weighting)
        assert list(got["sides"]) == [63 - (1 << b) for b in range(6)] and (got["status"] == 5).all() and got["neighbours"].min() >= 27
        got = check(e, q, u, None, np.array(out), radius=7, weighting=weighting, require_enclosed=0)
        assert list(got["sides"]) == [63 - (1 << b) for b in range(6)] and (got["status"] == 0).all()
    # 4: coplanar and collinear POIs
    plane = q[:, 2] == 6
    got = check(e, q[plane], u[plane], None, np.array([mid, [6.4, 5.7, 6.0]]), radius=7, min_neighbours=4, require_enclosed=0)
    assert (got["status"] == 4).all() and got["neighbours"].min() >= 16
    assert list(check(e, q[plane], u[plane], None, np.array([mid, [6.4, 5.7, 6.0]]), radius=7, min_neighbours=4)["status"]) == [5, 4]
    line = plane & (q[:, 1] == 3)
    got = check(e, q[line], u[line], None, np.array([[6.4, 3.0, 6.0]]), radius=30, min_neighbours=4, weighting=0)
    assert (got["status"] == 4).all() and (got["neighbours"] == 5).all()
    # invalid and non-finite POIs are ignored whatever their byte says; duplicates each count
    valid = np.ones(len(q), np.uint8)
    valid[[31, 62]] = 0
    holes = u.copy()
    holes[63, 1] = np.nan
    holes[61, 2] = -np.inf
    holes[31] = 9.0
    got = check(e, q, holes, valid, mid[None], radius=4)
    assert (got["status"][0], got["neighbours"][0]) == (0, 23)
    dup = np.concatenate([q, q[60:66]]).astype(np.int32)
    udup = np.concatenate([u, u[60:66] + 0.02])
    got = check(e, dup, udup, None, mid[None], radius=4)
    assert (got["status"][0], got["neighbours"][0]) == (0, 30)
    # nobody contributes
    got = check(e, q, u, np.zeros(len(q), np.uint8), xs[:3], radius=6)
    assert list(got["status"]) == [1, 2, 2] and not got["neighbours"].any()


def test_continuity(e):
    """the query slides across the position where one outlying POI enters the window: the largest step-to-step change of disp is the
    restatement's, and smaller under the biweight than under uniform weights.  Measured: uniform 2.619e-01, biweight
    7.803e-03 voxels per step of 0.01."""
    q, u, xs = ref.continuity_inputs()
    bar = ref.bar(e, ref.largest_u(u))
    step = {}
    for weighting in ref.WEIGHTINGS:
        want = ref.evaluate(q, u, None, xs, weighting=weighting, **ref.CONTINUITY_OPTIONS)
        got = capi.field_eval(q, u, None, xs, weighting=weighting, **ref.CONTINUITY_OPTIONS)
        agree(got, want, bar)
        assert (got["status"] == 0).all() and got["neighbours"][-1] == got["neighbours"][0] + 1
        step[weighting] = ref.largest_step(got["disp"])
        print(f"weighting {weighting}: largest step of disp {step[weighting]:.3e}, the restatement's {ref.largest_step(want['disp']):.3e}")
        assert abs(step[weighting] - ref.largest_step(want["disp"])) <= bar
    assert step[1] < step[0]


def test_device_pointers_and_repeatability():
    import torch

    q, u, valid, xs = ref.parity_inputs()
    dev = [torch.from_numpy(a).cuda() for a in (q, u, valid, xs)]
    for radius in (2, 16):
        for weighting in ref.WEIGHTINGS:
            opts = dict(radius=radius, min_neighbours=ref.PARITY_MIN_NEIGHBOURS, weighting=weighting)
            a = capi.field_eval(q, u, valid, xs, **opts)
            assert same_bytes(a, capi.field_eval(q, u, valid, xs, **opts))
            assert same_bytes(a, capi.field_eval(*dev, **opts))
    every = capi.field_eval(dev[0], dev[1], None, dev[3], radius=7)
    assert same_bytes(every, capi.field_eval(q, u, np.ones(len(q), np.uint8), xs, radius=7))
    with pytest.raises(ValueError):
        capi.field_eval(dev[0], u, None, xs)


def test_long_call_loops_the_capped_grid(e):
    """300000 queries on 500 POIs: more than one sweep of the capped grid.  The queries are 3000 distinct positions, each 100 times,
    in an order that spreads the copies of a position over the sweeps; every one is compared."""
    rng = np.random.default_rng(14)
    q = rng.integers(0, 40, (500, 3)).astype(np.int32)
    u = ref.smooth_field(q) + rng.normal(0, 0.1, (500, 3))
    base = rng.random((3000, 3)) * 44.0 - 2.0
    pick = rng.permutation(np.repeat(np.arange(3000), 100))
    opts = dict(radius=9, min_neighbours=6)
    want = ref.evaluate(q, u, None, base, **opts)
    got = capi.field_eval(q, u, None, base[pick], **opts)
    assert len(got["status"]) == 300000
    agree(got, {k: v[pick] for k, v in want.items()}, ref.bar(e, ref.largest_u(u)))
    first = {k: got[k][np.argsort(pick, kind="stable")[::100]] for k in FIELDS}   # a copy of every position
    again = capi.field_eval(q, u, None, base, **opts)
    assert all(np.array_equal(first[k], again[k]) for k in FIELDS)


def test_empty_calls():
    xs = np.array([[1.0, 2.0, 3.0], [np.nan, 0, 0], [0.5, 0.5, 2.0 ** 25]])
    got = capi.field_eval(np.zeros((0, 3), np.int32), np.zeros((0, 3)), None, xs)
    assert list(got["status"]) == [1, 2, 2] and not got["neighbours"].any() and not got["sides"].any()
    assert not any(got[k].any() for k in ref.FLOATS)
    got = capi.field_eval(np.zeros((5, 3), np.int32), np.zeros((5, 3)), None, np.zeros((0, 3)))
    assert got["status"].shape == (0,) and got["G"].shape == (0, 3, 3) and got["disp"].shape == (0, 3) and len(got["records"]) == 0
    got = capi.field_eval(np.zeros((0, 3), np.int32), np.zeros((0, 3)), None, np.zeros((0, 3)))
    assert got["status"].shape == (0,)


def test_shell(tmp_path):
    out, _ = field_shell.run(tmp_path)
    field_shell.check_gpu_output(out)


def affine_truth(shape, L, t):
    """the displacement of x -> L (x - mid) + mid + t at positions (n, 3), as icgn_ref.scene moves its blobs"""
    mid = (np.array(shape[::-1], np.float64) - 1) / 2
    return lambda x: (np.asarray(x, np.float64) - mid) @ np.asarray(L).T + mid + np.asarray(t) - np.asarray(x, np.float64)


def rounded_start(u):
    init = np.zeros((len(u), 12))
    init[:, [0, 4, 8]] = np.round(u)
    return init


def lattice(lo, hi, step):
    g = np.arange(lo, hi + 1, step)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(np.int32)


SUBSET = 8   # IC-GN's subset radius in the chain: at 12, the radius of the IC-GN -> strain chain test, a zero start still converges at every POI


def test_chain_of_two_load_steps(e):
    """ref, mid = ref under (A1, b1), end = mid under (A2, b2) at the shape of the IC-GN -> strain chain test; the total translation is
    6.2 voxels.  Step A: IC-GN ref -> mid at 4^3 POIs; step B: IC-GN mid -> end at a 7^3 lattice of mid, both started from the truth's
    translation rounded to voxels; the field of step B at p + u_A(p), composed with step A, against the analytic total.
    Measured (INTEGRATION.md records them): eps_A = 4.639e-03, eps_B = 5.454e-03, composed error 6.975e-03 under the bar 1.019e-02;
    from zeros 11 of the 64 POIs do not converge (9 run out of iterations, 2 warp their subset out of the volume); coarse to fine seeds all 343 POIs within
    4.257e-03 of the truth."""
    shape = (96, 96, 96)
    A1, b1 = 1.01 * icgn_ref.rot(0.5, -0.4, 0.6), np.array([2.5, -1.5, 1.2])
    A2, b2 = 0.995 * icgn_ref.rot(-0.3, 0.5, 0.4), np.array([2.4, -1.6, 1.1])
    ref_vol, mid_vol, _ = icgn_ref.scene(shape, Lmat=A1, tvec=b1, seed=7)
    _, end_vol, _ = icgn_ref.scene(shape, Lmat=A2 @ A1, tvec=A2 @ b1 + b2, seed=7)
    true_a, true_b, true_t = affine_truth(shape, A1, b1), affine_truth(shape, A2, b2), affine_truth(shape, A2 @ A1, A2 @ b1 + b2)
    p = lattice(30, 66, 12)
    pb = lattice(24, 72, 8)
    assert np.abs(true_t(p) - (true_a(p) + true_b(p + true_a(p)))).max() < 1e-12 and 5.5 < np.linalg.norm(A2 @ b1 + b2) < 7.0

    res_a = capi.icgn(ref_vol, mid_vol, p, init=rounded_start(true_a(p)), subset_radius=SUBSET)
    ua, ga, va = capi.validate_input_from_icgn(res_a, zncc_min=0.5)
    res_b = capi.icgn(mid_vol, end_vol, pb, init=rounded_start(true_b(pb)), subset_radius=SUBSET)
    ub, vb = capi.strain_input_from_icgn(res_b, zncc_min=0.5)
    assert va.sum() >= 60 and vb.sum() >= 330, (res_a["status"], res_b["status"])
    eps_a = np.abs(ua - true_a(p))[va != 0].max()
    eps_b = np.abs(ub - true_b(pb))[vb != 0].max()

    at_b = check(e, pb, ub, vb, capi.field_queries(p, ua), radius=12)
    disp, grad, valid = capi.compose_displacements(ua, ga, va, at_b)
    assert np.array_equal(valid, va & (at_b["status"] == 0)) and valid.sum() >= 60
    err = np.abs(disp - true_t(p))[valid != 0].max()
    gerr = np.abs(grad.reshape(-1, 3, 3) - (A2 @ A1 - np.eye(3)))[valid != 0].max()
    bar = eps_a * (1.0 + np.abs(A2 - np.eye(3)).sum(1).max()) + eps_b + 1e-9
    print(f"eps_A = {eps_a:.3e}, eps_B = {eps_b:.3e}, composed error = {err:.3e} (bar {bar:.3e}), composed gradient error = {gerr:.3e}")
    assert err <= bar

    # the composed field starts ref -> end, which a zero start does not reach
    init, count = capi.icgn_init_from_field(disp, grad, valid, init=np.zeros((len(p), 12)))
    assert count == valid.sum()
    res = capi.icgn(ref_vol, end_vol, p, init=init, subset_radius=SUBSET)
    assert (res["status"][valid != 0] == 0).all(), res["status"]
    assert np.abs(res["displacement"] - true_t(p))[valid != 0].max() < 0.05
    cold = capi.icgn(ref_vol, end_vol, p, subset_radius=SUBSET)
    print(f"from the composed field: iterations {res['iterations'][valid != 0].max()} at most; from zeros: status counts "
          f"{np.bincount(cold['status'], minlength=7).tolist()}")
    assert (cold["status"] != 0).any()

    # coarse to fine: the measured total at the 4^3 POIs seeds a lattice twice as dense
    fine = lattice(30, 66, 6)
    total_u, _, total_v = capi.validate_input_from_icgn(res, zncc_min=0.5)
    seed = check(e, p, total_u, total_v & valid, fine.astype(np.float64), radius=25)
    su, sg, sv = capi.field_unpack(seed)
    assert sv.sum() >= 300
    init, count = capi.icgn_init_from_field(su, sg, sv, init=np.zeros((len(fine), 12)))
    dense = capi.icgn(ref_vol, end_vol, fine, init=init, subset_radius=SUBSET)
    assert (dense["status"][sv != 0] == 0).all(), dense["status"]
    print(f"coarse to fine: {sv.sum()} of {len(fine)} POIs seeded, seed error {np.abs(su - true_t(fine))[sv != 0].max():.3e}, "
          f"iterations {dense['iterations'][sv != 0].max()} at most")
