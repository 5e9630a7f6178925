"""GPU tests of the per-body RANSAC fits (sift3d_fit_rigid_bodies, sift3d_labels_at_positions; cases: tests/body_cases.py,
restatement: tests/body_ref.py): every body's record equals rigid_ref.fit on the body's pairs with p = L -- hyp, the counts and the
statuses bit for bit, A to the refit's tolerance -- at the seams of the kernel (c around 3, the wave, the 256-pair chunk; H around the
256-hypothesis round), for one body that holds every pair and for thousands of small ones; the statuses per body; a body's record does
not depend on the other bodies' pairs, two calls and host / device inputs return the same bytes; and on the spheres scene the fits
recover every grain's rotation and start IC-GN closer to the truth near a contact than the k-nearest-pairs fits do."""
import importlib

import numpy as np
import pytest

import body_cases as cases
import body_ref as ref
import rigid_ref

pytestmark = pytest.mark.gpu

capi = importlib.import_module("3dsift_amd.capi")
MODELS = ("rigid", "similarity")
RECORD = ("A", "hyp", "status", "candidates", "best_hypothesis", "best_count", "inliers", "rms")


def same_bits(a, b):
    """the same doubles; where one holds a NaN the other does too (a NaN's sign and payload are unspecified)"""
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint64), b[~nb].view(np.uint64))


def check_fit(got, want, pairs, tau=3.0):
    """test_gpu_rigid.check_fit's rule: hyp and the counts exactly, A to the refit's tolerance, the mask away from the threshold"""
    assert got["status"] == want["status"]
    assert got["candidates"] == want["candidates"]
    assert got["best_hypothesis"] == want["best_hypothesis"]
    assert got["best_count"] == want["best_count"]
    assert same_bits(got["hyp"], want["hyp"])
    if want["status"] in (1, 2):
        assert not np.asarray(got["A"]).any() and got["inliers"] == 0 and not got["mask"].any()
        return
    A = np.asarray(got["A"], np.float64).reshape(3, 4)
    if np.isnan(want["A"]).any():
        assert same_bits(A, want["A"])
        return
    np.testing.assert_allclose(A.ravel(), want["A"], rtol=1e-9, atol=1e-9)
    with np.errstate(all="ignore"):
        d2 = ((pairs[:, :3].astype(np.float64) @ A[:, :3].T + A[:, 3] - pairs[:, 3:]) ** 2).sum(1)
    near = np.abs(d2 - tau * tau) <= 1e-6 * tau * tau
    assert np.array_equal(got["mask"][~near], want["mask"][~near])
    assert got["inliers"] == int(got["mask"].sum())
    assert abs(got["inliers"] - want["inliers"]) <= int(near.sum())


def body(got, L, rows):
    """body L's record of a call's result, with its mask bytes"""
    d = {k: got[k][L - 1] for k in RECORD}
    d["mask"] = got["mask"][rows]
    return d


def check_call(got, pairs, labels, count, tau=3.0, **opts):
    want, wmask = ref.fit_bodies(pairs, labels, count, **opts)
    assert got["A"].shape == (count, 3, 4) and got["status"].shape == (count,) and got["mask"].shape == (len(pairs),)
    for L, w in enumerate(want, 1):
        check_fit(body(got, L, w["rows"]), w, pairs[w["rows"]], tau)
    nobody = (labels < 1) | (labels > count)
    assert not got["mask"][nobody].any()
    return want


def record_bytes(got, L=None):
    """the bytes of the records (of body L), NaNs included"""
    sel = slice(None) if L is None else slice(L - 1, L)
    return b"".join(np.ascontiguousarray(got[k][sel]).tobytes() for k in RECORD)


# ---- the seams ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("H", cases.SEAM_H)
def test_seams_bit_for_bit(H):
    pairs, labels, count = cases.seams()
    for model in MODELS:
        got = capi.fit_rigid_bodies(pairs, labels, count, model=model, iterations=H, seed=H)
        want = check_call(got, pairs, labels, count, model=model, iterations=H, seed=H)
        assert got["seconds"] > 0
        assert [w["status"] for w in want[:2]] == [1, 1] and list(got["candidates"]) == list(cases.SEAM_SIZES)
        # refine = 0: the hypothesis itself, and its mask exactly
        got0 = capi.fit_rigid_bodies(pairs, labels, count, model=model, iterations=H, seed=H, refine=0)
        want0, mask0 = ref.fit_bodies(pairs, labels, count, model=model, iterations=H, seed=H, refine=0)
        for L, w in enumerate(want0, 1):
            assert same_bits(got0["hyp"][L - 1], w["hyp"]) and same_bits(got0["A"][L - 1], w["hyp"])
            assert got0["inliers"][L - 1] == w["inliers"] and (w["status"] != 0 or w["inliers"] == got0["best_count"][L - 1])
        assert np.array_equal(got0["mask"], mask0)


def test_default_iterations_and_refit_rounds():
    pairs, labels, count = cases.seams()
    got = capi.fit_rigid_bodies(pairs, labels, count)
    check_call(got, pairs, labels, count, iterations=256)    # iterations 0 means 256
    assert same_bits(got["hyp"], capi.fit_rigid_bodies(pairs, labels, count, iterations=256)["hyp"])
    for model in MODELS:
        for refine in range(5):
            got = capi.fit_rigid_bodies(pairs, labels, count, model=model, iterations=257, refine=refine)
            check_call(got, pairs, labels, count, model=model, iterations=257, refine=refine)


def test_one_body_holds_everything():
    rng = np.random.default_rng(20000)
    pairs, R, b, good = rigid_ref.synth_pairs(20000, rng, noise=0.3, outliers=0.4)
    one = capi.fit_rigid_bodies(pairs, np.ones(len(pairs), np.int32), 1)
    check_call(one, pairs, np.ones(len(pairs), np.int32), 1)
    assert one["status"][0] == 0 and one["candidates"][0] == 20000 and np.abs(one["A"][0][:, :3] - R).max() <= 2e-3
    two = capi.fit_rigid_bodies(pairs, np.full(len(pairs), 2, np.int32), 2)
    check_call(two, pairs, np.full(len(pairs), 2, np.int32), 2)
    assert two["status"][0] == 1 and two["candidates"][0] == 0 and two["status"][1] == 0
    assert two["best_hypothesis"][1] != one["best_hypothesis"][0]   # p = 2 draws other samples than p = 1


def test_many_small_bodies():
    rng = np.random.default_rng(3000)
    sizes = tuple(int(v) for v in rng.integers(3, 9, 3000))
    pairs, labels, count = cases.bodies_of(sizes, 3000, noise=0.05, outliers=0.0)
    got = capi.fit_rigid_bodies(pairs, labels, count, iterations=64)
    want = check_call(got, pairs, labels, count, iterations=64)
    assert count == 3000 and (got["status"] == 0).mean() > 0.9 and {0} <= set(got["status"])
    assert list(got["candidates"]) == list(sizes)


# ---- statuses ----------------------------------------------------------------------------------------------------------------------

def test_statuses_per_body():
    rng = np.random.default_rng(5)
    healthy_a, _, _, _ = rigid_ref.synth_pairs(100, rng, outliers=0.2)
    healthy_b, _, _, _ = rigid_ref.synth_pairs(40, rng, outliers=0.0, noise=0.1)
    line = (np.outer(rng.uniform(0, 50, 40), [1, 2, 3]) + 10).astype(np.float32)
    collinear = np.concatenate([line, line + 1], 1)                                     # status 2: every sample degenerate
    r = np.concatenate([np.outer(np.arange(20.0), [1, 2, 3]) + 10, [[50, 0, 0], [0, 60, 0]]])
    t = r + 2
    t[-2:] += 40
    pairs3 = np.concatenate([r, t], 1).astype(np.float32)                               # status 3 (test_gpu_rigid.test_statuses)
    few = healthy_a[:2]                                                                 # status 1
    groups = [healthy_a, collinear, pairs3, few, healthy_b]
    pairs = np.concatenate(groups)
    labels = np.concatenate([np.full(len(g), L, np.int32) for L, g in enumerate(groups, 1)])
    order = rng.permutation(len(pairs))
    pairs, labels = np.ascontiguousarray(pairs[order]), np.ascontiguousarray(labels[order])
    for model in MODELS:
        got = capi.fit_rigid_bodies(pairs, labels, 5, model=model, iterations=64, inlier_thresh=1.0)
        want = check_call(got, pairs, labels, 5, tau=1.0, model=model, iterations=64, inlier_thresh=1.0)
        assert list(got["status"]) == [0, 2, 3, 1, 0], got["status"]
        assert got["inliers"][2] == want[2]["inliers"] == (20 if model == "rigid" else 5) and same_bits(got["A"][2], got["hyp"][2])
        assert np.array_equal(got["mask"][labels == 3], want[2]["mask"])
        # the healthy bodies' records and mask bytes are those of the call that holds only them
        keep = np.isin(labels, (1, 5))
        alone = capi.fit_rigid_bodies(pairs[keep], labels[keep], 5, model=model, iterations=64, inlier_thresh=1.0)
        for L in (1, 5):
            assert record_bytes(got, L) == record_bytes(alone, L)
            assert np.array_equal(got["mask"][labels == L], alone["mask"][labels[keep] == L])
        assert list(alone["status"]) == [0, 1, 1, 1, 0]
        # min_det above every triangle: status 2 everywhere a fit was possible
        big = capi.fit_rigid_bodies(pairs, labels, 5, model=model, iterations=64, min_det=1e9)
        assert list(big["status"]) == [2, 2, 2, 1, 2] and not big["mask"].any() and not big["A"].any()
    # n = 0 and count = 0
    none = capi.fit_rigid_bodies(np.zeros((0, 6), np.float32), np.zeros(0, np.int32), 3)
    assert list(none["status"]) == [1, 1, 1] and list(none["candidates"]) == [0, 0, 0] and list(none["best_hypothesis"]) == [-1, -1, -1]
    zero = capi.fit_rigid_bodies(pairs, labels, 0)
    assert zero["A"].shape == (0, 3, 4) and zero["status"].shape == (0,) and not zero["mask"].any() and len(zero["mask"]) == len(pairs)


# ---- independence, determinism, input paths ----------------------------------------------------------------------------------------------

def test_independence_determinism_and_device_input():
    import torch

    pairs, labels, count = cases.seams()
    opts = dict(iterations=300, seed=9)
    a = capi.fit_rigid_bodies(pairs, labels, count, **opts)
    b = capi.fit_rigid_bodies(pairs, labels, count, **opts)
    assert record_bytes(a) == record_bytes(b) and np.array_equal(a["mask"], b["mask"])
    d = capi.fit_rigid_bodies(torch.from_numpy(pairs.copy()).cuda(), torch.from_numpy(labels.copy()).cuda(), count, **opts)
    assert record_bytes(a) == record_bytes(d) and np.array_equal(a["mask"], d["mask"])
    with pytest.raises(ValueError):
        capi.fit_rigid_bodies(torch.from_numpy(pairs.copy()).cuda(), labels[:3], count)
    rng = np.random.default_rng(12)
    for L in (3, 6, 9, 11):   # c = 3, 64, 256, 1000
        mine = np.flatnonzero(labels == L)
        others = np.flatnonzero(labels != L)
        # the other pairs permuted among their own places: body L's pairs keep their places and their order
        p2, l2 = pairs.copy(), labels.copy()
        perm = rng.permutation(others)
        p2[others], l2[others] = pairs[perm], labels[perm]
        c = capi.fit_rigid_bodies(p2, l2, count, **opts)
        assert record_bytes(a, L) == record_bytes(c, L) and np.array_equal(a["mask"][mine], c["mask"][mine])
        # body L's pairs moved to other places, in the same relative order
        places = np.sort(rng.choice(len(pairs), len(mine), replace=False))
        rest = np.setdiff1d(np.arange(len(pairs)), places)
        p3, l3 = np.empty_like(pairs), np.empty_like(labels)
        p3[places], l3[places] = pairs[mine], labels[mine]
        p3[rest], l3[rest] = pairs[others], labels[others]
        e = capi.fit_rigid_bodies(p3, l3, count, **opts)
        assert record_bytes(a, L) == record_bytes(e, L) and np.array_equal(a["mask"][mine], e["mask"][places])
        # foreign pairs turned non-finite
        p4 = pairs.copy()
        p4[others[::3]] = np.nan
        p4[others[1::3], 3:] = np.inf
        f = capi.fit_rigid_bodies(p4, labels, count, **opts)
        assert record_bytes(a, L) == record_bytes(f, L) and np.array_equal(a["mask"][mine], f["mask"][mine])


def test_labels_at_positions_on_device():
    import torch

    labels, pos = cases.position_battery()
    want = capi.labels_at_positions(labels, pos)
    assert np.array_equal(want, ref.labels_at_positions(labels, pos))
    got = capi.labels_at_positions(torch.from_numpy(labels.copy()).cuda(), torch.from_numpy(pos.copy()).cuda())
    assert got.dtype == np.int32 and np.array_equal(got, want)
    six = np.ascontiguousarray(np.concatenate([pos, pos[::-1]], 1))
    assert np.array_equal(capi.labels_at_positions(torch.from_numpy(labels.copy()).cuda(), torch.from_numpy(six).cuda()), want)
    assert len(capi.labels_at_positions(torch.from_numpy(labels.copy()).cuda(), torch.zeros((0, 3), dtype=torch.float32).cuda())) == 0
    with pytest.raises(ValueError):
        capi.labels_at_positions(torch.from_numpy(labels.copy()).cuda(), pos)


# ---- grains ------------------------------------------------------------------------------------------------------------------------

def test_grains():
    pairs, label, count = cases.grains()
    lab = cases.sphere_labels()
    assert np.array_equal(capi.labels_at_positions(lab, pairs), label)
    got = capi.fit_rigid_bodies(pairs, label, count, inlier_thresh=cases.TAU)
    want, wmask = cases.grains_reference()
    for L, w in enumerate(want, 1):
        check_fit(body(got, L, w["rows"]), w, pairs[w["rows"]], cases.TAU)
    planted, _ = cases.planted()
    rot = capi.fit_rotation(got)
    errs = []
    for L in range(1, count + 1):
        if got["candidates"][L - 1] < cases.MIN_PAIRS:
            continue
        assert got["status"][L - 1] == 0
        errs.append(cases.rotation_error(got["A"][L - 1], L))
        Rp = planted[L - 1][:, :3]
        angle = np.degrees(np.arccos(np.clip((np.trace(Rp) - 1) / 2, -1, 1)))
        # an element error of e moves the angle by at most ~ e * sqrt(2) radians
        assert abs(rot["angle_deg"][L - 1] - angle) <= np.degrees(cases.ROT_BOUND * np.sqrt(2)), (L, rot["angle_deg"][L - 1], angle)
        assert abs(rot["scale"][L - 1] - 1) <= 1e-12
    print("rotation errors", np.round(errs, 5))
    assert len(errs) == 10 and max(errs) <= cases.ROT_BOUND, errs
    # the start of IC-GN near a contact: the body's own fit against the fit of the 16 nearest pairs, whichever grain they lie in
    q, u, qlab = cases.contact_pois()
    assert np.array_equal(capi.labels_at(lab, q), qlab)
    start_body = capi.icgn_init_from_body_fits(got, qlab, q)[:, [0, 4, 8]]
    local = capi.fit_rigid_local(pairs, q.astype(np.float32), k=16, inlier_thresh=cases.TAU)
    start_local = capi.icgn_init_from_fits(local, q)[:, [0, 4, 8]]
    eb = np.abs(start_body - u).max()
    with np.errstate(invalid="ignore"):
        el = np.nanmax(np.abs(start_local - u)) if np.isfinite(start_local).any() else np.inf
    print(f"start error near a contact: body fits {eb:.4f}, local fits {el:.4f} voxel ({int(np.isnan(start_local).any(1).sum())} local fits failed)")
    assert np.isfinite(start_body).all() and eb < el
