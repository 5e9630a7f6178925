"""CPU tests of the rigid / similarity fits: the restatement of the contract (tests/rigid_ref.py) against an independent SVD Kabsch,
the triad on exact samples, the degeneracy rules' common units, the mirrored set, and what the library does without a GPU --
sift3d_fit_rotation and the argument checks of the three entry points (checked before any device call)."""
import ctypes as C
import importlib
import os
import shutil
import subprocess

import numpy as np
import pytest

import ransac_ref
import rigid_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["sift3d_fit_rigid", "sift3d_fit_rigid_local", "sift3d_fit_rotation"]
ERR_ARG = 1
# the restatement against Kabsch: about 200 x the worst difference seen over 400 random sets (4.7e-15), for the different operation
# order; the offset b = tbar - L rbar carries the coordinates' size
TOL_R = 1e-12


@pytest.fixture(scope="module")
def capi():
    m = importlib.import_module("3dsift_amd.capi")
    if not os.path.exists(m.LIB_PATH):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "3dsift_amd", "csrc"), "-j8"])
    return m


def _sets():
    """(name, r, t, model, sR, b): planted transforms on coordinates up to 512 rounded to fp32, n = 3 .. 200, also planar"""
    rng = np.random.default_rng(2024)
    rots = [("identity", np.eye(3)), ("half-turn-x", ref.rotation([1, 0, 0], 180.0)), ("half-turn-d", ref.rotation([1, 1, 0], 180.0))]
    rots += [(f"random{i}", ref.rotation(rng.normal(size=3), rng.uniform(-180, 180))) for i in range(4)]
    out = []
    for name, R in rots:
        for n in (3, 4, 7, 50, 200):
            for planar in (False, True):
                for model, s in ((0, 1.0), (1, 0.5), (1, 2.0)):
                    r = rng.uniform(0, 512 if s <= 1 else 256, (n, 3))
                    if planar:
                        r[:, 2] = 100.0
                    r = r.astype(np.float32).astype(np.float64)
                    b = rng.uniform(-20, 20, 3)
                    t = (s * r @ R.T + b + rng.normal(0, 0.2, (n, 3))).astype(np.float32).astype(np.float64)
                    out.append((f"{name}-n{n}-{'plane' if planar else 'bulk'}-s{s}", r, t, model, s * R, b))
    return out


SETS = _sets()


def test_restatement_equals_kabsch():
    worst = 0.0
    for name, r, t, model, sR, b in SETS:
        A, e2 = ref.horn(r, t, 1.0, model)
        assert A is not None, name
        A = A.reshape(3, 4)
        L, off = ref.kabsch(r, t, model)
        scale = max(1.0, np.cbrt(np.linalg.det(L)))
        worst = max(worst, np.abs(A[:, :3] - L).max() / scale)
        assert np.abs(A[:, :3] - L).max() <= TOL_R * scale, (name, np.abs(A[:, :3] - L).max())
        assert np.abs(A[:, 3] - off).max() <= TOL_R * scale * (1 + np.abs(np.concatenate([r, t])).max()), name
        # a proper rotation times the scale
        s = np.cbrt(np.linalg.det(A[:, :3]))
        assert s > 0 and np.abs(A[:, :3] @ A[:, :3].T - s * s * np.eye(3)).max() <= 1e-13 * s * s, name
        if model == 0:
            assert abs(s - 1) <= 1e-14
    print("worst |L - Kabsch| / scale", worst)


def test_sweeps_needed():
    """8 sweeps are converged: more change nothing to rounding (the contract's count is not the cause of any error above)"""
    rng = np.random.default_rng(3)
    for _ in range(50):
        S = rng.normal(size=(3, 3)) * 10 ** rng.uniform(0, 6)
        N = ref.horn_matrix(S)
        lam8, V8 = ref.jacobi4(N, 8)
        lam, V = np.linalg.eigh(N)
        assert np.abs(np.sort(lam8) - lam).max() <= 1e-13 * np.abs(lam).max()
        q = V8[:, int(np.argmax(lam8))]
        assert abs(abs(q @ V[:, 3]) - 1) <= 1e-13
        assert np.abs(V8.T @ V8 - np.eye(4)).max() <= 1e-14


@pytest.mark.parametrize("model,s", [(0, 1.0), (1, 0.5), (1, 2.0)])
def test_triad_reproduces_planted_rotation(model, s):
    rng = np.random.default_rng(11)
    for R in [np.eye(3), ref.rotation([0, 0, 1], 180.0)] + [ref.rotation(rng.normal(size=3), rng.uniform(-180, 180)) for _ in range(30)]:
        P = rng.uniform(0, 256, (3, 3))
        b = rng.uniform(-30, 30, 3)
        T = s * P @ R.T + b
        A, ok = ref.triad(P[None], T[None], 1.0, model)
        assert ok[0]
        A = A[0].reshape(3, 4)
        assert np.abs(A[:, :3] - s * R).max() <= 1e-13 * max(s, 1.0)  # exact samples: rounding of the samples' own coordinates only
        assert np.abs(A[:, 3] - b).max() <= 1e-10
    # the rigid model ignores a scale in the samples; the similarity model reads it
    A, ok = ref.triad(P[None], (3.0 * P @ R.T)[None], 1.0, 0)
    assert abs(np.cbrt(np.linalg.det(A[0].reshape(3, 4)[:, :3])) - 1) <= 1e-14


def test_triad_degeneracy_rule():
    P = np.array([[0, 0, 0], [2, 0, 0], [0, 1, 0]], np.float64)  # twice the area: 2
    T = P + 5
    assert ref.triad(P[None], T[None], 2.0)[1][0] and not ref.triad(P[None], T[None], 2.0001)[1][0]
    col = np.array([[0, 0, 0], [1, 1, 1], [3, 3, 3]], np.float64)
    assert not ref.triad(col[None], T[None], 1.0)[1][0]  # collinear reference samples
    assert not ref.triad(P[None], col[None], 1.0)[1][0]  # collinear target samples: c'.c' = 0
    nan = P.copy()
    nan[1, 1] = np.nan
    assert not ref.triad(nan[None], T[None], 0.0)[1][0] and not ref.triad(P[None], nan[None], 0.0)[1][0]


def test_e2_of_three_points_is_cc_over_three():
    rng = np.random.default_rng(5)
    for _ in range(100):
        P = rng.uniform(0, 300, (3, 3))
        d = P - P.mean(0)
        c = np.cross(P[1] - P[0], P[2] - P[0])
        assert abs(ref.e2_of(d.T @ d) - (c @ c) / 3) <= 1e-11 * (c @ c)


def test_sampler_is_the_affine_samplers_first_three_draws():
    for c in (4, 5, 64, 1000):
        assert np.array_equal(ref.draws3(7, 3, 500, c), ransac_ref.draws(7, 3, 500, c)[:, :3])
    d = ref.draws3(7, 3, 500, 3)
    assert np.array_equal(np.sort(d, 1), np.tile(np.arange(3), (500, 1)))
    assert len({tuple(x) for x in d}) == 6  # every order of the three turns up


def test_mirrored_set_stays_a_rotation():
    rng = np.random.default_rng(8)
    r = rng.uniform(0, 256, (300, 3)).astype(np.float32)
    t = r * np.float32([1, 1, -1]) + np.float32([3, 4, 300])
    pairs = np.concatenate([r, t], 1)
    for model in (0, 1):
        f = ref.fit(pairs, iterations=256, model=model)
        assert f["status"] == 0
        for key in ("hyp", "A"):
            L = f[key].reshape(3, 4)[:, :3]
            assert abs(np.linalg.det(L) - 1) <= (1e-12 if model == 0 else 0.5) and np.linalg.det(L) > 0
        assert f["inliers"] <= 0.2 * len(pairs)  # a reflection is no rotation: only the pairs near the sample's plane fit


def test_restated_fit_recovers_planted_transform():
    rng = np.random.default_rng(1)
    for model, s in ((0, 1.0), (1, 1.7)):
        pairs, R, b, good = ref.synth_pairs(600, rng, s=s, noise=0.3, outliers=0.4, extent=140.0)
        f = ref.fit(pairs, iterations=512, model=model)
        assert f["status"] == 0 and f["inliers"] >= 0.9 * good.sum()
        A = f["A"].reshape(3, 4)
        assert np.abs(A[:, :3] - s * R).max() <= 2e-3 and np.abs(A[:, 3] - b).max() <= 0.3
    flat, R, b, good = ref.synth_pairs(300, rng, planar=True, outliers=0.3)
    assert ransac_ref.fit(flat, iterations=256)["status"] == 2  # the affine contract: every sample coplanar
    f = ref.fit(flat, iterations=256)
    assert f["status"] == 0 and np.abs(f["A"].reshape(3, 4)[:, :3] - R).max() <= 5e-3
    # collinear inliers under a valid hypothesis: status 3, the hypothesis kept
    line = np.outer(np.arange(20.0), [1, 2, 3]) + 10
    r = np.concatenate([line, [[50, 0, 0], [0, 60, 0]]])
    t = r + 2
    t[-2:] += 40  # the two points off the line do not fit the translation
    pairs = np.concatenate([r, t], 1).astype(np.float32)
    f = ref.fit(pairs, iterations=64, inlier_thresh=1.0)
    assert f["status"] == 3 and np.array_equal(f["A"], f["hyp"]) and f["inliers"] == 20


# ---- the library without a GPU ------------------------------------------------------------------------------------------------------

PROBE = r"""
#include "sift3d_hip.h"
int probe(const float *pairs, int n, const float *pts, int m) {
	sift3d_ransac_options o;
	sift3d_affine_fit f[2];
	unsigned char mask[4];
	int nb[64];
	double s, q[8], sc[2], an[2];
	sift3d_default_ransac_options(&o);
	return sift3d_fit_rigid(pairs, n, 0, &o, 0, 0, f, mask, &s) + sift3d_fit_rigid_local(pairs, n, pts, m, 16, 0.f, 1, &o, 0, 0, f, nb, &s) +
	       sift3d_fit_rotation(f, 2, q, sc, an);
}
"""


@pytest.mark.parametrize("lang", ["c", "c++"])
def test_header_compiles(tmp_path, lang):
    cc = shutil.which("gcc" if lang == "c" else "g++")
    if not cc:
        pytest.skip("no host compiler")
    src = tmp_path / ("probe.c" if lang == "c" else "probe.cpp")
    src.write_text(PROBE)
    std = "-std=c11" if lang == "c" else "-std=c++14"
    r = subprocess.run([cc, std, "-Wall", "-Werror", "-c", str(src), "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "probe.o")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_exports(capi):
    L = capi.lib()
    for n in NEW:
        assert hasattr(L, n), n
        assert n in capi.SYMBOLS


def test_bad_arguments_refused(capi):
    L = capi.lib()
    p = np.zeros((8, 6), np.float32)
    q = np.zeros((2, 3), np.float32)
    f = np.zeros(2, capi.FIT_DTYPE)
    P, Q, F = (a.ctypes.data_as(C.c_void_p) for a in (p, q, f))
    o = capi.RansacOptions()
    L.sift3d_default_ransac_options(C.byref(o))
    o.refine = 5
    # global: the model, n < 0, NULL pairs with n > 0, NULL output, a bad option
    for model in (-1, 2, 7, -2**31):
        assert L.sift3d_fit_rigid(P, 8, model, None, 0, 0, F, None, None) == ERR_ARG, model
        assert L.sift3d_fit_rigid_local(P, 8, Q, 2, 16, 0.0, model, None, 0, 0, F, None, None) == ERR_ARG, model
    for model in (0, 1):
        assert L.sift3d_fit_rigid(P, -1, model, None, 0, 0, F, None, None) == ERR_ARG
        assert L.sift3d_fit_rigid(None, 8, model, None, 0, 0, F, None, None) == ERR_ARG
        assert L.sift3d_fit_rigid(P, 8, model, None, 0, 0, None, None, None) == ERR_ARG
        assert L.sift3d_fit_rigid(P, 8, model, C.byref(o), 0, 0, F, None, None) == ERR_ARG
        assert b"sift3d_fit_rigid: bad argument" in L.sift3d_last_error()
        # local: n < 0, m < 0, k outside 3..64, non-finite radius, NULL pairs / points / output, a bad option
        for n, m, k, rad in [(-1, 2, 16, 0.0), (8, -1, 16, 0.0), (8, 2, 2, 0.0), (8, 2, 65, 0.0), (8, 2, 0, 0.0), (8, 2, 16, float("nan")),
                             (8, 2, 16, float("inf"))]:
            assert L.sift3d_fit_rigid_local(P, n, Q, m, k, rad, model, None, 0, 0, F, None, None) == ERR_ARG, (n, m, k, rad)
        assert L.sift3d_fit_rigid_local(None, 8, Q, 2, 16, 0.0, model, None, 0, 0, F, None, None) == ERR_ARG
        assert L.sift3d_fit_rigid_local(P, 8, None, 2, 16, 0.0, model, None, 0, 0, F, None, None) == ERR_ARG
        assert L.sift3d_fit_rigid_local(P, 8, Q, 2, 16, 0.0, model, None, 0, 0, None, None, None) == ERR_ARG
        assert L.sift3d_fit_rigid_local(P, 8, Q, 2, 16, 0.0, model, C.byref(o), 0, 0, F, None, None) == ERR_ARG
        assert b"sift3d_fit_rigid_local: bad argument" in L.sift3d_last_error()
    # the rotation: m < 0, a NULL pointer with m > 0; m = 0 needs none
    D = np.zeros(8).ctypes.data_as(C.c_void_p)
    assert L.sift3d_fit_rotation(F, -1, D, D, D) == ERR_ARG
    for args in [(None, 1, D, D, D), (F, 1, None, D, D), (F, 1, D, None, D), (F, 1, D, D, None)]:
        assert L.sift3d_fit_rotation(*args) == ERR_ARG
    assert L.sift3d_fit_rotation(None, 0, None, None, None) == 0
    with pytest.raises(ValueError):
        capi.fit_rigid(p, model="affine")


def test_fit_rotation(capi):
    rng = np.random.default_rng(17)
    cases = [(np.eye(3), 1.0, 0.0)]
    for axis in ([1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 1], [1, -2, 0.5]):  # 180 degrees: every Shepperd branch but the trace's
        cases.append((ref.rotation(axis, 180.0), 1.0, 180.0))
    for _ in range(40):
        deg = rng.uniform(0, 180)
        cases.append((ref.rotation(rng.normal(size=3), deg), float(rng.choice([1.0, 0.5, 2.0, 1.37])), deg))
    A = np.zeros((len(cases), 3, 4))
    for i, (R, s, deg) in enumerate(cases):
        A[i, :, :3] = s * R
        A[i, :, 3] = rng.uniform(-100, 100, 3)
    status = np.zeros(len(cases), np.int32)
    status[3] = 2
    got = capi.fit_rotation({"A": A, "status": status})
    for i, (R, s, deg) in enumerate(cases):
        q = got["quat"][i]
        if status[i]:
            assert np.isnan(q).all() and np.isnan(got["scale"][i]) and np.isnan(got["angle_deg"][i])
            continue
        assert abs(got["scale"][i] - s) <= 1e-14 * s
        assert abs(q @ q - 1) <= 1e-14 and q[0] >= 0
        assert np.abs(ref.rotation_of(q) - R).max() <= 1e-13, i
        # near 0 and 180 degrees the angle is the arc of a quaternion known to 1e-16: atan2 keeps it to 1e-12 degree
        assert abs(got["angle_deg"][i] - deg) <= 1e-6, (i, got["angle_deg"][i], deg)
    one = capi.fit_rotation({"A": A[7], "status": 0})
    assert np.array_equal(one["quat"], got["quat"][7]) and one["scale"] == got["scale"][7] and one["angle_deg"] == got["angle_deg"][7]
    small = ref.rotation([0, 0, 1], 1e-3)
    assert abs(capi.fit_rotation({"A": np.concatenate([small, np.zeros((3, 1))], 1), "status": 0})["angle_deg"] - 1e-3) <= 1e-12
