"""GPU tests of the RANSAC rigid / similarity fits (sift3d_fit_rigid / sift3d_fit_rigid_local): the sampler, the triad and the scoring
equal the CPU restatement (tests/rigid_ref.py) bit for bit, the Horn refit equals it to the affine refit's tolerance, the statuses,
coplanar pairs (which the affine fits cannot fit), the local neighbour lists and seams, the displacement gradient a local fit hands
to IC-GN, reproducibility, device input and the C++ shell.  Sizes sit at the kernels' seams: the 256-wide hypothesis tile and pair
chunk of the global fit, 4 points per workgroup and 64 hypotheses per batch of the local fit."""
import importlib
import os
import shutil
import subprocess

import numpy as np
import pytest

import ransac_ref
import rigid_ref as ref

pytestmark = pytest.mark.gpu

capi = importlib.import_module("3dsift_amd.capi")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS = ("rigid", "similarity")


def same_bits(a, b):
    """the same doubles; where one holds a NaN the other does too (a NaN's sign and payload are unspecified)"""
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint64), b[~nb].view(np.uint64))


def check_fit(got, want, pairs, tau=3.0):
    """one fit against the restatement: hyp and the counts exactly, A to the refit's tolerance, the mask away from the threshold"""
    assert got["status"] == want["status"]
    assert got["candidates"] == want["candidates"]
    assert got["best_hypothesis"] == want["best_hypothesis"]
    assert got["best_count"] == want["best_count"]
    assert same_bits(got["hyp"], want["hyp"])
    if want["status"] in (1, 2):
        assert not np.asarray(got["A"]).any() and got["inliers"] == 0
        return
    A = np.asarray(got["A"], np.float64).reshape(3, 4)
    if np.isnan(want["A"]).any():
        assert same_bits(A, want["A"])
        return
    np.testing.assert_allclose(A.ravel(), want["A"], rtol=1e-9, atol=1e-9)
    if "mask" in got:
        with np.errstate(all="ignore"):
            d2 = ((pairs[:, :3].astype(np.float64) @ A[:, :3].T + A[:, 3] - pairs[:, 3:]) ** 2).sum(1)
        near = np.abs(d2 - tau * tau) <= 1e-6 * tau * tau
        assert np.array_equal(got["mask"][~near], want["mask"][~near])
        assert got["inliers"] == int(got["mask"].sum())
        assert abs(got["inliers"] - want["inliers"]) <= int(near.sum())


# ---- the global fit ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("H", [1, 255, 256, 257, 4096])
@pytest.mark.parametrize("n", [3, 4, 255, 256, 257, 1000])
def test_global_bit_for_bit(n, H):
    for mi, model in enumerate(MODELS):
        for outl in (0.0, 0.4):
            rng = np.random.default_rng(1000 * n + H + mi)
            pairs, R, b, good = ref.synth_pairs(n, rng, s=1.0 if mi == 0 else 1.3, noise=0.3, outliers=outl, extent=150.0)
            seed = n + H
            got = capi.fit_rigid(pairs, model=model, iterations=H, seed=seed)
            want = ref.fit(pairs, model=model, iterations=H, seed=seed)
            check_fit(got, want, pairs)
            assert got["seconds"] > 0
            if outl == 0.0:
                assert got["status"] == 0 and got["inliers"] >= 3
            # refine = 0: the hypothesis itself, and its mask exactly
            got0 = capi.fit_rigid(pairs, model=model, iterations=H, seed=seed, refine=0)
            want0 = ref.fit(pairs, model=model, iterations=H, seed=seed, refine=0)
            assert same_bits(got0["hyp"], want0["hyp"]) and same_bits(got0["A"], want0["hyp"])
            assert np.array_equal(got0["mask"], want0["mask"]) and got0["inliers"] == want0["inliers"] == got0["best_count"]


def test_refit_rounds():
    rng = np.random.default_rng(9)
    for model in MODELS:
        pairs, R, b, good = ref.synth_pairs(1000, rng, s=1.0 if model == "rigid" else 0.8, noise=0.5, outliers=0.4)
        for refine in range(5):
            got = capi.fit_rigid(pairs, model=model, refine=refine, iterations=512)
            want = ref.fit(pairs, model=model, refine=refine, iterations=512)
            assert got["status"] == 0
            check_fit(got, want, pairs)
        L = got["A"][:, :3]
        s = np.cbrt(np.linalg.det(L))
        assert np.abs(L.T @ L - s * s * np.eye(3)).max() <= 1e-12 and (model == "similarity" or abs(s - 1) <= 1e-13)
        assert np.abs(L - (1.0 if model == "rigid" else 0.8) * R).max() <= 2e-3


def test_statuses():
    rng = np.random.default_rng(5)
    for model in MODELS:
        for n in (0, 1, 2):  # fewer than 3 pairs: status 1
            f = capi.fit_rigid(np.ones((n, 6), np.float32), model=model)
            assert (f["status"], f["best_hypothesis"], f["inliers"], f["candidates"]) == (1, -1, 0, n)
            assert not f["mask"].any() and not f["A"].any() and len(f["mask"]) == n
        # every pair on one line: every sample is degenerate
        line = (np.outer(rng.uniform(0, 50, 40), [1, 2, 3]) + 10).astype(np.float32)
        f = capi.fit_rigid(np.concatenate([line, line + 1], 1), model=model, iterations=300)
        assert (f["status"], f["best_hypothesis"], f["inliers"]) == (2, -1, 0) and not f["mask"].any() and not f["A"].any()
        same = np.tile(np.float32([1, 2, 3, 4, 5, 6]), (20, 1))
        assert capi.fit_rigid(same, model=model)["status"] == 2
        # min_det above twice the area of every sample's triangle
        pairs, R, b, good = ref.synth_pairs(100, rng, outliers=0.0)
        assert capi.fit_rigid(pairs, model=model, min_det=1e9, iterations=64)["status"] == 2
        # collinear inliers under a valid hypothesis: the refit refuses, keeps the hypothesis, status 3
        r = np.concatenate([np.outer(np.arange(20.0), [1, 2, 3]) + 10, [[50, 0, 0], [0, 60, 0]]])
        t = r + 2
        t[-2:] += 40
        pairs3 = np.concatenate([r, t], 1).astype(np.float32)
        got = capi.fit_rigid(pairs3, model=model, iterations=64, inlier_thresh=1.0)
        want = ref.fit(pairs3, model=model, iterations=64, inlier_thresh=1.0)
        assert got["status"] == want["status"] == 3 and got["inliers"] == 20
        assert same_bits(got["A"], got["hyp"]) and same_bits(got["hyp"], want["hyp"])
        assert np.array_equal(got["mask"], want["mask"])


@pytest.mark.parametrize("H", [1, 64])
def test_non_finite_pairs(H):
    """a NaN or an infinity goes where the contract's IEEE operations carry it: the restatement decides"""
    rng = np.random.default_rng(31)
    seen_nan_hyp = False
    for seed in range(12):
        pairs, R, b, good = ref.synth_pairs(40, rng, noise=0.1, outliers=0.0, extent=100.0)
        bad = rng.random((40, 6))
        pairs[bad < 0.05] = np.nan
        pairs[(bad >= 0.05) & (bad < 0.12)] = np.inf
        pairs[(bad >= 0.12) & (bad < 0.15)] = -np.inf
        for model in MODELS:
            got = capi.fit_rigid(pairs, model=model, iterations=H, seed=seed)
            with np.errstate(all="ignore"):
                want = ref.fit(pairs, model=model, iterations=H, seed=seed)
            check_fit(got, want, pairs)
            seen_nan_hyp |= bool(np.isnan(want["hyp"]).any())
    allinf = np.full((10, 6), np.inf, np.float32)
    assert capi.fit_rigid(allinf, iterations=32)["status"] == 2
    if H == 1:
        assert seen_nan_hyp  # (an infinite sampled target: a NaN transform with no inlier that still is the only hypothesis)


# ---- the capability: coplanar pairs -------------------------------------------------------------------------------------------------

def _coplanar(rng, n):
    R = ref.rotation([0.2, 1.0, -0.4], 12.0)
    b = np.array([5.0, -8.0, 3.0])
    r = rng.uniform(0, 128, (n, 3))
    r[:, 2] = 17.0
    r = r.astype(np.float32)
    return np.concatenate([r, (r.astype(np.float64) @ R.T + b).astype(np.float32)], 1), R, b


def test_coplanar_pairs_global():
    pairs, R, b = _coplanar(np.random.default_rng(2), 300)
    assert capi.fit_affine(pairs, iterations=512)["status"] == 2
    for model in MODELS:
        f = capi.fit_rigid(pairs, model=model, iterations=512, inlier_thresh=0.01)
        assert f["status"] == 0 and f["inliers"] == 300 and f["mask"].all()
        # fp32 targets: 128 * 2^-24 per coordinate over lever arms of ~50 voxels and 300 pairs
        assert np.abs(f["A"][:, :3] - R).max() <= 1e-6 and np.abs(f["A"][:, 3] - b).max() <= 1e-4
        rot = capi.fit_rotation(f)
        assert abs(rot["angle_deg"] - 12.0) <= 1e-4 and abs(rot["scale"] - 1) <= 1e-6


def test_coplanar_pairs_local():
    rng = np.random.default_rng(3)
    pairs, R, b = _coplanar(rng, 2000)
    pts = np.concatenate([rng.uniform(10, 118, (50, 2)), np.full((50, 1), 17.0)], 1).astype(np.float32)
    aff = capi.fit_affine_local(pairs, pts, k=16)
    assert (aff["status"] == 2).all()
    for model in MODELS:
        f = capi.fit_rigid_local(pairs, pts, k=16, model=model, inlier_thresh=0.01)
        assert (f["status"] == 0).all() and (f["inliers"] == 16).all()
        # 16 neighbours span ~10 voxels: 128 * 2^-24 / 10 per entry, with a margin
        assert np.abs(f["A"][:, :, :3] - R).max() <= 2e-5
        assert np.abs(capi.fit_rotation(f)["angle_deg"] - 12.0).max() <= 2e-3


# ---- the local fits ------------------------------------------------------------------------------------------------------------------

def _check_local(pairs, pts, got, which, k, radius, **opts):
    want = ref.fit_local(pairs, pts, k=k, radius=radius, which=which, **opts)
    for p, w in zip(which, want):
        assert np.array_equal(got["neighbours"][p], w["neighbours"]), p
        check_fit({f: got[f][p] for f in ("A", "hyp", "status", "candidates", "best_hypothesis", "best_count", "inliers")}, w, pairs)
        assert int(got["inliers"][p]) == w["inliers"], p


LOCAL = [  # (m, k, H): 4 points per workgroup, the ends of k, 64 hypotheses per batch
    (1, 3, 1), (1, 64, 256), (4, 4, 64), (4, 63, 65), (5, 3, 65), (5, 64, 64), (257, 4, 1), (257, 16, 256), (257, 63, 64),
]


@pytest.mark.parametrize("m,k,H", LOCAL)
def test_local_bit_for_bit(m, k, H):
    rng = np.random.default_rng(100 * m + k + H)
    for mi, model in enumerate(MODELS):
        pairs, R, b, good = ref.synth_pairs(700, rng, s=1.0 if mi == 0 else 1.2, noise=0.3, outliers=0.3, extent=64.0)
        pts = rng.uniform(0, 64, (m, 3)).astype(np.float32)
        got = capi.fit_rigid_local(pairs, pts, k=k, model=model, iterations=H, seed=m + k)
        assert got["A"].shape == (m, 3, 4) and got["neighbours"].shape == (m, k) and (got["candidates"] == k).all()
        which = list(range(m)) if m <= 5 else list(range(0, m, 9)) + [m - 2, m - 1]
        _check_local(pairs, pts, got, which, k, 0.0, iterations=H, seed=m + k, model=model)


@pytest.mark.parametrize("n,c", [(2, 2), (3, 3), (64, 64), (200, 64)])
def test_local_candidates_found(n, c):
    rng = np.random.default_rng(n)
    pairs, R, b, good = ref.synth_pairs(n, rng, noise=0.2, outliers=0.0, extent=40.0)
    pts = rng.uniform(0, 40, (9, 3)).astype(np.float32)
    for model in MODELS:
        got = capi.fit_rigid_local(pairs, pts, k=64, model=model)
        assert (got["candidates"] == c).all() and (got["neighbours"][:, c:] == -1).all()
        assert (got["status"] == (1 if c < 3 else 0)).all()
        _check_local(pairs, pts, got, list(range(9)), 64, 0.0, model=model)


def test_local_ties_and_radius():
    rng = np.random.default_rng(77)
    # integer coordinates on a small grid: many equal distances, resolved by pair index
    r = rng.integers(0, 12, (3000, 3)).astype(np.float32)
    t = (r.astype(np.float64) @ ref.rotation([1, 2, 3], 4.0).T + rng.normal(0, 0.2, r.shape) + [1, 2, 3]).astype(np.float32)
    pairs = np.concatenate([r, t], 1)
    pts = np.concatenate([rng.integers(0, 12, (40, 3)), rng.uniform(-5, 17, (40, 3))]).astype(np.float32)
    for k, radius in [(64, 0.0), (3, 0.0), (17, 2.5), (32, 1.0), (64, 1.5)]:
        got = capi.fit_rigid_local(pairs, pts, k=k, radius=radius, iterations=64, seed=k)
        _check_local(pairs, pts, got, list(range(0, 80, 3)), k, radius, iterations=64, seed=k)
        if radius > 0:
            assert (got["neighbours"] < 0).any() and (got["status"] == 1).any()


def test_gradient_recovery_and_icgn_init():
    """a planted 5 degree rotation under 0.3-voxel match noise: the local rigid fit hands IC-GN a gradient without strain, closer to
    the planted one than the local affine fit of the same pairs"""
    rng = np.random.default_rng(4)
    R = ref.rotation([0.4, -0.3, 0.85], 5.0)
    pairs, _, b, good = ref.synth_pairs(6000, rng, R=R, noise=0.3, outliers=0.0, extent=128.0)
    q = rng.integers(16, 112, (256, 3)).astype(np.int32)
    qf = q.astype(np.float32)
    rig = capi.fit_rigid_local(pairs, qf, k=16)
    aff = capi.fit_affine_local(pairs, qf, k=16)
    assert (rig["status"] == 0).all() and (aff["status"] == 0).all()
    L = rig["A"][:, :, :3]
    # no strain: L^T L = I, so the Green-Lagrange strain of the init is zero to rounding ...
    assert np.abs(np.einsum("pki,pkj->pij", L, L) - np.eye(3)).max() <= 1e-12
    assert np.abs(np.linalg.det(L) - 1).max() <= 1e-12
    # ... and L - I is skew but for the second-order term (cos(angle) - 1)(I - a a^T) of the fit's own rotation
    rot = capi.fit_rotation(rig)
    v = rot["quat"][:, 1:]
    a = v / np.linalg.norm(v, axis=1)[:, None]
    second = (np.cos(np.radians(rot["angle_deg"])) - 1)[:, None, None] * (np.eye(3) - np.einsum("pi,pj->pij", a, a))
    G = L - np.eye(3)
    assert np.abs(0.5 * (G + G.transpose(0, 2, 1)) - second).max() <= 1e-12
    err_rig = np.abs(L - R).max()
    err_aff = np.abs(aff["A"][:, :, :3] - R).max()
    print("worst |L - R| over the points: rigid", err_rig, "affine", err_aff)
    assert err_rig < err_aff
    # icgn_init_from_fits takes the rigid fits as they are
    init = capi.icgn_init_from_fits(rig, q)
    A, qd = rig["A"], q.astype(np.float64)
    want = np.zeros((len(q), 12))
    for i in range(3):
        want[:, 4 * i] = (((A[:, i, 0] * qd[:, 0] + A[:, i, 1] * qd[:, 1]) + A[:, i, 2] * qd[:, 2]) + A[:, i, 3]) - qd[:, i]
        for j in range(3):
            want[:, 4 * i + 1 + j] = A[:, i, j] - (1.0 if i == j else 0.0)
    assert same_bits(init, want)
    assert np.abs(init[:, [0, 4, 8]] - (qd @ R.T + b - qd)).max() <= 1.0


def test_reproducible_and_device_input():
    import torch

    rng = np.random.default_rng(21)
    pairs, R, b, good = ref.synth_pairs(1500, rng, noise=0.3, outliers=0.5)
    pts = rng.uniform(0, 256, (301, 3)).astype(np.float32)
    dp, dq = torch.from_numpy(pairs).cuda(), torch.from_numpy(pts).cuda()
    for model in MODELS:
        a, b2, c = capi.fit_rigid(pairs, model=model), capi.fit_rigid(pairs, model=model), capi.fit_rigid(dp, model=model)
        for k in ("A", "hyp", "mask", "status", "inliers", "rms", "best_hypothesis", "best_count"):
            assert np.array_equal(np.asarray(a[k]), np.asarray(b2[k])), k
            assert np.array_equal(np.asarray(a[k]), np.asarray(c[k])), k
        la, lb, lc = (capi.fit_rigid_local(x, y, k=20, model=model) for x, y in ((pairs, pts), (pairs, pts), (dp, dq)))
        for k in ("A", "hyp", "neighbours", "status", "inliers", "rms", "best_hypothesis", "best_count"):
            assert np.array_equal(la[k], lb[k]) and np.array_equal(la[k], lc[k]), k
    assert not np.array_equal(capi.fit_rigid(pairs, model="rigid")["A"], capi.fit_rigid(pairs, model="similarity")["A"])


CXX = r"""
#include <cstdio>
#include <vector>
#include "cRegistration.h"
using namespace CPUSIFT;
static void show(const AffineFit &a) {
	double q[4], s, ang;
	FitRotation(a, q, &s, &ang);
	std::printf("%d %d", a.status, a.inliers);
	for (int i = 0; i < 12; i++) std::printf(" %.17g", a.A[i]);
	std::printf(" %.17g %.17g %.17g %.17g %.17g %.17g\n", q[0], q[1], q[2], q[3], s, ang);
}
int main(int argc, char **argv) {
	FILE *f = std::fopen(argv[1], "rb");
	int n = 0, m = 0;
	if (!f || std::fread(&n, sizeof(int), 1, f) != 1 || std::fread(&m, sizeof(int), 1, f) != 1) return 2;
	std::vector<float> p(6 * (size_t)n), q(3 * (size_t)m);
	if (std::fread(p.data(), sizeof(float), p.size(), f) != p.size() || std::fread(q.data(), sizeof(float), q.size(), f) != q.size()) return 3;
	std::fclose(f);
	std::vector<Cvec> ref, tar, pts;
	for (int i = 0; i < n; i++) {
		ref.push_back(Cvec(p[6 * i], p[6 * i + 1], p[6 * i + 2]));
		tar.push_back(Cvec(p[6 * i + 3], p[6 * i + 4], p[6 * i + 5]));
	}
	for (int i = 0; i < m; i++) pts.push_back(Cvec(q[3 * i], q[3 * i + 1], q[3 * i + 2]));
	for (int model = 0; model < 2; model++) {
		std::vector<int> mask;
		AffineFit a = EstimateRigid(ref, tar, (FitModel)model, RansacOptions(), &mask);
		int nin = 0;
		for (int v : mask) nin += v;
		if (nin != a.inliers) return 4;
		show(a);
		for (const AffineFit &l : EstimateLocalRigid(ref, tar, pts, (FitModel)model)) show(l);
	}
	return 0;
}
"""


def test_cpp_shell_agrees_with_python(tmp_path):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no host compiler")
    d = os.path.join(ROOT, "3dsift_amd")
    src = tmp_path / "rigid.cpp"
    src.write_text(CXX)
    exe = tmp_path / "rigid"
    subprocess.check_call([cxx, "-std=c++14", "-O2", "-o", str(exe), str(src), "-I", os.path.join(d, "host", "Include"), "-L" + d, "-lsift3d",
                           "-lsift3d_hip", "-Wl,-rpath," + d])
    rng = np.random.default_rng(6)
    pairs, R, b, good = ref.synth_pairs(800, rng, noise=0.3, outliers=0.4, extent=100.0)
    pts = rng.uniform(0, 100, (7, 3)).astype(np.float32)
    blob = tmp_path / "in.bin"
    with open(blob, "wb") as fh:
        fh.write(np.int32([len(pairs), len(pts)]).tobytes())
        fh.write(pairs.tobytes())
        fh.write(pts.tobytes())
    out = subprocess.run([str(exe), str(blob)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    rows = np.array([[float(x) for x in line.split()] for line in out.stdout.strip().splitlines()])
    assert rows.shape == (2 * (1 + len(pts)), 20)
    for mi, model in enumerate(MODELS):
        g = capi.fit_rigid(pairs, model=model)
        l = capi.fit_rigid_local(pairs, pts, model=model)  # (the shell's default k is the binding's: 16)
        A = np.concatenate([g["A"][None], l["A"]]).reshape(-1, 12)
        rot = capi.fit_rotation({"A": A.reshape(-1, 3, 4), "status": np.concatenate([[g["status"]], l["status"]])})
        blk = rows[mi * (1 + len(pts)):(mi + 1) * (1 + len(pts))]
        assert np.array_equal(blk[:, 0].astype(int), np.concatenate([[g["status"]], l["status"]]))
        assert np.array_equal(blk[:, 1].astype(int), np.concatenate([[g["inliers"]], l["inliers"]]))
        assert same_bits(blk[:, 2:14], A)
        assert same_bits(blk[:, 14:18], rot["quat"]) and same_bits(blk[:, 18], rot["scale"]) and same_bits(blk[:, 19], rot["angle_deg"])
        assert g["status"] == 0 and np.abs(g["A"][:, :3] - R).max() <= 2e-3
