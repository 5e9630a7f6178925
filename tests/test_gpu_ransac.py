"""GPU tests of the RANSAC affine fits (sift3d_fit_affine / sift3d_fit_affine_local): the sampler, the minimal solve and the scoring
equal the CPU restatement (tests/ransac_ref.py) bit for bit, the refit equals a least-squares fit on the same inliers, the local
neighbour lists equal the restatement exactly, known transforms are recovered -- also end to end through extraction and
enhancedMatch, from Python and from the C++ shell."""
import importlib
import os
import shutil
import subprocess

import numpy as np
import pytest

import ransac_ref as ref

pytestmark = pytest.mark.gpu

capi = importlib.import_module("3dsift_amd.capi")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.uint64), np.asarray(b, np.float64).view(np.uint64))


GLOBAL = [  # (n, H, seed, outliers)
    (4, 64, 1, 0.0), (5, 64, 2, 0.3), (63, 4096, 3, 0.5), (64, 1, 4, 0.3), (65, 65536, 5, 0.6), (1000, 4096, 6, 0.4),
    (11292, 4096, 7, 0.5), (100000, 64, 8, 0.3), (1000, 65536, 9, 0.6),
]


@pytest.mark.parametrize("n,H,seed,outl", GLOBAL)
def test_global_bit_for_bit(n, H, seed, outl):
    rng = np.random.default_rng(100 + n + seed)
    pairs, L, b, good = ref.synth_pairs(n, rng, noise=0.3, outliers=outl)
    got = capi.fit_affine(pairs, iterations=H, seed=seed, refine=0)
    want = ref.fit(pairs, iterations=H, seed=seed, refine=0)
    assert got["status"] == want["status"] == 0
    assert got["best_hypothesis"] == want["best_hypothesis"]
    assert got["best_count"] == want["best_count"] == got["inliers"]
    assert same_bits(got["hyp"].ravel(), want["hyp"]) and same_bits(got["A"].ravel(), want["hyp"])
    assert np.array_equal(got["mask"], want["mask"])
    assert got["candidates"] == n and got["seconds"] > 0


def test_too_few_pairs_status_1():
    for n in (0, 1, 3):
        f = capi.fit_affine(np.ones((n, 6), np.float32))
        assert (f["status"], f["best_hypothesis"], f["inliers"], f["candidates"]) == (1, -1, 0, n)
        assert not f["mask"].any() and not f["A"].any()


def test_degenerate_sets_status_2():
    rng = np.random.default_rng(5)
    r = rng.uniform(0, 100, (50, 3)).astype(np.float32)
    r[:, 2] = 7.0  # coplanar
    f = capi.fit_affine(np.concatenate([r, r + 1], 1), iterations=512)
    assert (f["status"], f["best_hypothesis"], f["inliers"]) == (2, -1, 0) and not f["mask"].any()
    same = np.tile(np.float32([1, 2, 3, 4, 5, 6]), (20, 1))  # all identical
    assert capi.fit_affine(same)["status"] == 2
    assert ref.fit(same)["status"] == 2


def test_four_pairs_fit_exactly():
    L = np.array([[1.25, -0.5, 0.0], [0.5, 1.0, 0.25], [0.0, -0.25, 0.75]])
    b = np.array([3.0, -7.5, 12.25])
    r = np.array([[10, 20, 30], [50, 22, 31], [12, 70, 28], [15, 25, 90]], np.float64)
    pairs = np.concatenate([r, r @ L.T + b], 1).astype(np.float32)
    f = capi.fit_affine(pairs, iterations=16, inlier_thresh=1e-3)
    assert f["status"] == 0 and f["inliers"] == 4 and f["mask"].all()
    np.testing.assert_allclose(f["A"], np.concatenate([L, b[:, None]], 1), rtol=0, atol=1e-11)
    assert same_bits(f["hyp"].ravel(), ref.fit(pairs, iterations=16, inlier_thresh=1e-3)["hyp"])


@pytest.mark.parametrize("n,seed", [(1000, 1), (11292, 2)])
def test_refit_is_least_squares(n, seed):
    rng = np.random.default_rng(seed)
    sigma = 0.3
    pairs, L, b, good = ref.synth_pairs(n, rng, noise=sigma, outliers=0.5)
    tau = 3.0
    got = capi.fit_affine(pairs, seed=seed, refine=1, inlier_thresh=tau)
    hyp = ref.fit(pairs, seed=seed, refine=0, inlier_thresh=tau)
    assert got["best_hypothesis"] == hyp["best_hypothesis"] and same_bits(got["hyp"].ravel(), hyp["hyp"])
    # one round: least squares on the inliers of the best hypothesis
    m = hyp["mask"]
    X = np.concatenate([pairs[m, :3].astype(np.float64), np.ones((m.sum(), 1))], 1)
    Y = pairs[m, 3:].astype(np.float64)
    sol = np.linalg.lstsq(X, Y, rcond=None)[0].T
    np.testing.assert_allclose(got["A"], sol, rtol=1e-9, atol=1e-9 * np.abs(sol).max())
    # the final mask: the restatement's, except pairs on the threshold to rounding
    want = ref.fit(pairs, seed=seed, refine=1, inlier_thresh=tau)
    A = got["A"]
    d2 = ((pairs[:, :3].astype(np.float64) @ A[:, :3].T + A[:, 3] - pairs[:, 3:]) ** 2).sum(1)
    near = np.abs(d2 - tau * tau) <= 1e-6 * tau * tau
    assert np.array_equal(got["mask"][~near], want["mask"][~near])
    assert got["inliers"] == int(got["mask"].sum())
    assert abs(got["rms"] - np.sqrt(d2[got["mask"]].mean())) <= 1e-5 * got["rms"]
    # the known transform, to what the noise allows: sigma / (extent * sqrt(inliers)) per entry of L, with a wide margin
    k = int(got["inliers"])
    assert k >= 0.4 * n
    tolL = 20 * sigma / (256.0 / np.sqrt(12)) / np.sqrt(k)
    assert np.abs(got["A"][:, :3] - L).max() <= tolL, np.abs(got["A"][:, :3] - L).max()
    centre = np.full(3, 128.0)
    assert np.abs(got["A"][:, :3] @ centre + got["A"][:, 3] - (L @ centre + b)).max() <= 20 * sigma / np.sqrt(k)


def test_refit_rounds_and_singular_status():
    rng = np.random.default_rng(9)
    pairs, L, b, good = ref.synth_pairs(3000, rng, noise=0.5, outliers=0.4)
    for refine in range(5):
        got = capi.fit_affine(pairs, refine=refine, iterations=1024)
        want = ref.fit(pairs, refine=refine, iterations=1024)
        assert got["status"] == want["status"] == 0
        np.testing.assert_allclose(got["A"], want["A"].reshape(3, 4), rtol=1e-9, atol=1e-9)
        assert abs(got["inliers"] - want["inliers"]) <= 2
    # min_det above every sample's |det|: every hypothesis is degenerate
    got = capi.fit_affine(pairs, min_det=1e30, iterations=64)
    assert got["status"] == 2
    r = rng.uniform(0, 100, (200, 3))
    pairs2 = np.concatenate([r, r + 2], 1).astype(np.float32)
    got = capi.fit_affine(pairs2, min_det=1e3, iterations=64, refine=2, inlier_thresh=0.5)
    want = ref.fit(pairs2, min_det=1e3, iterations=64, refine=2, inlier_thresh=0.5)
    assert got["status"] == want["status"] == 0
    # a sample passes min_det but no covariance of 4+ inliers can: the refit refuses, keeps the hypothesis, status 3
    # (unit tetrahedron: |det| of a sample 1, det of the inliers' covariance 0.25)
    four = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float64) + 10
    pairs3 = np.concatenate([four, four + 1], 1).astype(np.float32)
    got = capi.fit_affine(pairs3, min_det=0.5, iterations=8)
    want = ref.fit(pairs3, min_det=0.5, iterations=8)
    assert got["status"] == want["status"] == 3
    assert same_bits(got["A"].ravel(), got["hyp"].ravel())


def test_reproducible_and_device_input():
    import torch

    rng = np.random.default_rng(21)
    pairs, L, b, good = ref.synth_pairs(5000, rng, noise=0.3, outliers=0.5)
    pts = rng.uniform(0, 256, (777, 3)).astype(np.float32)
    a = capi.fit_affine(pairs)
    b2 = capi.fit_affine(pairs)
    dp = torch.from_numpy(pairs).cuda()
    dq = torch.from_numpy(pts).cuda()
    c = capi.fit_affine(dp)
    for k in ("A", "hyp", "mask", "status", "inliers", "rms", "best_hypothesis"):
        assert np.array_equal(np.asarray(a[k]), np.asarray(b2[k])), k
        assert np.array_equal(np.asarray(a[k]), np.asarray(c[k])), k
    la = capi.fit_affine_local(pairs, pts, k=40)
    lb = capi.fit_affine_local(pairs, pts, k=40)
    lc = capi.fit_affine_local(dp, dq, k=40)
    for k in ("A", "hyp", "neighbours", "status", "inliers", "rms", "best_hypothesis", "best_count"):
        assert same_bits(la[k], lb[k]) if la[k].dtype == np.float64 else np.array_equal(la[k], lb[k]), k
        assert same_bits(la[k], lc[k]) if la[k].dtype == np.float64 else np.array_equal(la[k], lc[k]), k


def _check_local(pairs, pts, got, which, k, radius, **opts):
    want = ref.fit_local(pairs, pts, k=k, radius=radius, which=which, **opts)
    for p, w in zip(which, want):
        assert np.array_equal(got["neighbours"][p], w["neighbours"]), p
        assert got["status"][p] == w["status"], p
        assert got["candidates"][p] == w["candidates"], p
        assert got["best_hypothesis"][p] == w["best_hypothesis"], p
        assert got["best_count"][p] == w["best_count"], p
        assert same_bits(got["hyp"][p].ravel(), w["hyp"]), p
        if w["status"] == 0:
            np.testing.assert_allclose(got["A"][p].ravel(), w["A"], rtol=1e-9, atol=1e-9)


@pytest.mark.parametrize("m,check", [(1, None), (1000, None), (100000, 400)])
def test_local_bit_for_bit(m, check):
    rng = np.random.default_rng(m)
    pairs, L, b, good = ref.synth_pairs(11292, rng, noise=0.3, outliers=0.4)
    pts = rng.uniform(0, 256, (m, 3)).astype(np.float32)
    got = capi.fit_affine_local(pairs, pts, k=32)
    assert got["A"].shape == (m, 3, 4) and got["neighbours"].shape == (m, 32)
    which = range(m) if check is None else np.sort(rng.choice(m, check, replace=False))
    _check_local(pairs, pts, got, list(which), 32, 0.0)
    assert (got["status"] == 0).mean() > 0.99


def test_local_ties_radius_and_few_pairs():
    rng = np.random.default_rng(77)
    # integer coordinates on a small grid: many equal distances, resolved by pair index
    r = rng.integers(0, 12, (3000, 3)).astype(np.float32)
    t = r + rng.normal(0, 0.2, r.shape).astype(np.float32) + np.float32([1, 2, 3])
    pairs = np.concatenate([r, t], 1)
    pts = np.concatenate([rng.integers(0, 12, (300, 3)), rng.uniform(-5, 17, (300, 3))]).astype(np.float32)
    for k, radius in [(64, 0.0), (4, 0.0), (17, 2.5), (32, 1.0), (64, 1.5)]:
        got = capi.fit_affine_local(pairs, pts, k=k, radius=radius, iterations=64, seed=k)
        _check_local(pairs, pts, got, list(range(0, 600, 7)), k, radius, iterations=64, seed=k)
        if radius > 0:
            nb = got["neighbours"]
            assert (nb < 0).any() and (got["status"] == 1).any()
    # fewer pairs than k: every pair, -1 padded; fewer than 4: status 1
    for n in (10, 3, 0):
        got = capi.fit_affine_local(pairs[:n], pts[:20], k=32)
        _check_local(pairs[:n], pts[:20], got, list(range(20)), 32, 0.0)
        assert (got["candidates"] == n).all() and (got["neighbours"][:, n:] == -1).all()
        assert (got["status"] == (1 if n < 4 else 0)).all()


def test_local_gradient_recovery():
    """a smooth displacement u(r) = a sin(2 pi r / lam) per axis: each local fit gives u and its gradient at the query point"""
    rng = np.random.default_rng(4)
    n, a, lam, ext = 100000, 2.0, 128.0, 128.0
    r = rng.uniform(0, ext, (n, 3))
    w = 2 * np.pi / lam

    def u(x):
        return np.stack([a * np.sin(w * x[:, 1]), a * np.sin(w * x[:, 2]), a * np.sin(w * x[:, 0])], 1)

    t = r + u(r) + rng.normal(0, 0.1, r.shape)
    bad = rng.random(n) < 0.3
    t[bad] = rng.uniform(0, ext, (int(bad.sum()), 3))
    pairs = np.concatenate([r, t], 1).astype(np.float32)
    q = rng.uniform(20, ext - 20, (2000, 3)).astype(np.float32)
    got = capi.fit_affine_local(pairs, q, k=64, inlier_thresh=1.0)
    assert (got["status"] == 0).all()
    qd = q.astype(np.float64)
    G = np.zeros((len(q), 3, 3))
    G[:, 0, 1] = a * w * np.cos(w * qd[:, 1])
    G[:, 1, 2] = a * w * np.cos(w * qd[:, 2])
    G[:, 2, 0] = a * w * np.cos(w * qd[:, 0])
    Gf = got["A"][:, :, :3] - np.eye(3)
    disp = np.einsum("pij,pj->pi", got["A"][:, :, :3], qd) + got["A"][:, :, 3] - qd
    # 64 neighbours at 0.7 * 100000 / 128^3 inliers per voxel span a ball of radius ~8: the curvature of u moves the local fit by
    # ~ a w^2 R^2 / 10 ~ 0.03 voxel, the noise (0.1) moves the gradient by ~ 0.1 / (3.5 sqrt(45)) ~ 0.005
    assert np.median(np.abs(Gf - G)) < 0.01 and np.percentile(np.abs(Gf - G), 99) < 0.05
    assert np.median(np.abs(disp - u(qd))) < 0.1 and np.percentile(np.abs(disp - u(qd)), 99) < 0.5


# ---- end to end: extraction + enhancedMatch + the fit ----------------------------------------------------------------------------

def render(shape, centres, sg, am):
    """synth.blobs' rendering with explicit blob centres (x, y, z): isotropic blobs moved rigidly are an exact rigid rendering"""
    nz, ny, nx = shape
    vol = np.zeros(shape, np.float64)
    for (x0, y0, z0), s, a in zip(centres, sg, am):
        rr = 5.0 * s
        xl, xh = max(0, int(np.floor(x0 - rr))), min(nx - 1, int(np.ceil(x0 + rr)))
        yl, yh = max(0, int(np.floor(y0 - rr))), min(ny - 1, int(np.ceil(y0 + rr)))
        zl, zh = max(0, int(np.floor(z0 - rr))), min(nz - 1, int(np.ceil(z0 + rr)))
        if xl > xh or yl > yh or zl > zh:
            continue
        gx = np.exp(-0.5 * ((np.arange(xl, xh + 1) - x0) / s) ** 2)
        gy = np.exp(-0.5 * ((np.arange(yl, yh + 1) - y0) / s) ** 2)
        gz = np.exp(-0.5 * ((np.arange(zl, zh + 1) - z0) / s) ** 2)
        vol[zl:zh + 1, yl:yh + 1, xl:xh + 1] += a * gz[:, None, None] * gy[None, :, None] * gx[None, None, :]
    return vol.astype(np.float32)


def rot(deg_x, deg_y, deg_z):
    ax, ay, az = np.radians([deg_x, deg_y, deg_z])
    Rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
    Ry = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]])
    Rz = np.array([[np.cos(az), -np.sin(az), 0], [np.sin(az), np.cos(az), 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


E2E = [("shift", np.eye(3), np.array([1.0, 0.0, 0.0])), ("rotation", rot(4.0, -3.0, 9.0), np.array([3.0, -2.0, 1.0]))]


def _matched_pairs(synth, R, tvec, size=128):
    shape = (size, size, size)
    cx, cy, cz, sg, am = synth.blob_params(shape, seed=1234)
    c = np.stack([cx, cy, cz], 1)
    mid = np.full(3, (size - 1) / 2.0)
    c2 = (c - mid) @ R.T + mid + tvec
    va, vb = render(shape, c, sg, am), render(shape, c2, sg, am)
    desc, xyz = [], []
    for v in (va, vb):
        g = capi.CSIFT3D(v).KpSiftAlgorithm()
        kp, d = g.GetKeypoints()
        desc.append(d)
        xyz.append(np.stack([kp["rx"], kp["ry"], kp["rz"]], 1).astype(np.float32))
        g.close()
    m = capi.muBruteMatcher().enhancedMatch(desc[0], xyz[0], desc[1], xyz[1], 0.85)
    truth = np.concatenate([R, (mid + tvec - R @ mid)[:, None]], 1)
    return m["pairs"], truth, mid


@pytest.mark.parametrize("name,R,tvec", E2E, ids=[e[0] for e in E2E])
def test_end_to_end_python(synth, name, R, tvec):
    pairs, truth, mid = _matched_pairs(synth, R, tvec)
    f = capi.fit_affine(pairs)
    assert f["status"] == 0 and f["inliers"] >= 12, (len(pairs), f["inliers"])
    A = f["A"]
    assert np.linalg.norm(A[:, :3] - truth[:, :3]) <= 0.01, (A, truth)
    assert np.abs(A[:, :3] @ mid + A[:, 3] - (truth[:, :3] @ mid + truth[:, 3])).max() <= 0.5


CXX_E2E = r"""
#include <cstdio>
#include <vector>
#include "cRegistration.h"
int main(int argc, char **argv) {
	FILE *f = std::fopen(argv[1], "rb");
	int n = 0;
	if (!f || std::fread(&n, sizeof(int), 1, f) != 1) return 2;
	std::vector<float> p(6 * (size_t)n);
	if (std::fread(p.data(), sizeof(float), p.size(), f) != p.size()) return 3;
	std::fclose(f);
	std::vector<CPUSIFT::Cvec> ref, tar;
	for (int i = 0; i < n; i++) {
		ref.push_back(CPUSIFT::Cvec(p[6 * i], p[6 * i + 1], p[6 * i + 2]));
		tar.push_back(CPUSIFT::Cvec(p[6 * i + 3], p[6 * i + 4], p[6 * i + 5]));
	}
	std::vector<int> mask;
	CPUSIFT::AffineFit a = CPUSIFT::EstimateAffine(ref, tar, CPUSIFT::RansacOptions(), &mask);
	int nin = 0;
	for (int v : mask) nin += v;
	std::printf("%d %d %d", a.status, a.inliers, nin);
	for (int i = 0; i < 12; i++) std::printf(" %.17g", a.A[i]);
	std::printf("\n");
	return 0;
}
"""


def test_end_to_end_cpp(synth, tmp_path):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no host compiler")
    d = os.path.join(ROOT, "3dsift_amd")
    src = tmp_path / "e2e.cpp"
    src.write_text(CXX_E2E)
    exe = tmp_path / "e2e"
    subprocess.check_call([cxx, "-std=c++14", "-O2", "-o", str(exe), str(src), "-I", os.path.join(d, "host", "Include"), "-L" + d, "-lsift3d",
                           "-lsift3d_hip", "-Wl,-rpath," + d])
    name, R, tvec = E2E[1]
    pairs, truth, mid = _matched_pairs(synth, R, tvec)
    blob = tmp_path / "pairs.bin"
    with open(blob, "wb") as fh:
        fh.write(np.int32(len(pairs)).tobytes())
        fh.write(np.ascontiguousarray(pairs, np.float32).tobytes())
    out = subprocess.run([str(exe), str(blob)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    v = out.stdout.split()
    status, inl, nmask = int(v[0]), int(v[1]), int(v[2])
    A = np.array([float(x) for x in v[3:15]]).reshape(3, 4)
    assert status == 0 and inl == nmask and inl >= 12
    assert np.linalg.norm(A[:, :3] - truth[:, :3]) <= 0.01
    assert np.abs(A[:, :3] @ mid + A[:, 3] - (truth[:, :3] @ mid + truth[:, 3])).max() <= 0.5
    # the shell and the Python binding run the same fit
    py = capi.fit_affine(pairs)
    assert np.array_equal(py["A"], A) and py["inliers"] == inl
