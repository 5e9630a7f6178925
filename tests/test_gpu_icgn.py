"""GPU tests of the IC-GN displacement refinement (sift3d_icgn): fixed-length runs agree with the NumPy restatement
(tests/icgn_ref.py) for every subset size and both interpolations, known deformations rendered exactly by moving isotropic blobs
are recovered, every status returns the parameters the contract names, results are reproducible bit for bit and equal for host and
device inputs, and the chain extract -> enhancedMatch -> local affine fits -> IC-GN runs on the device from Python and from C++."""
import importlib
import os
import shutil
import subprocess

import numpy as np
import pytest

import icgn_ref as ref

pytestmark = pytest.mark.gpu

capi = importlib.import_module("3dsift_amd.capi")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRAD = [k for k in range(12) if k % 4]


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.uint64), np.asarray(b, np.float64).view(np.uint64))


def perturbed(truth, rng, du, dg):
    return truth + np.where(np.arange(12) % 4 == 0, rng.uniform(-du, du, truth.shape), rng.uniform(-dg, dg, truth.shape))


@pytest.fixture(scope="module")
def agree_scene():
    return ref.scene((64, 64, 64), ref.rot(2.0, -1.0, 3.0), (0.4, -0.3, 0.25), seed=7)


# (r, POIs): the restatement costs ~ (2r+1)^3 * 64 gathers per pass
AGREE = [(r, mi, interp) for r in (2, 5, 10, 16) for mi in (1, 5) for interp in (0, 1)]


@pytest.mark.parametrize("r,max_it,interp", AGREE, ids=[f"r{a}-it{b}-{'cubic' if c == 0 else 'linear'}" for a, b, c in AGREE])
def test_agrees_with_restatement(agree_scene, r, max_it, interp):
    R, T, truth = agree_scene
    m = 40 if r <= 10 else 16
    rng = np.random.default_rng(100 * r + 10 * max_it + interp)
    q = rng.integers(r + 4, 64 - r - 5, (m, 3)).astype(np.int32)
    init = perturbed(truth(q), rng, 0.25, 0.005)
    opts = dict(subset_radius=r, max_iterations=max_it, tolerance=0.0, interpolation=interp)
    got = capi.icgn(R, T, q, init=init, **opts)
    want = ref.icgn(R, T, q, init=init, **opts)
    assert np.array_equal(got["status"], want["status"]), (got["status"], want["status"])
    assert np.array_equal(got["iterations"], want["iterations"])
    assert (got["status"] == 1).mean() >= 0.9
    dd = np.abs(got["p"][:, [0, 4, 8]] - want["p"][:, [0, 4, 8]]).max()
    dg = np.abs(got["p"][:, GRAD] - want["p"][:, GRAD]).max()
    dz = np.abs(got["zncc"] - want["zncc"]).max()
    assert dd <= 1e-4 and dg <= 1e-5 and dz <= 1e-5, (dd, dg, dz)
    assert got["seconds"] > 0


RECOVER = [("translation", np.eye(3), (0.37, -0.52, 0.21), False), ("rotation", ref.rot(4.0, -3.0, 9.0), (3.0, -2.0, 1.0), True),
           ("dilation", 1.02 * np.eye(3), (0.0, 0.0, 0.0), True)]


@pytest.mark.parametrize("name,L,t,guess", RECOVER, ids=[c[0] for c in RECOVER])
def test_recovers_known_deformation(name, L, t, guess):
    R, T, truth = ref.scene((96, 96, 96), L, t, seed=11)
    g = np.arange(30, 67, 12)
    q = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(np.int32)
    tr = truth(q)
    init = perturbed(tr, np.random.default_rng(3), 0.4, 0.01) if guess else None
    got = capi.icgn(R, T, q, init=init)
    ok = got["status"] == 0
    assert ok.mean() >= 0.9, got["status"]
    err = np.abs(got["p"] - tr)[ok]
    assert err[:, [0, 4, 8]].max() <= 0.02, err[:, [0, 4, 8]].max()
    assert err[:, GRAD].max() <= 2e-3, err[:, GRAD].max()
    assert (got["zncc"][ok] > 0.99).all()
    assert got["iterations"][ok].mean() < 20
    assert np.array_equal(got["displacement"], got["p"][:, [0, 4, 8]])
    assert np.array_equal(got["gradient"], got["p"].reshape(-1, 3, 4)[:, :, 1:])


def test_each_status():
    R, T, truth = ref.scene((48, 48, 48), tvec=(0.3, -0.2, 0.1), seed=5)
    q = np.array([[2, 24, 24], [24, 24, 24], [24, 24, 24], [24, 24, 24], [24, 24, 24]], np.int32)
    init = np.zeros((5, 12))
    init[2, 0] = 40.0     # pushes the subset out of T
    init[3, 5] = np.nan   # not finite
    got = capi.icgn(R, T, q, init=init, subset_radius=6)
    assert list(got["status"][[0, 2, 3]]) == [2, 3, 5]
    for i in (0, 2, 3):
        assert same_bits(got["p"][i], init[i]) and got["iterations"][i] == 0 and got["zncc"][i] == 0
    assert got["status"][1] == 0 and got["status"][4] == 0 and got["zncc"][1] > 0.99
    flat = capi.icgn(np.ones_like(R), T, q[1:2], subset_radius=6)
    assert (flat["status"][0], flat["iterations"][0], flat["zncc"][0]) == (4, 0, 0.0) and not flat["p"].any()
    one = capi.icgn(R, T, q[1:2], subset_radius=6, max_iterations=1, tolerance=1e-12)
    assert (one["status"][0], one["iterations"][0]) == (1, 1) and one["last_step"][0] > 0
    want = ref.icgn(R, T, q[1:2], subset_radius=6, max_iterations=1, tolerance=1e-12)
    assert np.abs(one["p"] - want["p"]).max() <= 1e-4
    # a step that leaves T: the last in-domain p is returned with its iteration count
    w = ref.refine(R, T, (24, 24, 24), init=[17.0] + [0] * 11, subset_radius=6)
    g = capi.icgn(R, T, [[24, 24, 24]], init=np.array([[17.0] + [0] * 11]), subset_radius=6)
    assert g["status"][0] == w["status"] and g["iterations"][0] == w["iterations"]


def test_reproducible_and_input_paths():
    import torch

    R, T, truth = ref.scene((64, 56, 72), ref.rot(1.0, 2.0, -1.5), (0.3, 0.2, -0.4), seed=9)
    T2 = T[2:60, 1:50, 3:70].copy()  # different dimensions: T2(x) = T(x + (3, 1, 2))
    rng = np.random.default_rng(2)
    q = np.stack([rng.integers(20, 52, 60), rng.integers(18, 38, 60), rng.integers(18, 46, 60)], 1).astype(np.int32)
    init = perturbed(truth(q), rng, 0.3, 0.005)
    a = capi.icgn(R, T, q, init=init, subset_radius=10)
    b = capi.icgn(R, T, q, init=init, subset_radius=10)
    d = capi.icgn(torch.from_numpy(R).cuda(), torch.from_numpy(T).cuda(), torch.from_numpy(q).cuda(), init=torch.from_numpy(init).cuda(),
                  subset_radius=10)
    for k in ("p", "zncc", "last_step", "iterations", "status"):
        assert same_bits(a[k], b[k]) if a[k].dtype == np.float64 else np.array_equal(a[k], b[k]), k
        assert same_bits(a[k], d[k]) if a[k].dtype == np.float64 else np.array_equal(a[k], d[k]), k
    assert (a["status"] == 0).mean() >= 0.9
    init2 = init.copy()
    init2[:, [0, 4, 8]] -= (3, 1, 2)
    c = capi.icgn(R, T2, q, init=init2, subset_radius=10)
    ok = (c["status"] == 0) & (a["status"] == 0)
    assert ok.mean() >= 0.8
    assert np.abs(c["p"][ok][:, [0, 4, 8]] + (3, 1, 2) - a["p"][ok][:, [0, 4, 8]]).max() <= 1e-3
    empty = capi.icgn(R, T, np.zeros((0, 3), np.int32))
    assert empty["p"].shape == (0, 12) and empty["status"].shape == (0,)


# ---- end to end: extraction + enhancedMatch + local affine fits + IC-GN -----------------------------------------------------------

E2E_L, E2E_T = ref.rot(4.0, -3.0, 9.0), (3.0, -2.0, 1.0)


def _chain(synth):
    size = 128
    shape = (size, size, size)
    cx, cy, cz, sg, am = synth.blob_params(shape, seed=1234)
    c = np.stack([cx, cy, cz], 1)
    mid = np.full(3, (size - 1) / 2.0)
    c2 = (c - mid) @ E2E_L.T + mid + np.asarray(E2E_T)
    R, T = ref.render(shape, c, sg, am), ref.render(shape, c2, sg, am)
    desc, xyz = [], []
    for v in (R, T):
        g = capi.CSIFT3D(v).KpSiftAlgorithm()
        kp, d = g.GetKeypoints()
        desc.append(d)
        xyz.append(np.stack([kp["rx"], kp["ry"], kp["rz"]], 1).astype(np.float32))
        g.close()
    pairs = capi.muBruteMatcher().enhancedMatch(desc[0], xyz[0], desc[1], xyz[1], 0.85)["pairs"]
    g = np.arange(28, 101, 12)
    q = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)[:, ::-1].astype(np.int32).copy()

    def truth(points):
        p = np.asarray(points, np.float64)
        u = (p - mid) @ E2E_L.T + mid + np.asarray(E2E_T) - p
        return u, E2E_L - np.eye(3)

    return R, T, pairs, q, truth


def test_end_to_end_python(synth):
    R, T, pairs, q, truth = _chain(synth)
    fits = capi.fit_affine_local(pairs, q.astype(np.float32), k=32)
    init = capi.icgn_init_from_fits(fits, q)
    got = capi.icgn(R, T, q, init=init)
    u, G = truth(q)
    ok = got["status"] == 0
    assert ok.mean() >= 0.8, np.bincount(got["status"] + 1)
    e0 = np.abs(init[:, [0, 4, 8]] - u).max(1)[ok]
    e1 = np.abs(got["displacement"] - u).max(1)[ok]
    assert np.median(e1) <= 0.25 * np.median(e0), (np.median(e1), np.median(e0))
    assert e1.max() <= 0.02, e1.max()


CXX_E2E = r"""
#include <cstdio>
#include <vector>
#include "cRegistration.h"
template <class V> static bool rd(FILE *f, V &v, size_t n) { v.resize(n); return std::fread(v.data(), sizeof(v[0]), n, f) == n; }
int main(int argc, char **argv) {
	FILE *f = std::fopen(argv[1], "rb");
	int h[3];
	std::vector<float> R, T, P;
	std::vector<int> Q;
	if (!f || std::fread(h, sizeof(int), 3, f) != 3) return 2;
	const int n = h[0], np_ = h[1], m = h[2];
	if (!rd(f, R, (size_t)n * n * n) || !rd(f, T, (size_t)n * n * n) || !rd(f, P, 6 * (size_t)np_) || !rd(f, Q, 3 * (size_t)m)) return 3;
	std::fclose(f);
	std::vector<CPUSIFT::Cvec> ref, tar, pts;
	for (int i = 0; i < np_; i++) {
		ref.push_back(CPUSIFT::Cvec(P[6 * i], P[6 * i + 1], P[6 * i + 2]));
		tar.push_back(CPUSIFT::Cvec(P[6 * i + 3], P[6 * i + 4], P[6 * i + 5]));
	}
	for (int i = 0; i < m; i++) pts.push_back(CPUSIFT::Cvec((float)Q[3 * i], (float)Q[3 * i + 1], (float)Q[3 * i + 2]));
	std::vector<CPUSIFT::AffineFit> fits = CPUSIFT::EstimateLocalAffine(ref, tar, pts, 32);
	std::vector<CPUSIFT::IcgnResult> res = CPUSIFT::RefineDisplacements(R.data(), n, n, n, T.data(), n, n, n, pts, &fits);
	for (const CPUSIFT::IcgnResult &r : res) {
		std::printf("%d %d %.17g", r.status, r.iterations, r.zncc);
		for (int k = 0; k < 12; k++) std::printf(" %.17g", r.p[k]);
		std::printf("\n");
	}
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
    R, T, pairs, q, truth = _chain(synth)
    blob = tmp_path / "in.bin"
    with open(blob, "wb") as fh:
        fh.write(np.int32([R.shape[0], len(pairs), len(q)]).tobytes())
        for a in (R, T, np.ascontiguousarray(pairs, np.float32), q):
            fh.write(np.ascontiguousarray(a).tobytes())
    out = subprocess.run([str(exe), str(blob)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    rows = np.array([[float(x) for x in line.split()] for line in out.stdout.strip().splitlines()])
    assert rows.shape == (len(q), 15)
    py = capi.icgn(R, T, q, init=capi.icgn_init_from_fits(capi.fit_affine_local(pairs, q.astype(np.float32), k=32), q))
    assert np.array_equal(rows[:, 0].astype(int), py["status"]) and np.array_equal(rows[:, 1].astype(int), py["iterations"])
    assert same_bits(rows[:, 2], py["zncc"]) and same_bits(rows[:, 3:], py["p"])
