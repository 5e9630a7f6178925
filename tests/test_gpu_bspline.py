"""GPU tests of the cubic B-spline interpolation (sift3d_bspline_prefilter, sift3d_icgn_bspline): the prefilter agrees with the NumPy
restatement (tests/bspline_ref.py) on axes shorter than the filter, axes of length 1, sizes off every tile and across tile seams,
keeps constants and the restatement's non-finite footprint, and returns the same bytes for host and device volumes and for two
calls; the IC-GN mode agrees with the restatement at every subset size class, returns the same bytes whichever way it gets its
coefficients, reports every status the contract names, recovers known deformations at least four times more accurately than the
Keys mode, and runs from the C++ shell and in the chain to strain."""
import importlib
import os
import shutil
import subprocess

import numpy as np
import pytest

import bspline_ref as bref
import icgn_ref as ref

pytestmark = pytest.mark.gpu

capi = importlib.import_module("3dsift_amd.capi")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRAD = [k for k in range(12) if k % 4]
KEYS = ("p", "zncc", "last_step", "iterations", "status")


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def same_results(a, b):
    return all(same_bits(a[k], b[k]) for k in KEYS)


def perturbed(truth, rng, du, dg):
    return truth + np.where(np.arange(12) % 4 == 0, rng.uniform(-du, du, truth.shape), rng.uniform(-dg, dg, truth.shape))


# ---- the prefilter ----------------------------------------------------------------------------------------------------------------

SHAPES = [(5, 1, 7), (2, 2, 2), (33, 17, 70), (3, 3, 300), (64, 64, 64)]
INPUTS = ("noise", "blobs", "constant", "ct")


def volume(shape, kind):
    rng = np.random.default_rng(sum(shape) + len(kind))
    if kind == "noise":
        return rng.uniform(-1, 1, shape).astype(np.float32)
    if kind == "blobs":
        return ref.scene(shape, seed=3)[0]
    if kind == "constant":
        return np.full(shape, 1234.5678, np.float32)
    return np.round(30000 + 200 * rng.standard_normal(shape)).astype(np.float32)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("kind", INPUTS)
def test_prefilter_agrees_with_restatement(shape, kind):
    T = volume(shape, kind)
    got = capi.bspline_prefilter(T)
    assert got.dtype == np.float32 and got.shape == T.shape
    exact, rounded = bref.prefilter(T), bref.prefilter(T, f32=True)
    e = np.abs(rounded - exact).max()
    err = np.abs(got - exact).max()
    bar = 4 * e + 1e-7 * np.abs(T).max()
    print(f"{shape} {kind}: max |GPU - fp64| = {err:.3e}, e = {e:.3e}, bar {bar:.3e}")
    assert err <= bar, (err, e, bar)
    if kind == "constant":
        assert same_bits(got, T)


@pytest.mark.parametrize("shape,at", [((64, 64, 64), (31, 30, 33)), ((33, 17, 70), (16, 8, 40)), ((3, 3, 300), (1, 2, 150)), ((5, 1, 7), (2, 0, 3))],
                         ids=["64", "33x17x70", "3x3x300", "5x1x7"])
def test_prefilter_non_finite_footprint(shape, at):
    for bad in (np.nan, np.inf):
        T = volume(shape, "noise")
        clean = capi.bspline_prefilter(T)
        T[at] = bad
        got = capi.bspline_prefilter(T)
        want = ~np.isfinite(bref.prefilter(T, f32=True))
        assert np.array_equal(~np.isfinite(got), want), bad
        assert same_bits(got[~want], clean[~want]), bad
    if shape == (64, 64, 64):  # an interior voxel: exactly the (2K+1)^3 cube
        cube = np.zeros(shape, bool)
        cube[15:48, 14:47, 17:50] = True
        assert np.array_equal(want, cube)


def test_prefilter_input_paths_and_repeats():
    import torch

    for shape in ((33, 17, 70), (64, 64, 64)):
        T = volume(shape, "ct")
        a, b = capi.bspline_prefilter(T), capi.bspline_prefilter(T)
        d, sec = capi.bspline_prefilter(torch.from_numpy(T).cuda(), with_seconds=True)
        assert same_bits(a, b) and same_bits(a, d.cpu().numpy()) and sec > 0
    t = torch.zeros((4, 4, 4), device="cuda")
    assert capi.lib().sift3d_bspline_prefilter(t.data_ptr(), 4, 4, 4, t.data_ptr(), 1, 0, None) == 1   # in place: refused


# ---- IC-GN on the coefficients ------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def agree_scene():
    R, T, truth = ref.scene((64, 64, 64), ref.rot(2.0, -1.0, 3.0), (0.4, -0.3, 0.25), seed=7)
    return R, T, truth, bref.prefilter(T, f32=True)


AGREE = [(2, 3), (5, 3), (10, 2), (16, 2)]


@pytest.mark.parametrize("r,max_it", AGREE, ids=[f"r{a}-it{b}" for a, b in AGREE])
def test_icgn_agrees_with_restatement(agree_scene, r, max_it):
    R, T, truth, coef = agree_scene
    m = 24 if r <= 10 else 8
    rng = np.random.default_rng(100 * r + 10 * max_it)
    q = rng.integers(r + 4, 64 - r - 5, (m, 3)).astype(np.int32)
    init = perturbed(truth(q), rng, 0.25, 0.005)
    opts = dict(subset_radius=r, max_iterations=max_it, tolerance=0.0)
    got = capi.icgn_bspline(R, T, q, init=init, **opts)
    want = bref.icgn(R, coef, q, init=init, coefficients_given=True, **opts)
    assert np.array_equal(got["status"], want["status"]), (got["status"], want["status"])
    assert np.array_equal(got["iterations"], want["iterations"])
    assert (got["status"] == 1).mean() >= 0.9
    dd = np.abs(got["p"][:, [0, 4, 8]] - want["p"][:, [0, 4, 8]]).max()
    dg = np.abs(got["p"][:, GRAD] - want["p"][:, GRAD]).max()
    dz = np.abs(got["zncc"] - want["zncc"]).max()
    print(f"r {r}: max difference displacement {dd:.3e}, gradient {dg:.3e}, zncc {dz:.3e}")
    assert dd <= 1e-4 and dg <= 1e-5 and dz <= 1e-5, (dd, dg, dz)
    assert got["seconds"] > 0


def test_coefficient_paths():
    import torch

    R, T, truth = ref.scene((64, 56, 72), ref.rot(1.0, 2.0, -1.5), (0.3, 0.2, -0.4), seed=9)
    rng = np.random.default_rng(2)
    q = np.stack([rng.integers(20, 52, 40), rng.integers(18, 38, 40), rng.integers(18, 46, 40)], 1).astype(np.int32)
    init = perturbed(truth(q), rng, 0.3, 0.005)
    a = capi.icgn_bspline(R, T, q, init=init, subset_radius=10)
    assert (a["status"] == 0).mean() >= 0.9
    assert same_results(a, capi.icgn_bspline(R, T, q, init=init, subset_radius=10))
    coef = capi.bspline_prefilter(T)
    assert same_results(a, capi.icgn_bspline(R, coef, q, init=init, coefficients=True, subset_radius=10))
    dR, dT, dq, di = (torch.from_numpy(v).cuda() for v in (R, T, q, init))
    assert same_results(a, capi.icgn_bspline(dR, dT, dq, init=di, subset_radius=10))
    assert same_results(a, capi.icgn_bspline(dR, capi.bspline_prefilter(dT), dq, init=di, coefficients=True, subset_radius=10))
    # not the Keys mode under another name, and the Keys mode is as it was
    k = capi.icgn(R, T, q, init=init, subset_radius=10)
    assert not same_bits(k["p"], a["p"]) and np.abs(k["p"] - a["p"])[:, [0, 4, 8]].max() < 0.05
    with pytest.raises(capi.Sift3dError):
        capi.icgn_bspline(R, T, q, interpolation=1)
    empty = capi.icgn_bspline(R, T, np.zeros((0, 3), np.int32))
    assert empty["p"].shape == (0, 12) and empty["status"].shape == (0,)


def test_each_status():
    R, T, truth = ref.scene((48, 48, 48), tvec=(0.3, -0.2, 0.1), seed=5)
    q = np.array([[2, 24, 24], [24, 24, 24], [24, 24, 24], [24, 24, 24], [24, 24, 24]], np.int32)
    init = np.zeros((5, 12))
    init[2, 0] = 40.0     # starts outside T's domain
    init[3, 5] = np.nan   # not finite
    got = capi.icgn_bspline(R, T, q, init=init, subset_radius=6)
    want = bref.icgn(R, T, q, init=init, subset_radius=6)
    assert list(got["status"]) == list(want["status"]) and list(got["status"][[0, 2, 3]]) == [2, 3, 5]
    for i in (0, 2, 3):
        assert same_bits(got["p"][i], init[i]) and got["iterations"][i] == 0 and got["zncc"][i] == 0
    assert got["status"][1] == 0 and got["status"][4] == 0 and got["zncc"][1] > 0.99
    # 4: R flat; T constant (dT = 0 exactly: constant coefficients, taps shifted before they are weighted)
    flat = capi.icgn_bspline(np.ones_like(R), T, q[1:2], subset_radius=6)
    assert (flat["status"][0], flat["iterations"][0], flat["zncc"][0]) == (4, 0, 0.0) and not flat["p"].any()
    for c in (0.0, 1234.5678):
        const = capi.icgn_bspline(R, np.full_like(T, c), q[1:2], subset_radius=6)
        w = bref.refine(R, np.full_like(T, c), q[1], subset_radius=6)
        assert (const["status"][0], const["iterations"][0], const["zncc"][0]) == (4, 0, 0.0) == (w["status"], w["iterations"], w["zncc"])
        assert not const["p"].any()
    # 3 after a step: the last in-domain p is returned with its iteration count
    # (u = 15: the corner at x = 24 + 6 + 15 = 45 has its last tap at 47 = n - 1, so the start is inside; the update leaves)
    start = np.array([[15.0] + [0] * 11])
    w = bref.refine(R, T, (24, 24, 24), init=start[0], subset_radius=6)
    g = capi.icgn_bspline(R, T, [[24, 24, 24]], init=start, subset_radius=6)
    assert w["status"] == 3 and w["iterations"] >= 1 and len(w["steps"]) == w["iterations"] + 1
    assert (g["status"][0], g["iterations"][0]) == (3, w["iterations"]) and g["last_step"][0] > 0
    assert not same_bits(g["p"][0], start[0])   # the last in-domain p, not the start
    # the parity bars (1e-4 voxel, 1e-5 gradient) are set for starts within 0.25 voxel of the answer; the fp32 interpolation error
    # enters a step in proportion to the residual, so for this far start they scale with the first step's norm over 0.25
    k = max(1.0, w["steps"][0] / 0.25)
    assert np.abs(g["p"][0] - w["p"])[[0, 4, 8]].max() <= 1e-4 * k and np.abs(g["p"][0] - w["p"])[GRAD].max() <= 1e-5 * k
    assert abs(g["last_step"][0] - w["last_step"]) <= 1e-3 * w["last_step"]


def test_nan_voxel_reach():
    """a NaN voxel of T: a POI whose subset sees it through the prefilter's footprint gets the restatement's status; a POI more than
    K + r + 2 voxels away is untouched, to the bytes of a run without the NaN"""
    r = 6
    R, T, truth = ref.scene((48, 48, 96), tvec=(0.3, -0.2, 0.1), seed=5)
    q = np.array([[14, 24, 24], [30, 24, 24], [12 + bref.K + r + 2 + 2, 24, 24], [80, 24, 24]], np.int32)
    clean = capi.icgn_bspline(R, T, q, subset_radius=r)
    Tn = T.copy()
    Tn[24, 24, 12] = np.nan
    got = capi.icgn_bspline(R, Tn, q, subset_radius=r)
    want = bref.icgn(R, Tn, q, subset_radius=r)
    assert np.array_equal(got["status"], want["status"]) and np.array_equal(got["iterations"], want["iterations"])
    assert got["status"][0] != 0 and got["status"][1] != 0   # inside the subset; outside it but inside the filter's reach
    for i in (2, 3):
        assert all(same_bits(got[k][i], clean[k][i]) for k in KEYS), i


# ---- accuracy ----------------------------------------------------------------------------------------------------------------------

RECOVER = [("translation", np.eye(3), (0.37, -0.52, 0.21), False), ("rotation", ref.rot(4.0, -3.0, 9.0), (3.0, -2.0, 1.0), True),
           ("dilation", 1.02 * np.eye(3), (0.0, 0.0, 0.0), True)]


@pytest.mark.parametrize("name,L,t,guess", RECOVER, ids=[c[0] for c in RECOVER])
def test_recovers_known_deformation_four_times_better(name, L, t, guess):
    R, T, truth = ref.scene((96, 96, 96), L, t, seed=11)
    g = np.array([28, 48, 68])
    q = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(np.int32)
    tr = truth(q)
    init = perturbed(tr, np.random.default_rng(3), 0.4, 0.01) if guess else None
    keys = capi.icgn(R, T, q, init=init, subset_radius=12)
    bsp = capi.icgn_bspline(R, T, q, init=init, subset_radius=12)
    assert (keys["status"] == 0).all() and (bsp["status"] == 0).all(), (keys["status"], bsp["status"])
    ek, eb = np.abs(keys["p"] - tr), np.abs(bsp["p"] - tr)
    print(f"{name}: max displacement error Keys {ek[:, [0, 4, 8]].max():.3e}, B-spline {eb[:, [0, 4, 8]].max():.3e}; "
          f"max gradient error Keys {ek[:, GRAD].max():.3e}, B-spline {eb[:, GRAD].max():.3e}")
    assert eb[:, [0, 4, 8]].max() <= 0.25 * ek[:, [0, 4, 8]].max()
    assert (bsp["zncc"] > 0.99).all()


def test_chain_icgn_bspline_to_strain():
    """test_gpu_strain.test_chain_icgn_to_strain's scene (96^3 dilated by 1.02, a 4 x 4 x 4 grid, r = 12, strain window 36) with the
    B-spline call: the error of E against the true (1.02^2 - 1) / 2 I is printed next to the Keys figure, not asserted"""
    R, T, truth = ref.scene((96, 96, 96), Lmat=1.02 * np.eye(3), seed=7)
    g = np.arange(30, 67, 12)
    q = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(np.int32)
    true_e = np.array([0.5 * (1.02 ** 2 - 1)] * 3 + [0.0] * 3)
    line = []
    for name, res in (("Keys", capi.icgn(R, T, q, subset_radius=12)), ("B-spline", capi.icgn_bspline(R, T, q, subset_radius=12))):
        disp, valid = capi.strain_input_from_icgn(res, zncc_min=0.5)
        assert valid.sum() >= 48, (name, res["status"], res["zncc"])
        got = capi.strain(q, disp, valid, radius=36)
        assert (got["status"] == 0).all()
        ok = valid != 0
        line.append(f"{name}: max |E - true| = {np.abs(got['E'] - true_e).max():.3e}, max |u - true| = "
                    f"{np.abs(disp[ok] - truth(q)[ok][:, [0, 4, 8]]).max():.3e}")
    print("; ".join(line))


# ---- the C++ shell -----------------------------------------------------------------------------------------------------------------

CXX = r"""
#include <cstdio>
#include <vector>
#include "cRegistration.h"
template <class V> static bool rd(FILE *f, V &v, size_t n) { v.resize(n); return std::fread(v.data(), sizeof(v[0]), n, f) == n; }
int main(int argc, char **argv) {
	FILE *f = std::fopen(argv[1], "rb");
	int h[2];
	std::vector<float> R, T;
	std::vector<int> Q;
	if (!f || std::fread(h, sizeof(int), 2, f) != 2) return 2;
	const int n = h[0], m = h[1];
	if (!rd(f, R, (size_t)n * n * n) || !rd(f, T, (size_t)n * n * n) || !rd(f, Q, 3 * (size_t)m)) return 3;
	std::fclose(f);
	std::vector<CPUSIFT::Cvec> pts;
	for (int i = 0; i < m; i++) pts.push_back(CPUSIFT::Cvec((float)Q[3 * i], (float)Q[3 * i + 1], (float)Q[3 * i + 2]));
	CPUSIFT::IcgnOptions o;
	o.subset_radius = 6;
	o.interpolation = 2;
	std::vector<float> C(T.size());
	if (!CPUSIFT::PrefilterBSpline(T.data(), n, n, n, C.data())) return 4;
	for (int pass = 0; pass < 2; pass++) {
		std::vector<CPUSIFT::IcgnResult> res = pass == 0 ? CPUSIFT::RefineDisplacements(R.data(), n, n, n, T.data(), n, n, n, pts, nullptr, o)
		                                                 : CPUSIFT::RefineDisplacements(R.data(), n, n, n, C.data(), n, n, n, pts, nullptr, o, nullptr, true);
		for (const CPUSIFT::IcgnResult &r : res) {
			std::printf("%d %d %.17g", r.status, r.iterations, r.zncc);
			for (int k = 0; k < 12; k++) std::printf(" %.17g", r.p[k]);
			std::printf("\n");
		}
	}
	return 0;
}
"""


def test_host_shell(tmp_path):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no host compiler")
    d = os.path.join(ROOT, "3dsift_amd")
    src = tmp_path / "bspline.cpp"
    src.write_text(CXX)
    exe = tmp_path / "bspline"
    subprocess.check_call([cxx, "-std=c++14", "-O2", "-o", str(exe), str(src), "-I", os.path.join(d, "host", "Include"), "-L" + d, "-lsift3d",
                           "-lsift3d_hip", "-Wl,-rpath," + d])
    R, T, truth = ref.scene((48, 48, 48), ref.rot(1.0, -1.0, 2.0), (0.3, -0.2, 0.1), seed=5)
    g = np.array([18, 30])
    q = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(np.int32)
    blob = tmp_path / "in.bin"
    with open(blob, "wb") as fh:
        fh.write(np.int32([R.shape[0], len(q)]).tobytes())
        for a in (R, T, q):
            fh.write(np.ascontiguousarray(a).tobytes())
    out = subprocess.run([str(exe), str(blob)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    rows = np.array([[float(x) for x in line.split()] for line in out.stdout.strip().splitlines()])
    assert rows.shape == (2 * len(q), 15)
    py = capi.icgn_bspline(R, T, q, subset_radius=6)
    assert (py["status"] == 0).all()
    for part in (rows[:len(q)], rows[len(q):]):
        assert np.array_equal(part[:, 0].astype(int), py["status"]) and np.array_equal(part[:, 1].astype(int), py["iterations"])
        assert same_bits(part[:, 2], py["zncc"]) and same_bits(part[:, 3:], py["p"])
