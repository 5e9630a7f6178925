"""GPU tests of the second-order IC-GN (sift3d_icgn2): fixed-length runs agree with the NumPy restatement (tests/icgn2_ref.py) for every
subset size and all three interpolations, the quadratic scene's displacement is recovered ten times better than by the first-order
fit, every status the restatement reaches returns the parameters the contract names (the new domain rule on its own included), results
are reproducible bit for bit and equal for host and device inputs and for coefficients made inside or outside the call, and the chain
icgn -> icgn2 -> strain runs from Python and from C++."""
import importlib
import os
import shutil
import subprocess

import numpy as np
import pytest

import icgn2_ref as ref2
import icgn_ref as ref

pytestmark = pytest.mark.gpu

capi = importlib.import_module("3dsift_amd.capi")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q = ref2.POIS
KINDS = {0: "keys", 1: "linear", 2: "bspline"}


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.uint64), np.asarray(b, np.float64).view(np.uint64))


def same_results(a, b):
    return all(same_bits(a[k], b[k]) if a[k].dtype == np.float64 else np.array_equal(a[k], b[k])
               for k in ("p", "zncc", "last_step", "iterations", "status"))


@pytest.fixture(scope="module")
def scene():
    R, T, truth = ref2.quadratic_scene()
    R.setflags(write=False)
    T.setflags(write=False)
    return R, T, truth


def perturbed(tr, rng):
    """the truth moved by up to 0.25 voxel, 0.005 and 0.0005 in the three parameter classes"""
    k = np.arange(30) % 10
    amp = np.where(k == 0, 0.25, np.where(k < 4, 0.005, 0.0005))
    return tr + rng.uniform(-1, 1, tr.shape) * amp


AGREE = [(r, kind) for r in (2, 5, 10, 16) for kind in (0, 1, 2)]


@pytest.mark.parametrize("r,kind", AGREE, ids=[f"r{r}-{KINDS[k]}" for r, k in AGREE])
def test_agrees_with_restatement(scene, r, kind):
    """bars: the project's own for u, the first derivatives and zncc (1e-4, 1e-5, 1e-5), 2e-5 / r for the second derivatives, each
    widened to 4 x the difference between the restatement's fp32 and fp64 forms on the case.
    Measured on one MI355X (GPU - fp64 restatement in u; Keys, trilinear, B-spline): r = 2: 1.6e-5, 5.5e-6, 8.9e-6 (the fp32
    restatement: 3.0e-5, 1.4e-5, 1.4e-5); r = 5: 7.2e-8, 1.1e-7, 6.2e-8; r = 10: 2.8e-8, 4.0e-8, 5.1e-8; r = 16: 3.2e-8, 3.0e-8, 2.3e-8;
    zncc <= 4e-8 everywhere.  r = 2 is the sensitive case (125 voxels for 30 parameters): it is what shows a per-voxel product
    g T' rounded to fp32, which enters b directly and is amplified by 1 / lambda_min(H)."""
    R, T, truth = scene
    init = perturbed(truth(Q), np.random.default_rng(10 * r + kind))
    opts = dict(subset_radius=r, max_iterations=3, tolerance=0.0, interpolation=kind)
    got = capi.icgn2(R, T, Q, init=init, **opts)
    want = ref2.icgn2(R, T, Q, init=init, **opts)
    w32 = ref2.icgn2(R, T, Q, init=init, f32=True, **opts)
    assert np.array_equal(got["status"], want["status"]), (got["status"], want["status"])
    assert np.array_equal(got["iterations"], want["iterations"])
    assert (want["status"] == 1).all() and (want["iterations"] == 3).all()
    bars = {"u": 1e-4, "first": 1e-5, "second": 2e-5 / r, "zncc": 1e-5}
    cols = {"u": ref2.DISP, "first": ref2.FIRST, "second": ref2.SECOND}
    for name, bar in bars.items():
        g, w, s = (got["zncc"], want["zncc"], w32["zncc"]) if name == "zncc" else (got["p"][:, cols[name]], want["p"][:, cols[name]], w32["p"][:, cols[name]])
        diff, sens = np.abs(g - w).max(), np.abs(s - w).max()
        print(f"r={r} {KINDS[kind]} {name}: GPU - restatement {diff:.3e}, fp32 - fp64 restatement {sens:.3e}, bar {max(bar, 4 * sens):.3e}")
        assert diff <= max(bar, 4 * sens), (name, diff, bar, sens)
    assert got["seconds"] > 0
    assert np.array_equal(got["displacement"], got["p"][:, ref2.DISP])
    assert np.array_equal(got["gradient"], got["p"].reshape(-1, 3, 10)[:, :, 1:4])
    assert np.array_equal(got["second"], got["p"].reshape(-1, 3, 10)[:, :, 4:]) and got["second"].shape == (len(Q), 3, 6)


@pytest.mark.parametrize("kind", [0, 2], ids=["keys", "bspline"])
def test_recovers_the_quadratic_field(scene, kind):
    """the CPU recovery test's assertion on the GPU: second order from the first-order result, and from zero, is at least ten times
    closer than first order"""
    R, T, truth = scene
    tr = truth(Q)
    first = capi.icgn(R, T, Q, subset_radius=10) if kind == 0 else capi.icgn_bspline(R, T, Q, subset_radius=10)
    assert np.isin(first["status"], (0, 1)).all()
    e1 = np.abs(first["p"][:, [0, 4, 8]] - tr[:, ref2.DISP]).max()
    for name, init in (("from first order", capi.icgn2_init_from_icgn(first)), ("from zero", None)):
        got = capi.icgn2(R, T, Q, init=init, subset_radius=10, interpolation=kind)
        assert (got["status"] == 0).all(), got["status"]
        e = np.abs(got["p"] - tr)
        print(f"{KINDS[kind]} {name}: first order {e1:.3e}; second order u {e[:, ref2.DISP].max():.3e}, first derivatives "
              f"{e[:, ref2.FIRST].max():.3e}, second derivatives {e[:, ref2.SECOND].max():.3e}; iterations {got['iterations']}")
        assert e[:, ref2.DISP].max() <= 0.1 * e1, (e[:, ref2.DISP].max(), e1)
        assert (got["zncc"] > 0.999).all()


def test_each_status(scene):
    R, T, truth = scene
    q = np.array([[2, 32, 32], [32, 32, 32], [32, 32, 32], [32, 32, 32], [32, 32, 32]], np.int32)
    init = np.zeros((5, 30))
    init[2, 0] = 40.0      # pushes the subset out of T: 3 at the start
    init[3, 17] = np.nan   # 5
    got = capi.icgn2(R, T, q, init=init, subset_radius=10)
    assert list(got["status"][[0, 2, 3]]) == [2, 3, 5]
    for i in (0, 2, 3):
        assert same_bits(got["p"][i], init[i]) and got["iterations"][i] == 0 and got["zncc"][i] == 0
    assert got["status"][1] == 0 and got["status"][4] == 0 and got["zncc"][1] > 0.99
    assert same_bits(got["p"][1], got["p"][4])
    flat = capi.icgn2(np.ones_like(R), T, q[1:2], subset_radius=10)
    assert (flat["status"][0], flat["iterations"][0], flat["zncc"][0]) == (4, 0, 0.0) and not flat["p"].any()
    one = capi.icgn2(R, T, q[1:2], subset_radius=10, max_iterations=1, tolerance=1e-12)
    assert (one["status"][0], one["iterations"][0]) == (1, 1) and one["last_step"][0] > 0
    want = ref2.icgn2(R, T, q[1:2], subset_radius=10, max_iterations=1, tolerance=1e-12)
    assert np.abs(one["p"] - want["p"])[:, ref2.DISP].max() <= 1e-4


def test_status_3_after_a_step(scene):
    """T cropped to 61 voxels along x: the zero start is inside the domain (corner 58, taps to 60), the true displacement of 1.4 voxel
    is not, so the first step leaves T: the last in-domain p (the start) is returned with the step's norm"""
    R, T, truth = scene
    Tc = np.ascontiguousarray(T[:, :, :61])
    q = (48, 32, 32)
    w = ref2.refine(R, Tc, q, subset_radius=10)
    assert w["status"] == 3 and w["last_step"] > 1.0, (w["status"], w["last_step"])
    g = capi.icgn2(R, Tc, [q], subset_radius=10)
    assert g["status"][0] == 3 and g["iterations"][0] == w["iterations"] and not g["p"].any()
    assert abs(g["last_step"][0] - w["last_step"]) <= 1e-3 and abs(g["zncc"][0] - w["zncc"]) <= 1e-5


def test_status_3_by_the_new_rule_alone(scene):
    """the affine corners lie inside T (x up to 54.4) and B_x = r^2 |cxx| / 2 = 8 pushes the widened corner to 62.4, whose taps would
    reach 64; the same init with its second-order terms zeroed runs"""
    R, T, truth = scene
    q = np.array([[44, 32, 32]], np.int32)
    init = np.zeros((1, 30))
    init[0, 0] = 0.4
    init[0, 4] = 0.16
    assert ref.in_domain(T.shape, ref2.first_order_of(init[0]), q[0], 10, True)
    assert not ref2.in_domain(T.shape, init[0], q[0], 10, True)
    got = capi.icgn2(R, T, q, init=init, subset_radius=10)
    assert (got["status"][0], got["iterations"][0], got["zncc"][0]) == (3, 0, 0.0) and same_bits(got["p"][0], init[0])
    init[0, 4] = 0.0
    runs = capi.icgn2(R, T, q, init=init, subset_radius=10)
    assert runs["status"][0] in (0, 1) and runs["iterations"][0] >= 1


def test_reproducible_and_input_paths(scene):
    import torch

    R, T, truth = scene
    init = perturbed(truth(Q), np.random.default_rng(2))
    for kind in (0, 2):
        a = capi.icgn2(R, T, Q, init=init, subset_radius=10, interpolation=kind)
        b = capi.icgn2(R, T, Q, init=init, subset_radius=10, interpolation=kind)
        d = capi.icgn2(torch.from_numpy(R.copy()).cuda(), torch.from_numpy(T.copy()).cuda(), torch.from_numpy(Q).cuda(),
                       init=torch.from_numpy(init).cuda(), subset_radius=10, interpolation=kind)
        assert same_results(a, b) and same_results(a, d), kind
        assert (a["status"] == 0).all()
    c = capi.icgn2(R, capi.bspline_prefilter(T), Q, init=init, coefficients=True, subset_radius=10, interpolation=2)
    assert same_results(a, c)
    empty = capi.icgn2(R, T, np.zeros((0, 3), np.int32))
    assert empty["p"].shape == (0, 30) and empty["status"].shape == (0,) and empty["second"].shape == (0, 3, 6)


def test_chain_to_strain(scene):
    """icgn2 -> strain_input_from_icgn2 -> strain; the fitted gradient's error is printed, not asserted (8 POIs on a 2 x 2 x 2 grid
    fit a plane to a quadratic field)"""
    R, T, truth = scene
    got = capi.icgn2(R, T, Q, subset_radius=10)
    disp, valid = capi.strain_input_from_icgn2(got)
    assert valid.all() and np.array_equal(disp, got["displacement"])
    st = capi.strain(Q, disp, valid, radius=16, min_neighbours=4)
    assert (st["status"] == 0).all(), st["status"]
    G = truth(Q).reshape(-1, 3, 10)[:, :, 1:4]
    print(f"strain: fitted gradient - truth at the POI {np.abs(st['G'] - G).max():.3e}; icgn2's own gradient - truth "
          f"{np.abs(got['gradient'] - G).max():.3e}")


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
	o.subset_radius = 10;
	std::vector<CPUSIFT::IcgnResult> first = CPUSIFT::RefineDisplacements(R.data(), n, n, n, T.data(), n, n, n, pts, nullptr, o);
	std::vector<CPUSIFT::Icgn2Result> res = CPUSIFT::RefineDisplacementsSecondOrder(R.data(), n, n, n, T.data(), n, n, n, pts, first, o);
	CPUSIFT::StrainOptions so;
	so.min_neighbours = 4;
	std::vector<CPUSIFT::StrainResult> st = CPUSIFT::ComputeStrains(pts, res, so);
	for (size_t i = 0; i < res.size(); i++) {
		double G[9], S[18];
		res[i].Gradient(G);
		res[i].SecondDerivatives(S);
		if (G[0] != res[i].p[1] || G[8] != res[i].p[23] || S[0] != res[i].p[4] || S[17] != res[i].p[29]) return 4;
		std::printf("%d %d %d %.17g", st[i].status, res[i].status, res[i].iterations, res[i].zncc);
		for (int k = 0; k < 30; k++) std::printf(" %.17g", res[i].p[k]);
		std::printf("\n");
	}
	return 0;
}
"""


def test_cpp_shell(scene, tmp_path):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no host compiler")
    d = os.path.join(ROOT, "3dsift_amd")
    src = tmp_path / "second.cpp"
    src.write_text(CXX)
    exe = tmp_path / "second"
    subprocess.check_call([cxx, "-std=c++14", "-O2", "-o", str(exe), str(src), "-I", os.path.join(d, "host", "Include"), "-L" + d, "-lsift3d",
                           "-lsift3d_hip", "-Wl,-rpath," + d])
    R, T, truth = scene
    blob = tmp_path / "in.bin"
    with open(blob, "wb") as fh:
        fh.write(np.int32([R.shape[0], len(Q)]).tobytes())
        for a in (R, T, Q):
            fh.write(np.ascontiguousarray(a).tobytes())
    out = subprocess.run([str(exe), str(blob)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    rows = np.array([[float(x) for x in line.split()] for line in out.stdout.strip().splitlines()])
    assert rows.shape == (len(Q), 34)
    py = capi.icgn2(R, T, Q, init=capi.icgn2_init_from_icgn(capi.icgn(R, T, Q, subset_radius=10)), subset_radius=10)
    assert (rows[:, 0] == 0).all()
    assert np.array_equal(rows[:, 1].astype(int), py["status"]) and np.array_equal(rows[:, 2].astype(int), py["iterations"])
    assert same_bits(rows[:, 3], py["zncc"]) and same_bits(rows[:, 4:], py["p"])
