"""CPU tests of the RANSAC affine fits' boundary (sift3d_fit_affine / sift3d_fit_affine_local, include/sift3d_hip.h): the header compiles
as C and C++ with its layout guards, the library exports the entry points, the defaults need no GPU, bad arguments are refused before
any device call, the CPU restatement (tests/ransac_ref.py) recovers a known affine, and the C++ shell's cRegistration.h links."""
import ctypes as C
import importlib
import os
import shutil
import subprocess

import numpy as np
import pytest

import ransac_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["sift3d_default_ransac_options", "sift3d_fit_affine", "sift3d_fit_affine_local"]
ERR_ARG = 1


@pytest.fixture(scope="module")
def capi():
    m = importlib.import_module("3dsift_amd.capi")
    if not os.path.exists(m.LIB_PATH):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "3dsift_amd", "csrc"), "-j8"])
    return m


PROBE = r"""
#include <stddef.h>
#include "sift3d_hip.h"
SIFT3D_STATIC_ASSERT(sizeof(sift3d_ransac_options) == 32, "options");
SIFT3D_STATIC_ASSERT(offsetof(sift3d_ransac_options, min_det) == 16 && offsetof(sift3d_ransac_options, reserved) == 20, "options offsets");
SIFT3D_STATIC_ASSERT(sizeof(sift3d_affine_fit) == 224, "fit");
SIFT3D_STATIC_ASSERT(offsetof(sift3d_affine_fit, hyp) == 96 && offsetof(sift3d_affine_fit, status) == 192 &&
                     offsetof(sift3d_affine_fit, inliers) == 208 && offsetof(sift3d_affine_fit, rms) == 212, "fit offsets");
int probe(const float *pairs, int n, const float *pts, int m) {
	sift3d_ransac_options o;
	sift3d_affine_fit f[2];
	unsigned char mask[4];
	int nb[64];
	double s;
	sift3d_default_ransac_options(&o);
	o.iterations = 512;
	return sift3d_fit_affine(pairs, n, &o, 0, 0, f, mask, &s) + sift3d_fit_affine_local(pairs, n, pts, m, 32, 0.f, &o, 0, 0, f, nb, &s);
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


def test_defaults_without_gpu(capi):
    o = capi.RansacOptions()
    C.memset(C.byref(o), 0x5A, C.sizeof(o))
    capi.lib().sift3d_default_ransac_options(C.byref(o))
    assert (o.iterations, o.inlier_thresh, o.seed, o.refine, o.min_det) == (0, 3.0, 1, 1, 1.0)
    assert list(o.reserved) == [0, 0, 0]
    assert capi.default_ransac_options() == {"iterations": 0, "inlier_thresh": 3.0, "seed": 1, "refine": 1, "min_det": 1.0}
    assert capi.FIT_DTYPE.itemsize == 224 and capi.FIT_DTYPE.fields["status"][1] == 192 and capi.FIT_DTYPE.fields["rms"][1] == 212


def _opts(capi, **kw):
    o = capi.RansacOptions()
    capi.lib().sift3d_default_ransac_options(C.byref(o))
    for k, v in kw.items():
        if k == "reserved":
            o.reserved[v] = 1
        else:
            setattr(o, k, v)
    return o


BAD_OPTS = [dict(iterations=-1), dict(iterations=65537), dict(refine=-1), dict(refine=5), dict(inlier_thresh=float("nan")),
            dict(inlier_thresh=float("inf")), dict(inlier_thresh=-1.0), dict(min_det=float("nan")), dict(min_det=float("inf")),
            dict(reserved=0), dict(reserved=2)]


@pytest.mark.parametrize("bad", BAD_OPTS, ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))
def test_bad_options_refused(capi, bad):
    L = capi.lib()
    p = np.zeros((8, 6), np.float32)
    q = np.zeros((2, 3), np.float32)
    o = _opts(capi, **bad)
    f = np.zeros(2, capi.FIT_DTYPE)
    assert L.sift3d_fit_affine(p.ctypes.data_as(C.c_void_p), 8, C.byref(o), 0, 0, f.ctypes.data_as(C.c_void_p), None, None) == ERR_ARG
    assert L.sift3d_fit_affine_local(p.ctypes.data_as(C.c_void_p), 8, q.ctypes.data_as(C.c_void_p), 2, 32, 0.0, C.byref(o), 0, 0,
                                     f.ctypes.data_as(C.c_void_p), None, None) == ERR_ARG
    assert b"bad argument" in L.sift3d_last_error()


def test_bad_arguments_refused(capi):
    L = capi.lib()
    p = np.zeros((8, 6), np.float32)
    q = np.zeros((2, 3), np.float32)
    f = np.zeros(2, capi.FIT_DTYPE)
    P, Q, F = (a.ctypes.data_as(C.c_void_p) for a in (p, q, f))
    # global: n < 0, NULL pairs with n > 0, NULL output
    assert L.sift3d_fit_affine(P, -1, None, 0, 0, F, None, None) == ERR_ARG
    assert L.sift3d_fit_affine(None, 8, None, 0, 0, F, None, None) == ERR_ARG
    assert L.sift3d_fit_affine(P, 8, None, 0, 0, None, None, None) == ERR_ARG
    # local: n < 0, m < 0, k outside 4..64, non-finite radius, NULL pairs / points / output
    for n, m, k, rad in [(-1, 2, 32, 0.0), (8, -1, 32, 0.0), (8, 2, 3, 0.0), (8, 2, 65, 0.0), (8, 2, 0, 0.0), (8, 2, 32, float("nan")),
                         (8, 2, 32, float("inf"))]:
        assert L.sift3d_fit_affine_local(P, n, Q, m, k, rad, None, 0, 0, F, None, None) == ERR_ARG, (n, m, k, rad)
    assert L.sift3d_fit_affine_local(None, 8, Q, 2, 32, 0.0, None, 0, 0, F, None, None) == ERR_ARG
    assert L.sift3d_fit_affine_local(P, 8, None, 2, 32, 0.0, None, 0, 0, F, None, None) == ERR_ARG
    assert L.sift3d_fit_affine_local(P, 8, Q, 2, 32, 0.0, None, 0, 0, None, None, None) == ERR_ARG


def test_restatement_recovers_exact_affine():
    """noise-free pairs whose coordinates and transform are exact in fp32: every inlier is found and the fit is the transform"""
    rng = np.random.default_rng(3)
    L = np.array([[1.25, -0.5, 0.0], [0.5, 1.0, 0.25], [0.0, -0.25, 0.75]])
    b = np.array([3.0, -7.5, 12.25])
    r = rng.integers(0, 200, (400, 3)).astype(np.float64)
    t = r @ L.T + b
    bad = rng.random(400) < 0.4
    t[bad] = rng.integers(0, 200, (int(bad.sum()), 3))
    pairs = np.concatenate([r, t], 1).astype(np.float32)
    assert np.array_equal(pairs[:, 3:].astype(np.float64)[~bad], t[~bad])
    for refine in (0, 1):
        f = ref.fit(pairs, iterations=256, refine=refine, inlier_thresh=0.5)
        assert f["status"] == 0
        assert np.array_equal(f["mask"], ~bad)
        assert f["inliers"] == int((~bad).sum())
        A = f["A"].reshape(3, 4)
        np.testing.assert_allclose(A[:, :3], L, rtol=0, atol=1e-12)
        np.testing.assert_allclose(A[:, 3], b, rtol=0, atol=1e-10)
        assert f["rms"] < 1e-9


def test_restatement_sampler_draws_distinct():
    for c in (4, 5, 7, 64, 1000):
        idx = ref.draws(11, 3, 512, c)
        assert idx.min() >= 0 and idx.max() < c
        assert all(len(set(row)) == 4 for row in idx.tolist())


SHELL = r"""
#include <cstdio>
#include <vector>
#include "cRegistration.h"
int main() {
	std::vector<CPUSIFT::Cvec> ref, tar, pts;
	for (int i = 0; i < 16; i++) { ref.push_back(CPUSIFT::Cvec(i, 2 * i % 7, i * i % 5)); tar.push_back(ref.back()); }
	pts.push_back(CPUSIFT::Cvec(1, 2, 3));
	CPUSIFT::RansacOptions o;
	o.iterations = 64;
	std::vector<int> mask;
	CPUSIFT::AffineFit f = CPUSIFT::EstimateAffine(ref, tar, o, &mask);
	std::vector<CPUSIFT::AffineFit> lf = CPUSIFT::EstimateLocalAffine(ref, tar, pts, 8, 0.f, o);
	double G[9];
	f.Gradient(G);
	CPUSIFT::Cvec d = f.Displacement(pts[0]);
	std::printf("%d %d %zu %zu %g %g\n", f.status, f.inliers, mask.size(), lf.size(), G[0], (double)d.x);
	return 0;
}
"""


def test_shell_registration_links(tmp_path):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no host compiler")
    d = os.path.join(ROOT, "3dsift_amd")
    lib = os.path.join(d, "libsift3d.so")
    if not os.path.exists(lib):
        subprocess.check_call(["make", "-C", os.path.join(d, "host")])
    src = tmp_path / "reg.cpp"
    src.write_text(SHELL)
    r = subprocess.run([cxx, "-std=c++14", "-Wall", "-Werror", "-o", str(tmp_path / "reg"), str(src), "-I", os.path.join(d, "host", "Include"),
                        "-L" + d, "-lsift3d", "-lsift3d_hip", "-Wl,-rpath," + d], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
