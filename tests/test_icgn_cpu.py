"""CPU tests of the IC-GN displacement refinement's boundary (sift3d_icgn, sift3d_icgn_init_from_fits, include/sift3d_hip.h): the header
compiles as C and C++ with its layout guards, the library exports the entry points, the defaults need no GPU, bad arguments are
refused before any device call, the init from affine fits is exact, the CPU restatement (tests/icgn_ref.py) recovers known
deformations, and the C++ shell's RefineDisplacements links."""
import ctypes as C
import importlib
import os
import shutil
import subprocess

import numpy as np
import pytest

import icgn_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["sift3d_default_icgn_options", "sift3d_icgn_init_from_fits", "sift3d_icgn"]
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
SIFT3D_STATIC_ASSERT(sizeof(sift3d_icgn_options) == 32, "options");
SIFT3D_STATIC_ASSERT(offsetof(sift3d_icgn_options, tolerance) == 8 && offsetof(sift3d_icgn_options, reserved) == 16, "options offsets");
SIFT3D_STATIC_ASSERT(sizeof(sift3d_icgn_result) == 128, "result");
SIFT3D_STATIC_ASSERT(offsetof(sift3d_icgn_result, zncc) == 96 && offsetof(sift3d_icgn_result, iterations) == 112 &&
                     offsetof(sift3d_icgn_result, status) == 116, "result offsets");
int probe(const float *r, const float *t, const int *pts, int m, const sift3d_affine_fit *fits, double *init, sift3d_icgn_result *out) {
	sift3d_icgn_options o;
	double s;
	sift3d_default_icgn_options(&o);
	o.subset_radius = 10;
	return sift3d_icgn_init_from_fits(fits, pts, m, init) + sift3d_icgn(r, 64, 64, 64, t, 64, 64, 64, pts, m, init, &o, 0, 0, out, &s);
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
    o = capi.IcgnOptions()
    C.memset(C.byref(o), 0x5A, C.sizeof(o))
    capi.lib().sift3d_default_icgn_options(C.byref(o))
    assert (o.subset_radius, o.max_iterations, o.interpolation) == (16, 20, 0) and o.tolerance == np.float32(1e-3)
    assert list(o.reserved) == [0, 0, 0, 0]
    assert capi.default_icgn_options() == {"subset_radius": 16, "max_iterations": 20, "tolerance": float(np.float32(1e-3)), "interpolation": 0}
    assert capi.ICGN_DTYPE.itemsize == 128 and capi.ICGN_DTYPE.fields["zncc"][1] == 96 and capi.ICGN_DTYPE.fields["status"][1] == 116


def _opts(capi, **kw):
    o = capi.IcgnOptions()
    capi.lib().sift3d_default_icgn_options(C.byref(o))
    for k, v in kw.items():
        if k == "reserved":
            o.reserved[v] = 1
        else:
            setattr(o, k, v)
    return o


BAD_OPTS = [dict(subset_radius=1), dict(subset_radius=33), dict(max_iterations=0), dict(max_iterations=101), dict(tolerance=-1e-3),
            dict(tolerance=float("nan")), dict(tolerance=float("inf")), dict(interpolation=2), dict(interpolation=-1),
            dict(reserved=0), dict(reserved=3)]


def _call(capi, o=None, ref=True, tar=True, pts=True, out=True, m=2, dims=(64, 64, 64, 64, 64, 64)):
    v = np.zeros((4, 4, 4), np.float32)
    q = np.zeros((2, 3), np.int32)
    res = np.zeros(2, capi.ICGN_DTYPE)
    P = lambda a, on: a.ctypes.data_as(C.c_void_p) if on else None  # noqa: E731
    return capi.lib().sift3d_icgn(P(v, ref), dims[0], dims[1], dims[2], P(v, tar), dims[3], dims[4], dims[5], P(q, pts), m, None,
                                  C.byref(o) if o is not None else None, 0, 0, P(res, out), None)


@pytest.mark.parametrize("bad", BAD_OPTS, ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))
def test_bad_options_refused(capi, bad):
    assert _call(capi, _opts(capi, **bad)) == ERR_ARG
    assert b"bad argument" in capi.lib().sift3d_last_error()


def test_bad_arguments_refused(capi):
    assert _call(capi, m=-1) == ERR_ARG
    for k in range(6):
        dims = [64] * 6
        dims[k] = 0
        assert _call(capi, dims=tuple(dims)) == ERR_ARG, k
    assert _call(capi, ref=False) == ERR_ARG
    assert _call(capi, tar=False) == ERR_ARG
    assert _call(capi, out=False) == ERR_ARG
    assert _call(capi, out=False, m=0) == ERR_ARG
    assert _call(capi, pts=False) == ERR_ARG
    L = capi.lib()
    assert L.sift3d_icgn_init_from_fits(None, None, -1, None) == ERR_ARG
    assert L.sift3d_icgn_init_from_fits(None, None, 2, None) == ERR_ARG
    assert L.sift3d_icgn_init_from_fits(None, None, 0, None) == 0


def test_init_from_fits_exact(capi):
    rng = np.random.default_rng(5)
    m = 50
    A = np.zeros((m, 3, 4))
    A[:, :, :3] = np.eye(3) + rng.normal(0, 0.05, (m, 3, 3))
    A[:, :, 3] = rng.normal(0, 4, (m, 3))
    status = np.where(rng.random(m) < 0.2, rng.integers(1, 4, m), 0).astype(np.int32)
    pts = rng.integers(0, 512, (m, 3)).astype(np.int32)
    got = capi.icgn_init_from_fits({"A": A, "status": status}, pts)
    want = ref.init_from_fits(A, status, pts)
    assert got.shape == (m, 12)
    ok = status == 0
    assert np.isnan(got[~ok]).all()
    assert np.array_equal(got[ok].view(np.uint64), want[ok].view(np.uint64))
    # hand-checked row: L = I, b = (1, 2, 3) gives u = b and a zero gradient at any point
    one = capi.icgn_init_from_fits({"A": np.array([[[1.0, 0, 0, 1], [0, 1, 0, 2], [0, 0, 1, 3]]]), "status": np.zeros(1, np.int32)}, [[7, 8, 9]])
    assert np.array_equal(one[0], [1, 0, 0, 0, 2, 0, 0, 0, 3, 0, 0, 0])


def test_restatement_recovers_translation():
    R, T, truth = ref.scene((48, 48, 48), tvec=(0.37, -0.52, 0.21))
    q = np.array([[24, 24, 24], [20, 27, 23], [27, 21, 26]])
    res = ref.icgn(R, T, q, subset_radius=12)
    assert (res["status"] == 0).all(), res["status"]
    err = np.abs(res["p"] - truth(q))
    assert err[:, [0, 4, 8]].max() <= 0.02, err
    assert (res["zncc"] > 0.99).all()


def test_restatement_recovers_rotation():
    R, T, truth = ref.scene((48, 48, 48), ref.rot(1.0, -2.0, 1.5), (0.2, 0.1, -0.3))
    q = np.array([[24, 24, 24], [21, 26, 23]])
    tr = truth(q)
    rng = np.random.default_rng(1)
    init = tr + np.where(np.arange(12) % 4 == 0, rng.uniform(-0.3, 0.3, (len(q), 12)), rng.uniform(-0.01, 0.01, (len(q), 12)))
    res = ref.icgn(R, T, q, init=init, subset_radius=12)
    assert (res["status"] == 0).all(), res["status"]
    err = np.abs(res["p"] - tr)
    assert err[:, [0, 4, 8]].max() <= 0.02, err
    assert np.delete(err, [0, 4, 8], 1).max() <= 2e-3, err


def test_restatement_statuses():
    R, T, truth = ref.scene((40, 40, 40), tvec=(0.3, 0.0, 0.0))
    assert ref.refine(R, T, (3, 20, 20), subset_radius=5)["status"] == 2
    assert ref.refine(R, T, (20, 20, 20), init=[np.nan] + [0] * 11, subset_radius=5)["status"] == 5
    w = ref.refine(R, T, (20, 20, 20), init=[30.0] + [0] * 11, subset_radius=5)
    assert (w["status"], w["iterations"], w["zncc"]) == (3, 0, 0.0) and w["p"][0] == 30.0
    flat = np.ones_like(R)
    assert ref.refine(flat, T, (20, 20, 20), subset_radius=5)["status"] == 4
    assert ref.refine(R, T, (20, 20, 20), subset_radius=5, max_iterations=1, tolerance=1e-12)["status"] == 1
    w = ref.refine(R, T, (20, 20, 20), subset_radius=5, max_iterations=3, tolerance=0.0)
    assert (w["status"], w["iterations"]) == (1, 3)


SHELL = r"""
#include <cstdio>
#include <vector>
#include "cRegistration.h"
int main() {
	std::vector<float> v(32 * 32 * 32, 1.f);
	std::vector<CPUSIFT::Cvec> pts(1, CPUSIFT::Cvec(16, 16, 16));
	std::vector<CPUSIFT::AffineFit> fits(1);
	CPUSIFT::IcgnOptions o;
	o.subset_radius = 5;
	std::vector<CPUSIFT::IcgnResult> r = CPUSIFT::RefineDisplacements(v.data(), 32, 32, 32, v.data(), 32, 32, 32, pts, &fits, o);
	double G[9];
	r[0].Gradient(G);
	CPUSIFT::Cvec d = r[0].Displacement();
	std::printf("%zu %d %g %g\n", r.size(), r[0].status, G[0], (double)d.x);
	return 0;
}
"""


def test_shell_refine_links(tmp_path):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no host compiler")
    d = os.path.join(ROOT, "3dsift_amd")
    if not os.path.exists(os.path.join(d, "libsift3d.so")):
        subprocess.check_call(["make", "-C", os.path.join(d, "host")])
    src = tmp_path / "icgn.cpp"
    src.write_text(SHELL)
    r = subprocess.run([cxx, "-std=c++14", "-Wall", "-Werror", "-o", str(tmp_path / "icgn"), str(src), "-I", os.path.join(d, "host", "Include"),
                        "-L" + d, "-lsift3d", "-lsift3d_hip", "-Wl,-rpath," + d], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
