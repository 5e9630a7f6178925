"""CPU tests of the strain fields' boundary (sift3d_strain, sift3d_strain_input_from_icgn, include/sift3d_hip.h): the header compiles
as C and C++ with its layout guards, the library exports the entry points, the defaults need no GPU, bad arguments are refused before
any device call, the input from IC-GN results is exact, the CPU restatement (tests/strain_ref.py) recovers a known affine field, its
two solves agree to e (the figure the GPU test's bar is made of), and the C++ shell's ComputeStrains links and reports a failed call."""
import ctypes as C
import importlib
import os
import shutil
import subprocess

import numpy as np
import pytest

import strain_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["sift3d_default_strain_options", "sift3d_strain_input_from_icgn", "sift3d_strain"]
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
SIFT3D_STATIC_ASSERT(sizeof(sift3d_strain_options) == 32, "options");
SIFT3D_STATIC_ASSERT(sizeof(sift3d_strain_result) == 192, "result");
SIFT3D_STATIC_ASSERT(offsetof(sift3d_strain_result, G) == 24 && offsetof(sift3d_strain_result, E) == 96 &&
                     offsetof(sift3d_strain_result, principal) == 144 && offsetof(sift3d_strain_result, equivalent) == 168 &&
                     offsetof(sift3d_strain_result, rms) == 176 && offsetof(sift3d_strain_result, neighbours) == 184 &&
                     offsetof(sift3d_strain_result, status) == 188, "result offsets");
int probe(const sift3d_icgn_result *ic, const int *pts, int m, double *disp, unsigned char *valid, sift3d_strain_result *out) {
	sift3d_strain_options o;
	double s;
	sift3d_default_strain_options(&o);
	o.radius = 8;
	return sift3d_strain_input_from_icgn(ic, m, 0.5, 0, disp, valid) + sift3d_strain(pts, disp, valid, m, &o, 0, 0, out, &s);
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


def test_sizes_and_defaults_without_gpu(capi):
    o = capi.StrainOptions()
    C.memset(C.byref(o), 0x5A, C.sizeof(o))
    capi.lib().sift3d_default_strain_options(C.byref(o))
    assert (o.radius, o.min_neighbours, o.measure) == (16, 10, 0)
    assert list(o.reserved) == [0] * 5
    assert capi.default_strain_options() == {"radius": 16, "min_neighbours": 10, "measure": 0}
    f = capi.STRAIN_DTYPE.fields
    assert capi.STRAIN_DTYPE.itemsize == 192 and C.sizeof(capi.StrainOptions) == 32
    assert [f[k][1] for k in ("disp", "G", "E", "principal", "equivalent", "rms", "neighbours", "status")] == [0, 24, 96, 144, 168, 176, 184, 188]


def _opts(capi, **kw):
    o = capi.StrainOptions()
    capi.lib().sift3d_default_strain_options(C.byref(o))
    for k, v in kw.items():
        if k == "reserved":
            o.reserved[v] = 1
        else:
            setattr(o, k, v)
    return o


BAD_OPTS = [dict(radius=0), dict(radius=4097), dict(radius=-1), dict(min_neighbours=3), dict(min_neighbours=1048577), dict(measure=-1),
            dict(measure=2)] + [dict(reserved=k) for k in range(5)]


def _call(capi, o=None, pts=True, disp=True, out=True, m=2):
    q = np.zeros((2, 3), np.int32)
    u = np.zeros((2, 3), np.float64)
    res = np.zeros(2, capi.STRAIN_DTYPE)
    P = lambda a, on: a.ctypes.data_as(C.c_void_p) if on else None  # noqa: E731
    return capi.lib().sift3d_strain(P(q, pts), P(u, disp), None, m, C.byref(o) if o is not None else None, 0, 0, P(res, out), None)


@pytest.mark.parametrize("bad", BAD_OPTS, ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))
def test_bad_options_refused(capi, bad):
    assert _call(capi, _opts(capi, **bad)) == ERR_ARG
    assert b"bad argument" in capi.lib().sift3d_last_error()


def test_bad_arguments_refused(capi):
    assert _call(capi, m=-1) == ERR_ARG
    assert _call(capi, out=False) == ERR_ARG
    assert _call(capi, out=False, m=0) == ERR_ARG
    assert _call(capi, pts=False) == ERR_ARG
    assert _call(capi, disp=False) == ERR_ARG
    assert b"bad argument" in capi.lib().sift3d_last_error()
    # the extremes of every option are accepted: the call gets as far as looking for a device
    for good in (dict(radius=1, min_neighbours=4, measure=1), dict(radius=4096, min_neighbours=1048576)):
        assert _call(capi, _opts(capi, **good)) != ERR_ARG


def test_no_device_error(capi):
    if capi.device_count() > 0:
        pytest.skip("a GPU is visible here")
    with pytest.raises(capi.Sift3dError, match="no CPU fallback"):
        capi.strain(np.zeros((5, 3), np.int32), np.zeros((5, 3)))
    with pytest.raises(capi.Sift3dError, match="no CPU fallback"):
        capi.strain(np.zeros((0, 3), np.int32), np.zeros((0, 3)))
    with pytest.raises(TypeError):
        capi.strain(np.zeros((5, 3), np.int32), np.zeros((5, 3)), window=3)


def test_strain_input_from_icgn(capi):
    rng = np.random.default_rng(5)
    m = 14
    res = {"p": rng.normal(0, 1, (m, 12)), "zncc": np.full(m, 0.9), "status": np.array([0, 1, 2, 3, 4, 5, 6, 0, 0, 0, 0, 1, 0, 0], np.int32)}
    res["p"][7, 4] = np.nan        # v
    res["p"][8, 8] = np.inf        # w
    res["p"][9, 5] = np.nan        # a gradient term: not a displacement, the POI stays valid
    res["zncc"][10] = 0.49         # under the threshold
    res["zncc"][12] = 0.5          # at the threshold
    res["zncc"][13] = np.nan
    disp, valid = capi.strain_input_from_icgn(res, zncc_min=0.5)
    assert disp.shape == (m, 3) and valid.dtype == np.uint8
    assert np.array_equal(disp.view(np.uint64), res["p"][:, [0, 4, 8]].copy().view(np.uint64))
    assert list(valid) == [1, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 1, 0]
    _, valid = capi.strain_input_from_icgn(res, zncc_min=0.5, accept_unconverged=True)
    assert list(valid) == [1, 1, 0, 0, 0, 0, 0, 0, 0, 1, 0, 1, 1, 0]
    _, valid = capi.strain_input_from_icgn(res)   # zncc_min 0
    assert list(valid) == [1, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 0, 1, 0]
    d0, v0 = capi.strain_input_from_icgn({"p": np.zeros((0, 12)), "zncc": [], "status": []})
    assert d0.shape == (0, 3) and v0.shape == (0,)
    L = capi.lib()
    buf = np.zeros(8)
    ptr = buf.ctypes.data_as(C.c_void_p)
    assert L.sift3d_strain_input_from_icgn(None, -1, 0.0, 0, None, None) == ERR_ARG
    assert L.sift3d_strain_input_from_icgn(None, 2, 0.0, 0, ptr, ptr) == ERR_ARG
    assert L.sift3d_strain_input_from_icgn(ptr, 2, 0.0, 0, None, ptr) == ERR_ARG
    assert L.sift3d_strain_input_from_icgn(ptr, 2, 0.0, 0, ptr, None) == ERR_ARG
    for bad in (float("nan"), float("inf"), -float("inf")):
        assert L.sift3d_strain_input_from_icgn(None, 0, bad, 0, None, None) == ERR_ARG
    assert b"bad argument" in L.sift3d_last_error()
    assert L.sift3d_strain_input_from_icgn(None, 0, 0.0, 0, None, None) == 0


G0 = np.array([[0.010, -0.004, 0.002], [0.003, -0.020, 0.001], [-0.002, 0.005, 0.015]])
B0 = np.array([1.25, -2.5, 0.75])


def affine_grid():
    g = [np.arange(n) * 3 for n in (9, 8, 7)]
    q = np.stack(np.meshgrid(*g, indexing="ij"), -1).reshape(-1, 3).astype(np.int32)
    return q, q @ G0.T + B0


@pytest.mark.parametrize("solve", ["normal", "lstsq"])
def test_restatement_on_a_known_field(solve):
    q, u = affine_grid()
    for measure in ref.MEASURES:
        got = ref.strain(q, u, radius=6, measure=measure, solve=solve)
        assert (got["status"] == 0).all() and got["neighbours"].min() == 27 and got["neighbours"].max() == 125
        E, pr, eq = ref.strain_of(G0, measure)
        assert np.abs(got["G"] - G0).max() < 1e-13 and np.abs(got["disp"] - u).max() < 1e-12
        assert np.abs(got["E"] - E).max() < 1e-13 and np.abs(got["principal"] - pr).max() < 1e-13
        assert np.abs(got["equivalent"] - eq).max() < 1e-13 and got["rms"].max() < 1e-12
    # the closed forms of E, written out
    E = ref.strain_of(G0, 0)[0]
    assert abs(E[0] - (G0[0, 0] + 0.5 * (G0[:, 0] ** 2).sum())) < 1e-16
    assert abs(E[3] - 0.5 * (G0[0, 1] + G0[1, 0] + G0[:, 0] @ G0[:, 1])) < 1e-16
    assert abs(ref.strain_of(G0, 1)[0][5] - 0.5 * (G0[2, 0] + G0[0, 2])) < 1e-16
    const = ref.strain(q, np.tile(B0, (len(q), 1)), radius=6, solve="normal")
    assert not const["G"].any() and not const["E"].any() and not const["rms"].any() and (const["disp"] == B0).all()


def test_restatement_statuses():
    q, u = affine_grid()
    plane = q[:, 2] == 6
    assert (ref.strain(q[plane], u[plane], radius=6, min_neighbours=4)["status"] == 4).all()
    line = plane & (q[:, 1] == 3)
    assert (ref.strain(q[line], u[line], radius=30, min_neighbours=4)["status"] == 4).all()
    few = ref.strain(q, u, radius=2)
    assert (few["status"] == 1).all() and (few["neighbours"] == 1).all()
    far = q.copy()
    far[0, 0] = 2 ** 24 + 1
    got = ref.strain(far, u, radius=6)
    assert got["status"][0] == 2 and got["neighbours"][0] == 0 and (got["status"][1:] == 0).all()


def test_value_of_e():
    e = ref.parity_error()
    q, u, valid = ref.parity_inputs()
    print(f"e = {e:.3e}, bar of the parity inputs = {ref.bar(e, ref.largest_u(u)):.3e}")
    assert len(np.unique(q, axis=0)) == len(q) == 1500 and 0.05 < 1 - valid.mean() < 0.15 and 5.0 < np.abs(u).max() <= 10.0
    assert 0.0 < e < 1e-9   # a sanity cap, not the bar
    counts = {r: np.bincount(ref.parity_reference(r, 0)["status"], minlength=5) for r in ref.PARITY_RADII}
    assert counts[1][1] == 1500 and counts[3][0] > 100 and counts[3][1] > 100 and counts[64][0] == 1500


SHELL = r"""
#include <cstdio>
#include <vector>
#include "cRegistration.h"
int main() {
	std::vector<CPUSIFT::Cvec> pts;
	std::vector<CPUSIFT::IcgnResult> disp;
	for (int i = 0; i < 27; i++) {
		pts.push_back(CPUSIFT::Cvec((float)(4 * (i % 3)), (float)(4 * (i / 3 % 3)), (float)(4 * (i / 9))));
		CPUSIFT::IcgnResult r;
		r.status = 0;
		r.zncc = 0.99;
		r.p[0] = 0.01 * pts.back().x;
		disp.push_back(r);
	}
	CPUSIFT::StrainOptions o;
	o.radius = 8;
	o.measure = 1;
	std::vector<CPUSIFT::StrainResult> s = CPUSIFT::ComputeStrains(pts, disp, o, 0.5, true);
	std::vector<CPUSIFT::StrainResult> s0 = CPUSIFT::ComputeStrains(pts, disp);
	disp.pop_back();
	std::vector<CPUSIFT::StrainResult> bad = CPUSIFT::ComputeStrains(pts, disp);
	std::printf("%zu %zu %zu %d %d %d %g %g\n", s.size(), s0.size(), bad.size(), s[0].status, s0[26].status, bad[0].status, s[13].E[0], s[0].seconds);
	return 0;
}
"""


def test_shell_strain_links_and_reports_failure(tmp_path, capi):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no host compiler")
    d = os.path.join(ROOT, "3dsift_amd")
    if not os.path.exists(os.path.join(d, "libsift3d.so")):
        subprocess.check_call(["make", "-C", os.path.join(d, "host")])
    src = tmp_path / "strain.cpp"
    src.write_text(SHELL)
    r = subprocess.run([cxx, "-std=c++14", "-Wall", "-Werror", "-o", str(tmp_path / "strain"), str(src), "-I", os.path.join(d, "host", "Include"),
                        "-L" + d, "-lsift3d", "-lsift3d_hip", "-Wl,-rpath," + d], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(tmp_path / "strain")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    out = r.stdout.split()
    if capi.device_count() > 0:   # u = 0.01 x on a 3 x 3 x 3 grid: fitted everywhere, exx = 0.01; the call with 26 displacements fails
        assert out[:7] == ["27", "27", "27", "0", "0", "-1", "0.01"] and float(out[7]) > 0, r.stdout
        return
    assert out == ["27", "27", "27", "-1", "-1", "-1", "0", "0"], r.stdout
    assert "ComputeStrains" in r.stderr and "no CPU fallback" in r.stderr
