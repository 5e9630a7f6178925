"""CPU tests of the second-order IC-GN's boundary and restatement (sift3d_icgn2, sift3d_icgn2_init_from_icgn,
sift3d_strain_input_from_icgn2, include/sift3d_hip.h; tests/icgn2_ref.py): the library exports the entry points and the record has the
size and offsets the header asserts, bad arguments are refused before any device call, the two host functions follow their rules, the
restated warp matrix, composition and domain rule reduce to the first-order ones, the host-only logic of the entry passes a stand-alone
program built with the address and undefined-behaviour sanitizers, and on the restatement the second-order fit recovers the quadratic
scene at least ten times more accurately than the first-order fit."""
import ctypes as C
import importlib
import os
import subprocess

import numpy as np
import pytest

import bspline_ref as bref
import icgn2_ref as ref2
import icgn_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "3dsift_amd", "csrc")
NEW = ["sift3d_icgn2", "sift3d_icgn2_init_from_icgn", "sift3d_strain_input_from_icgn2"]
ERR_ARG = 1


@pytest.fixture(scope="module")
def capi():
    m = importlib.import_module("3dsift_amd.capi")
    if not os.path.exists(m.LIB_PATH):
        subprocess.check_call(["make", "-C", CSRC, "-j8"])
    return m


def test_exports_and_record(capi):
    L = capi.lib()
    for n in NEW:
        assert hasattr(L, n), n
        assert n in capi.SYMBOLS
    d = capi.ICGN2_DTYPE
    assert d.itemsize == 272
    assert [d.fields[k][1] for k in ("p", "zncc", "last_step", "iterations", "status", "reserved")] == [0, 240, 248, 256, 260, 264]
    assert hasattr(capi, "icgn2") and hasattr(capi, "icgn2_init_from_icgn") and hasattr(capi, "strain_input_from_icgn2")


# ---- refusals that need no GPU ----------------------------------------------------------------------------------------------------

def _opts(capi, **kw):
    o = capi.IcgnOptions()
    capi.lib().sift3d_default_icgn_options(C.byref(o))
    for k, v in kw.items():
        if k == "reserved":
            o.reserved[v] = 1
        else:
            setattr(o, k, v)
    return o


def _icgn2(capi, o=None, ref=True, tar=True, pts=True, out=True, m=2, dims=(64, 64, 64, 64, 64, 64), coef=0):
    v = np.zeros((4, 4, 4), np.float32)
    q = np.zeros((2, 3), np.int32)
    res = np.zeros(2, capi.ICGN2_DTYPE)
    P = lambda a, on: a.ctypes.data_as(C.c_void_p) if on else None  # noqa: E731
    return capi.lib().sift3d_icgn2(P(v, ref), dims[0], dims[1], dims[2], P(v, tar), dims[3], dims[4], dims[5], P(q, pts), m, None,
                                   C.byref(o) if o is not None else None, coef, 0, 0, P(res, out), None)


BAD_OPTS = [dict(subset_radius=1), dict(subset_radius=33), dict(max_iterations=0), dict(max_iterations=101), dict(tolerance=-1e-3),
            dict(tolerance=float("nan")), dict(tolerance=float("inf")), dict(interpolation=3), dict(interpolation=-1), dict(reserved=0),
            dict(reserved=3)]


@pytest.mark.parametrize("bad", BAD_OPTS, ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))
def test_bad_options_refused(capi, bad):
    assert _icgn2(capi, _opts(capi, **bad)) == ERR_ARG
    assert b"sift3d_icgn2: bad argument" in capi.lib().sift3d_last_error()


def test_bad_arguments_refused(capi):
    for kind in (0, 1, 2):
        o = _opts(capi, interpolation=kind)
        assert _icgn2(capi, o, m=-1) == ERR_ARG
        for k in range(6):
            dims = [64] * 6
            dims[k] = 0
            assert _icgn2(capi, o, dims=tuple(dims)) == ERR_ARG, k
        assert _icgn2(capi, o, ref=False) == ERR_ARG
        assert _icgn2(capi, o, tar=False) == ERR_ARG
        assert _icgn2(capi, o, out=False) == ERR_ARG
        assert _icgn2(capi, o, out=False, m=0) == ERR_ARG
        assert _icgn2(capi, o, pts=False) == ERR_ARG
        for coef in (2, -1):
            assert _icgn2(capi, o, coef=coef) == ERR_ARG
    # coefficients have a meaning for the B-spline interpolation only
    for kind in (0, 1):
        assert _icgn2(capi, _opts(capi, interpolation=kind), coef=1) == ERR_ARG
    assert _icgn2(capi, None, coef=1) == ERR_ARG  # NULL options: the defaults, interpolation 0
    # a target too large for a prefilter pass is refused where the call would prefilter it
    big = (64, 64, 64, 4, 4, 1 << 25)
    assert _icgn2(capi, _opts(capi, interpolation=2), dims=big, coef=0) == ERR_ARG


def test_init_from_icgn(capi):
    rng = np.random.default_rng(0)
    p = rng.standard_normal((9, 12))
    status = np.array([0, 1, 2, 3, 4, 5, 6, -1, 0])
    got = capi.icgn2_init_from_icgn({"p": p, "status": status})
    want = ref2.init_from_icgn(p, status)
    assert got.shape == (9, 30)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.isnan(got[2:8]).all()
    ok = [0, 1, 8]
    assert np.array_equal(got[ok], want[ok]) and not got[ok][:, ref2.SECOND].any()
    assert np.array_equal(ref2.first_order_of(got[ok]), p[ok])
    assert capi.icgn2_init_from_icgn({"p": np.zeros((0, 12)), "status": []}).shape == (0, 30)
    L = capi.lib()
    buf = np.zeros(30)
    rec = np.zeros(1, capi.ICGN_DTYPE)
    assert L.sift3d_icgn2_init_from_icgn(rec.ctypes.data_as(C.c_void_p), -1, buf.ctypes.data_as(C.c_void_p)) == ERR_ARG
    assert b"sift3d_icgn2_init_from_icgn: bad argument" in L.sift3d_last_error()
    assert L.sift3d_icgn2_init_from_icgn(None, 1, buf.ctypes.data_as(C.c_void_p)) == ERR_ARG
    assert L.sift3d_icgn2_init_from_icgn(rec.ctypes.data_as(C.c_void_p), 1, None) == ERR_ARG
    assert L.sift3d_icgn2_init_from_icgn(None, 0, None) == 0


def test_strain_input_from_icgn2(capi):
    p = np.arange(5 * 30, dtype=np.float64).reshape(5, 30)
    p[3, 10] = np.inf
    res = {"p": p, "zncc": np.array([0.99, 0.5, 0.99, 0.99, 0.99]), "status": np.array([0, 0, 1, 0, 3])}
    disp, valid = capi.strain_input_from_icgn2(res, zncc_min=0.9)
    assert np.array_equal(disp, p[:, ref2.DISP]) and list(valid) == [1, 0, 0, 0, 0]
    assert list(capi.strain_input_from_icgn2(res, zncc_min=0.9, accept_unconverged=True)[1]) == [1, 0, 1, 0, 0]
    assert list(capi.strain_input_from_icgn2(res)[1]) == [1, 1, 0, 0, 0]
    L = capi.lib()
    rec, d, v = np.zeros(1, capi.ICGN2_DTYPE), np.zeros(3), np.zeros(1, np.uint8)
    P = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert L.sift3d_strain_input_from_icgn2(P(rec), -1, 0.0, 0, P(d), P(v)) == ERR_ARG
    assert L.sift3d_strain_input_from_icgn2(P(rec), 1, float("nan"), 0, P(d), P(v)) == ERR_ARG
    assert L.sift3d_strain_input_from_icgn2(None, 1, 0.0, 0, P(d), P(v)) == ERR_ARG
    assert L.sift3d_strain_input_from_icgn2(P(rec), 1, 0.0, 0, None, P(v)) == ERR_ARG
    assert L.sift3d_strain_input_from_icgn2(P(rec), 1, 0.0, 0, P(d), None) == ERR_ARG
    assert L.sift3d_strain_input_from_icgn2(None, 0, 0.0, 0, None, None) == 0


# ---- the host-only logic of the entry, as a sanitized stand-alone program ----------------------------------------------------------

PROGRAM = r"""
#include <stdio.h>
#include <string.h>

#include <vector>

#include "icgn_host.h"

#define CHECK(c) do { if (!(c)) { printf("line %d: %s\n", __LINE__, #c); return 1; } } while (0)

int main() {
	using namespace s3d;
	// the conversions
	std::vector<sift3d_icgn_result> first(7);
	memset(first.data(), 0, sizeof(sift3d_icgn_result) * first.size());
	for (int i = 0; i < 7; i++) {
		first[i].status = i;
		for (int k = 0; k < 12; k++) first[i].p[k] = 100 * i + k;
	}
	std::vector<double> p30(30 * first.size(), -1.0);
	for (size_t i = 0; i < first.size(); i++) icgn2_init_row(first[i], p30.data() + 30 * i);
	for (int i = 0; i < 7; i++)
		for (int a = 0; a < 3; a++)
			for (int k = 0; k < 10; k++) {
				const double v = p30[30 * i + 10 * a + k];
				if (i > 1) CHECK(v != v);
				else CHECK(v == (k < 4 ? 100 * i + 4 * a + k : 0));
			}
	std::vector<sift3d_icgn2_result> second(3);
	memset(second.data(), 0, sizeof(sift3d_icgn2_result) * second.size());
	second[0].zncc = 0.95;
	second[1].zncc = 0.95;
	second[1].status = 1;
	second[2].zncc = 0.95;
	second[2].p[20] = INFINITY;
	for (int i = 0; i < 3; i++) second[i].p[0] = 1 + i, second[i].p[10] = 2 + i;
	double d[3];
	CHECK(icgn2_strain_row(second[0], 0.9, 0, d) == 1 && d[0] == 1 && d[1] == 2 && d[2] == 0);
	CHECK(icgn2_strain_row(second[0], 0.96, 0, d) == 0);
	CHECK(icgn2_strain_row(second[1], 0.9, 0, d) == 0 && icgn2_strain_row(second[1], 0.9, 1, d) == 1);
	CHECK(icgn2_strain_row(second[2], 0.9, 0, d) == 0 && d[2] == INFINITY);
	// the layout: pieces in order, aligned, absent pieces take no room; second order (30 parameters, 272-byte records), then first
	// order (12 parameters, 128-byte records)
	for (int order = 2; order >= 1; order--)
		for (int m : {1, 7, 30000})
			for (int dev = 0; dev < 2; dev++)
				for (int ini = 0; ini < 2; ini++)
					for (int fil = 0; fil < 2; fil++) {
						const size_t nr = 64 * 64 * 64, nt = 61 * 64 * 64, sb = order == 2 ? 4224 : 1368;
						const size_t rb = order == 2 ? sizeof(sift3d_icgn2_result) : sizeof(sift3d_icgn_result), np = order == 2 ? 30 : 12;
						const IcgnLayout L = icgn_layout(m, nr, nt, dev, ini, fil, sb, rb, (int)np);
						const size_t at[8] = {0, L.o_state, L.o_ref, L.o_tar, L.o_pts, L.o_opt, L.o_coef, L.o_tmp};
						const size_t by[8] = {L.res_bytes, sb * m, dev ? 0 : 4 * nr, dev ? 0 : 4 * nt, dev ? 0 : (size_t)12 * m,
						                      dev || !ini ? 0 : (size_t)8 * np * m, fil ? 4 * nt : 0, fil ? 4 * nt : 0};
						CHECK(L.res_bytes == (size_t)(order == 2 ? 272 : 128) * m);
						size_t end = 0;
						for (int i = 0; i < 8; i++) {
							CHECK(at[i] == end && at[i] % 256 == 0);
							end += al256(by[i]);
						}
						CHECK(L.end == end);
					}
	// the argument check: sift3d_icgn2 (interpolation 0..2, coefficients only with 2)
	int r, it, kind;
	double tol;
	int x = 0;
	sift3d_icgn_options o = {10, 5, 0.f, 2, {0, 0, 0, 0}};
	CHECK(icgn_args_ok(&x, 1, 1, 1, &x, 1, 1, 1, &x, 1, &o, 2, false, 1, &x, r, it, tol, kind) && r == 10 && it == 5 && tol == 0 && kind == 2);
	CHECK(icgn_args_ok(&x, 1, 1, 1, &x, 1, 1, 1, nullptr, 0, nullptr, 2, false, 0, &x, r, it, tol, kind) && r == 16 && it == 20 && kind == 0);
	CHECK(!icgn_args_ok(&x, 1, 1, 1, &x, 1, 1, 1, nullptr, 1, nullptr, 2, false, 0, &x, r, it, tol, kind));
	CHECK(!icgn_args_ok(&x, 1, 1, 1, &x, 1, 1, 1, &x, 1, nullptr, 2, false, 1, &x, r, it, tol, kind));
	CHECK(!icgn_args_ok(&x, 1, 1, 1, &x, 1, 1, 1, &x, 1, &o, 2, false, 2, &x, r, it, tol, kind));
	o.interpolation = 3;
	CHECK(!icgn_args_ok(&x, 1, 1, 1, &x, 1, 1, 1, &x, 1, &o, 2, false, 0, &x, r, it, tol, kind));
	// sift3d_icgn (interpolation 0 or 1, no coefficients)
	for (int k = -1; k <= 3; k++) {
		o.interpolation = k;
		const bool ok = icgn_args_ok(&x, 1, 1, 1, &x, 1, 1, 1, &x, 1, &o, 1, false, 0, &x, r, it, tol, kind);
		CHECK(ok == (k == 0 || k == 1));
		if (ok) CHECK(kind == k && r == 10 && it == 5);
	}
	CHECK(icgn_args_ok(&x, 1, 1, 1, &x, 1, 1, 1, &x, 1, nullptr, 1, false, 0, &x, r, it, tol, kind) && r == 16 && it == 20 && kind == 0);
	// sift3d_icgn_bspline (interpolation 0 only, run as kind 2; tar_is_coefficients 0 or 1)
	for (int k = -1; k <= 3; k++)
		for (int coef = -1; coef <= 2; coef++) {
			o.interpolation = k;
			const bool ok = icgn_args_ok(&x, 1, 1, 1, &x, 1, 1, 1, &x, 1, &o, 0, true, coef, &x, r, it, tol, kind);
			CHECK(ok == (k == 0 && (coef == 0 || coef == 1)));
			if (ok) CHECK(kind == 2);
		}
	CHECK(icgn_args_ok(&x, 1, 1, 1, &x, 1, 1, 1, &x, 1, nullptr, 0, true, 1, &x, r, it, tol, kind) && kind == 2 && r == 16);
	// the defaults come from one place
	const sift3d_icgn_options def = icgn_default_options();
	CHECK(def.subset_radius == 16 && def.max_iterations == 20 && def.tolerance == 1e-3f && def.interpolation == 0);
	CHECK(!def.reserved[0] && !def.reserved[1] && !def.reserved[2] && !def.reserved[3]);
	printf("ok\n");
	return 0;
}
"""


def test_host_logic_sanitized(tmp_path):
    src, exe = tmp_path / "icgn2_host_check.cpp", tmp_path / "icgn2_host_check"
    src.write_text(PROGRAM)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + CSRC, "-o", str(exe), str(src)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


# ---- the restatement against the first-order one ----------------------------------------------------------------------------------

def _affine(rng):
    p = np.zeros(30)
    p[ref2.DISP] = rng.uniform(-2, 2, 3)
    p[ref2.FIRST] = rng.uniform(-0.05, 0.05, 9)
    return p


def test_affine_parameters_compose_like_the_4x4_matrices():
    rng = np.random.default_rng(1)
    for _ in range(20):
        p, dp = _affine(rng), _affine(rng)
        got = ref2.compose(p, dp)
        want = ref.p_of(ref.M_of(ref2.first_order_of(p)) @ np.linalg.inv(ref.M_of(ref2.first_order_of(dp))))
        assert np.abs(ref2.first_order_of(got) - want).max() <= 1e-14
        assert np.abs(got[ref2.SECOND]).max() <= 1e-14  # the LU's rounding, as in the first class
    assert ref2.compose(np.zeros(30), np.zeros(30)).tolist() == [0.0] * 30
    sing = np.zeros(30)
    sing[[1, 12, 23]] = -1.0  # F = 0
    assert ref2.compose(np.zeros(30), sing) is None


def test_warp_matrix_maps_the_monomials():
    rng = np.random.default_rng(2)
    d = ref.offsets(3)
    p = _affine(rng)
    assert np.abs(ref2.M_of(p) @ ref2.xi(d).T - ref2.xi(ref2.warp(p, np.zeros(3), d)).T).max() <= 1e-12  # exact for an affine p
    # with second-order terms the rows 4..9 differ by the dropped terms of degree 3 and 4: 2 (linear part)(quadratic part) +
    # (quadratic part)^2, with |linear part| <= 3 * 1.05 * 3 and |quadratic part| <= 6 * 1e-3 * 9 on |d| <= 3
    p[ref2.SECOND] = rng.uniform(-1e-3, 1e-3, 18)
    M, X = ref2.M_of(p) @ ref2.xi(d).T, ref2.xi(ref2.warp(p, np.zeros(3), d)).T
    assert np.abs(M[:4] - X[:4]).max() <= 1e-12
    lin, quad = 3 * 1.05 * 3, 6 * 1e-3 * 9
    assert np.abs(M[4:] - X[4:]).max() <= 2 * lin * quad + quad * quad
    assert np.abs(M[4:] - X[4:]).max() > 0


def test_domain_rule_is_the_first_order_rule_without_second_order_terms():
    rng = np.random.default_rng(3)
    shape = (40, 44, 48)
    seen = set()
    for _ in range(400):
        p = _affine(rng)
        p[ref2.DISP] = rng.uniform(-14, 14, 3)
        q = rng.integers(8, 36, 3)
        for cubic in (True, False):
            a = ref2.in_domain(shape, p, q, 6, cubic)
            assert a == ref.in_domain(shape, ref2.first_order_of(p), q, 6, cubic)
            seen.add(a)
    assert seen == {True, False}
    p = np.zeros(30)
    assert ref2.in_domain(shape, p, (20, 20, 20), 6, True)
    p[4] = np.nan
    assert not ref2.in_domain(shape, p, (20, 20, 20), 6, True)
    p[4] = 2 * 13.5 / 36  # B_x = 13.5: 26 + 13.5 = 39.5, taps to 41 > 39 ... and 14 - 13.5 = 0.5, tap -1
    assert not ref2.in_domain(shape, p, (20, 20, 20), 6, True)


# ---- recovery on the quadratic scene ----------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def scene():
    return ref2.quadratic_scene()


def test_truth_is_the_expansion_of_the_map(scene):
    R, T, truth = scene
    assert R.shape == T.shape == (64, 64, 64) and R.dtype == np.float32
    tr = truth(ref2.POIS)
    assert np.array_equal(tr[:, ref2.SECOND].reshape(-1, 3, 6)[0], np.array(ref2.Q_SEC))
    mid = 31.5
    for q, p in zip(ref2.POIS, tr.reshape(-1, 3, 10)):
        e = q - mid
        for a in range(3):
            xx, yy, zz, xy, xz, yz = ref2.Q_SEC[a]
            u = ref2.T_VEC[a] + np.dot(ref2.G_MAT[a], e) + 0.5 * (xx * e[0] ** 2 + yy * e[1] ** 2 + zz * e[2] ** 2) + xy * e[0] * e[1] + \
                xz * e[0] * e[2] + yz * e[1] * e[2]
            g = np.array(ref2.G_MAT[a]) + [xx * e[0] + xy * e[1] + xz * e[2], xy * e[0] + yy * e[1] + yz * e[2], xz * e[0] + yz * e[1] + zz * e[2]]
            assert abs(p[a, 0] - u) <= 1e-14 and np.abs(p[a, 1:4] - g).max() <= 1e-15


@pytest.mark.parametrize("kind", [0, 2], ids=["keys", "bspline"])
def test_second_order_is_ten_times_closer(scene, kind):
    """the first-order bias kappa r (r + 1) / 6 is 0.07 .. 0.1 voxel here, the interpolation and stopping floor below 5e-3: a factor of
    10 at least (measured: 28 for Keys)"""
    R, T, truth = scene
    q, tr = ref2.POIS, truth(ref2.POIS)
    first = ref.icgn(R, T, q, subset_radius=10) if kind == 0 else bref.icgn(R, T, q, subset_radius=10, f32=True)
    assert (first["status"] == 0).all()
    second = ref2.icgn2(R, T, q, init=ref2.init_from_icgn(first["p"], first["status"]), subset_radius=10, interpolation=kind, f32=kind == 2)
    assert (second["status"] == 0).all(), second["status"]
    e1 = np.abs(first["p"] - ref2.first_order_of(tr))
    e2 = np.abs(second["p"] - tr)
    print(f"{'Keys' if kind == 0 else 'B-spline'}: first order u {e1[:, [0, 4, 8]].max():.3e}, gradient {np.delete(e1, [0, 4, 8], 1).max():.3e}; "
          f"second order u {e2[:, ref2.DISP].max():.3e}, first derivatives {e2[:, ref2.FIRST].max():.3e}, second derivatives "
          f"{e2[:, ref2.SECOND].max():.3e}; iterations {second['iterations']}, zncc >= {second['zncc'].min():.6f}")
    assert e2[:, ref2.DISP].max() <= 0.1 * e1[:, [0, 4, 8]].max()
