"""CPU tests of the field evaluation's boundary (sift3d_field_eval and its host helpers, include/sift3d_hip.h): the header compiles as C
and C++ with its layout guards, the library exports the entry points, the defaults need no GPU, bad arguments are refused before any
device call, the four host helpers equal their restatement (tests/field_ref.py) bit for bit, the restatement recovers an affine and a
constant field under both weightings, its two solves agree to e (the figure the GPU test's bar is made of), the weighted fit moves
less than the uniform one where a POI enters the window, and the C++ shell links and reports a failed call."""
import ctypes as C
import importlib
import os
import shutil
import subprocess

import numpy as np
import pytest

import field_ref as ref
import field_shell

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["sift3d_default_field_options", "sift3d_field_eval", "sift3d_field_queries_from_displacements", "sift3d_field_unpack",
       "sift3d_compose_displacements", "sift3d_icgn_init_from_field"]
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
SIFT3D_STATIC_ASSERT(sizeof(sift3d_field_options) == 32, "options");
SIFT3D_STATIC_ASSERT(sizeof(sift3d_field_result) == 128, "result");
SIFT3D_STATIC_ASSERT(offsetof(sift3d_field_result, G) == 24 && offsetof(sift3d_field_result, rms) == 96 &&
                     offsetof(sift3d_field_result, wsum) == 104 && offsetof(sift3d_field_result, neighbours) == 112 &&
                     offsetof(sift3d_field_result, sides) == 116 && offsetof(sift3d_field_result, status) == 120, "result offsets");
int probe(const int *pts, const double *uA, const double *gA, int m, double *x, sift3d_field_result *out, double *u, double *g,
          unsigned char *valid, double *init12) {
	sift3d_field_options o;
	double s;
	int count;
	sift3d_default_field_options(&o);
	o.radius = 8;
	return sift3d_field_queries_from_displacements(pts, uA, m, x) + sift3d_field_eval(pts, uA, 0, m, x, m, &o, 0, 0, out, &s) +
	       sift3d_compose_displacements(uA, gA, 0, out, m, u, g, valid) + sift3d_field_unpack(out, m, u, g, valid) +
	       sift3d_icgn_init_from_field(u, g, valid, m, 1, init12, &count);
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
    o = capi.FieldOptions()
    C.memset(C.byref(o), 0x5A, C.sizeof(o))
    capi.lib().sift3d_default_field_options(C.byref(o))
    assert (o.radius, o.min_neighbours, o.weighting, o.require_enclosed) == (16, 10, 1, 1)
    assert list(o.reserved) == [0] * 4
    assert capi.default_field_options() == {"radius": 16, "min_neighbours": 10, "weighting": 1, "require_enclosed": 1}
    assert C.sizeof(capi.FieldOptions) == 32
    assert [getattr(capi.FieldOptions, k).offset for k in ("radius", "min_neighbours", "weighting", "require_enclosed", "reserved")] == [0, 4, 8, 12, 16]
    f = capi.FIELD_DTYPE.fields
    assert capi.FIELD_DTYPE.itemsize == 128
    assert [f[k][1] for k in ("disp", "G", "rms", "wsum", "neighbours", "sides", "status", "reserved")] == [0, 24, 96, 104, 112, 116, 120, 124]


def _opts(capi, **kw):
    o = capi.FieldOptions()
    capi.lib().sift3d_default_field_options(C.byref(o))
    for k, v in kw.items():
        if k == "reserved":
            o.reserved[v] = 1
        else:
            setattr(o, k, v)
    return o


BAD_OPTS = [dict(radius=0), dict(radius=4096), dict(radius=-1), dict(min_neighbours=3), dict(min_neighbours=1048577), dict(weighting=-1),
            dict(weighting=2), dict(require_enclosed=-1), dict(require_enclosed=2)] + [dict(reserved=k) for k in range(4)]


def _call(capi, o=None, pts=True, disp=True, qry=True, out=True, m=2, nq=2):
    q = np.zeros((2, 3), np.int32)
    u = np.zeros((2, 3), np.float64)
    x = np.zeros((2, 3), np.float64)
    res = np.zeros(2, capi.FIELD_DTYPE)
    P = lambda a, on: a.ctypes.data_as(C.c_void_p) if on else None  # noqa: E731
    return capi.lib().sift3d_field_eval(P(q, pts), P(u, disp), None, m, P(x, qry), nq, C.byref(o) if o is not None else None, 0, 0, P(res, out),
                                        None)


@pytest.mark.parametrize("bad", BAD_OPTS, ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))
def test_bad_options_refused(capi, bad):
    assert _call(capi, _opts(capi, **bad)) == ERR_ARG
    assert b"bad argument" in capi.lib().sift3d_last_error()


def test_bad_arguments_refused_before_the_device_is_looked_for(capi):
    assert _call(capi, m=-1) == ERR_ARG
    assert _call(capi, nq=-1) == ERR_ARG
    assert _call(capi, out=False) == ERR_ARG
    assert _call(capi, qry=False) == ERR_ARG
    assert _call(capi, pts=False) == ERR_ARG
    assert _call(capi, disp=False) == ERR_ARG
    assert _call(capi, pts=False, m=0, nq=-1) == ERR_ARG
    assert b"bad argument" in capi.lib().sift3d_last_error()
    # what is allowed gets as far as looking for a device: the extremes of every option, absent arrays with a zero count
    for good in (dict(radius=1, min_neighbours=4, weighting=0, require_enclosed=0), dict(radius=4095, min_neighbours=1048576)):
        assert _call(capi, _opts(capi, **good)) != ERR_ARG
    assert _call(capi, pts=False, disp=False, m=0) != ERR_ARG
    assert _call(capi, qry=False, out=False, nq=0) != ERR_ARG


def test_no_device_error(capi):
    if capi.device_count() > 0:
        pytest.skip("a GPU is visible here")
    with pytest.raises(capi.Sift3dError, match="no CPU fallback"):
        capi.field_eval(np.zeros((5, 3), np.int32), np.zeros((5, 3)), None, np.zeros((2, 3)))
    with pytest.raises(capi.Sift3dError, match="no CPU fallback"):
        capi.field_eval(np.zeros((0, 3), np.int32), np.zeros((0, 3)), None, np.zeros((0, 3)))
    with pytest.raises(TypeError):
        capi.field_eval(np.zeros((5, 3), np.int32), np.zeros((5, 3)), None, np.zeros((2, 3)), window=3)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def records(capi, rng, m):
    """field records with every status and random doubles, as the dict field_eval returns"""
    rec = np.zeros(m, capi.FIELD_DTYPE)
    rec["disp"], rec["G"] = rng.normal(0, 3, (m, 3)), rng.normal(0, 0.05, (m, 9))
    rec["rms"], rec["wsum"] = rng.random(m), rng.random(m) * 50
    rec["status"] = np.array([0, 0, 1, 2, 4, 5, 0])[np.arange(m) % 7]
    return rec, {"disp": rec["disp"].copy(), "G": rec["G"].reshape(-1, 3, 3).copy(), "status": rec["status"].copy()}


def test_field_queries(capi):
    rng = np.random.default_rng(1)
    q = rng.integers(-2 ** 24, 2 ** 24, (50, 3)).astype(np.int32)
    u = rng.normal(0, 5, (50, 3))
    u[3, 1], u[4, 0], u[5, 2] = np.nan, np.inf, -np.inf
    got = capi.field_queries(q, u)
    assert np.array_equal(bits(got), bits(ref.queries(q, u)))
    assert np.isnan(got[3, 1]) and got[4, 0] == np.inf and got[5, 2] == -np.inf and np.isfinite(got[6:]).all()
    assert capi.field_queries(np.zeros((0, 3), np.int32), np.zeros((0, 3))).shape == (0, 3)
    L, ptr = capi.lib(), np.zeros(8).ctypes.data_as(C.c_void_p)
    assert L.sift3d_field_queries_from_displacements(None, None, -1, None) == ERR_ARG
    assert L.sift3d_field_queries_from_displacements(None, ptr, 1, ptr) == ERR_ARG
    assert L.sift3d_field_queries_from_displacements(ptr, None, 1, ptr) == ERR_ARG
    assert L.sift3d_field_queries_from_displacements(ptr, ptr, 1, None) == ERR_ARG
    assert L.sift3d_field_queries_from_displacements(None, None, 0, None) == 0


def test_field_unpack(capi):
    rec, res = records(capi, np.random.default_rng(2), 40)
    assert set(rec["status"]) == {0, 1, 2, 4, 5}
    d, g, v = capi.field_unpack(rec)
    wd, wg, wv = ref.unpack(res)
    assert np.array_equal(bits(d), bits(wd)) and np.array_equal(bits(g), bits(wg)) and np.array_equal(v, wv) and v.dtype == np.uint8
    d2, g2, v2 = capi.field_unpack({"records": rec})
    assert np.array_equal(d2, d) and np.array_equal(g2, g) and np.array_equal(v2, v)
    # grad9 and valid may be absent
    L = capi.lib()
    out = np.full((40, 3), np.nan)
    assert L.sift3d_field_unpack(rec.ctypes.data_as(C.c_void_p), 40, out.ctypes.data_as(C.c_void_p), None, None) == 0
    assert np.array_equal(bits(out), bits(wd))
    ptr = out.ctypes.data_as(C.c_void_p)
    assert L.sift3d_field_unpack(None, 2, ptr, None, None) == ERR_ARG
    assert L.sift3d_field_unpack(ptr, 2, None, None, None) == ERR_ARG
    assert L.sift3d_field_unpack(None, -1, None, None, None) == ERR_ARG
    assert L.sift3d_field_unpack(None, 0, None, None, None) == 0


def test_compose_displacements(capi):
    rng = np.random.default_rng(3)
    m = 60
    rec, res = records(capi, rng, m)
    uA, gA = rng.normal(0, 4, (m, 3)), rng.normal(0, 0.08, (m, 9))
    vA = (rng.random(m) > 0.3).astype(np.uint8)
    for grad in (gA, None):
        for valid in (vA, None):
            d, g, v = capi.compose_displacements(uA, grad, valid, rec)
            wd, wg, wv = ref.compose(uA, grad, valid, res)
            assert np.array_equal(bits(d), bits(wd)) and np.array_equal(v, wv)
            assert (g is None and wg is None) if grad is None else np.array_equal(bits(g), bits(wg))
            assert not d[v == 0].any() and (grad is None or not g[v == 0].any())
            assert 0 < v.sum() < m
    # the product is G_B G_A, not G_A G_B, and the association is the header's
    d, g, v = capi.compose_displacements(uA, gA, None, rec)
    k = int(np.flatnonzero(v)[0])
    GA, GB = gA[k].reshape(3, 3), rec["G"][k].reshape(3, 3)
    assert np.abs(g[k].reshape(3, 3) - (GA + GB + GB @ GA)).max() < 1e-15 and np.abs(GB @ GA - GA @ GB).max() > 1e-6
    assert np.abs((np.eye(3) + g[k].reshape(3, 3)) - (np.eye(3) + GB) @ (np.eye(3) + GA)).max() < 1e-15
    # NaN displacements of step A pass through where the record is valid
    uN = uA.copy()
    uN[k, 1] = np.nan
    d, _, v = capi.compose_displacements(uN, None, None, rec)
    assert v[k] == 1 and np.isnan(d[k, 1]) and np.array_equal(bits(d), bits(ref.compose(uN, None, None, res)[0]))
    # a gradient is asked for and step A has none: refused
    L = capi.lib()
    P = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    out3, out9, outv = np.zeros((m, 3)), np.zeros((m, 9)), np.zeros(m, np.uint8)
    assert L.sift3d_compose_displacements(P(uA), None, None, P(rec), m, P(out3), P(out9), P(outv)) == ERR_ARG
    assert b"bad argument" in L.sift3d_last_error()
    assert L.sift3d_compose_displacements(P(uA), None, None, P(rec), 0, P(out3), P(out9), P(outv)) == ERR_ARG
    assert L.sift3d_compose_displacements(P(uA), P(gA), None, P(rec), m, P(out3), None, None) == 0
    assert np.array_equal(bits(out3), bits(ref.compose(uA, None, None, res)[0]))
    assert L.sift3d_compose_displacements(None, None, None, P(rec), m, P(out3), None, None) == ERR_ARG
    assert L.sift3d_compose_displacements(P(uA), None, None, None, m, P(out3), None, None) == ERR_ARG
    assert L.sift3d_compose_displacements(P(uA), None, None, P(rec), m, None, None, None) == ERR_ARG
    assert L.sift3d_compose_displacements(None, None, None, None, -1, None, None, None) == ERR_ARG
    assert L.sift3d_compose_displacements(None, None, None, None, 0, None, None, None) == 0


def test_icgn_init_from_field(capi):
    rng = np.random.default_rng(4)
    m = 30
    u, g = rng.normal(0, 4, (m, 3)), rng.normal(0, 0.08, (m, 9))
    u[7, 0] = np.nan
    valid = (rng.random(m) > 0.4).astype(np.uint8)
    init = rng.normal(0, 1, (m, 12))
    for grad in (g, None):
        for only_valid in (True, False):
            for v in (valid, None):
                got, count = capi.icgn_init_from_field(u, grad, v, only_valid=only_valid, init=init)
                want, wcount = ref.init_from_field(u, grad, v, only_valid, init)
                assert np.array_equal(bits(got), bits(want)) and count == wcount
    got, count = capi.icgn_init_from_field(u, g, valid)   # init None: the rows not written stay NaN
    assert count == valid.sum() and np.isnan(got[valid == 0]).all() and np.array_equal(got[valid != 0][:, [0, 4, 8]], u[valid != 0], equal_nan=True)
    assert np.array_equal(got[valid != 0][:, [1, 2, 3, 5, 6, 7, 9, 10, 11]], g[valid != 0])
    got, count = capi.icgn_init_from_field(u, None, valid, only_valid=False)
    assert count == m and not got[:, [1, 2, 3, 5, 6, 7, 9, 10, 11]].any()
    e0, c0 = capi.icgn_init_from_field(np.zeros((0, 3)))
    assert e0.shape == (0, 12) and c0 == 0
    L, ptr = capi.lib(), np.zeros(16).ctypes.data_as(C.c_void_p)
    assert L.sift3d_icgn_init_from_field(None, None, None, -1, 0, None, None) == ERR_ARG
    assert L.sift3d_icgn_init_from_field(None, None, None, 1, 0, ptr, None) == ERR_ARG
    assert L.sift3d_icgn_init_from_field(ptr, None, None, 1, 0, None, None) == ERR_ARG
    assert L.sift3d_icgn_init_from_field(ptr, None, None, 1, 1, ptr, None) == 0   # no count wanted
    assert L.sift3d_icgn_init_from_field(None, None, None, 0, 0, None, None) == 0


G0 = np.array([[0.010, -0.004, 0.002], [0.003, -0.020, 0.001], [-0.002, 0.005, 0.015]])
B0 = np.array([1.25, -2.5, 0.75])


@pytest.mark.parametrize("solve", ["normal", "lstsq"])
def test_restatement_on_a_known_field(solve):
    rng = np.random.default_rng(6)
    q = ref.jittered_lattice(rng, (7, 6, 5))
    xs = 4.0 + rng.random((60, 3)) * np.array([20.0, 16.0, 12.0])
    u = q @ G0.T + B0
    for weighting in ref.WEIGHTINGS:
        got = ref.evaluate(q, u, None, xs, radius=7, weighting=weighting, solve=solve)
        assert (got["status"] == 0).all() and (got["sides"] == 63).all() and got["neighbours"].min() >= 27
        assert np.abs(got["G"] - G0).max() < 1e-13 and np.abs(got["disp"] - (xs @ G0.T + B0)).max() < 1e-12 and got["rms"].max() < 1e-12
        assert (got["wsum"] == got["neighbours"]).all() if weighting == 0 else (got["wsum"] < got["neighbours"]).all()
        const = ref.evaluate(q, np.tile(B0, (len(q), 1)), None, xs, radius=7, weighting=weighting, solve="normal")
        assert (const["status"] == 0).all() and not const["G"].any() and not const["rms"].any() and (const["disp"] == B0).all()


def test_restatement_statuses_and_faces():
    g = 3 * np.arange(5)
    q = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(np.int32)
    u = q @ G0.T + B0
    x = np.array([[6.0, 6.0, 6.0], [np.nan, 6, 6], [6, np.inf, 6], [6, 6, 2.0 ** 24 + 1], [-0.5, 6.0, 6.0], [6.5, 6.25, 5.75]])
    # a POI at |d| = radius exactly is a member with weight 1 under weighting 0 and has weight 0 under weighting 1
    a = ref.evaluate(q, u, None, x, radius=3, min_neighbours=4, weighting=0)
    b = ref.evaluate(q, u, None, x, radius=3, min_neighbours=4, weighting=1)
    assert list(a["status"]) == [0, 2, 2, 2, 5, 0] and list(a["neighbours"]) == [27, 0, 0, 0, 9, 8] and list(a["sides"]) == [63, 0, 0, 0, 62, 63]
    assert list(b["status"]) == [1, 2, 2, 2, 1, 0] and list(b["neighbours"]) == [1, 0, 0, 0, 1, 8] and list(b["sides"]) == [63, 0, 0, 0, 62, 63]
    assert ref.evaluate(q, u, None, x, radius=3, min_neighbours=4, weighting=0, require_enclosed=0)["status"][4] == 4   # one plane x = 0
    plane = q[:, 2] == 6
    assert ref.evaluate(q[plane], u[plane], None, x[:1], radius=7, min_neighbours=4, require_enclosed=0)["status"][0] == 4
    same = ref.enclosed(ref.evaluate(q, u, None, x, radius=3, min_neighbours=4, weighting=0, require_enclosed=0))
    assert all(np.array_equal(same[k], a[k]) for k in a)


def test_value_of_e():
    e = ref.parity_error()
    q, u, valid, xs = ref.parity_inputs()
    print(f"e = {e:.3e}, bar of the parity inputs = {ref.bar(e, ref.largest_u(u)):.3e}")
    assert len(q) == 2445 <= 4000 and len(xs) == 1500 and q.min() >= 0 and q.max() < 64 and 0.05 < 1 - valid.mean() < 0.15 and 5.0 < np.abs(u).max() <= 10.0
    assert len(np.unique(q, axis=0)) < len(q)
    assert 0.0 < e < 1e-9   # a sanity cap, not the bar
    for wt in ref.WEIGHTINGS:
        counts = {r: np.bincount(ref.parity_reference(r, wt)["status"], minlength=6) for r in ref.PARITY_RADII}
        print(wt, {r: c.tolist() for r, c in counts.items()})
        assert all(c[0] >= 50 and c[1] >= 40 for c in counts.values()) and counts[1][4] > 10
        assert np.bincount(ref.enclosed(ref.parity_reference(16, wt))["status"], minlength=6)[5] > 20
        assert (ref.parity_reference(40, wt)["sides"] != 63).sum() > 100


def test_cell_inputs_are_as_well_posed_as_the_parity_inputs():
    """the bar is made of e, the gap between the two solves on the parity inputs: an input whose own gap is larger asks more of the
    kernel's sums than the bar allows for"""
    q, u, xs = ref.cell_inputs()
    for wt in ref.WEIGHTINGS:
        a = ref.evaluate(q, u, None, xs, weighting=wt, require_enclosed=0, **ref.CELL_OPTIONS)
        gap = ref.solve_gap(a, ref.evaluate(q, u, None, xs, weighting=wt, require_enclosed=0, solve="lstsq", **ref.CELL_OPTIONS))
        print(f"weighting {wt}: gap of the two solves {gap:.3e}, status counts {np.bincount(a['status'], minlength=6).tolist()}")
        assert gap <= ref.parity_error()


def test_continuity_precondition():
    """where the outlying POI enters the window the uniform fit jumps and the weighted one does not"""
    q, u, xs = ref.continuity_inputs()
    step = {}
    for wt in ref.WEIGHTINGS:
        got = ref.evaluate(q, u, None, xs, weighting=wt, **ref.CONTINUITY_OPTIONS)
        assert (got["status"] == 0).all()
        n = got["neighbours"]
        assert n[-1] == n[0] + 1 and (np.diff(n) >= 0).all()   # one POI enters, none leaves
        step[wt] = ref.largest_step(got["disp"])
    print(f"largest step of disp along the slide: uniform {step[0]:.3e}, biweight {step[1]:.3e}")
    assert step[1] < step[0] and step[0] > 1e-3


def test_shell_field_links_and_reports_failure(tmp_path, capi):
    out, err = field_shell.run(tmp_path)
    assert out[:5] == ["2", "64", "64", "64", "2"], out
    if capi.device_count() > 0:
        field_shell.check_gpu_output(out)
        return
    assert out[5:] == ["-1", "-1", "-1", "-1", "1", "-1", "0.000000", "0.000000", "0.000000", "-1"], out
    assert "EvaluateField" in err and "no CPU fallback" in err
