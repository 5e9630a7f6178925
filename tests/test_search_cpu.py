"""CPU tests of the ZNCC integer search's boundary (sift3d_zncc_search, sift3d_icgn_init_from_search, include/sift3d_hip.h): the
header compiles as C and C++ with its layout guards, the library exports the entry points, the defaults need no GPU, bad arguments
are refused before any device call, the init from search results is exact, the CPU restatement (tests/zncc_search_ref.py) recovers
known shifts and gives every status, the inputs of the GPU parity test and of tests/test_gpu_search_plans.py (every launch plan, the long call, the
invariance pair, the voxel classes) have the margin that lets them compare d exactly and a float32 error e under the cap, and the C++
shell's SearchDisplacements and RefineDisplacements with a fallback link."""
import ctypes as C
import importlib
import os
import shutil
import subprocess

import numpy as np
import pytest

import icgn_ref
import zncc_search_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["sift3d_default_search_options", "sift3d_zncc_search", "sift3d_icgn_init_from_search"]
ERR_ARG = 1
INT_MAX = 2 ** 31 - 1


@pytest.fixture(scope="module")
def capi():
    m = importlib.import_module("3dsift_amd.capi")
    if not os.path.exists(m.LIB_PATH):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "3dsift_amd", "csrc"), "-j8"])
    return m


PROBE = r"""
#include <stddef.h>
#include "sift3d_hip.h"
SIFT3D_STATIC_ASSERT(sizeof(sift3d_search_options) == 32, "options");
SIFT3D_STATIC_ASSERT(sizeof(sift3d_search_result) == 48, "result");
SIFT3D_STATIC_ASSERT(offsetof(sift3d_search_result, status) == 12 && offsetof(sift3d_search_result, zncc) == 16 &&
                     offsetof(sift3d_search_result, zncc_second) == 24 && offsetof(sift3d_search_result, candidates) == 32, "result offsets");
int probe(const float *r, const float *t, const int *pts, const int *guess, int m, double *init, sift3d_search_result *out) {
	sift3d_search_options o;
	double s;
	sift3d_default_search_options(&o);
	o.search_radius = 4;
	return sift3d_zncc_search(r, 64, 64, 64, t, 64, 64, 64, pts, m, guess, &o, 0, 0, out, &s) + sift3d_icgn_init_from_search(out, m, 1, init);
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
    o = capi.SearchOptions()
    C.memset(C.byref(o), 0x5A, C.sizeof(o))
    capi.lib().sift3d_default_search_options(C.byref(o))
    assert (o.subset_radius, o.search_radius) == (8, 8)
    assert list(o.reserved) == [0] * 6
    assert capi.default_search_options() == {"subset_radius": 8, "search_radius": 8}
    f = capi.SEARCH_DTYPE.fields
    assert capi.SEARCH_DTYPE.itemsize == 48 and C.sizeof(capi.SearchOptions) == 32
    assert (f["status"][1], f["zncc"][1], f["zncc_second"][1], f["candidates"][1]) == (12, 16, 24, 32)


def _opts(capi, **kw):
    o = capi.SearchOptions()
    capi.lib().sift3d_default_search_options(C.byref(o))
    for k, v in kw.items():
        if k == "reserved":
            o.reserved[v] = 1
        else:
            setattr(o, k, v)
    return o


BAD_OPTS = [dict(subset_radius=1), dict(subset_radius=17), dict(search_radius=0), dict(search_radius=17), dict(reserved=0), dict(reserved=5)]


def _call(capi, o=None, ref=True, tar=True, pts=True, out=True, m=2, dims=(64, 64, 64, 64, 64, 64)):
    v = np.zeros((4, 4, 4), np.float32)
    q = np.zeros((2, 3), np.int32)
    res = np.zeros(2, capi.SEARCH_DTYPE)
    P = lambda a, on: a.ctypes.data_as(C.c_void_p) if on else None  # noqa: E731
    return capi.lib().sift3d_zncc_search(P(v, ref), dims[0], dims[1], dims[2], P(v, tar), dims[3], dims[4], dims[5], P(q, pts), m, None,
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
    assert _call(capi, pts=False, m=2) == ERR_ARG
    assert b"bad argument" in capi.lib().sift3d_last_error()


def test_init_from_search(capi):
    rng = np.random.default_rng(7)
    m = 40
    res = {"d": rng.integers(-20, 21, (m, 3)).astype(np.int32), "status": rng.choice([0, 0, 0, 2, 3, 4], m).astype(np.int32)}
    init = rng.normal(0, 1, (m, 12))
    missing = rng.random(m) < 0.5
    init[missing, rng.integers(0, 12, missing.sum())] = np.nan
    init[np.flatnonzero(missing)[0], 3] = np.inf
    ok = res["status"] == 0
    assert (ok & missing).any() and (ok & ~missing).any() and (~ok & missing).any()
    rows = np.zeros((m, 12))
    rows[:, [0, 4, 8]] = res["d"]
    bits = lambda a: np.ascontiguousarray(a, np.float64).view(np.uint64)  # noqa: E731
    got = capi.icgn_init_from_search(res, init, only_missing=True)
    touched = ok & missing
    assert np.array_equal(got[touched], rows[touched])
    assert np.array_equal(bits(got[~touched]), bits(init[~touched]))
    assert np.array_equal(bits(got), bits(ref.init_from_search(res, init, True)))
    got = capi.icgn_init_from_search(res, init, only_missing=False)
    assert np.array_equal(got[ok], rows[ok])
    assert np.array_equal(bits(got[~ok]), bits(init[~ok]))
    # no init: NaN rows, filled where the search succeeded
    got = capi.icgn_init_from_search(res)
    assert np.array_equal(got[ok], rows[ok]) and np.isnan(got[~ok]).all()
    one = capi.icgn_init_from_search({"d": [[6, -5, 4]], "status": [0]})
    assert np.array_equal(one[0], [6, 0, 0, 0, -5, 0, 0, 0, 4, 0, 0, 0])
    L = capi.lib()
    assert L.sift3d_icgn_init_from_search(None, -1, 1, None) == ERR_ARG
    assert L.sift3d_icgn_init_from_search(None, 2, 1, None) == ERR_ARG
    assert b"bad argument" in L.sift3d_last_error()
    assert L.sift3d_icgn_init_from_search(None, 0, 1, None) == 0


def test_restatement_recovers_shifts():
    q = np.array([[24, 24, 24], [20, 27, 23], [27, 21, 26]])
    R, T, _ = icgn_ref.scene((48, 48, 48), tvec=(3.0, -2.0, 4.0))
    res = ref.search(R, T, q, subset_radius=6, search_radius=5)
    assert (res["status"] == 0).all() and (res["d"] == (3, -2, 4)).all() and (res["zncc"] > 0.999).all()
    assert (res["candidates"] == 11 ** 3).all() and (res["zncc_second"] < res["zncc"]).all()
    # an integer-plus-fraction move of narrow blobs (icgn_ref.render): every subset has texture on each axis, so the rounded shift is
    # the best integer
    R, T = ref.scene((48, 48, 48), (3.37, -2.7, 4.21), seed=3, per=48, sigma=(1.0, 2.0))
    for f32 in (False, True):
        res = ref.search(R, T, q, subset_radius=6, search_radius=5, f32=f32)
        assert (res["status"] == 0).all() and (res["d"] == (3, -3, 4)).all(), res
    # the same through a guess that leaves the truth at the corner of a small search range
    res = ref.search(R, T, q, guess=np.tile([2, -2, 5], (3, 1)), subset_radius=6, search_radius=1)
    assert (res["status"] == 0).all()
    assert (res["d"] == (3, -3, 4)).all() and (res["candidates"] == 27).all()


def test_restatement_statuses():
    R, T, _ = icgn_ref.scene((40, 40, 40), tvec=(1.0, 0.0, 0.0))
    one = lambda R_, T_, q, g=(0, 0, 0): ref.search(R_, T_, [q], [g], subset_radius=5, search_radius=3)  # noqa: E731
    a = one(R, T, (4, 20, 20), (1, 2, 3))
    assert (a["status"][0], list(a["d"][0]), a["zncc"][0], a["zncc_second"][0], a["candidates"][0]) == (2, [1, 2, 3], 0.0, -2.0, 0)
    assert one(R, T, (5, 20, 20))["status"][0] == 0
    assert one(np.ones_like(R), T, (20, 20, 20))["status"][0] == 4
    for g in ((10 ** 6, 0, 0), (INT_MAX, 0, 0), (0, -INT_MAX - 1, 0), (0, 0, 2 ** 24 + 1)):
        a = one(R, T, (20, 20, 20), g)
        assert (a["status"][0], list(a["d"][0]), a["candidates"][0]) == (3, list(g), 0), g
    for const in (0.0, 1.0, 3e7):
        Tc = T.copy()
        Tc[20 - 8:20 + 9, 20 - 8:20 + 9, 20 - 8:20 + 9] = const  # the whole search region of the POI
        for f32 in (False, True):
            st, tab = ref.scores(R, Tc, (20, 20, 20), subset_radius=5, search_radius=3, f32=f32)
            assert st == 3 and not np.isfinite(tab).any(), const
    # the window hangs over T's faces: only admissible candidates are scored
    a = one(R, T, (6, 20, 33), (0, 0, 0))
    assert a["status"][0] == 0 and a["candidates"][0] == 5 * 7 * 5


@pytest.mark.parametrize("r,s", list(ref.PARITY), ids=[f"r{a}-s{b}" for a, b in ref.PARITY])
def test_parity_inputs_have_margin(r, s):
    """what lets tests/test_gpu_search.py compare d exactly and exclude no POI: on each of its inputs the restatement's best score
    beats every other scored candidate by at least 0.05, in fp64 and in float32, and both choose the same d (the truth)"""
    for edge in ref.EDGES:
        R, T, q, g, d = ref.parity_case(r, s, edge)
        assert R.shape != T.shape or (r, s) == (16, 16)
        a, b = ref.parity_reference(r, s, edge), ref.parity_reference(r, s, edge, True)
        assert (a["status"] == 0).all() and (b["status"] == 0).all()
        assert np.array_equal(a["d"], b["d"]) and (a["d"] == d).all()
        assert np.array_equal(a["candidates"], b["candidates"])
        if edge:
            assert ((a["d"][:, 0] - g[:, 0]) == edge * s).all()  # the truth lies at the edge of the search range
        for res in (a, b):
            for tab in res["tables"]:
                v = np.sort(tab[np.isfinite(tab)])[::-1]
                assert v[0] - v[1] >= 0.05, (r, s, edge, v[:3])


def test_parity_bar():
    e = ref.parity_error()
    print(f"e = {e:.3e}, bar = {ref.parity_bar():.3e}")
    assert 0.0 < e < 1e-4  # a float32 evaluation of a score in [-1, 1] over at most 33^3 voxels
    assert ref.parity_bar() >= 1e-6


def margin(tab):
    v = np.sort(tab[np.isfinite(tab)])[::-1]
    return v[0] - v[1] if len(v) > 1 else 1.0


def check_margins(a, b, truth):
    """the best score beats every other by at least 0.05 in fp64 (a) and in float32 (b), and both choose the truth"""
    ok = a["status"] == 0
    assert np.array_equal(a["status"], b["status"]) and np.array_equal(a["d"], b["d"]) and np.array_equal(a["candidates"], b["candidates"])
    assert (a["d"][ok] == truth).all(), a["d"]
    for res in (a, b):
        for i in np.flatnonzero(ok):
            assert margin(res["tables"][i]) >= 0.05, (i, margin(res["tables"][i]))


def test_search_plan_regimes():
    """the restated search_plan enters the regimes that tests/test_gpu_search_plans.py is there for"""
    plan = {p: ref.search_plan(*p) for p in ref.PAIRS}
    assert len(plan) == 240
    assert [plan[p] for p in ((2, 1), (4, 2), (5, 3), (5, 7), (8, 8), (16, 16))] == [(3, 5), (5, 9), (7, 11), (5, 11), (4, 9), (1, 3)]
    assert sorted(p for p, (ec, zs) in plan.items() if zs == 1) == [(13, 5), (14, 5), (15, 4), (15, 5), (15, 6), (16, 4), (16, 5), (16, 6)]
    free = lambda s: min(max(1280 // (2 * s + 1) ** 2, 1), 2 * s + 1)  # noqa: E731  ec before the LDS bound lowers it
    assert sorted(p for p, (ec, zs) in plan.items() if ec < free(p[1])) == [(15, 5), (16, 4), (16, 5)]
    full = [p for p, (ec, zs) in plan.items() if ec == 2 * p[1] + 1 and (2 * p[0] + 1) % zs]
    assert len(full) == 28 and (8, 3) in full and (16, 2) in full
    assert sorted(p for p, (ec, zs) in plan.items() if ec == 1 and zs == 2 * p[0] + 1) == [(r, s) for r in (2, 3, 4) for s in (13, 14, 15, 16)]
    assert sum(1 for (r, s), (ec, zs) in plan.items() if (2 * s + 1) % ec and (2 * r + 1) % zs) == 63
    for (r, s), (ec, zs) in plan.items():
        D, E = 2 * r + 1, 2 * s + 1
        assert 1 <= ec <= E and 1 <= zs <= D and (ec * E * E <= 1280 or ec == 1)
        assert (zs + ec - 1) * (D + 2 * s) ** 2 + zs * D * D <= ref.LDS_FLOATS


@pytest.mark.parametrize("r", range(2, 17))
def test_plan_inputs_have_margin(r):
    """every input of test_every_plan: the geometry of its three POIs and the margin that lets the GPU test compare d exactly"""
    for s in range(1, 17):
        R, T, q = ref.plan_case(r, s)
        assert R.shape == T.shape == ref.PLAN_SHAPE and len(set(R.shape)) == 3
        E, (ec, _) = 2 * s + 1, ref.search_plan(r, s)
        rng = [[ref.admissible(q[i][ax], 0, r, s, n) for ax, n in enumerate(R.shape[::-1])] for i in range(3)]
        assert all(lo == 0 and hi == E - 1 for lo, hi in rng[0])
        (xl, xh), _, (zl, zh) = rng[1]
        assert zl > 0 and zh == E - 1 and xl == 0 and xh < E - 1 and (ec == 1 or (zh - zl + 1) % ec)
        _, (yl, yh), (zl, zh) = rng[2]
        assert zl == 0 and zh < E - 1 and yl > 0 and yh == E - 1
        a, b = ref.plan_reference(r, s), ref.plan_reference(r, s, True)
        assert (a["status"] == 0).all() and a["candidates"][0] == E ** 3 and (a["candidates"][1:] < E ** 3).all()
        check_margins(a, b, ref.PLAN_D)


def test_long_inputs_have_margin():
    R, T, q, g, kinds = ref.long_case()
    M = ref.MAX_GROUPS
    assert len(q) == 2 * M + 37 and all(kinds[i] != kinds[i + M] for i in range(M + 37))
    assert any(kinds[j] == "full" and kinds[j + M] == "clipped" for j in range(M))
    a, b = ref.long_reference(), ref.long_reference(True)
    want = {"full": 0, "clipped": 0, "st2": 2, "st4": 4, "st3": 3}
    assert [int(v) for v in a["status"]] == [want[k] for k in kinds]
    cand = a["candidates"]
    assert all(cand[i] == 125 for i, k in enumerate(kinds) if k == "full") and all(27 <= cand[i] <= 80 for i, k in enumerate(kinds) if k == "clipped")
    check_margins(a, b, ref.LONG_D)


def test_plan_bar():
    e = ref.plan_error()
    print(f"plans and long call: e = {e:.3e}, bar = {ref.plan_bar():.3e}")
    assert 0.0 < e < 1e-4


def test_invariance_inputs_have_margin():
    R, T, q = ref.invariance_case()
    assert np.array_equal(R, np.round(R)) and np.array_equal(T, np.round(T)) and 0 < min(R.min(), T.min()) and max(R.max(), T.max()) < 2 ** 12
    for off in (False, True):
        a, b = ref.invariance_reference(off), ref.invariance_reference(off, True)
        assert (a["status"] == 0).all() and len(set(a["candidates"])) > 2
        check_margins(a, b, ref.INV_D)
    e = ref.invariance_error()
    print(f"invariance pair: e = {e:.3e}, bar = {ref.invariance_bar():.3e}")
    assert 0.0 < e < 1e-4
    base = ref.invariance_reference()
    for add in ref.INV_T_OFFSETS:  # the restatement itself: an integer added to T changes no scored set and no d
        got = ref.search(R, T + np.float32(add), q, subset_radius=ref.INV_R, search_radius=ref.INV_S)
        assert np.array_equal(got["candidates"], base["candidates"]) and np.array_equal(got["d"], base["d"])
        assert np.abs(got["zncc"] - base["zncc"]).max() < 1e-12


@pytest.mark.parametrize("name", ref.CLASSES)
def test_class_inputs(name):
    """the voxel classes of tests/test_gpu_search_plans.py: what each is named for, e under the cap, and the margins"""
    R, T, q = ref.class_case(name)
    r, s = ref.CLASS_R, ref.CLASS_S
    a, b = ref.class_reference(name), ref.class_reference(name, True)
    e, same = ref.class_error(name)
    print(f"class {name}: e = {e:.3e}, bar = {ref.class_bar(name):.3e}")
    assert e < 1e-4
    full = np.array([(2 * s + 1) ** 3] * 6)
    if name == "huge":
        assert (a["status"] == 0).all() and (b["status"] == 3).all() and not b["candidates"].any()
        return
    assert same
    if name in ("nan_subset", "inf_subset"):
        assert (a["status"] == 4).all() and (b["status"] == 4).all()
        return
    assert (a["status"] == 0).all()
    check_margins(a, b, ref.CLASS_D)
    assert np.abs(b["zncc"]).max() <= 1.0 + ref.class_bar(name) and np.abs(b["zncc_second"]).max() <= 1.0 + ref.class_bar(name)
    if name in ("nan_corner", "inf_corner"):
        assert np.array_equal(a["candidates"][:6], full - 1) and all(np.isnan(t[0, 0, 0]) for t in a["tables"][:6])
    elif name == "nan_tc":  # the candidates whose subset holds q + g are skipped, the others scored
        assert np.array_equal(a["candidates"][:6], full - (2 * r + 1) ** 3)
        assert all(np.isnan(t[s - r:s + r + 1, s - r:s + r + 1, s - r:s + r + 1]).all() for t in a["tables"])
    else:
        assert np.array_equal(a["candidates"][:6], full)
    assert a["candidates"][6] < full[0]  # the last POI's window hangs over T's high x face
    if name.startswith("outlier"):
        v = 0.0 if name.startswith("outlier0") else 65535.0
        assert all(T[z, y, x] == v for x, y, z in q) and (T == v).sum() == len(q) and abs(np.median(T) - 30000) < 300
        assert max(abs(c) for c in ref.CLASS_D) > r  # the subset of the best candidate does not hold the outlier
        for i in range(len(q)):
            for j in range(len(q)):
                assert i == j or np.abs(q[i] - q[j]).max() > r + s  # no POI's outlier lies in another's window


def test_centre_resists_one_voxel():
    """the level the sums are centred on: a voxel of T within the subset's spread, whatever the voxel at q + g holds"""
    R, T, q = ref.class_case("outlier0")
    for x, y, z in q:
        tc = ref.centre(T, (x, y, z), ref.CLASS_R)
        assert 29900 < tc < 30400 and (T == tc).any()
    flat = np.full((9, 9, 9), 3e7, np.float32)
    assert ref.centre(flat, (4, 4, 4), 3) == np.float32(3e7) and ref.centre(flat, (-50, 100, 4), 3) == np.float32(3e7)
    flat[4, 4, 4] = np.nan
    assert ref.centre(flat, (4, 4, 4), 3) == np.float32(3e7)
    assert ref.centre(np.full((9, 9, 9), np.nan, np.float32), (4, 4, 4), 3) == 0.0


SHELL = r"""
#include <cstdio>
#include <vector>
#include "cRegistration.h"
int main() {
	std::vector<float> v(32 * 32 * 32, 1.f);
	std::vector<CPUSIFT::Cvec> pts(1, CPUSIFT::Cvec(16, 16, 16)), guess(1, CPUSIFT::Cvec(1, 0, -1));
	std::vector<CPUSIFT::AffineFit> fits(1);
	CPUSIFT::SearchOptions so;
	so.subset_radius = 5;
	so.search_radius = 3;
	std::vector<CPUSIFT::SearchResult> s = CPUSIFT::SearchDisplacements(v.data(), 32, 32, 32, v.data(), 32, 32, 32, pts, &guess, so);
	std::vector<CPUSIFT::SearchResult> s0 = CPUSIFT::SearchDisplacements(v.data(), 32, 32, 32, v.data(), 32, 32, 32, pts, nullptr);
	CPUSIFT::IcgnOptions o;
	o.subset_radius = 5;
	std::vector<CPUSIFT::IcgnResult> r = CPUSIFT::RefineDisplacements(v.data(), 32, 32, 32, v.data(), 32, 32, 32, pts, &fits, o, &s);
	std::vector<CPUSIFT::IcgnResult> r5 = CPUSIFT::RefineDisplacements(v.data(), 32, 32, 32, v.data(), 32, 32, 32, pts, &fits, o);
	CPUSIFT::Cvec d = s[0].Displacement();
	std::printf("%zu %zu %d %d %g %g %d %d\n", s.size(), s0.size(), s[0].status, s[0].candidates, (double)d.x, s[0].zncc_second, r[0].status, r5[0].status);
	return 0;
}
"""


def test_shell_search_links(tmp_path):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no host compiler")
    d = os.path.join(ROOT, "3dsift_amd")
    if not os.path.exists(os.path.join(d, "libsift3d.so")):
        subprocess.check_call(["make", "-C", os.path.join(d, "host")])
    src = tmp_path / "search.cpp"
    src.write_text(SHELL)
    r = subprocess.run([cxx, "-std=c++14", "-Wall", "-Werror", "-o", str(tmp_path / "search"), str(src), "-I", os.path.join(d, "host", "Include"),
                        "-L" + d, "-lsift3d", "-lsift3d_hip", "-Wl,-rpath," + d], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
