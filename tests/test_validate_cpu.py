"""CPU tests of the displacement validation's boundary (sift3d_validate_displacements and its host-only helpers, include/sift3d_hip.h):
the header compiles as C and C++ with its layout guards, the library exports the entry points, the defaults need no GPU, bad arguments
are refused before any device call, the host-only helpers agree with the restatement (tests/validate_ref.py), the C++ shell's
ValidateDisplacements / KeepMask / SeedsFromValidation link and report a failed call, and the cases of tests/validate_cases.py do what
they claim on the restatement alone, none of them with a score near the threshold."""
import ctypes as C
import importlib
import os
import shutil
import subprocess

import numpy as np
import pytest

import validate_cases as cases
import validate_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["sift3d_default_validate_options", "sift3d_validate_input_from_icgn", "sift3d_validate_input_from_icgn2", "sift3d_validate_displacements",
       "sift3d_validate_keep", "sift3d_icgn_init_from_validation", "sift3d_validate_stage_capacity"]
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
#include "sift3d_hip_test.h"
SIFT3D_STATIC_ASSERT(sizeof(sift3d_validate_options) == 48, "options");
SIFT3D_STATIC_ASSERT(offsetof(sift3d_validate_options, threshold) == 16 && offsetof(sift3d_validate_options, eps) == 24, "option offsets");
SIFT3D_STATIC_ASSERT(sizeof(sift3d_validate_result) == 72, "result");
SIFT3D_STATIC_ASSERT(offsetof(sift3d_validate_result, mad) == 24 && offsetof(sift3d_validate_result, score) == 48 &&
                     offsetof(sift3d_validate_result, neighbours) == 56 && offsetof(sift3d_validate_result, status) == 60 &&
                     offsetof(sift3d_validate_result, flagged) == 64 && offsetof(sift3d_validate_result, pass) == 68, "result offsets");
int probe(const sift3d_icgn_result *ic, const sift3d_icgn2_result *ic2, const int *pts, int m, double *disp, double *grad, unsigned char *valid,
          sift3d_validate_result *out, double *init12) {
	sift3d_validate_options o;
	double s;
	int n, cap;
	sift3d_default_validate_options(&o);
	o.radius = 8;
	return sift3d_validate_input_from_icgn(ic, m, 0.5, 0, disp, grad, valid) + sift3d_validate_input_from_icgn2(ic2, m, 0.5, 0, disp, grad, valid) +
	       sift3d_validate_displacements(pts, disp, grad, valid, m, &o, 0, 0, out, &s) + sift3d_validate_keep(out, valid, m, valid) +
	       sift3d_icgn_init_from_validation(out, m, init12, &n) + sift3d_validate_stage_capacity(&cap);
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
    o = capi.ValidateOptions()
    C.memset(C.byref(o), 0x5A, C.sizeof(o))
    capi.lib().sift3d_default_validate_options(C.byref(o))
    assert (o.radius, o.min_neighbours, o.passes, o.threshold, o.eps) == (16, 6, 2, 2.0, 0.1)
    assert o.reserved0 == 0 and list(o.reserved) == [0] * 4
    assert capi.default_validate_options() == dict(ref.DEFAULTS)
    assert C.sizeof(capi.ValidateOptions) == 48 and capi.ValidateOptions.threshold.offset == 16 and capi.ValidateOptions.reserved.offset == 32
    f = capi.VALIDATE_DTYPE.fields
    assert capi.VALIDATE_DTYPE.itemsize == 72 and capi.VALIDATE_DTYPE == ref.RESULT_DTYPE
    assert [f[k][1] for k in ("median", "mad", "score", "neighbours", "status", "flagged", "pass")] == [0, 24, 48, 56, 60, 64, 68]
    cap = capi.validate_stage_capacity()
    assert 64 <= cap <= 4096   # a few KB of LDS per wave
    assert capi.lib().sift3d_validate_stage_capacity(None) == ERR_ARG


def _opts(capi, **kw):
    o = capi.ValidateOptions()
    capi.lib().sift3d_default_validate_options(C.byref(o))
    for k, v in kw.items():
        if k == "reserved":
            o.reserved[v] = 1
        else:
            setattr(o, k, v)
    return o


BAD_OPTS = [dict(radius=0), dict(radius=4097), dict(radius=-1), dict(min_neighbours=2), dict(min_neighbours=1048577), dict(passes=0), dict(passes=9),
            dict(threshold=0.0), dict(threshold=-1.0), dict(threshold=float("nan")), dict(threshold=float("inf")), dict(eps=0.0), dict(eps=-0.1),
            dict(eps=float("nan")), dict(eps=float("inf")), dict(reserved0=1)] + [dict(reserved=k) for k in range(4)]


def _call(capi, o=None, pts=True, disp=True, out=True, m=2):
    q = np.zeros((2, 3), np.int32)
    u = np.zeros((2, 3), np.float64)
    res = np.zeros(2, capi.VALIDATE_DTYPE)
    P = lambda a, on: a.ctypes.data_as(C.c_void_p) if on else None  # noqa: E731
    return capi.lib().sift3d_validate_displacements(P(q, pts), P(u, disp), None, None, m, C.byref(o) if o is not None else None, 0, 0, P(res, out), None)


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
    for good in (dict(radius=1, min_neighbours=3, passes=1, threshold=5e-324, eps=5e-324),
                 dict(radius=4096, min_neighbours=1048576, passes=8, threshold=1e308, eps=1e308)):
        assert _call(capi, _opts(capi, **good)) != ERR_ARG


def test_no_device_error(capi):
    if capi.device_count() > 0:
        pytest.skip("a GPU is visible here")
    with pytest.raises(capi.Sift3dError, match="no CPU fallback"):
        capi.validate(np.zeros((5, 3), np.int32), np.zeros((5, 3)))
    with pytest.raises(capi.Sift3dError, match="no CPU fallback"):
        capi.validate(np.zeros((0, 3), np.int32), np.zeros((0, 3)), np.zeros((0, 9)))
    with pytest.raises(TypeError):
        capi.validate(np.zeros((5, 3), np.int32), np.zeros((5, 3)), window=3)


@pytest.mark.parametrize("width", [12, 30])
def test_input_from_icgn(capi, width):
    rng = np.random.default_rng(5)
    m = 14
    w = width // 3
    res = {"p": rng.normal(0, 1, (m, width)), "zncc": np.full(m, 0.9), "status": np.array([0, 1, 2, 3, 4, 5, 6, 0, 0, 0, 0, 1, 0, 0], np.int32)}
    res["p"][7, w] = np.nan            # v
    res["p"][8, 2 * w] = np.inf        # w
    res["p"][9, w + 1] = np.nan        # a gradient term: the byte stays set, the validation itself drops the POI
    res["zncc"][10] = 0.49
    res["zncc"][12] = 0.5
    res["zncc"][13] = np.nan
    for zmin, acc in ((0.5, False), (0.5, True), (0.0, False)):
        disp, grad, valid = capi.validate_input_from_icgn(res, zncc_min=zmin, accept_unconverged=acc)
        d0, g0, v0 = ref.input_from_icgn(res["p"], res["zncc"], res["status"], zmin, acc)
        assert disp.shape == (m, 3) and grad.shape == (m, 9) and valid.dtype == np.uint8
        assert np.array_equal(disp.view(np.uint64), d0.view(np.uint64)) and np.array_equal(grad.view(np.uint64), g0.view(np.uint64))
        assert list(valid) == list(v0)
        # the same bytes and displacements as the strain input
        sd, sv = (capi.strain_input_from_icgn if width == 12 else capi.strain_input_from_icgn2)(res, zncc_min=zmin, accept_unconverged=acc)
        assert np.array_equal(sd.view(np.uint64), disp.view(np.uint64)) and list(sv) == list(valid)
    assert list(capi.validate_input_from_icgn(res, zncc_min=0.5)[2]) == [1, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 1, 0]
    assert np.array_equal(grad[0], res["p"][0, [1, 2, 3, w + 1, w + 2, w + 3, 2 * w + 1, 2 * w + 2, 2 * w + 3]])
    e = capi.validate_input_from_icgn({"p": np.zeros((0, width)), "zncc": [], "status": []})
    assert e[0].shape == (0, 3) and e[1].shape == (0, 9) and e[2].shape == (0,)
    fn = getattr(capi.lib(), "sift3d_validate_input_from_icgn" + ("" if width == 12 else "2"))
    buf = np.zeros(64)
    ptr = buf.ctypes.data_as(C.c_void_p)
    assert fn(None, -1, 0.0, 0, None, None, None) == ERR_ARG
    assert fn(None, 1, 0.0, 0, ptr, ptr, ptr) == ERR_ARG
    assert fn(ptr, 1, 0.0, 0, None, ptr, ptr) == ERR_ARG
    assert fn(ptr, 1, 0.0, 0, ptr, ptr, None) == ERR_ARG
    assert fn(None, 0, float("nan"), 0, None, None, None) == ERR_ARG
    assert fn(None, 0, 0.0, 0, None, None, None) == 0
    assert fn(ptr, 1, 0.0, 0, ptr, None, ptr) == 0   # the gradients are optional


def _records():
    """records of every status, flagged and not, with distinct medians"""
    rec = np.zeros(10, ref.RESULT_DTYPE)
    rec["status"] = [0, 0, 1, 1, 2, 3, 3, 0, 0, 3]
    rec["flagged"] = [0, 1, 0, 1, 0, 0, 0, 1, 0, 0]
    rec["pass"] = rec["flagged"] * 2
    rec["median"] = np.arange(30).reshape(10, 3) + 0.5
    rec["median"][7] = [-0.0, 1e300, 5e-324]
    return rec


def test_keep_and_seeds(capi):
    rec = _records()
    assert list(capi.validate_keep(rec)) == list(ref.keep(rec)) == [1, 0, 0, 0, 0, 0, 0, 0, 1, 0]
    vin = np.array([1, 1, 1, 1, 1, 1, 1, 1, 0, 1], np.uint8)
    assert list(capi.validate_keep(rec, vin)) == list(ref.keep(rec, vin)) == [1] + [0] * 9
    assert list(capi.validate_keep({"records": rec}, vin * 7)) == [1] + [0] * 9
    assert capi.validate_keep(rec[:0]).shape == (0,)
    init = np.random.default_rng(3).normal(0, 1, (10, 12))
    init[2] = np.nan
    got, count = capi.icgn_init_from_validation(rec, init)
    want, n = ref.init_from_validation(rec, init)
    assert count == n == 5 and np.array_equal(got.view(np.uint64), want.view(np.uint64))
    assert np.array_equal(got[1], [3.5, 0, 0, 0, 4.5, 0, 0, 0, 5.5, 0, 0, 0]) and np.array_equal(got[0], init[0])
    got, count = capi.icgn_init_from_validation(rec)   # no rows given: the others stay NaN
    assert count == 5 and np.isnan(got[[0, 2, 3, 4, 8]]).all() and np.isfinite(got[[1, 5, 6, 7, 9]]).all()
    L = capi.lib()
    ptr = np.zeros(64).ctypes.data_as(C.c_void_p)
    assert L.sift3d_validate_keep(None, None, -1, None) == ERR_ARG
    assert L.sift3d_validate_keep(None, None, 1, ptr) == ERR_ARG
    assert L.sift3d_validate_keep(ptr, None, 1, None) == ERR_ARG
    assert L.sift3d_validate_keep(None, None, 0, None) == 0
    assert L.sift3d_icgn_init_from_validation(None, -1, None, None) == ERR_ARG
    assert L.sift3d_icgn_init_from_validation(None, 1, ptr, None) == ERR_ARG
    assert L.sift3d_icgn_init_from_validation(ptr, 1, None, None) == ERR_ARG
    assert b"bad argument" in L.sift3d_last_error()
    assert L.sift3d_icgn_init_from_validation(None, 0, None, None) == 0


# ---- the restatement and the cases ---------------------------------------------------------------------------------------------------
def test_restatement_median():
    assert ref.median(np.array([3.0])) == 3.0
    assert ref.median(np.array([4.0, 1.0])) == 2.5
    assert ref.median(np.array([5.0, -1.0, 2.0])) == 2.0
    assert ref.median(np.array([0.25, 0.25, 0.25, 9.0])) == 0.25
    assert ref.median(np.array([1.0, 2.0, 3.0, 4.0, 5.0, 6.0])) == 3.5
    rng = np.random.default_rng(1)
    for n in (2, 3, 10, 11, 64, 65, 1000, 1001):
        v = np.round(rng.normal(0, 3, n) * 4) / 4
        s = np.sort(v)
        assert ref.median(v) == (s[n // 2] if n & 1 else 0.5 * (s[n // 2 - 1] + s[n // 2]))


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_no_score_near_the_threshold(name):
    rec, trace = cases.reference(name)
    thr = cases.get(name)["opts"].get("threshold", ref.DEFAULTS["threshold"])
    s = np.array([t[2] for t in trace] + list(rec["score"]))
    assert np.isfinite(s).all()
    gap = np.abs(s - thr).min() / thr
    print(f"{name}: {len(trace)} scores in the passes, nearest to the threshold {gap:.3e} (relative)")
    assert gap > 1e-6


@pytest.mark.parametrize("name", [n for n in sorted(cases.CASES) if n.startswith("planted")])
def test_planted_outliers_are_the_flagged_set(name):
    rec, trace = cases.reference(name)
    c = cases.get(name)
    assert len(c["points"]) == 729 and len(c["planted"]) == 36
    assert np.array_equal(np.flatnonzero(rec["flagged"]), c["planted"]) and (rec["status"] == 0).all()
    assert (rec["pass"][c["planted"]] >= 1).all() and not rec["pass"][rec["flagged"] == 0].any()
    clear = rec["score"][rec["flagged"] == 0].max()
    print(f"{name}: largest final score of an unflagged POI {clear:.3f}")
    assert clear < 2.0


def test_gradients_clear_a_curved_field():
    """what the gradient form is for: at curvature 2e-3 the plain test's largest unflagged score is several times the gradient form's"""
    plain = cases.reference("planted-k0.002-n0-plain")[0]
    grad = cases.reference("planted-k0.002-n0-grad")[0]
    a, b = plain["score"][plain["flagged"] == 0].max(), grad["score"][grad["flagged"] == 0].max()
    print(f"plain {a:.3f}, with gradients {b:.3f}")
    assert b < 0.5 * a


def test_passes_on_the_shifted_block():
    c = cases.get("block-p1")
    one = cases.reference("block-p1")[0]
    two = cases.reference("block-p2")[0]
    inside, centre = c["block"], c["centre"]
    q = c["points"]
    on_faces = ((q == 12) | (q == 20)).sum(1)   # 3 corner, 2 edge, 1 face, 0 centre (inside the block)
    assert inside.sum() == 27 and one["flagged"].sum() == 20 and not one["flagged"][~inside].any()
    assert np.array_equal(one["flagged"] != 0, inside & (on_faces >= 2)) and (one["pass"][one["flagged"] != 0] == 1).all()
    assert two["flagged"].sum() == 26 and (two["pass"] == 2).sum() == 6 and np.array_equal(two["pass"] == 2, inside & (on_faces == 1))
    assert not two["flagged"][~inside].any()
    assert two["flagged"][centre] == 0 and two["status"][centre] == 1 and two["neighbours"][centre] == 0
    for p in (3, 4):
        assert not ref.same(cases.reference(f"block-p{p}")[0], two)


def test_counts_and_rules_on_the_restatement(capi):
    assert cases.reference("m1")[0]["status"].tolist() == [1] and cases.reference("m1")[0]["neighbours"].tolist() == [0]
    assert cases.reference("m2")[0]["neighbours"].tolist() == [1, 1]
    below, at = cases.reference("n-min-minus-1")[0], cases.reference("n-min-even")[0]
    assert (below["status"] == 1).all() and (below["neighbours"] == 5).all() and not below["median"].any()
    assert (at["status"] == 0).all() and (at["neighbours"] == 6).all()
    assert (cases.reference("n-odd")[0]["neighbours"] == 7).all() and (cases.reference("n-min-3")[0]["status"] == 0).all()
    flags = cases.reference("n-odd-flags")[0]
    assert flags["flagged"].sum() > 0 and flags["pass"].max() >= 2
    inv = cases.reference("all-invalid")[0]
    assert (inv["status"] == 1).all() and not inv["neighbours"].any() and not inv["flagged"].any()
    c = cases.get("rules")
    r = cases.reference("rules")[0]
    q = c["points"].astype(np.int64)
    assert q[:, 0].max() - q[:, 0].min() > 2 ** 25 and (q < 0).any()
    assert np.flatnonzero(r["status"] == 2).tolist() == c["out_of_range"] and not r["neighbours"][c["out_of_range"]].any()
    assert r["status"][251] != 2                                     # a coordinate of exactly 2^24 is in range
    off = [3, 40, 130, 131, 10, 60, 140, 20, 150]                    # valid byte 0, non-finite disp, non-finite grad
    assert set(r["status"][off]) <= {1, 3} and (r["status"] == 3).sum() >= 5 and not r["flagged"][off].any() and not r["score"][off].any()
    assert r["status"][7] in (0, 1)                                  # any non-zero byte is valid
    # a duplicate is a neighbour, the POI itself is not: the pair at 255 / 256 sees one POI more than its spot would alone
    quiet = dict(c["opts"], threshold=1e308)                         # nothing is flagged: the counts are the windows'
    both = ref.validate(c["points"], c["disp"], c["grad"], c["valid"], **quiet)
    lone = ref.validate(*(np.delete(c[k], 256, 0) for k in ("points", "disp", "grad", "valid")), **quiet)
    assert both["neighbours"][255] == lone["neighbours"][255] + 1 == both["neighbours"][256]
    lg, lp = cases.reference("linear-grad")[0], cases.reference("linear-plain")[0]
    assert (lg["status"] == 0).all() and lg["score"].max() < 1e-9 and not lg["flagged"].any()
    corners = np.flatnonzero(lg["neighbours"] == 7)
    print("plain form at the corners of a linear field:", lp["score"][corners])
    assert len(corners) == 8 and lp["score"][corners].min() > 1e-9
    cap = capi.validate_stage_capacity()
    for name, n1 in (("cap-minus-1", cap - 1), ("cap", cap), ("cap-plus-1", cap + 1), ("cap-plus-2", cap + 2)):
        c = cases.get(name, cap)
        rec, trace = cases.reference(name, cap)
        first = ref.validate(c["points"], c["disp"], c["grad"], c["valid"], **dict(c["opts"], passes=1, threshold=1e308))
        assert first["neighbours"][c["centre"]] == n1 and rec["neighbours"][c["centre"]] == n1 - 1
        assert np.flatnonzero(rec["flagged"]).tolist() == [c["big"]]
        u = c["disp"]
        assert (u == 0).sum() > 20 and np.signbit(u[u == 0]).any() and (~np.signbit(u[u == 0])).any()       # both zeros
        assert ((u != 0) & (np.abs(u) < 2.3e-308)).any() and np.abs(u).max() == 1e300 and (u < 0).any()    # subnormals, the huge POI
        s = np.array([t[2] for t in trace])
        assert np.abs(s - 1e3).min() / 1e3 > 1e-6


def test_capacity_case_far_above(capi):
    cap = capi.validate_stage_capacity()
    rec, trace = cases.reference("cap-times-3", cap)
    c = cases.get("cap-times-3", cap)
    assert rec["neighbours"][c["centre"]] >= 3 * cap - 1 and (rec["neighbours"] > cap).sum() > 100 and (rec["neighbours"] <= cap).sum() > 100
    s = np.array([t[2] for t in trace])
    assert np.abs(s - 1e3).min() / 1e3 > 1e-6


SHELL = r"""
#include <cstdio>
#include <vector>
#include "cRegistration.h"
int main() {
	std::vector<CPUSIFT::Cvec> pts;
	std::vector<CPUSIFT::IcgnResult> disp;
	std::vector<CPUSIFT::Icgn2Result> disp2;
	for (int i = 0; i < 27; i++) {
		pts.push_back(CPUSIFT::Cvec((float)(4 * (i % 3)), (float)(4 * (i / 3 % 3)), (float)(4 * (i / 9))));
		CPUSIFT::IcgnResult r;
		r.status = 0;
		r.zncc = 0.99;
		r.p[0] = 0.01 * pts.back().x + (i == 13 ? 3.0 : 0.0);
		r.p[1] = 0.01;
		disp.push_back(r);
		CPUSIFT::Icgn2Result r2;
		r2.status = 0;
		r2.zncc = 0.99;
		r2.p[0] = r.p[0];
		r2.p[1] = 0.01;
		disp2.push_back(r2);
	}
	CPUSIFT::ValidationOptions o;
	o.radius = 8;
	std::vector<CPUSIFT::ValidationResult> v = CPUSIFT::ValidateDisplacements(pts, disp, o, 0.5, true);
	std::vector<CPUSIFT::ValidationResult> v2 = CPUSIFT::ValidateDisplacements(pts, disp2, o, 0.5, false, false);
	std::vector<unsigned char> keep = CPUSIFT::KeepMask(v);
	std::vector<CPUSIFT::AffineFit> seeds = CPUSIFT::SeedsFromValidation(pts, disp, v);
	CPUSIFT::StrainOptions so;
	so.radius = 8;
	so.measure = 1;
	std::vector<CPUSIFT::StrainResult> s = CPUSIFT::ComputeStrains(pts, disp, keep, so, 0.5);
	std::vector<CPUSIFT::StrainResult> s2 = CPUSIFT::ComputeStrains(pts, disp2, keep, so, 0.5);
	disp.pop_back();
	std::vector<CPUSIFT::ValidationResult> bad = CPUSIFT::ValidateDisplacements(pts, disp);
	std::printf("%zu %zu %zu %zu %zu %zu %d %d %d %d %d %d %d %g %g %g %g\n", v.size(), v2.size(), keep.size(), seeds.size(), s.size(), bad.size(),
	            v[0].status, v[13].flagged, v2[13].flagged, bad[0].status, (int)keep[0], (int)keep[13], seeds[13].status, seeds[13].A[3], seeds[0].A[0],
	            s[13].E[0] + s2[13].E[0], v[0].seconds);
	// a hand-made validation: the seeds need no GPU
	std::vector<CPUSIFT::ValidationResult> w(27);
	disp.push_back(disp[0]);
	for (int i = 0; i < 27; i++) w[i].status = i % 4;   // 0 kept, 1, 2: no start, 3: restarts from the median
	w[4].flagged = 1;
	for (int i = 0; i < 27; i++) w[i].median[0] = 7.0, w[i].median[1] = -1.0, w[i].median[2] = 0.5;
	std::vector<CPUSIFT::AffineFit> t = CPUSIFT::SeedsFromValidation(pts, disp, w);
	std::vector<unsigned char> k = CPUSIFT::KeepMask(w);
	CPUSIFT::Cvec d4 = t[4].Displacement(pts[4]), d8 = t[8].Displacement(pts[8]), d3 = t[3].Displacement(pts[3]);
	std::printf("%d %d %d %d %d %g %g %g %g %g %g %g %d %d %d\n", t[0].status, t[1].status, t[2].status, t[3].status, t[4].status, d4.x, d4.y, d4.z,
	            d8.x, t[8].A[0], t[8].A[1], d3.x, (int)k[0], (int)k[4], (int)k[3]);
	return 0;
}
"""


def test_shell_links_and_reports_failure(tmp_path, capi):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no host compiler")
    d = os.path.join(ROOT, "3dsift_amd")
    if not os.path.exists(os.path.join(d, "libsift3d.so")):
        subprocess.check_call(["make", "-C", os.path.join(d, "host")])
    src = tmp_path / "validate.cpp"
    src.write_text(SHELL)
    r = subprocess.run([cxx, "-std=c++14", "-Wall", "-Werror", "-o", str(tmp_path / "validate"), str(src), "-I", os.path.join(d, "host", "Include"),
                        "-L" + d, "-lsift3d", "-lsift3d_hip", "-Wl,-rpath," + d], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(tmp_path / "validate")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    first, second = [line.split() for line in r.stdout.strip().splitlines()]
    # POI 4 is flagged with status 0 and POI 3 has status 3: both restart from the median (7, -1, 0.5); POI 8 is kept: L = I + G of its own
    # result (ux = 0.01), displacement u = 0.01 x = 0.08 at x = 8
    assert second[:5] == ["0", "1", "1", "0", "0"] and [float(v) for v in second[5:8]] == [7.0, -1.0, 0.5]
    assert abs(float(second[8]) - 0.08) < 1e-6 and float(second[9]) == 1.01 and float(second[10]) == 0.0 and float(second[11]) == 7.0
    assert second[12:] == ["1", "0", "0"]
    assert first[:6] == ["27"] * 6
    if capi.device_count() > 0:   # u = 0.01 x with POI 13 off by 3 voxels: flagged with and without gradients, restarted from the median
        assert first[6:13] == ["0", "1", "1", "-1", "1", "0", "0"], r.stdout
        assert abs(float(first[13]) - 0.04) < 1e-9 and float(first[14]) == 1.01 and abs(float(first[15]) - 0.02) < 1e-9 and float(first[16]) > 0
        return
    assert first[6:] == ["-1", "0", "0", "-1", "0", "0", "1", "0", "0", "0", "0"], r.stdout
    assert "ValidateDisplacements" in r.stderr and "no CPU fallback" in r.stderr
