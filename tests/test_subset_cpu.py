"""CPU tests of the subset screening's boundary (sift3d_subset_quality, sift3d_subset_group_by_radius, include/sift3d_hip.h): the
header compiles as C and C++ with its layout guards, the library exports the entry points, the layouts agree with capi, the defaults
need no GPU, bad options and arguments are refused before any device call, the grouping is exact, and the restatement
(tests/subset_ref.py) holds the contract's consequences: c(rho) does not decrease, its sums are IC-GN's H block, integer-valued
inputs give the exact sums, and both of its forms agree.  It also checks what the GPU tests rely on: every threshold and fraction
they use has the margin, icgn_ref converges on the chain's status-0 POIs, and the bars are measured here and printed.

Measured (this file prints them): e = 5.1e-13 (the largest |plain fp64 sum - exact sum| / sum |term| over the parity inputs at
radius 16, the linear order and 16 seeded permutations; the restatement adds sequentially and the layered volumes, whose terms
repeat, set the figure), so the GPU bar is max(4 e, 1e-13) = 2.0e-12 of sum |term|; the Jacobi solve differs from
numpy.linalg.eigvalsh by at most 3.5e-16 of the trace."""
import ctypes as C
import fractions
import importlib
import os
import shutil
import subprocess

import numpy as np
import pytest

import icgn_ref
import subset_cases as cs
import subset_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["sift3d_default_subset_options", "sift3d_subset_quality", "sift3d_subset_group_by_radius"]
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
SIFT3D_STATIC_ASSERT(sizeof(sift3d_subset_options) == 48, "options");
SIFT3D_STATIC_ASSERT(sizeof(sift3d_subset_result) == 104, "result");
SIFT3D_STATIC_ASSERT(offsetof(sift3d_subset_options, threshold) == 16 && offsetof(sift3d_subset_options, level) == 24 &&
                     offsetof(sift3d_subset_options, fraction_min) == 32 && offsetof(sift3d_subset_options, reserved) == 40, "option offsets");
SIFT3D_STATIC_ASSERT(offsetof(sift3d_subset_result, G) == 16 && offsetof(sift3d_subset_result, eig) == 64 &&
                     offsetof(sift3d_subset_result, radius) == 88 && offsetof(sift3d_subset_result, material) == 100, "result offsets");
int probe(const float *r, const int *pts, int m, sift3d_subset_result *out, int *order, int *offsets) {
	sift3d_subset_options o;
	double s;
	int count;
	sift3d_default_subset_options(&o);
	o.r_min = 4;
	return sift3d_subset_quality(r, 64, 64, 64, pts, m, &o, 0, 0, out, &s) + sift3d_subset_group_by_radius(out, m, 4, 16, order, offsets, &count);
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


def test_layouts_and_defaults_without_gpu(capi):
    o = capi.SubsetOptions()
    C.memset(C.byref(o), 0x5A, C.sizeof(o))
    capi.lib().sift3d_default_subset_options(C.byref(o))
    assert (o.r_min, o.r_max, o.criterion, o.reserved0) == (8, 16, 0, 0)
    assert (o.threshold, o.level, o.fraction_min) == (0.0, -np.inf, 0.0) and list(o.reserved) == [0, 0]
    assert capi.default_subset_options() == {"r_min": 8, "r_max": 16, "criterion": 0, "threshold": 0.0, "level": -np.inf, "fraction_min": 0.0}
    assert capi.default_subset_options() == ref.DEFAULTS
    assert C.sizeof(capi.SubsetOptions) == 48
    S = capi.SubsetOptions
    assert [getattr(S, k).offset for k in ("r_min", "r_max", "criterion", "reserved0", "threshold", "level", "fraction_min", "reserved")] == \
        [0, 4, 8, 12, 16, 24, 32, 40]
    f = capi.SUBSET_DTYPE.fields
    assert capi.SUBSET_DTYPE.itemsize == 104
    assert [f[k][1] for k in ("mean", "dR", "G", "eig", "radius", "status", "feasible", "material")] == [0, 8, 16, 64, 88, 92, 96, 100]
    assert tuple(capi.SUBSET_FIELDS) == ref.FIELDS


def _opts(capi, **kw):
    o = capi.SubsetOptions()
    capi.lib().sift3d_default_subset_options(C.byref(o))
    for k, v in kw.items():
        if k == "reserved":
            o.reserved[v] = 1
        else:
            setattr(o, k, v)
    return o


BAD_OPTS = [dict(r_min=1), dict(r_min=33, r_max=33), dict(r_min=9, r_max=8), dict(r_max=33), dict(criterion=-1), dict(criterion=2),
            dict(reserved0=1), dict(reserved=0), dict(reserved=1), dict(threshold=-1e-300), dict(threshold=np.inf), dict(threshold=np.nan),
            dict(level=np.nan), dict(fraction_min=-1e-9), dict(fraction_min=1.0000001), dict(fraction_min=np.nan)]
GOOD_OPTS = [dict(r_min=2, r_max=2), dict(r_min=32, r_max=32), dict(level=np.inf), dict(level=-np.inf), dict(fraction_min=1.0), dict(threshold=1e300)]


def _call(capi, o=None, ref_=True, pts=True, out=True, m=2, dims=(64, 64, 64), device=0):
    v = np.zeros((4, 4, 4), np.float32)
    q = np.zeros((2, 3), np.int32)
    res = np.zeros(2, capi.SUBSET_DTYPE)
    P = lambda a, on: a.ctypes.data_as(C.c_void_p) if on else None  # noqa: E731
    return capi.lib().sift3d_subset_quality(P(v, ref_), dims[0], dims[1], dims[2], P(q, pts), m, C.byref(o) if o is not None else None, 0,
                                            device, P(res, out), None)


@pytest.mark.parametrize("bad", BAD_OPTS, ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))
def test_bad_options_refused(capi, bad):
    assert _call(capi, _opts(capi, **bad)) == ERR_ARG
    assert b"bad argument" in capi.lib().sift3d_last_error()


@pytest.mark.parametrize("good", GOOD_OPTS, ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))
def test_good_options_pass_the_argument_check(capi, good):
    # m = 0 and a device index no machine has: what comes back is not the argument check's answer
    rc = _call(capi, _opts(capi, **good), m=0, device=10 ** 6)
    assert rc != 0 and b"sift3d_subset_quality: bad argument" not in capi.lib().sift3d_last_error()


def test_bad_arguments_refused(capi):
    assert _call(capi, m=-1) == ERR_ARG
    for k in range(3):
        dims = [64] * 3
        dims[k] = 0
        assert _call(capi, dims=tuple(dims)) == ERR_ARG, k
    assert _call(capi, ref_=False) == ERR_ARG
    assert _call(capi, out=False) == ERR_ARG
    assert _call(capi, pts=False, m=2) == ERR_ARG
    assert b"sift3d_subset_quality: bad argument" in capi.lib().sift3d_last_error()
    # the argument check comes first: a bad option with a bad device index is a bad argument
    assert _call(capi, _opts(capi, r_min=1), device=10 ** 6) == ERR_ARG


# ---- sift3d_subset_group_by_radius --------------------------------------------------------------------------------------------------

def _group(capi, radius, status, r_min, r_max, order=True, offsets=True, count=True, res=True, m=None):
    n = len(radius)
    rec = np.zeros(max(n, 1), capi.SUBSET_DTYPE)
    rec["radius"][:n], rec["status"][:n] = radius, status
    od = np.full(max(n, 1), -7, np.int32)
    of = np.full(40, -7, np.int32)
    cnt = C.c_int(-7)
    P = lambda a, on: a.ctypes.data_as(C.c_void_p) if on else None  # noqa: E731
    rc = capi.lib().sift3d_subset_group_by_radius(P(rec, res), n if m is None else m, r_min, r_max, P(od, order), P(of, offsets),
                                                  C.byref(cnt) if count else None)
    return rc, od, of, cnt.value


def test_group_by_radius(capi):
    rng = np.random.default_rng(3)
    m = 500
    radius = rng.choice([4, 5, 7, 8, 16], m).astype(np.int32)  # 6 and 9 .. 15: empty groups
    status = rng.choice([0, 0, 0, 1, 2, 3], m).astype(np.int32)
    radius[status == 2] = 0       # what the kernel reports; skipped, not refused
    radius[status == 1] = 99      # a non-zero status is skipped whatever its radius
    rc, od, of, cnt = _group(capi, radius, status, 4, 16)
    assert rc == 0
    want = ref.group_by_radius(radius, status, 4, 16)
    assert cnt == (status == 0).sum() == sum(len(i) for _, i in want)
    assert of[0] == 0 and of[13] == cnt and (np.diff(of[:14]) >= 0).all() and (of[14:] == -7).all()
    for r in range(4, 17):
        idx = od[of[r - 4]:of[r - 3]]
        assert np.array_equal(idx, np.flatnonzero((status == 0) & (radius == r))), r  # ascending index: a stable order
    assert (od[cnt:] == -7).all()
    got = capi.subset_groups({"radius": radius, "status": status}, 4, 16)
    assert [r for r, _ in got] == [r for r, _ in want] == [4, 5, 7, 8, 16]
    assert all(np.array_equal(a[1], b[1]) for a, b in zip(got, want))
    # a status-0 radius outside the range is refused, on either side
    for bad in (3, 17):
        r2 = radius.copy()
        r2[np.flatnonzero(status == 0)[5]] = bad
        assert _group(capi, r2, status, 4, 16)[0] == ERR_ARG
        assert b"bad argument" in capi.lib().sift3d_last_error()
    # bad ranges, NULL pointers, m < 0
    for r_min, r_max in ((1, 8), (8, 7), (4, 33), (33, 33)):
        assert _group(capi, radius, status, r_min, r_max)[0] == ERR_ARG
    for kw in (dict(order=False), dict(offsets=False), dict(count=False), dict(res=False)):
        assert _group(capi, radius, status, 4, 16, **kw)[0] == ERR_ARG
    assert _group(capi, radius, status, 4, 16, m=-1)[0] == ERR_ARG
    # m = 0: nothing listed, the offsets all zero; NULL tables pass
    rc, od, of, cnt = _group(capi, [], [], 2, 32)
    assert rc == 0 and cnt == 0 and (of[:32] == 0).all() and (of[32:] == -7).all()
    assert _group(capi, [], [], 2, 32, order=False, res=False)[0] == 0
    assert capi.subset_groups({"radius": [], "status": []}, 2, 32) == []
    # one group, one record
    rc, od, of, cnt = _group(capi, [2], [0], 2, 2)
    assert rc == 0 and cnt == 1 and list(of[:2]) == [0, 1] and od[0] == 0


# ---- the restatement -------------------------------------------------------------------------------------------------------------------

def test_criterion_does_not_decrease():
    for name in cs.FLOAT + cs.INTEGER:
        for q, c0, c1 in zip(cs.pois(), cs.all_criteria(name, 0), cs.all_criteria(name, 1)):
            # criterion 0: sums of squares grow term by term, and rounding is monotone -- exactly non-decreasing
            assert (np.diff(c0) >= 0).all(), (name, q)
            # criterion 1: G(rho + 1) = G(rho) + a positive semidefinite shell, so eig[2] cannot decrease beyond the solve's rounding
            tr = np.array([sum(ref.direct(cs.volumes()[name], q, cs.R_MIN + i)["G"][:3]) for i in (0, len(c1) - 1)]).max() if len(c1) else 0
            assert (np.diff(c1) >= -1e-14 * tr).all(), (name, q)


@pytest.mark.parametrize("name", ["scene", "half_flat", "uint16"])
def test_sums_are_the_icgn_hessian_block(name, monkeypatch):
    """G, dR and mean at radius r are H[0][0], H[4][4], H[8][8], H[0][4], H[0][8], H[4][8], dR and Rm of icgn_ref at that r"""
    R = cs.volumes()[name]
    seen = {}
    real = icgn_ref.positive_definite

    def spy(H):
        seen["H"] = np.array(H)
        return real(H)

    monkeypatch.setattr(icgn_ref, "positive_definite", spy)
    for q, r in (((24, 23, 22), 4), ((24, 23, 22), 9), ((30, 17, 26), 16)):
        seen.clear()
        icgn_ref.refine(R, R, q, subset_radius=r, max_iterations=1)
        if "H" not in seen:   # a flat subset: icgn_ref stops at dR = 0 before it forms H
            assert ref.direct(R, q, r)["dR"] == 0
            continue
        H = seen["H"]
        mine = ref.direct(R, q, r)
        want = np.array([H[0, 0], H[4, 4], H[8, 8], H[0, 4], H[0, 8], H[4, 8]])
        scale = ref.abs_sums(R, q, r)[2:8]
        assert (np.abs(mine["G"] - want) <= 1e-12 * scale).all(), (name, q, r)
        # icgn_ref's own Rm and dR, restated: the mean, then the two-pass deviation
        t = ref.terms(R, q, r)
        Rs = t["v"].astype(np.float64)
        Rm = Rs.mean()
        dR = np.sqrt(np.sum((Rs - Rm) ** 2))
        assert abs(mine["mean"] - Rm) <= 1e-12 * np.abs(Rs).max()
        assert abs(mine["dR"] - dR) <= 1e-9 * dR  # Q - S^2 / N against two passes: the cancellation costs digits, not the contract


def test_integer_inputs_are_exact():
    """on integer-valued volumes the sums equal integer / rational arithmetic, in both forms and bit for bit"""
    for name in cs.INTEGER:
        R = cs.volumes()[name]
        Ri = R.astype(np.int64)
        for q, rho in (((24, 23, 22), 4), ((17, 28, 26), 11), ((30, 17, 17), 16)):
            x, y, z = q
            s = lambda c, o=0: slice(c - rho + o, c + rho + 1 + o)  # noqa: E731
            a = (Ri[s(z), s(y), s(x)] - Ri[z, y, x]).ravel()
            g2 = [(Ri[s(z), s(y), s(x, 1)] - Ri[s(z), s(y), s(x, -1)]).ravel(), (Ri[s(z), s(y, 1), s(x)] - Ri[s(z), s(y, -1), s(x)]).ravel(),
                  (Ri[s(z, 1), s(y), s(x)] - Ri[s(z, -1), s(y), s(x)]).ravel()]  # twice the gradient
            S, Q = int(a.sum()), int((a * a).sum())
            G = [fractions.Fraction(int((g2[i] * g2[j]).sum()), 4) for i, j in ref.PAIRS]
            N = (2 * rho + 1) ** 3
            assert Q < 2 ** 53 and all(abs(v) < 2 ** 53 for v in G)
            d = ref.direct(R, q, rho)
            p = ref.profile(R, q, cs.R_MIN, rho)[-1]
            for w in (d, p):
                assert [fractions.Fraction(float(v)) for v in w["G"]] == G, (name, q, rho)
                assert w["mean"] == float(Ri[z, y, x]) + float(S) / float(N)
                assert w["dR"] == np.sqrt(max(float(Q) - float(S) * float(S) / float(N), 0.0))
            assert d["G"].tobytes() == p["G"].tobytes() and d["eig"].tobytes() == p["eig"].tobytes()
            assert (d["mean"], d["dR"], d["material"]) == (p["mean"], p["dR"], p["material"])


@pytest.fixture(scope="module")
def measured():
    """e over the parity inputs (the interior POIs at the largest radius of the plan) and the Jacobi solve's distance from eigvalsh"""
    e, Gs = 0.0, []
    for name in cs.FLOAT:
        R = cs.volumes()[name]
        for k, q in enumerate(cs.pois()[[0, 13, 26]]):
            e = max(e, ref.summation_error(R, q, cs.R_MAX, seed=k))
        w = cs.parity_reference(name, 0)
        Gs.append(w["G"][w["status"] != 2])
    ej = ref.jacobi_error(np.concatenate(Gs))
    print(f"e = {e:.3e}, GPU bar = {ref.bar_rel(e):.3e} x sum |term|; Jacobi vs eigvalsh = {ej:.3e} x trace")
    return e, ej


def test_bars_are_measured(measured):
    e, ej = measured
    assert 0 < e < 1e-12   # a plain fp64 sum of 33^3 terms: far below a part in 10^12 of sum |term|
    assert ej < 1e-14


def test_both_forms_agree_within_the_bar(measured):
    rel = ref.bar_rel(measured[0])
    for name in cs.FLOAT:
        R = cs.volumes()[name]
        for q in cs.pois()[[0, 13, 26]]:
            for rec in ref.profile(R, q, cs.R_MIN, cs.R_MAX)[::4]:
                d = ref.direct(R, q, rec["radius"])
                b = ref.field_bars(R, q, rec["radius"], rel, measured[1])
                assert (np.abs(d["G"] - rec["G"]) <= b["G"]).all()
                assert abs(d["mean"] - rec["mean"]) <= b["mean"] and abs(d["dR"] ** 2 - rec["dR"] ** 2) <= b["dR2"]
                assert np.abs(d["eig"] - rec["eig"]).max() <= b["eig"]
                assert d["material"] == rec["material"]


# ---- what the GPU tests rely on ------------------------------------------------------------------------------------------------------------

def test_thresholds_have_the_margin():
    for name in cs.FLOAT + cs.INTEGER:
        for criterion in (0, 1):
            assert cs.clear_of(cs.threshold(name, criterion), [v for c in cs.all_criteria(name, criterion) for v in c]), (name, criterion)
    for criterion in (0, 1):
        c = cs.centre_criteria(criterion)
        plan = cs.selection_plan(criterion)
        assert [rho for rho, _ in plan] == list(range(2, 33))
        for rho, t in plan:
            assert cs.clear_of(t, c), (criterion, rho)
            got, _ = ref.screen(cs.edge_volume(), cs.EDGE_CENTRE, r_min=2, r_max=32, criterion=criterion, threshold=t)
            assert (got["radius"], got["status"]) == (rho, 0)
    R, _, pts, _ = cs.chain_case()
    cc = [v for q in pts for v in ref.criteria(R, q, cs.CHAIN_R_MIN, cs.CHAIN_R_MAX, 0)[1]]
    assert cs.clear_of(cs.chain_threshold(), cc)
    N = float((2 * cs.MATERIAL_RADIUS + 1) ** 3)
    for level, m, below, above in cs.material_cases():
        for f in (below, above):
            assert 0 <= f <= 1 and abs(f - m / N) >= cs.MARGIN * max(f, m / N)
    levels = [c[0] for c in cs.material_cases()]
    assert levels[1] < levels[0] < levels[2] and cs.material_cases()[0][1] == cs.material_cases()[1][1] > cs.material_cases()[2][1]


def test_parity_cases_cover_the_statuses():
    w = cs.parity_reference("scene", 0)
    assert {0, 1, 2} <= set(w["status"].tolist()) and len(set(w["radius"][w["status"] == 0].tolist())) >= 2
    assert len(set(w["feasible"].tolist())) >= 6
    w = cs.parity_reference("half_flat", 0)
    assert len(set(w["radius"][w["status"] == 0].tolist())) >= 5
    for name in ("layered", "diagonal"):  # no texture along x (layered: nor y) / along z: the per-axis SSSIG is exactly 0
        w = cs.parity_reference(name, 0)
        assert (w["status"][w["status"] != 2] == 1).all() and (w["G"].min(axis=1) == 0).all()
    # texture along (1, 1, 0) and z only: every axis has gradient energy, G is singular
    w0, w1 = cs.parity_reference("diagonal_z", 0), cs.parity_reference("diagonal_z", 1)
    ok = w0["status"] != 2
    assert (w0["status"][ok] == 0).all() and (w1["status"][ok] == 1).all()
    assert (w1["eig"][ok, 2] <= 1e-12 * w1["eig"][ok, 0]).all()
    # the literal diagonal volume: threshold 0 accepts r_min under criterion 0; criterion 1 with a threshold refuses
    R = cs.volumes()["diagonal"]
    a = ref.quality(R, cs.pois(), r_min=cs.R_MIN, r_max=cs.R_MAX, criterion=0, threshold=0.0)
    assert (a["status"][ok] == 0).all() and (a["radius"][ok] == cs.R_MIN).all()
    assert (cs.parity_reference("diagonal", 1)["status"][ok] == 1).all()


def test_walk_order_is_a_walk():
    """block_order and shell_order list every voxel of the cube / the shell once"""
    for k in (1, 2, 3, 7, 32):
        s = cs.shell_order(k)
        assert len({tuple(v) for v in s.tolist()}) == len(s) == 24 * k * k + 2
        assert (np.abs(s).max(axis=1) == k).all()
    assert len({tuple(v) for v in cs.block_order(3).tolist()}) == 343
    tags = cs.seams(2, 32)
    assert "block2-last" in tags and "shell32-i256" in tags and "shell3-first" in tags and "shell3-i255" not in tags


def test_icgn_ref_converges_on_the_chain():
    """the chain test asserts convergence on the GPU: icgn_ref itself converges on every status-0 POI at its radius"""
    R, T, pts, u = cs.chain_case()
    w = cs.chain_reference()
    flat = pts[:, 0] + cs.CHAIN_R_MAX + 1 < CS_HALF
    assert flat.any() and (w["status"][flat] == 1).all() and (w["G"][flat] == 0).all()
    ok = np.flatnonzero(w["status"] == 0)
    assert 12 <= len(ok) and len(set(w["radius"][ok].tolist())) >= 3 and set(w["status"].tolist()) == {0, 1}
    err = 0.0
    for i in ok:
        o = icgn_ref.refine(R, T, pts[i], subset_radius=int(w["radius"][i]))
        assert o["status"] == 0, (pts[i], w["radius"][i], o["status"])
        err = max(err, float(np.abs(o["p"][[0, 4, 8]] - u[i]).max()))
    print(f"icgn_ref on the chain: largest displacement error {err:.4f} voxels")


CS_HALF = cs.CHAIN_SHAPE[2] // 2


SHELL = r"""
#include <cstdio>
#include <vector>
#include "cRegistration.h"
int main() {
	std::vector<float> v(32 * 32 * 32, 1.f);
	std::vector<CPUSIFT::Cvec> pts(2, CPUSIFT::Cvec(16, 16, 16));
	CPUSIFT::SubsetOptions so;
	so.r_min = 4;
	so.r_max = 9;
	so.threshold = 1.0;
	std::vector<CPUSIFT::SubsetQuality> s = CPUSIFT::SelectSubsets(v.data(), 32, 32, 32, pts, so);
	std::vector<CPUSIFT::SubsetQuality> q(5);
	const int radius[5] = {6, 4, 6, 9, 4}, status[5] = {0, 0, 0, 1, 0};
	for (int i = 0; i < 5; i++) { q[i].radius = radius[i]; q[i].status = status[i]; }
	std::vector<std::vector<int>> g;
	const bool ok = CPUSIFT::GroupSubsetsByRadius(q, 4, 9, g);
	std::printf("%zu %d %d %zu", s.size(), (int)ok, s[0].status == 1 || s[0].status == -1, g.size());
	for (size_t k = 0; k < g.size(); k++) {
		std::printf(" |");
		for (int i : g[k]) std::printf(" %d", i);
	}
	q[0].radius = 10;
	const bool bad = CPUSIFT::GroupSubsetsByRadius(q, 4, 9, g);  // a status-0 radius outside the range: refused, no groups
	std::printf(" ; %d %zu\n", (int)bad, g.size());
	return 0;
}
"""


def test_shell_select_subsets_links_and_groups(tmp_path):
    """the C++ shell's SelectSubsets links; its grouping helper needs no GPU and is run (a constant volume has status 1 on a GPU, the
    call fails with status -1 without one)"""
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no host compiler")
    d = os.path.join(ROOT, "3dsift_amd")
    subprocess.check_call(["make", "-C", os.path.join(d, "host")], stdout=subprocess.DEVNULL)
    src = tmp_path / "subset.cpp"
    src.write_text(SHELL)
    r = subprocess.run([cxx, "-std=c++14", "-Wall", "-Werror", "-o", str(tmp_path / "subset"), str(src), "-I", os.path.join(d, "host", "Include"),
                        "-L" + d, "-lsift3d", "-lsift3d_hip", "-Wl,-rpath," + d], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(tmp_path / "subset")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip() == "2 1 1 6 | 1 4 | | 0 2 | | | ; 0 0", (r.stdout, r.stderr)
