"""CPU tests of the RANSAC affine fits' boundary (sift3d_fit_affine / sift3d_fit_affine_local, include/sift3d_hip.h): the header compiles
as C and C++ with its layout guards, the library exports the entry points, the defaults need no GPU, bad arguments are refused before
any device call, the CPU restatement (tests/ransac_ref.py) recovers a known affine, and the C++ shell's cRegistration.h links.  The
inputs of tests/test_gpu_ransac_edges.py (tests/ransac_cases.py) have the properties they were built for, and every assertion of that
module holds with the restatement in the kernel's place."""
import ctypes as C
import importlib
import os
import shutil
import subprocess

import numpy as np
import pytest

import ransac_cases as cs
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


# ---- the inputs of tests/test_gpu_ransac_edges.py, and its assertions on the restatement -------------------------------------------

REF = cs.RefEngine


def test_nan_helper():
    a = np.array([1.0, np.nan, -0.0, np.inf])
    b = a.copy()
    b[1] = -np.nan
    assert cs.same_bits_or_nan(a, b) and cs.same_bits_or_nan(a, np.copysign(a, a))
    assert not cs.same_bits_or_nan(a, np.array([1.0, np.nan, 0.0, np.inf]))  # the sign of a zero is part of the contract
    assert not cs.same_bits_or_nan(a, np.array([1.0, 2.0, -0.0, np.inf])) and not cs.same_bits_or_nan(a, np.array([np.nan, np.nan, -0.0, np.inf]))
    assert not cs.same_bits_or_nan(a, np.nextafter(a, 2.0)) and not cs.same_bits_or_nan(a, a[:3])


def test_every_k_inputs():
    pairs, pts = cs.every_k_inputs()
    assert len(pairs) == 700 and len(pairs) % 64 and len(pts) == 24
    assert cs.EVERY_K == list(range(4, 65))
    on_site = (pts % 8 == 0).all(1) & (pts >= 0).all(1) & (pts <= 64).all(1)
    assert on_site.sum() == 12
    ties = 0
    for q in pts[on_site]:
        d2 = ref.distances(pairs, q)
        ties += len(d2) - len(np.unique(d2))
    assert ties > 1000  # equal distances, resolved by index
    c = np.array([len(ref.neighbours(pairs, q, 700, cs.EVERY_K_RADIUS)) for q in pts])
    for k in (4, 33, 64):
        assert (c < 4).any() and (c >= k).any() and (c == 4).any() and ((c >= 4) & (c < k)).any() == (k > 4), (k, c)


@pytest.mark.parametrize("k", cs.EVERY_K)
def test_every_k_restated(k):
    near, far = cs.check_every_k(REF, k)
    assert (far["status"] == 1).any() and (far["neighbours"] < 0).any()


@pytest.mark.parametrize("order", cs.HOSTILE_ORDERS)
@pytest.mark.parametrize("n", cs.HOSTILE_N)
def test_hostile_orders(n, order):
    assert sorted(cs.HOSTILE_N) == sorted([64 * j + d for j in (1, 2, 3) for d in (-1, 0, 1)] + [1000]) and cs.HOSTILE_K == [4, 5, 63, 64]
    pairs = cs.hostile_pairs(n, order)
    d2 = ref.distances(pairs, cs.HOSTILE_Q)
    assert d2.dtype == np.float32 and len(d2) == n and np.isfinite(d2).all()
    if order == "ascending":
        assert (np.diff(d2) > 0).all()
    elif order == "descending":
        assert (np.diff(d2) < 0).all()
    else:
        blocks = [d2[b:b + 64] for b in range(0, n, 64)]
        assert all((np.diff(b) < 0).all() for b in blocks)
        assert all(blocks[i].max() < blocks[i + 1].min() for i in range(len(blocks) - 1))
    cs.check_hostile(REF, n, order)


@pytest.mark.parametrize("n", cs.SPHERE_N)
def test_equal_distance_inputs(n):
    assert cs.SPHERE_N == [48 * 3, 200]
    pairs = cs.sphere_pairs(n)
    d2 = ref.distances(pairs, cs.SPHERE_Q)
    assert len(pairs) == n and (d2.view(np.uint32) == np.float32(441.0).view(np.uint32)).all()
    assert len(np.unique(pairs[:, :3], axis=0)) == 144
    cs.check_sphere(REF, n)


@pytest.mark.parametrize("k", cs.HOSTILE_K)
def test_rim_inputs(k):
    r2 = ref.radius2(cs.RIM_RADIUS)
    for c in (k - 1, k, k + 1):
        pairs, slot = cs.rim_pairs(c)
        d2 = ref.distances(pairs, cs.RIM_Q)
        inside = np.zeros(len(pairs), bool)
        inside[slot] = True
        assert inside.sum() == c and (d2[inside] <= r2).all() and (d2[inside] == r2).sum() == 1
        assert (~inside).sum() == cs.RIM_OUTSIDE >= 300 and (d2[~inside] == np.nextafter(r2, np.float32(np.inf))).all()
        assert inside[:len(pairs) // 2].any() and inside[len(pairs) // 2:].any() and len(np.unique(pairs[:, :3], axis=0)) > 200
    cs.check_rim(REF, k)


def test_status_inputs():
    pairs, pts, kinds = cs.status_inputs()
    assert len(pts) == cs.STATUS_M == 4 * 24 + 1 and kinds[:4].tolist() == [1, 2, 3, 0]
    orders = {tuple(kinds[g:g + 4]) for g in range(0, 96, 4)}
    assert all(sorted(o) == [0, 1, 2, 3] for o in orders) and len(orders) >= 8
    c = np.array([len(ref.neighbours(pairs, q, cs.STATUS_K, cs.STATUS_RADIUS)) for q in pts])
    assert set(c[kinds == 1]) == {0, 3} and (c[kinds == 3] == 4).all() and (c[kinds == 2] == 8).all() and (c[kinds == 0] == 8).all()
    o = cs.STATUS_OPTS
    a, b, traces = cs.local_margins(pairs, pts, cs.STATUS_K, cs.STATUS_RADIUS, **o)
    assert cs.margins_ok(o["inlier_thresh"], a, b), (a, b)
    cs.check_statuses(REF)


@pytest.mark.parametrize("n,H", cs.GLOBAL_TAILS)
def test_global_tails_restated(n, H):
    assert {x for x, _ in cs.GLOBAL_TAILS} == {255, 256, 257, 511, 513} and {x for _, x in cs.GLOBAL_TAILS} == {1, 2, 255, 257, 300}
    cs.check_global_tail(REF, n, H)


def test_local_tails_restated():
    assert cs.LOCAL_TAIL_H == [1, 63, 65, 100, 129] and cs.LOCAL_TAIL_M == [2, 3, 5] and len(cs.local_tail_inputs()[1]) == 40
    for H in cs.LOCAL_TAIL_H:
        cs.check_local_tail_h(REF, H)
    for m in cs.LOCAL_TAIL_M:
        cs.check_local_tail_m(REF, m)


REFIT_SEEN = set()


@pytest.mark.parametrize("tau", cs.REFIT_TAU)
@pytest.mark.parametrize("k", cs.REFIT_K)
def test_refit_inputs_have_margin(k, tau):
    assert cs.REFIT_K == [8, 32, 64] and cs.REFIT_TAU == [0.0, 0.5, 3.0] and cs.REFIT_ROUNDS == [0, 1, 2, 3, 4]
    worst = [np.inf, np.inf]
    for refine in cs.REFIT_ROUNDS:
        pairs, pts, o = cs.refit_case(k, tau, refine)
        a, b, traces = cs.local_margins(pairs, pts, k, 0.0, **o)
        worst = [min(worst[0], a), min(worst[1], b)]
        assert cs.margins_ok(tau, a, b), (refine, a, b)
        for w, tr in zip(cs.want_local(pairs, pts, k, 0.0, **o), traces):
            if w["status"] == 3:
                REFIT_SEEN.add("status 3")
            if w["status"] == 0 and len(tr) <= refine and (tr[-1]["d2"] <= ref.tau2_of(tau)).sum() < 4:
                REFIT_SEEN.add("stops early")
            if w["status"] == 0 and refine > 0 and len(tr) == refine + 1:
                REFIT_SEEN.add("last round")
            if tau == 0:  # the refit never starts: the only scoring is that of hyp, bit for bit
                assert len(tr) == (w["status"] == 0) and w["best_count"] < 4 and w["status"] in (0, 2)
    print(f"k={k} tau={tau}: smallest d2 margin {worst[0]:.3e}, smallest det margin {worst[1]:.3e}")
    cs.check_refit(REF, k, tau)


def test_refit_paths_all_seen():
    """after the cases above: each path of the refit occurs in at least one of them"""
    if len(REFIT_SEEN) < 3:  # run alone: look through the cases here
        for k in cs.REFIT_K:
            for tau in cs.REFIT_TAU:
                test_refit_inputs_have_margin(k, tau)
    assert REFIT_SEEN == {"status 3", "stops early", "last round"}
    pairs, pts = cs.refit_inputs()
    outl = np.linalg.norm(pairs[:, 3:].astype(np.float64) - (pairs[:, :3].astype(np.float64) @ _true_L().T + [7.5, -3.25, 11.0]), axis=1) > 3
    assert 0.25 < outl.mean() < 0.35


def _true_L():
    th = 0.2
    R = np.array([[np.cos(th), -np.sin(th), 0], [np.sin(th), np.cos(th), 0], [0, 0, 1]])
    return R @ np.diag([1.05, 0.97, 1.02])


@pytest.mark.parametrize("name", cs.VALUE_CLASSES)
def test_value_class_reaches_its_path(name):
    pairs, pts, radius, o = cs.value_inputs(name)
    base = cs.value_inputs("nan_query")[0]
    assert len(pts) == 30 and len(base) == 600
    ho = dict(iterations=o["iterations"], seed=o["seed"], min_det=o.get("min_det", 1.0), inlier_thresh=o.get("inlier_thresh", 3.0))
    idx, A, counts = ref.hypotheses(pairs, **ho)
    want = cs.want_local(pairs, pts, cs.VALUE_K, radius, **o)
    nb = np.array([w["neighbours"] for w in want])
    d2 = np.array([ref.distances(pairs, q) for q in pts])
    if name in ("nan_ref", "nan_tar", "inf_ref", "inf_tar"):
        cols = slice(0, 3) if name.endswith("ref") else slice(3, 6)
        bad = np.nonzero(~np.isfinite(pairs[:, cols]).all(1))[0]
        assert len(bad) == 30 and (~np.isfinite(pairs)).sum() == 30  # 5 % of the pairs, one coordinate each
        assert (np.isnan(pairs).sum() == 30) == name.startswith("nan")
        hit = np.isin(idx, bad).any(1)
        assert hit.any()
        if name == "nan_ref":  # never a neighbour; a hypothesis that samples one is degenerate
            assert (counts[hit] == -1).all() and not np.isin(nb, bad).any() and np.isnan(d2[:, bad]).all()
        if name == "nan_tar":  # a neighbour; a hypothesis that samples one is not degenerate (where its positions are not) and counts nothing
            clean = ref.hypotheses(base, **ho)[2]
            assert np.array_equal(counts < 0, clean < 0) and (counts[hit & (clean >= 0)] == 0).all() and (hit & (clean >= 0)).any()
            assert np.isin(nb, bad).any()
            assert any(np.isnan(w["hyp"]).any() or np.isin(w["neighbours"], bad).any() for w in want)
        if name == "inf_ref":  # at distance +inf: behind 570 finite pairs, never listed; a sample with one has det NaN or inf
            assert np.isinf(d2[:, bad]).all() and not np.isin(nb, bad).any() and (counts[hit] <= 0).all()
        if name == "inf_tar":
            assert np.isin(nb, bad).any() and (counts[hit] <= 0).all() and (counts[hit] == 0).any()
    if name in ("huge_ref", "huge_ref_radius"):
        far = np.nonzero(np.abs(pairs[:, :3]).max(1) > 1e19)[0]
        assert len(pairs) == 18 and len(far) == 8 and np.isinf(d2[:, far]).all() and np.isfinite(np.delete(d2, far, 1)).all()
        assert np.isin(nb, far).any() == (name == "huge_ref")  # +inf-distance neighbours are listed without a radius only
        assert (np.delete(d2, far, 1) <= ref.radius2(1000.0)).all()
    if name == "nan_query":
        assert np.isnan(pts).any(1).sum() == 10 and np.isnan(d2[::3]).all() and all(w["status"] == 1 for w in want[::3])
    if name == "huge_query":
        assert (d2[::3] == np.inf).all() and np.isfinite(d2[1::3]).all()
    if name == "offset_2p20":
        assert (pairs >= 2.0 ** 20).mean() > 0.99 and pairs.min() > 2.0 ** 20 - 64  # fp32 spacing 1/8 (1/16 just below 2^20)
        assert np.array_equal(pairs * 16, np.round(pairs * 16)) and np.array_equal(pts * 8, np.round(pts * 8))
        assert counts.max() > 300
    if name == "tiny_extent":
        assert np.abs(pairs).max() < 0.02 and o["min_det"] == 0.0
        assert (ref.hypotheses(pairs, **dict(ho, min_det=1.0))[2] == -1).all() and counts.max() > 300  # only min_det = 0 accepts these
    if name == "duplicates":
        u, inv, cnt = np.unique(pairs, axis=0, return_inverse=True, return_counts=True)
        assert len(pairs) - len(u) == 120 and o["min_det"] == 0.0  # 20 % exact copies
        assert ((counts >= 0) & ~np.isfinite(A).all(1)).any()  # an accepted hypothesis with det = 0
        assert all(not np.isfinite(w["hyp"]).all() and w["status"] == 0 for w in want[:3])  # and one that is the best
    if name == "all_nan":
        assert np.isnan(pairs).all() and (counts == -1).all()
    cs.check_values(REF, name)


def test_independence_inputs():
    pairs, pts, other = cs.indep_inputs()
    assert len(pairs) == 5000 and len(pts) == len(other) == cs.INDEP_M == 203 and cs.INDEP_K == 24
    kept = np.arange(203) % 4 == 1
    assert np.array_equal(pts[kept], other[kept]) and not (pts[~kept] == other[~kept]).all(1).any()
    assert np.isnan(other).any(1).sum() > 30 and (np.abs(other) > 1e5).any(1).sum() > 30
    d = np.array([np.sort(ref.distances(pairs, q))[cs.INDEP_K - 1] for q in other])
    assert (d < 1.0).sum() > 30  # inside a dense cluster: 24 pairs within one voxel
    # every group of four has replaced points next to the kept one, and the kinds differ from group to group
    o = dict(iterations=64, seed=9, refine=1, inlier_thresh=3.0, min_det=1.0)
    a, b, _ = cs.local_margins(pairs, pts, cs.INDEP_K, 0.0, which=np.arange(1, 203, 4)[::2], **o)
    assert cs.margins_ok(3.0, a, b), (a, b)
    a, b, _ = cs.local_margins(pairs, other, cs.INDEP_K, 0.0, which=np.arange(0, 203, 5), **o)
    assert cs.margins_ok(3.0, a, b), (a, b)
    cs.check_independence(REF)
