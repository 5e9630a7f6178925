"""CPU tests of the per-body calls (sift3d_fit_rigid_bodies, sift3d_labels_at_positions, sift3d_icgn_init_from_body_fits,
sift3d_icgn_labelled; tests/body_ref.py, tests/body_cases.py): the cases do what they claim on the restatement alone -- in the spheres
scene every body of at least 17 pairs is fitted to within 5e-3 of its planted rotation while ONE global fit keeps under half of the
pairs -- the two host helpers equal their restatements (bit for bit, on every rounding seam of a position), the labelled IC-GN's
scratch pieces leave the other layouts where they were, and the four entries refuse bad arguments before any device call."""
import ctypes as C
import importlib
import os
import subprocess

import numpy as np
import pytest

import body_cases as cases
import body_ref as ref
import rigid_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "3dsift_amd", "csrc")
NEW = ["sift3d_fit_rigid_bodies", "sift3d_labels_at_positions", "sift3d_icgn_init_from_body_fits", "sift3d_icgn_labelled"]
ERR_ARG, ERR_NO_DEVICE = 1, 2


@pytest.fixture(scope="module")
def capi():
    m = importlib.import_module("3dsift_amd.capi")
    if not os.path.exists(m.LIB_PATH):
        subprocess.check_call(["make", "-C", CSRC, "-j8"])
    return m


def P(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def test_exports(capi):
    L = capi.lib()
    for n in NEW:
        assert hasattr(L, n), n
        assert n in capi.SYMBOLS
    assert all(hasattr(capi, f) for f in ("fit_rigid_bodies", "labels_at_positions", "icgn_init_from_body_fits", "icgn_labelled"))


# ---- the cases' claims, on the restatement --------------------------------------------------------------------------------------------

def test_grains_bodies_are_recovered_and_one_global_fit_is_not():
    pairs, label, count = cases.grains()
    assert count == 12 and label.min() == 0 and set(np.unique(label)) == set(range(13))
    sizes = np.bincount(label, minlength=13)[1:]
    assert (sizes >= np.array(cases.BODY_PAIRS)).all() and sorted(sizes)[:2] == sorted(sizes[sizes < cases.MIN_PAIRS]) and (sizes < 17).sum() == 2
    fits, mask = cases.grains_reference()
    errs = []
    for L, f in enumerate(fits, 1):
        assert f["candidates"] == sizes[L - 1]
        if sizes[L - 1] >= cases.MIN_PAIRS:
            assert f["status"] == 0, (L, f["status"])
            errs.append(cases.rotation_error(f["A"], L))
    print("rotation errors", np.round(errs, 5))
    assert len(errs) == 10 and max(errs) <= cases.ROT_BOUND, errs
    assert not mask[label == 0].any()
    with np.errstate(all="ignore"):
        g = rigid_ref.fit(pairs, p=0, iterations=cases.H, inlier_thresh=cases.TAU)
    print("global fit keeps", g["inliers"], "of", len(pairs), "; the bodies keep", int(mask.sum()))
    assert g["inliers"] < len(pairs) / 2 and g["inliers"] < mask.sum()


def test_contact_pois_exist():
    q, u, body = cases.contact_pois()
    assert len(q) == 36 and (body > 0).all() and len(np.unique(body)) >= 6
    assert len(cases.contact_pois(3.0)[0]) == 0 and len(cases.contact_pois(4.0)[0]) == 0   # the scene holds none any closer


def test_seams_hold_what_they_claim():
    pairs, labels, count = cases.seams()
    assert count == len(cases.SEAM_SIZES)
    assert tuple(np.bincount(labels[(labels >= 1) & (labels <= count)], minlength=count + 1)[1:]) == cases.SEAM_SIZES
    assert {0, -1, count + 1} <= set(labels)
    first = np.flatnonzero(labels == count)[:50]
    assert (np.diff(first) > 1).any()   # shuffled: a body's pairs do not stand together
    fits, mask = ref.fit_bodies(pairs, labels, count, iterations=64)
    assert [f["status"] for f in fits[:2]] == [1, 1] and all(f["status"] == 0 for f in fits[2:])
    assert not mask[(labels < 1) | (labels > count)].any()


def test_labelled_scene_holds_what_it_claims():
    lab = cases.labelled_volume()
    assert set(np.unique(lab)) == {-4, 0, 2, 5, 900}
    for r in cases.LABELLED_R:
        q, init = cases.labelled_pois(r)
        at = ref.labels_at(lab, q)
        assert {-4, 0, 2, 5, 900} <= set(at), (r, at)
        assert [tuple(v) for v in q[list(cases.JUNCTION_ROWS)]] == [(cases.X_CUT, 25, cases.DIAG - 25), (cases.X_CUT - 1, 25, cases.DIAG - 26)]
        assert (at[-4:-2] == 0).all() and at[-5] == 5   # outside R: label 0; on R's boundary: the voxel's label


# ---- the host helpers --------------------------------------------------------------------------------------------------------------

def test_labels_at_positions_host_path_equals_the_restatement(capi):
    labels, pos = cases.position_battery()
    want = ref.labels_at_positions(labels, pos)
    got = capi.labels_at_positions(labels, pos)
    assert got.dtype == np.int32 and np.array_equal(got, want)
    assert (want == 0).sum() > 20 and (want > 0).sum() > 100
    # k + 0.5 exactly belongs to voxel k + 1, -0.5 to voxel 0, n - 0.5 lies outside
    nz, ny, nx = labels.shape
    edge = np.array([[-0.5, 0, 0], [nx - 0.5, 0, 0], [2.5, 0, 0], [np.nextafter(np.float32(-0.5), np.float32(-1)), 0, 0]], np.float32)
    assert list(capi.labels_at_positions(labels, edge)) == [labels[0, 0, 0], 0, labels[0, 0, 3], 0]
    # stride 6: the reference positions of pairs
    six = np.concatenate([pos, pos[::-1]], 1)
    assert np.array_equal(capi.labels_at_positions(labels, six), want)
    assert len(capi.labels_at_positions(labels, np.zeros((0, 3), np.float32))) == 0
    # a larger stride straight through the entry
    wide = np.zeros((len(pos), 9), np.float32)
    wide[:, :3] = pos
    out = np.zeros(len(pos), np.int32)
    assert capi.lib().sift3d_labels_at_positions(P(labels), nx, ny, nz, P(wide), 9, len(pos), P(out), 0, 0) == 0
    assert np.array_equal(out, want)


def test_init_from_body_fits_is_init_from_fits_on_the_gathered_records(capi):
    rng = np.random.default_rng(3)
    count, m = 6, 40
    fits = {"A": rng.normal(size=(count, 3, 4)), "status": np.array([0, 3, 0, 2, 1, 0])}
    q = rng.integers(-5, 200, (m, 3)).astype(np.int32)
    lab = rng.integers(1, count + 1, m).astype(np.int32)
    lab[:6] = [0, -1, count + 1, 2 ** 31 - 1, -2 ** 31, count]
    got = capi.icgn_init_from_body_fits(fits, lab, q)
    ok = (lab >= 1) & (lab <= count)
    want = capi.icgn_init_from_fits({"A": fits["A"][lab[ok] - 1], "status": fits["status"][lab[ok] - 1]}, q[ok])
    assert np.array_equal(got[ok].view(np.uint64), want.view(np.uint64))
    assert np.isnan(got[~ok]).all() and (~ok).sum() == 5
    failed = ok & (fits["status"][np.clip(lab, 1, count) - 1] != 0)
    assert failed.any() and np.isnan(got[failed]).all() and np.isfinite(got[ok & ~failed]).all()
    assert capi.icgn_init_from_body_fits(fits, lab[:0], q[:0]).shape == (0, 12)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------

def test_fit_rigid_bodies_refusals(capi):
    L = capi.lib()
    pairs, labels = np.ones((8, 6), np.float32), np.ones(8, np.int32)
    out, mask = np.zeros(4, capi.FIT_DTYPE), np.zeros(8, np.uint8)

    def call(pairs=pairs, n=8, labels=labels, count=4, model=0, o=None, out=out, mask=mask):
        return L.sift3d_fit_rigid_bodies(P(pairs), n, P(labels), count, model, o, 0, 0, P(out), P(mask), None)

    assert call(n=-1) == ERR_ARG
    assert b"sift3d_fit_rigid_bodies: bad argument" in L.sift3d_last_error()
    assert call(count=-1) == ERR_ARG and call(pairs=None) == ERR_ARG and call(labels=None) == ERR_ARG and call(out=None) == ERR_ARG
    assert call(model=2) == ERR_ARG and call(model=-1) == ERR_ARG
    for field, bad in (("iterations", -1), ("iterations", 65537), ("refine", 5), ("inlier_thresh", -1.0), ("inlier_thresh", float("nan")),
                       ("min_det", -1.0), ("min_det", float("inf"))):
        o = capi.RansacOptions()
        L.sift3d_default_ransac_options(C.byref(o))
        setattr(o, field, bad)
        assert call(o=C.byref(o)) == ERR_ARG, (field, bad)
    o = capi.RansacOptions()
    L.sift3d_default_ransac_options(C.byref(o))
    o.reserved[1] = 1
    assert call(o=C.byref(o)) == ERR_ARG
    # what is no error: the mask is optional; with no pair or no body nothing is read
    if capi.device_count() == 0:
        assert call() == ERR_NO_DEVICE and call(mask=None) == ERR_NO_DEVICE
        assert call(n=0, pairs=None, labels=None) == ERR_NO_DEVICE and call(count=0, out=None) == ERR_NO_DEVICE
        with pytest.raises(capi.Sift3dError):
            capi.fit_rigid_bodies(pairs, labels, 4)
    with pytest.raises(ValueError):
        capi.fit_rigid_bodies(pairs, labels[:5], 4)


def test_labels_at_positions_and_init_refusals(capi):
    L = capi.lib()
    lab, pos, out = np.ones((6, 7, 9), np.int32), np.zeros((4, 3), np.float32), np.zeros(4, np.int32)
    f = L.sift3d_labels_at_positions
    assert f(None, 9, 7, 6, P(pos), 3, 4, P(out), 0, 0) == ERR_ARG
    assert b"sift3d_labels_at_positions: bad argument" in L.sift3d_last_error()
    assert f(P(lab), 9, 0, 6, P(pos), 3, 4, P(out), 0, 0) == ERR_ARG
    assert f(P(lab), 1 << 11, 1 << 10, 1 << 10, P(pos), 3, 4, P(out), 0, 0) == ERR_ARG
    assert f(P(lab), 9, 7, 6, None, 3, 4, P(out), 0, 0) == ERR_ARG and f(P(lab), 9, 7, 6, P(pos), 3, 4, None, 0, 0) == ERR_ARG
    assert f(P(lab), 9, 7, 6, P(pos), 2, 4, P(out), 0, 0) == ERR_ARG and f(P(lab), 9, 7, 6, P(pos), 3, -1, P(out), 0, 0) == ERR_ARG
    assert f(P(lab), 9, 7, 6, None, 3, 0, None, 0, 0) == 0
    if capi.device_count() == 0:
        assert f(P(lab), 9, 7, 6, P(pos), 3, 4, P(out), 1, 0) == ERR_NO_DEVICE
    g = L.sift3d_icgn_init_from_body_fits
    fits, q, l4, init = np.zeros(2, capi.FIT_DTYPE), np.zeros((4, 3), np.int32), np.ones(4, np.int32), np.zeros((4, 12))
    assert g(None, 2, P(l4), P(q), 4, P(init)) == ERR_ARG
    assert b"sift3d_icgn_init_from_body_fits: bad argument" in L.sift3d_last_error()
    assert g(P(fits), -1, P(l4), P(q), 4, P(init)) == ERR_ARG and g(P(fits), 2, P(l4), P(q), -1, P(init)) == ERR_ARG
    assert g(P(fits), 2, None, P(q), 4, P(init)) == ERR_ARG and g(P(fits), 2, P(l4), None, 4, P(init)) == ERR_ARG
    assert g(P(fits), 2, P(l4), P(q), 4, None) == ERR_ARG
    assert g(None, 0, P(l4), P(q), 4, P(init)) == 0 and np.isnan(init).all()   # no body: every row is NaN
    assert g(None, 0, None, None, 0, None) == 0


def test_icgn_labelled_refusals(capi):
    L = capi.lib()
    R, T = np.zeros((12, 12, 12), np.float32), np.zeros((12, 12, 12), np.float32)
    lab, q, out = np.ones((12, 12, 12), np.int32), np.full((2, 3), 6, np.int32), np.zeros(2, capi.ICGN_DTYPE)
    act, pl = np.zeros(2, np.int32), np.zeros(2, np.int32)
    o = capi.IcgnOptions()
    L.sift3d_default_icgn_options(C.byref(o))
    o.subset_radius = 3

    def call(R=R, rdims=(12, 12, 12), T=T, lab=lab, q=q, m=2, o=C.byref(o), mf=0.0, coef=0, out=out, act=act, pl=pl):
        return L.sift3d_icgn_labelled(P(R), *rdims, P(T), 12, 12, 12, P(lab), P(q), m, None, o, mf, coef, 0, 0, P(out), P(act), P(pl), None)

    assert call(lab=None) == ERR_ARG
    assert b"sift3d_icgn_labelled: bad argument" in L.sift3d_last_error()
    assert call(lab=None, m=0) == ERR_ARG
    assert call(R=None) == ERR_ARG and call(T=None) == ERR_ARG and call(q=None) == ERR_ARG and call(out=None) == ERR_ARG and call(m=-1) == ERR_ARG
    for mf in (-0.1, 1.5, float("nan")):
        assert call(mf=mf) == ERR_ARG
    assert call(coef=1) == ERR_ARG        # interpolation 0: no coefficients
    assert call(rdims=(1 << 11, 1 << 10, 1 << 10)) == ERR_ARG   # 2^31 voxels: the interior labels are indexed like the labels
    assert call(rdims=(0, 12, 12)) == ERR_ARG
    o2 = capi.IcgnOptions()
    L.sift3d_default_icgn_options(C.byref(o2))
    o2.interpolation = 3
    assert call(o=C.byref(o2)) == ERR_ARG
    if capi.device_count() == 0:
        assert call() == ERR_NO_DEVICE and call(act=None, pl=None) == ERR_NO_DEVICE
        with pytest.raises(capi.Sift3dError):
            capi.icgn_labelled(R, T, lab, q, subset_radius=3)
    with pytest.raises(ValueError):
        capi.icgn_labelled(R, T, lab[:5], q, subset_radius=3)


# ---- the scratch layout: the labelled pieces come last -----------------------------------------------------------------------------

LAYOUT_PROGRAM = r"""
#include <stdio.h>
#include "icgn_host.h"
using namespace s3d;
static void show(const IcgnLayout &g) {
	printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", g.res_bytes, g.o_state, g.o_ref, g.o_tar, g.o_pts, g.o_opt, g.o_coef, g.o_tmp,
	       g.o_act, g.o_count, g.o_mask, g.b_mask, g.count_bytes, g.end);
}
int main() {
	const int m = 37;
	const size_t nr = 1000, nt = 1331;
	for (int dev = 0; dev < 2; dev++)
		for (int filter = 0; filter < 2; filter++) {
			show(icgn_layout(m, nr, nt, dev, true, filter, 1400, 128, 12));
			show(icgn_layout(m, nr, nt, dev, true, filter, 1400, 128, 12, false, false));
			show(icgn_layout(m, nr, nt, dev, true, filter, 1400, 128, 12, true));
			show(icgn_layout(m, nr, nt, dev, true, filter, 1400, 128, 12, true, false));
			const IcgnLayout p = icgn_layout(m, nr, nt, dev, true, filter, 1400, 128, 12), l = icgn_layout(m, nr, nt, dev, true, filter, 1400, 128, 12, false, true);
			printf("%zu %zu %zu %zu %zu %zu %zu\n", p.end, l.o_interior, l.o_count, l.o_plabel, l.o_labels, l.b_labels, l.end);
		}
	return 0;
}
"""


def test_labelled_layout_appends_to_the_plain_one(tmp_path):
    src, exe = tmp_path / "layout.cpp", tmp_path / "layout"
    src.write_text(LAYOUT_PROGRAM)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I" + CSRC, "-o", str(exe), str(src)])
    lines = subprocess.check_output([str(exe)], text=True).strip().split("\n")
    al = lambda b: (b + 255) & ~255
    for k in range(4):
        block = lines[5 * k:5 * k + 5]
        assert block[0] == block[1] and block[2] == block[3]   # the new argument's default changes neither layout
        end, o_int, o_cnt, o_pl, o_lab, b_lab, lend = map(int, block[4].split())
        dev = k // 2
        assert o_int == end and o_cnt == o_int + al(4 * 1000) and o_pl == o_cnt + al(4 * 37) and o_lab == o_pl + al(4 * 37)
        assert b_lab == (0 if dev else 4000) and lend == o_lab + al(b_lab)


# ---- the C++ shell -------------------------------------------------------------------------------------------------------------------

SHELL_PROGRAM = r"""
#include "Include/cRegistration.h"
#include <cstdio>
using namespace CPUSIFT;
int main() {
	// host only: the start of every point is its body's fit; a point of no body gets no start
	std::vector<AffineFit> fits(2);
	fits[0].status = 0; fits[0].A[3] = 1.5;
	fits[1].status = 2;
	std::vector<AffineFit> seeds = SeedsFromBodyFits(fits, {1, 2, 0, 3, -1});
	if (seeds.size() != 5 || seeds[0].status != 0 || seeds[0].A[3] != 1.5 || seeds[1].status != 2) return 1;
	if (seeds[2].status != 1 || seeds[3].status != 1 || seeds[4].status != 1) return 2;
	// the calls that need a GPU: they must link, and a refused call reports itself
	int lab[8] = {1, 1, 1, 1, 2, 2, 2, 2};
	std::vector<Cvec> r = {Cvec(0, 0, 0), Cvec(1, 1, 1)}, t = r;
	std::vector<int> pl, inl;
	std::vector<AffineFit> f = EstimateBodyRigid(r, t, lab, 2, 2, 2, -1, Rigid, RansacOptions(), &pl, &inl);   // count < 0: refused
	if (!f.empty() || pl.size() != 2 || inl.size() != 2) return 3;
	float vol[8] = {0};
	std::vector<int> active, labels;
	std::vector<IcgnResult> res = RefineDisplacementsLabelled(vol, 2, 2, 2, vol, 2, 2, 2, nullptr, r, nullptr, IcgnOptions(), 0.f, &active, &labels);
	if (res.size() != 2 || res[0].status != -1 || active.size() != 2 || labels.size() != 2) return 4;
	printf("ok\n");
	return 0;
}
"""


def test_shell_declarations_link(tmp_path):
    pkg = os.path.join(ROOT, "3dsift_amd")
    subprocess.check_call(["make", "-C", CSRC, "-j8"], stdout=subprocess.DEVNULL)
    subprocess.check_call(["make", "-C", os.path.join(pkg, "host")], stdout=subprocess.DEVNULL)
    src, exe = tmp_path / "bodies.cpp", tmp_path / "bodies"
    src.write_text(SHELL_PROGRAM)
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-I" + os.path.join(pkg, "host"), "-o", str(exe), str(src), "-L" + pkg, "-lsift3d",
                           "-lsift3d_hip", "-Wl,-rpath," + pkg])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stdout[-1000:], r.stderr[-2000:])
    assert "EstimateBodyRigid" in r.stderr and "RefineDisplacementsLabelled" in r.stderr
