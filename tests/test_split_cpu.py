"""CPU tests of the distance transform and of the labels of touching bodies (sift3d_mask_distance, sift3d_mask_from_distance,
sift3d_distance_at_points, sift3d_mask_split, include/sift3d_hip.h; tests/split_ref.py, tests/split_cases.py): the restated transform
equals scipy's (where scipy imports), the three scenes give the figures the header's rule implies, the rule's consequences hold on the
restatement, scene A separates a per-body fit from a single one on the restatement of the fits, the entries refuse bad arguments before
any device call, and a program written against the C++ shell's new declarations compiles, links and is refused as it should be."""
import ctypes as C
import importlib
import os
import subprocess
import tempfile

import numpy as np
import pytest

import body_cases
import label_ref
import split_cases as cases
import split_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "3dsift_amd")
CSRC = os.path.join(PKG, "csrc")
NEW = ["sift3d_mask_distance", "sift3d_mask_from_distance", "sift3d_distance_at_points", "sift3d_default_split_options", "sift3d_mask_split"]
ERR_ARG, ERR_NO_DEVICE = 1, 2
CONNECTIVITIES = (6, 26)


@pytest.fixture(scope="module")
def capi():
    m = importlib.import_module("3dsift_amd.capi")
    if not os.path.exists(m.LIB_PATH):
        subprocess.check_call(["make", "-C", CSRC, "-j8"])
    return m


def in_voxels(name):
    return cases.scene(name) != 0


# ---- the transform ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("border", (0, 1))
@pytest.mark.parametrize("density", (0.5, 0.9, 0.99))
def test_restated_transform_equals_scipy(density, border):
    ndi = pytest.importorskip("scipy.ndimage")
    m = (np.random.default_rng(int(density * 100)).random((20, 33, 41)) < density).astype(np.uint8)
    assert not m.all()
    got = ref.distance(m, border)
    want = np.rint(ndi.distance_transform_edt(np.pad(m, 1)) ** 2)[1:-1, 1:-1, 1:-1] if border else np.rint(ndi.distance_transform_edt(m) ** 2)
    assert got.dtype == np.int32 and np.array_equal(got, want)


def test_transform_edges():
    assert not ref.distance(np.zeros((3, 4, 5), np.uint8), 0).any() and not ref.distance(np.zeros((3, 4, 5), np.uint8), 1).any()
    full = np.ones((3, 4, 5), np.uint8)
    assert (ref.distance(full, 0) == ref.NONE).all()
    d = ref.distance(full, 1)
    assert d[0].max() == 1 and d[1, 1:3, 2].tolist() == [4, 4] and d.max() == 4   # a face voxel is 1 from the layer outside
    one = full.copy()
    one[0, 0, 0] = 0
    z, y, x = np.indices(one.shape)
    assert np.array_equal(ref.distance(one, 0), x * x + y * y + z * z)
    assert np.array_equal(ref.mask_from_distance(d, 4), d >= 4) and ref.mask_from_distance(d, 4).dtype == np.uint8
    q = np.array([(2, 1, 1), (5, 0, 0), (-1, 0, 0), (0, 4, 0), (0, 0, 3), (4, 3, 2)])
    assert ref.distance_at(d, q).tolist() == [4, 0, 0, 0, 0, 1]


def test_edt_battery_shapes():
    """the GPU battery holds an axis longer than any staging on each axis in turn, and every ballot-word seam along x"""
    shapes = {n: cases.edt_mask(n).shape for n in cases.EDT_MASKS}
    assert shapes["long-x"] == (3, 3, 5000) and shapes["long-y"] == (3, 5000, 3) and shapes["long-z"] == (5000, 3, 2)
    assert shapes["two-runs"] == (2, 70, 130) and [shapes[f"x-{n}"][2] for n in (63, 64, 65, 129)] == [63, 64, 65, 129]
    assert cases.edt_mask("all-in").all() and not cases.edt_mask("all-out").any()
    assert (cases.edt_mask("one-out-corner") == 0).sum() == 1 and cases.edt_mask("one-in").sum() == 1
    assert (cases.edt_reference("all-in", 0) == ref.NONE).all()
    assert cases.edt_reference("long-y-one-out", 0).max() == 650 ** 2 + 1 + 4   # far beyond a staged run, found through the other passes


# ---- the scenes ------------------------------------------------------------------------------------------------------------------------

def test_scene_a():
    m = in_voxels("A")
    assert m.shape == (32, 32, 44) and label_ref.label(m, 6)[1] == 1 and label_ref.label(m, 26)[1] == 1
    d = cases.distance("A", 1)
    assert d[16, 16, 21] == 34 and d.max() == 82
    for connectivity, rounds in ((6, 12), (26, 7)):
        lab, count, info, d2 = cases.split("A", connectivity=connectivity, **cases.A_OPTS)
        assert count == 2 and info == {"cores": 2, "unreached_bodies": 0, "rounds": rounds, "unlabelled": 0}
        assert np.array_equal(d2, d)
        assert (lab[:, :, :21][m[:, :, :21]] == 1).all() and (lab[:, :, 22:][m[:, :, 22:]] == 2).all()
        assert m[:, :, 21].any() and (lab[:, :, 21][m[:, :, 21]] == 1).all()   # the plane between them: the tie goes to the smaller label
        assert not lab[~m].any()


def test_scene_b():
    m = in_voxels("B")
    assert m.shape == (32, 36, 44) and int(m.sum()) == 5535
    (c1, r1), (c2, r2) = [(np.array(b[:3], np.float64), b[3]) for b in cases.B_BALLS]
    z, y, x = np.indices(m.shape)
    p = np.stack([x, y, z], -1).astype(np.float64)
    power = (((p - c1) ** 2).sum(-1) - r1 ** 2) - (((p - c2) ** 2).sum(-1) - r2 ** 2)
    signed = power / (2 * np.linalg.norm(c2 - c1))   # the signed distance to the two spheres' radical plane
    side = np.where(signed <= 0, 1, 2)
    worst = {}
    for connectivity in CONNECTIVITIES:
        for core_dist2 in cases.B_CORE_DIST2:
            lab, count, info, _ = cases.split("B", connectivity=connectivity, core_dist2=core_dist2)
            assert count == 2 and info["cores"] == 2 and info["unlabelled"] == 0 and info["unreached_bodies"] == 0
            wrong = m & (lab != side)
            worst[(connectivity, core_dist2)] = (int(wrong.sum()), float(np.abs(signed[wrong]).max()))
    print(worst)
    assert all(16 <= n <= 45 for n, _ in worst.values())
    assert max(worst.values(), key=lambda v: v[1]) == worst[(6, 36)] and abs(worst[(6, 36)][1] - 1.55) < 0.005
    assert all(far <= 2.0 for _, far in worst.values())   # the measured worst plus the half voxel a lattice cannot resolve


def test_scene_c():
    m = in_voxels("C")
    assert m.shape == (32, 32, 60)
    small = m.copy()
    small[:, :, :40] = False
    assert int(small.sum()) == 257 and cases.distance("C", 1)[small].max() < cases.A_OPTS["core_dist2"]   # it holds no core
    lab, count, info, _ = cases.split("C", keep_unreached=0, **cases.A_OPTS)
    assert count == 2 and info["unlabelled"] == 257 and info["unreached_bodies"] == 0 and not lab[small].any()
    lab, count, info, _ = cases.split("C", keep_unreached=1, **cases.A_OPTS)
    assert count == 3 and info["unlabelled"] == 0 and info["unreached_bodies"] == 1 and (lab[small] == 3).all()
    assert np.array_equal(lab[:, :, :44], cases.split("A", **cases.A_OPTS)[0])
    # the size cut of the unreached components
    assert cases.split("C", min_voxels=257, **cases.A_OPTS)[1] == 3 and cases.split("C", min_voxels=258, **cases.A_OPTS)[1] == 2


def test_the_runs_of_the_gpu_test_cover_the_options():
    infos = [cases.split(name, **o)[2] for name, o in cases.SPLIT_RUNS]
    assert any(i["cores"] == 0 and i["unreached_bodies"] > 0 for i in infos) and any(i["rounds"] > 50 for i in infos)
    assert any(i["unlabelled"] > 0 for i in infos) and any(i["cores"] > 1000 for i in infos)
    assert label_ref.label(cases.scene("packing"), 26)[1] < cases.split("packing", core_dist2=16)[1]   # the packing's balls touch
    for name, o in cases.SPLIT_RUNS:
        if o.get("max_rounds"):
            assert cases.split(name, **o)[2]["rounds"] == o["max_rounds"]
            assert cases.split(name, **dict(o, max_rounds=0))[2]["rounds"] > o["max_rounds"]
    assert cases.split("packing", core_dist2=30)[2]["cores"] > cases.split("packing", core_dist2=30, min_core_voxels=40)[2]["cores"]


# ---- the rule's consequences ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("connectivity", CONNECTIVITIES)
@pytest.mark.parametrize("name", ("A", "packing", "random-0.6", "random-0.25"))
def test_consequence_a_core_dist2_1_is_the_plain_labelling(name, connectivity):
    for cut, keep in ((1, 1), (1, 0), (5, 0)):
        lab, count, info, _ = cases.split(name, core_dist2=1, connectivity=connectivity, min_core_voxels=cut, keep_unreached=keep)
        want, n = label_ref.label(cases.scene(name), connectivity, cut)
        assert count == n and info["rounds"] == 0 and info["cores"] == n and np.array_equal(lab, want)


def pieces_within_labels(lab, connectivity):
    """the number of connected pieces when only voxels of the same positive label join: label_ref.roots' sweep with that condition"""
    big = label_ref.BIG
    root = np.where(lab > 0, np.arange(lab.size, dtype=np.int64).reshape(lab.shape), big)
    while True:
        new = root
        for d in label_ref.offsets(connectivity):
            same = label_ref._shifted(lab, *d, 0) == lab
            new = np.minimum(new, np.where(same, label_ref._shifted(root, *d, big), big))
        new = np.where(lab > 0, new, big)
        if np.array_equal(new, root):
            return len(np.unique(root[lab > 0]))
        root = new


@pytest.mark.parametrize("name,opts", [("A", cases.A_OPTS), ("B", {"core_dist2": 30}), ("packing", {"core_dist2": 16}),
                                       ("random-0.6", {"core_dist2": 3}), ("random-0.3116", {"core_dist2": 2})])
@pytest.mark.parametrize("connectivity", CONNECTIVITIES)
def test_consequences_c_d_e(name, opts, connectivity):
    lab, count, info, d = cases.split(name, connectivity=connectivity, **opts)
    m = cases.scene(name) != 0
    plain, _ = label_ref.label(m, connectivity)
    # (c) every label's voxels are one component under the connectivity
    assert pieces_within_labels(lab, connectivity) == count == len(np.unique(lab[lab > 0]))
    # (d) the split only refines: a split label lies within one plain component
    pairs = np.unique(np.stack([lab[m & (lab > 0)], plain[m & (lab > 0)]], 1), axis=0)
    assert len(np.unique(pairs[:, 0])) == len(pairs)
    # (e) the labels on the core voxels are L0's
    L0, cores = label_ref.label(d >= opts["core_dist2"], connectivity, 1)
    assert cores == info["cores"] and np.array_equal(lab[L0 > 0], L0[L0 > 0])
    assert not lab[~m].any() and int((m & (lab == 0)).sum()) == info["unlabelled"]


# ---- end to end on the restatement of the fits -------------------------------------------------------------------------------------------

def test_scene_a_separates_the_per_body_fit_from_the_single_one():
    lab, count, info, _ = cases.split("A", **cases.A_OPTS)
    errors = cases.fit_errors(lab, count)
    print(errors)
    assert len(errors) == 2 and all(e[0] == 0 for e in errors)
    assert errors[0][1] <= body_cases.ROT_BOUND and errors[1][2] <= body_cases.ROT_BOUND
    plain, n = label_ref.label(cases.scene("A"), 6)
    single = cases.fit_errors(plain, n)
    print(single)
    assert len(single) == 1 and max(single[0][1:]) > body_cases.ROT_BOUND   # one motion cannot be both


# ---- the entries -------------------------------------------------------------------------------------------------------------------------

def P(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


BAD_DIMS = [(0, 4, 4), (4, -1, 4), (4, 4, 0), (1 << 11, 1 << 10, 1 << 10), (2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1),
            (46340, 1, 1), (32767, 32767, 1), (37838, 37838, 1)]   # the last three: a squared distance would not fit an int


def test_exports_and_defaults(capi):
    L = capi.lib()
    for n in NEW:
        assert hasattr(L, n), n
        assert n in capi.SYMBOLS
    assert all(hasattr(capi, f) for f in ("mask_distance", "mask_from_distance", "distance_at", "mask_split", "default_split_options"))
    assert capi.default_split_options() == ref.DEFAULTS and capi.DIST2_NONE == ref.NONE
    o = capi.SplitOptions(*([-7] * 7))
    L.sift3d_default_split_options(C.byref(o))
    assert [getattr(o, k) for k in capi.SPLIT_OPTIONS] == [6, 16, 1, 1, 0, 1, 1]
    L.sift3d_default_split_options(None)   # tolerated


def test_mask_distance_refusals(capi):
    L = capi.lib()
    mask, dist = np.ones((4, 4, 4), np.uint8), np.zeros((4, 4, 4), np.int32)

    def call(mask=mask, dims=(4, 4, 4), border=1, dist=dist):
        return L.sift3d_mask_distance(P(mask), dims[0], dims[1], dims[2], border, P(dist), 0, 0, None)

    assert call(mask=None) == ERR_ARG
    assert b"sift3d_mask_distance: bad argument" in L.sift3d_last_error()
    assert call(dist=None) == ERR_ARG
    for dims in BAD_DIMS:
        assert call(dims=dims) == ERR_ARG, dims
    for b in (-1, 2, 6):
        assert call(border=b) == ERR_ARG
    if capi.device_count() == 0:   # the argument check comes first, the device after it: there is no CPU fallback
        assert call() == ERR_NO_DEVICE and call(border=0) == ERR_NO_DEVICE
        assert call(dims=(46339, 1, 1)) == ERR_NO_DEVICE   # 46340^2 + 4 + 4 < 2^31: the longest row
        with pytest.raises(capi.Sift3dError):
            capi.mask_distance(mask)


def test_mask_from_distance_and_distance_at_refusals(capi):
    L = capi.lib()
    mask, dist = np.ones((4, 4, 4), np.uint8), np.zeros((4, 4, 4), np.int32)

    def erode(dist=dist, dims=(4, 4, 4), level2=4, mask=mask):
        return L.sift3d_mask_from_distance(P(dist), dims[0], dims[1], dims[2], level2, P(mask), 0, 0, None)

    assert erode(dist=None) == ERR_ARG
    assert b"sift3d_mask_from_distance: bad argument" in L.sift3d_last_error()
    assert erode(mask=None) == ERR_ARG
    for dims in ((0, 4, 4), (4, 0, 4), (4, 4, -3), (1 << 13, 1 << 13, 1 << 13), (2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1)):
        assert erode(dims=dims) == ERR_ARG
    if capi.device_count() == 0:
        assert erode() == ERR_NO_DEVICE and erode(level2=-5) == ERR_NO_DEVICE   # any int is a level
    out, one = np.zeros(4, np.int32), np.zeros((4, 3), np.int32)
    assert L.sift3d_distance_at_points(None, 4, 4, 4, P(one), 4, P(out), 0, 0) == ERR_ARG
    assert b"sift3d_distance_at_points: bad argument" in L.sift3d_last_error()
    assert L.sift3d_distance_at_points(P(dist), 4, 0, 4, P(one), 4, P(out), 0, 0) == ERR_ARG
    assert L.sift3d_distance_at_points(P(dist), 1 << 11, 1 << 10, 1 << 10, P(one), 4, P(out), 0, 0) == ERR_ARG
    assert L.sift3d_distance_at_points(P(dist), 4, 4, 4, None, 4, P(out), 0, 0) == ERR_ARG
    assert L.sift3d_distance_at_points(P(dist), 4, 4, 4, P(one), 4, None, 0, 0) == ERR_ARG
    assert L.sift3d_distance_at_points(P(dist), 4, 4, 4, P(one), -1, P(out), 0, 0) == ERR_ARG
    if capi.device_count() == 0:
        assert L.sift3d_distance_at_points(P(dist), 4, 4, 4, P(one), 4, P(out), 1, 0) == ERR_NO_DEVICE
    # the host path is NumPy indexing and needs no GPU
    rng = np.random.default_rng(8)
    d = rng.integers(0, 90, (6, 7, 9)).astype(np.int32)
    q = rng.integers(-3, 12, (300, 3)).astype(np.int32)
    q[:4] = [(8, 6, 5), (9, 0, 0), (2 ** 31 - 1, 0, 0), (-2 ** 31, 3, 3)]
    assert np.array_equal(capi.distance_at(d, q), ref.distance_at(d, q)) and len(capi.distance_at(d, np.zeros((0, 3), np.int32))) == 0


def test_mask_split_refusals(capi):
    L = capi.lib()
    mask, lab, dist, count = np.ones((4, 4, 4), np.uint8), np.zeros((4, 4, 4), np.int32), np.zeros((4, 4, 4), np.int32), C.c_int(0)
    info = capi.SplitInfo()

    def call(mask=mask, dims=(4, 4, 4), lab=lab, count=C.byref(count), dist=dist, info=C.byref(info), null_options=False, **opts):
        o = capi.SplitOptions()
        L.sift3d_default_split_options(C.byref(o))
        for k, v in opts.items():
            setattr(o, k, v)
        return L.sift3d_mask_split(P(mask), dims[0], dims[1], dims[2], None if null_options else C.byref(o), P(lab), count, P(dist), info, 0, 0, None)

    assert call(mask=None) == ERR_ARG
    assert b"sift3d_mask_split: bad argument" in L.sift3d_last_error()
    assert call(lab=None) == ERR_ARG and call(count=None) == ERR_ARG and call(null_options=True) == ERR_ARG
    for dims in BAD_DIMS:
        assert call(dims=dims) == ERR_ARG, dims
    bad = {"connectivity": (0, 8, 18, 27, -6), "core_dist2": (0, -1), "min_core_voxels": (0, -1), "border": (-1, 2), "max_rounds": (-1,),
           "keep_unreached": (-1, 2), "min_voxels": (0, -1)}
    assert set(bad) == set(capi.SPLIT_OPTIONS)
    for k, values in bad.items():
        for v in values:
            assert call(**{k: v}) == ERR_ARG, (k, v)
    if capi.device_count() == 0:
        assert call() == ERR_NO_DEVICE and call(dist=None, info=None) == ERR_NO_DEVICE   # both are optional
        assert call(connectivity=26, core_dist2=2 ** 31 - 1, max_rounds=2 ** 31 - 1, min_voxels=2 ** 31 - 1, border=0, keep_unreached=0) == ERR_NO_DEVICE
        with pytest.raises(capi.Sift3dError):
            capi.mask_split(mask)
    with pytest.raises(TypeError):
        capi.mask_split(mask, core=3)


# ---- the C++ shell -------------------------------------------------------------------------------------------------------------------------

SHELL_PROGRAM = r"""
#include "Include/cRegistration.h"
#include <cstdio>
using namespace CPUSIFT;
int main() {
	// host only: the distances at three points of a 4 x 3 x 2 volume whose entry is its linear index
	int d[24];
	for (int i = 0; i < 24; i++) d[i] = i;
	std::vector<Cvec> pts = {Cvec(1, 2, 1), Cvec(4, 0, 0), Cvec(3, 2, 1)};
	std::vector<int> at = DistancesAt(d, 4, 3, 2, pts);
	if (at.size() != 3 || at[0] != 21 || at[1] != 0 || at[2] != 23) return 1;
	if (!DistancesAt(d, 4, 3, 2, {Cvec(0.5f, 0, 0)}).empty()) return 2;
	// the calls that need a GPU: they must link, and a refused call reports itself
	unsigned char mask[8] = {1, 1, 1, 1, 1, 1, 1, 1};
	int labels[8], dist2[8], count = -1;
	if (DistanceTransform(mask, 2, 0, 2, true, dist2)) return 3;         // an extent of 0: refused before any device call
	if (ErodeMask(nullptr, 2, 2, 2, 4, mask)) return 4;
	SplitOptions o;
	if (o.connectivity != 6 || o.core_dist2 != 16 || o.min_core_voxels != 1 || !o.border || o.max_rounds != 0 || !o.keep_unreached ||
	    o.min_voxels != 1)
		return 5;
	o.connectivity = 18;
	SplitInfo info;
	if (SplitBodies(mask, 2, 2, 2, labels, &count, o, dist2, &info)) return 6;   // 18-connectivity: refused
	o.connectivity = 26;
	o.core_dist2 = 0;
	if (SplitBodies(mask, 2, 2, 2, labels, &count, o)) return 7;
	if (info.cores != 0 || info.rounds != 0) return 8;
	printf("ok\n");
	return 0;
}
"""


def test_shell_declarations_link():
    subprocess.check_call(["make", "-C", CSRC, "-j8"], stdout=subprocess.DEVNULL)
    subprocess.check_call(["make", "-C", os.path.join(PKG, "host")], stdout=subprocess.DEVNULL)
    with tempfile.TemporaryDirectory() as t:
        src, exe = os.path.join(t, "split.cpp"), os.path.join(t, "split")
        open(src, "w").write(SHELL_PROGRAM)
        subprocess.check_call(["g++", "-std=c++14", "-Wall", "-I" + os.path.join(PKG, "host"), "-o", exe, src, "-L" + PKG, "-lsift3d",
                               "-lsift3d_hip", "-Wl,-rpath," + PKG])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stdout[-1000:], r.stderr[-2000:])
    for who in ("DistanceTransform", "ErodeMask", "SplitBodies"):
        assert who in r.stderr
