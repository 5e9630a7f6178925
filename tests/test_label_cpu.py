"""CPU tests of the labels (sift3d_mask_label, sift3d_labels_at_points and the labelled window calls, include/sift3d_hip.h;
tests/label_ref.py, tests/label_cases.py): the restatement of the labelling equals scipy.ndimage.label on every mask at both
connectivities (where scipy imports), the cases do what they claim (component counts, the sweeps of the long and ramified ones, the
seam geometry relative to the tile T), the two scenes of several bodies give through the per-label wrappers the figures the GPU
tests rely on, the five entries refuse bad arguments before any device call, the host path of sift3d_labels_at_points is NumPy
indexing, and a program written against the C++ shell's new declarations compiles and links."""
import ctypes as C
import importlib
import os
import subprocess
import tempfile

import numpy as np
import pytest

import field_ref
import label_cases as cases
import label_ref as ref
import strain_ref
import validate_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "3dsift_amd")
CSRC = os.path.join(PKG, "csrc")
NEW = ["sift3d_mask_label", "sift3d_labels_at_points", "sift3d_strain_labelled", "sift3d_validate_displacements_labelled",
       "sift3d_field_eval_labelled", "sift3d_test_label_tile"]
ERR_ARG, ERR_NO_DEVICE = 1, 2
CONNECTIVITIES = (6, 26)


@pytest.fixture(scope="module")
def capi():
    m = importlib.import_module("3dsift_amd.capi")
    if not os.path.exists(m.LIB_PATH):
        subprocess.check_call(["make", "-C", CSRC, "-j8"])
    return m


def test_exports(capi):
    L = capi.lib()
    for n in NEW:
        assert hasattr(L, n), n
        assert n in capi.SYMBOLS
    assert all(hasattr(capi, f) for f in ("mask_label", "labels_at", "label_tile"))
    assert capi.label_tile() == cases.DEFAULT_TILE == cases.tile()


# ---- the restatement and the cases ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("connectivity", CONNECTIVITIES)
@pytest.mark.parametrize("name", sorted(cases.MASKS))
def test_restatement_equals_scipy(name, connectivity):
    ndi = pytest.importorskip("scipy.ndimage")
    want, count = ndi.label(cases.get(name), ndi.generate_binary_structure(3, 1 if connectivity == 6 else 3))
    got, n = cases.reference(name, connectivity)
    assert n == count
    assert got.dtype == np.int32 and np.array_equal(got, want)


def test_min_voxels_equals_scipy_with_the_small_components_removed():
    ndi = pytest.importorskip("scipy.ndimage")
    for name, connectivity, cut in cases.size_cuts():
        lab, count = ndi.label(cases.get(name), ndi.generate_binary_structure(3, 1 if connectivity == 6 else 3))
        sizes = np.bincount(lab.reshape(-1))
        kept = sizes >= cut
        kept[0] = False
        renumber = np.where(kept, np.cumsum(kept), 0)
        got, n = cases.reference(name, connectivity, cut)
        assert n == int(kept.sum()) and np.array_equal(got, renumber[lab])


# name -> (components under 6, under 26)
COUNTS = {"zero": (0, 0), "full": (1, 1), "line-x": (1, 1), "line-z": (1, 1), "serpentine": (1, 1), "u-shape": (2, 2),
          "seam-face-x": (1, 1), "seam-face-y": (1, 1), "seam-face-z": (1, 1), "seam-edge-x": (4, 2), "seam-edge-y": (4, 2),
          "seam-edge-z": (4, 2), "seam-corner": (8, 4),
          "random-0.10": (8473, 1678), "random-0.25": (9137, 66), "random-0.3116": (6732, 13), "random-0.6": (391, 1)}


@pytest.mark.parametrize("name", sorted(COUNTS))
def test_component_counts(name):
    assert tuple(cases.reference(name, c)[1] for c in CONNECTIVITIES) == COUNTS[name]


def test_the_plain_shapes():
    assert not cases.get("zero").any() and not cases.reference("zero", 6)[0].any()
    full = cases.get("full")
    assert full.all() and set(np.unique(full)) == {1, 128, 255}
    assert all(full.shape[2 - a] > t for a, t in enumerate(cases.tile()))   # several tiles along every axis
    assert all((cases.reference("full", c)[0] == 1).all() for c in CONNECTIVITIES)
    assert cases.get("line-x").shape == (1, 1, 300) and cases.get("line-z").shape == (300, 1, 1)
    board = cases.get("checkerboard")
    lab6, n6 = cases.reference("checkerboard", 6)
    assert n6 == int(board.sum()) and np.array_equal(lab6[board != 0], np.arange(1, n6 + 1))   # every in-voxel its own component, in order
    assert cases.reference("checkerboard", 26)[1] == 1


def test_the_extent_cases_cover_every_size_around_the_tile():
    tile = cases.tile()
    table = cases.extents()
    assert len(table) == 15
    for axis, t in enumerate(tile):
        assert sorted(n for a, n in table.values() if a == axis) == sorted({1, t - 1, t, t + 1, 2 * t + 1})
    for name, (axis, n) in table.items():
        shape = cases.get(name).shape[::-1]
        assert shape[axis] == n
        assert all(shape[a] % tile[a] != 0 and shape[a] < tile[a] for a in range(3) if a != axis), name
        assert cases.get(name).any()


def test_the_seam_contacts_straddle_tile_boundaries():
    tile = np.array(cases.tile())
    for name, pairs in cases.SEAM_PAIRS.items():
        m = cases.get(name)
        vox = np.argwhere(m)[:, ::-1]   # (x, y, z)
        assert len(vox) == 2 * pairs
        lab = cases.reference(name, 26)[0]
        assert cases.reference(name, 26)[1] == pairs
        for k in range(1, pairs + 1):
            a, b = np.argwhere(lab == k)[:, ::-1]
            d = np.abs(a - b)
            crossed = (a // tile) != (b // tile)
            assert d.max() == 1
            if "face" in name:
                axis = "xyz".index(name[-1])
                assert d.sum() == 1 and d[axis] == 1 and crossed[axis]
            elif "edge" in name:
                along = "xyz".index(name[-1])
                assert d.sum() == 2 and d[along] == 0 and crossed.sum() == 2   # only an edge is shared, across both other boundaries
            else:
                assert d.sum() == 3 and crossed.all()                          # only a corner is shared, where eight tiles meet
        # under 6 only a face joins
        assert cases.reference(name, 6)[1] == (pairs if "face" in name else 2 * pairs)
    # both diagonals of an edge, all four of the corner
    for name in ("seam-edge-x", "seam-edge-y", "seam-edge-z", "seam-corner"):
        lab = cases.reference(name, 26)[0]
        dirs = set()
        for k in range(1, cases.SEAM_PAIRS[name] + 1):
            a, b = np.argwhere(lab == k)[:, ::-1]
            dirs.add(tuple(int(v) for v in np.sign(b - a) * np.sign((b - a)[np.flatnonzero(b - a)[0]])))
        assert len(dirs) == cases.SEAM_PAIRS[name], (name, dirs)


def test_the_long_and_the_ramified_cases_need_many_sweeps():
    """what catches a merge that stops after a fixed number of hops: the sweeps of the iterated minimum, the last one changing nothing"""
    sweeps = {(n, c): cases.reference_roots(n, c)[1] for n in ("serpentine", "random-0.3116", "random-0.10") for c in CONNECTIVITIES}
    print(sweeps)
    assert cases.get("serpentine").shape == (9, 17, 33)
    assert sweeps[("serpentine", 6)] == 1529 and sweeps[("serpentine", 26)] == 1441   # more than 500 either way
    assert sweeps[("random-0.3116", 6)] == 211 and sweeps[("random-0.10", 26)] == 182    # the two percolation thresholds


def test_u_shape_numbers_by_the_lowest_voxel():
    m = cases.get("u-shape")
    tx = cases.tile()[0]
    lab, n = cases.reference("u-shape", 6)
    assert n == 2
    a, b = np.flatnonzero(lab.reshape(-1) == 1), np.flatnonzero(lab.reshape(-1) == 2)
    assert len(b) == 1 and a[0] < b[0]
    nx = m.shape[2]
    assert a[0] % nx >= tx                                       # A's lowest voxel lies in the second tile along x ...
    near = a[(a % nx) < tx]
    assert len(near) and near[0] > b[0]                          # ... and what the first tile holds of A comes after B


def test_min_voxels_cases():
    (n3, c3, cut3), (ns, cs, s), (nt, ct, s1), (n26, c26, cut26) = cases.size_cuts()
    assert (cut3, cut26, s1) == (3, 3, s + 1)
    assert cases.reference(n3, c3)[1] == 9137 and cases.reference(n3, c3, 3)[1] == 2439
    sizes = np.bincount(cases.reference(ns, cs)[0].reshape(-1))[1:]
    assert (sizes == s).sum() == 1 and (sizes > s).sum() == 1    # the cut at s keeps it, the cut at s + 1 drops it
    assert cases.reference(ns, cs, s)[1] == 2 and cases.reference(nt, ct, s1)[1] == 1
    kept = cases.reference(n3, c3, 3)[0]
    assert np.array_equal(kept != 0, np.isin(cases.reference(n3, c3)[0], np.flatnonzero(np.bincount(cases.reference(n3, c3)[0].reshape(-1)) >= 3)[1:]))


# ---- the scenes --------------------------------------------------------------------------------------------------------------------------

def test_two_bodies_scene():
    q, u, lab = cases.two_bodies()
    plain = strain_ref.strain(q, u, None, radius=cases.SCENE_RADIUS)
    assert abs(np.abs(plain["E"]).max() - 0.075) < 5e-4 and abs(plain["equivalent"].max() - 0.097) < 5e-4
    near = np.abs(q[:, 2] - 19.5) <= cases.SCENE_RADIUS
    assert (np.abs(plain["E"]).max(1) > 0.01)[near].all() and not np.abs(plain["E"])[~near].any()
    own = ref.strain(q, u, None, lab, radius=cases.SCENE_RADIUS)
    assert not own["status"].any() and own["neighbours"].min() == 27
    assert all(not own[k].any() for k in ("E", "G", "rms", "principal", "equivalent"))   # exactly 0
    assert np.array_equal(own["disp"], u)


def test_grain_scene():
    q, u, lab, x = cases.grain()
    assert (lab == 2).sum() == 27 and (lab == 1).sum() == 973
    plain = validate_ref.validate(q, u, radius=cases.SCENE_RADIUS)
    assert plain["flagged"][lab == 2].all() and not plain["flagged"][lab == 1].any()   # all 27 correct grain vectors, none in the matrix
    own = ref.validate(q, u, None, None, lab, radius=cases.SCENE_RADIUS)
    assert not own["flagged"].any() and not own["status"].any() and own["neighbours"].min() == 26
    blend = field_ref.evaluate(q, u, None, x, radius=cases.SCENE_RADIUS)
    assert blend["status"][0] == 0 and np.allclose(blend["disp"][0], (0.99, -0.39, 0.34), atol=5e-3)   # belongs to neither body
    for L, want in ((1, 0.01 * x[0, [1, 2, 0]]), (2, np.array([1.5, -0.75, 0.5]))):
        part = ref.evaluate(q, u, None, lab, x, [L], radius=cases.SCENE_RADIUS, require_enclosed=0)
        assert part["status"][0] == 0 and np.allclose(part["disp"][0], want, atol=1e-12)


def test_wrappers_give_status_1_to_labels_below_1():
    q, u, lab = cases.two_bodies()
    lab = lab.copy()
    lab[::7] = 0
    lab[3::11] = -4
    q = q.copy()
    q[0] = (2 ** 24 + 1, 0, 0)   # label 0 and out of range: status 2 comes first
    s = ref.strain(q, u, None, lab, radius=8)
    v = ref.validate(q, u, None, None, lab, radius=8)
    f = ref.evaluate(q, u, None, lab, q.astype(np.float64), lab, radius=8)
    low = lab <= 0
    for r in (s, v, f):
        assert r["status"][0] == 2 and (r["status"][low][1:] == 1).all() and not r["neighbours"][low].any()
    assert not f["sides"][low].any() and not v["flagged"][low].any()
    assert (s["status"][~low] == 0).all()


def test_wrappers_on_the_pois_of_a_label_alone_equal_the_literal_form():
    """the GPU tests use the fast form of the per-label wrappers: on inputs with invalid POIs and labels <= 0 it is the literal one"""
    rng = np.random.default_rng(1)
    q, u, valid = strain_ref.parity_inputs()
    lab = rng.integers(-1, 4, len(q))
    a, b = (ref.strain(q, u, valid, lab, literal=k, radius=20, min_neighbours=6) for k in (False, True))
    assert all(np.array_equal(a[k], b[k]) for k in a) and (a["status"] == 0).sum() > 500
    import validate_cases
    c = validate_cases.get("planted-k0.002-n0.02-grad")
    lab = rng.integers(-1, 3, len(c["points"]))
    a, b = (ref.validate(c["points"], c["disp"], c["grad"], c["valid"], lab, literal=k, **c["opts"]) for k in (False, True))
    assert a.tobytes() == b.tobytes() and a["flagged"].sum() > 0
    q, u, valid, xs = field_ref.parity_inputs()
    lab, qlab = rng.integers(-1, 3, len(q)), rng.integers(-1, 3, len(xs))
    a, b = (ref.evaluate(q, u, valid, lab, xs, qlab, literal=k, radius=16, min_neighbours=6, require_enclosed=0) for k in (False, True))
    assert all(np.array_equal(a[k], b[k]) for k in a) and (a["status"] == 0).sum() > 300


def test_spheres_scene():
    vol, centres, q, u, body = cases.spheres()
    assert vol.shape == (64, 80, 96) and len(centres) == 12
    mask = (vol >= cases.SPHERE_LEVEL).astype(np.uint8)
    for c in CONNECTIVITIES:   # at least one voxel of air between any two spheres, diagonals included
        lab, n = ref.label(mask, c)
        assert n == 12
        assert np.array_equal(ref.labels_at(lab, q), body)
    assert (np.bincount(body)[1:] >= 80).all()


# ---- the entries ----------------------------------------------------------------------------------------------------------------------

def P(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def test_mask_label_refusals(capi):
    L = capi.lib()
    mask, lab, count = np.ones((4, 4, 4), np.uint8), np.zeros((4, 4, 4), np.int32), C.c_int(0)

    def call(mask=mask, dims=(4, 4, 4), connectivity=6, min_voxels=1, lab=lab, count=C.byref(count)):
        return L.sift3d_mask_label(P(mask), dims[0], dims[1], dims[2], connectivity, min_voxels, P(lab), count, 0, 0, None)

    assert call(mask=None) == ERR_ARG
    assert b"sift3d_mask_label: bad argument" in L.sift3d_last_error()
    assert call(lab=None) == ERR_ARG and call(count=None) == ERR_ARG
    for a in range(3):
        for bad in (0, -1):
            dims = [4, 4, 4]
            dims[a] = bad
            assert call(dims=dims) == ERR_ARG
    assert call(dims=(1 << 11, 1 << 10, 1 << 10)) == ERR_ARG   # 2^31 voxels: linear indices are int
    assert call(dims=(2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1)) == ERR_ARG
    for c in (0, 4, 8, 18, 27, -6):
        assert call(connectivity=c) == ERR_ARG
    for v in (0, -1):
        assert call(min_voxels=v) == ERR_ARG
    if capi.device_count() == 0:   # the argument check comes first, the device after it: there is no CPU fallback
        for c in CONNECTIVITIES:
            assert call(connectivity=c) == ERR_NO_DEVICE
        assert call(min_voxels=2 ** 31 - 1) == ERR_NO_DEVICE
        with pytest.raises(capi.Sift3dError):
            capi.mask_label(mask)


def test_labelled_window_refusals(capi):
    L = capi.lib()
    q = np.zeros((4, 3), np.int32)
    u = np.zeros((4, 3))
    lab = np.ones(4, np.int32)
    x = np.zeros((2, 3))
    xl = np.ones(2, np.int32)
    s, v, f = np.zeros(4, capi.STRAIN_DTYPE), np.zeros(4, capi.VALIDATE_DTYPE), np.zeros(2, capi.FIELD_DTYPE)

    def strain(q=q, u=u, lab=lab, m=4, out=s):
        return L.sift3d_strain_labelled(P(q), P(u), None, P(lab), m, None, 0, 0, P(out), None)

    def validate(q=q, u=u, lab=lab, m=4, out=v):
        return L.sift3d_validate_displacements_labelled(P(q), P(u), None, None, P(lab), m, None, 0, 0, P(out), None)

    def field(q=q, u=u, lab=lab, m=4, x=x, xl=xl, nq=2, out=f):
        return L.sift3d_field_eval_labelled(P(q), P(u), None, P(lab), m, P(x), P(xl), nq, None, 0, 0, P(out), None)

    for call, name in ((strain, b"sift3d_strain_labelled"), (validate, b"sift3d_validate_displacements_labelled"),
                       (field, b"sift3d_field_eval_labelled")):
        assert call(lab=None) == ERR_ARG
        assert name + b": bad argument" in L.sift3d_last_error()
        assert call(lab=None, m=0) == ERR_ARG        # labels are an array, not an option
        assert call(q=None) == ERR_ARG and call(u=None) == ERR_ARG and call(out=None) == ERR_ARG and call(m=-1) == ERR_ARG
    assert field(xl=None) == ERR_ARG and field(x=None) == ERR_ARG and field(nq=-1) == ERR_ARG
    o = capi.StrainOptions()
    L.sift3d_default_strain_options(C.byref(o))
    o.radius = 0
    assert L.sift3d_strain_labelled(P(q), P(u), None, P(lab), 4, C.byref(o), 0, 0, P(s), None) == ERR_ARG
    if capi.device_count() == 0:
        assert strain() == ERR_NO_DEVICE and validate() == ERR_NO_DEVICE and field() == ERR_NO_DEVICE
        assert field(xl=None, nq=0) == ERR_NO_DEVICE   # no query, no query label needed
    # the unlabelled entries name themselves as before
    assert L.sift3d_strain(None, None, None, 4, None, 0, 0, P(s), None) == ERR_ARG
    assert b"sift3d_strain: bad argument" in L.sift3d_last_error()


def test_labels_at_host_path_is_numpy_indexing(capi):
    rng = np.random.default_rng(5)
    lab = rng.integers(-3, 50, (6, 7, 9)).astype(np.int32)
    q = rng.integers(-3, 12, (500, 3)).astype(np.int32)
    q[:8] = [(0, 0, 0), (8, 6, 5), (9, 0, 0), (0, 7, 0), (0, 0, 6), (-1, 0, 0), (2 ** 31 - 1, 0, 0), (-2 ** 31, 3, 3)]
    want = ref.labels_at(lab, q)
    inside = ((q >= 0) & (q < (9, 7, 6))).all(1)
    assert inside[:2].all() and not inside[2:8].any() and not want[~inside].any()
    assert np.array_equal(want[inside], lab[q[inside, 2], q[inside, 1], q[inside, 0]])
    assert np.array_equal(capi.labels_at(lab, q), want)           # needs no GPU
    assert len(capi.labels_at(lab, np.zeros((0, 3), np.int32))) == 0
    L = capi.lib()
    out = np.zeros(4, np.int32)
    one = np.zeros((4, 3), np.int32)
    assert L.sift3d_labels_at_points(None, 9, 7, 6, P(one), 4, P(out), 0, 0) == ERR_ARG
    assert b"sift3d_labels_at_points: bad argument" in L.sift3d_last_error()
    assert L.sift3d_labels_at_points(P(lab), 9, 0, 6, P(one), 4, P(out), 0, 0) == ERR_ARG
    assert L.sift3d_labels_at_points(P(lab), 1 << 11, 1 << 10, 1 << 10, P(one), 4, P(out), 0, 0) == ERR_ARG
    assert L.sift3d_labels_at_points(P(lab), 9, 7, 6, None, 4, P(out), 0, 0) == ERR_ARG
    assert L.sift3d_labels_at_points(P(lab), 9, 7, 6, P(one), 4, None, 0, 0) == ERR_ARG
    assert L.sift3d_labels_at_points(P(lab), 9, 7, 6, P(one), -1, P(out), 0, 0) == ERR_ARG
    if capi.device_count() == 0:
        assert L.sift3d_labels_at_points(P(lab), 9, 7, 6, P(one), 4, P(out), 1, 0) == ERR_NO_DEVICE


# ---- the C++ shell -------------------------------------------------------------------------------------------------------------------

SHELL_PROGRAM = r"""
#include "Include/cRegistration.h"
#include <cstdio>
using namespace CPUSIFT;
int main() {
	// host only: the labels of three points of a 4 x 3 x 2 volume whose label is its linear index
	int lab[24];
	for (int i = 0; i < 24; i++) lab[i] = i;
	std::vector<Cvec> pts = {Cvec(1, 2, 1), Cvec(4, 0, 0), Cvec(3, 2, 1)};
	std::vector<int> at = LabelsAt(lab, 4, 3, 2, pts);
	if (at.size() != 3 || at[0] != 21 || at[1] != 0 || at[2] != 23) return 1;
	if (!LabelsAt(lab, 4, 3, 2, {Cvec(0.5f, 0, 0)}).empty()) return 2;
	// the calls that need a GPU: they must link, and a refused call reports itself and returns records of status -1
	unsigned char mask[8] = {1, 1, 1, 1, 1, 1, 1, 1};
	int labels[8], count = -1;
	const bool ok = LabelMask(mask, 2, 2, 2, 18, 1, labels, &count);   // 18-connectivity: refused before any device call
	if (ok) return 3;
	std::vector<IcgnResult> disp(3);
	std::vector<Icgn2Result> disp2(3);
	std::vector<int> labs = {1, 1}, qlabs = {1};                       // two labels for three points: refused by the shell
	std::vector<unsigned char> keep(3, 1);
	std::vector<StrainResult> s = ComputeStrains(pts, disp, labs), s2 = ComputeStrains(pts, disp2, labs, &keep);
	std::vector<ValidationResult> v = ValidateDisplacements(pts, disp, labs), v2 = ValidateDisplacements(pts, disp2, labs);
	std::vector<FieldResult> f = EvaluateField(pts, disp, labs, std::vector<double>{1.0, 1.0, 1.0}, qlabs);
	if (s.size() != 3 || s2.size() != 3 || v.size() != 3 || v2.size() != 3 || f.size() != 1) return 4;
	if (s[0].status != -1 || s2[0].status != -1 || v[0].status != -1 || v2[0].status != -1 || f[0].status != -1) return 5;
	printf("ok\n");
	return 0;
}
"""


def test_shell_declarations_link():
    subprocess.check_call(["make", "-C", CSRC, "-j8"], stdout=subprocess.DEVNULL)
    subprocess.check_call(["make", "-C", os.path.join(PKG, "host")], stdout=subprocess.DEVNULL)
    with tempfile.TemporaryDirectory() as t:
        src, exe = os.path.join(t, "labels.cpp"), os.path.join(t, "labels")
        open(src, "w").write(SHELL_PROGRAM)
        subprocess.check_call(["g++", "-std=c++14", "-Wall", "-I" + os.path.join(PKG, "host"), "-o", exe, src, "-L" + PKG, "-lsift3d",
                               "-lsift3d_hip", "-Wl,-rpath," + PKG])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stdout[-1000:], r.stderr[-2000:])
    assert "LabelMask" in r.stderr and "labels for 3 points" in r.stderr
