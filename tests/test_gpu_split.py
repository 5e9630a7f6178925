"""GPU tests of the labels of touching bodies (sift3d_mask_split) against the NumPy restatement (tests/split_ref.py): labels, count and
info are EQUAL on the three scenes at both connectivities, on a packing of overlapping balls, on the percolation masks of
tests/label_cases.py, under max_rounds and under the two size cuts; with core_dist2 = 1 the call returns capi.mask_label's bytes; host
and device pointers and two calls return the same bytes; the dist2 output is capi.mask_distance's; and on scene A the split labels let
fit_rigid_bodies recover both grains' rotations where the single component's fit cannot."""
import importlib

import numpy as np
import pytest

import body_cases
import label_cases
import split_cases as cases

pytestmark = pytest.mark.gpu

capi = importlib.import_module("3dsift_amd.capi")
CONNECTIVITIES = (6, 26)


def agree(got, want, what):
    lab, count, info = got[:3]
    wlab, wcount, winfo = want[:3]
    assert lab.dtype == np.int32 and lab.shape == wlab.shape
    assert (count, info) == (wcount, winfo), (what, count, info, wcount, winfo)
    bad = np.flatnonzero(lab.reshape(-1) != wlab.reshape(-1))
    assert not len(bad), (what, len(bad), bad[:8].tolist(), lab.reshape(-1)[bad[:8]].tolist(), wlab.reshape(-1)[bad[:8]].tolist())


SCENE_OPTS = {"A": cases.A_OPTS, "B": {"core_dist2": 30}, "C": cases.A_OPTS}


@pytest.mark.parametrize("connectivity", CONNECTIVITIES)
@pytest.mark.parametrize("name", sorted(SCENE_OPTS))
def test_scenes_equal_restatement(name, connectivity):
    o = dict(SCENE_OPTS[name], connectivity=connectivity)
    lab, count, info, dist, seconds = capi.mask_split(cases.scene(name), return_distance=True, with_seconds=True, **o)
    assert seconds > 0
    agree((lab, count, info), cases.split(name, **o), (name, o))
    assert dist.tobytes() == capi.mask_distance(cases.scene(name), o["border"] if "border" in o else 1).tobytes()
    assert np.array_equal(dist, cases.split(name, **o)[3])
    if name == "C":
        o["keep_unreached"] = 0
        agree(capi.mask_split(cases.scene(name), **o), cases.split(name, **o), (name, o))
    if name == "B":
        for core_dist2 in cases.B_CORE_DIST2:
            o["core_dist2"] = core_dist2
            agree(capi.mask_split(cases.scene(name), **o), cases.split(name, **o), (name, o))


@pytest.mark.parametrize("run", range(len(cases.SPLIT_RUNS)))
def test_runs_equal_restatement(run):
    name, o = cases.SPLIT_RUNS[run]
    agree(capi.mask_split(cases.scene(name), **o), cases.split(name, **o), (name, o))


@pytest.mark.parametrize("connectivity", CONNECTIVITIES)
def test_core_dist2_1_returns_mask_label(connectivity):
    for name in ("A", "packing", "random-0.3116", "random-0.10", "u-shape", "zero", "full"):
        m = cases.scene(name)
        for cut, keep in ((1, 1), (4, 0)):
            lab, count, info = capi.mask_split(m, core_dist2=1, connectivity=connectivity, min_core_voxels=cut, keep_unreached=keep)
            want, n = capi.mask_label(m, connectivity, min_voxels=cut)
            assert count == n and info["rounds"] == 0 and info["cores"] == n and info["unreached_bodies"] == 0
            assert lab.tobytes() == want.tobytes(), (name, connectivity, cut)
    want, n = label_cases.reference("random-0.3116", connectivity)
    assert n == capi.mask_split(cases.scene("random-0.3116"), core_dist2=1, connectivity=connectivity)[1]


DEVICE_RUNS = (("A", cases.A_OPTS), ("C", dict(cases.A_OPTS, connectivity=26)), ("packing", {"core_dist2": 16}),
               ("random-0.6", {"core_dist2": 3}), ("A", dict(cases.A_OPTS, max_rounds=3)), ("zero", {}), ("full", {"border": 0}))


def test_device_pointers_and_repeatability():
    import torch

    for name, o in DEVICE_RUNS:
        m = cases.scene(name)
        want = cases.split(name, **o)
        d = torch.from_numpy(np.array(m)).cuda()
        lab, count, info, dist = capi.mask_split(d, return_distance=True, **o)
        assert lab.is_cuda and lab.dtype == torch.int32 and tuple(lab.shape) == m.shape and dist.is_cuda and dist.dtype == torch.int32
        first = lab.cpu().numpy()
        agree((first, count, info), want, (name, o, "device"))
        assert np.array_equal(dist.cpu().numpy(), want[3])
        again = capi.mask_split(d, **o)                      # without the distance output
        assert again[1:] == (count, info) and again[0].cpu().numpy().tobytes() == first.tobytes()
        host = capi.mask_split(m, return_distance=True, **o)
        assert host[1:3] == (count, info) and host[0].tobytes() == first.tobytes() and host[3].tobytes() == dist.cpu().numpy().tobytes()
        assert dist.cpu().numpy().tobytes() == capi.mask_distance(d, o.get("border", 1)).cpu().numpy().tobytes()


def test_split_labels_recover_both_grains_motions():
    pairs = cases.grain_pairs()
    m = cases.scene("A")
    lab, count, info = capi.mask_split(m, **cases.A_OPTS)
    assert count == 2
    fits = capi.fit_rigid_bodies(pairs, capi.labels_at_positions(lab, pairs), count, iterations=body_cases.H, inlier_thresh=body_cases.TAU)
    errors = [(int(fits["status"][k]), cases.rotation_error(fits["A"][k], 0), cases.rotation_error(fits["A"][k], 1)) for k in range(2)]
    print(errors)
    assert errors[0][0] == 0 and errors[1][0] == 0
    assert errors[0][1] <= body_cases.ROT_BOUND and errors[1][2] <= body_cases.ROT_BOUND
    plain, n = capi.mask_label(m, 6)
    assert n == 1
    one = capi.fit_rigid_bodies(pairs, capi.labels_at_positions(plain, pairs), n, iterations=body_cases.H, inlier_thresh=body_cases.TAU)
    single = (cases.rotation_error(one["A"][0], 0), cases.rotation_error(one["A"][0], 1))
    print(single)
    assert max(single) > body_cases.ROT_BOUND   # one motion cannot be both
