"""GPU tests of the distance transform (sift3d_mask_distance, sift3d_mask_from_distance, sift3d_distance_at_points) against the NumPy
restatement (tests/split_ref.py): dist2 is EQUAL for both border values on every mask of tests/label_cases.py (placed by the label
tile's extents), on the plain shapes (all out, all in, one out-voxel in a corner, one in-voxel), on shapes whose long axis exceeds what
a workgroup stages on each axis in turn, and on extents around the 64-bit ballot words along x; other byte values and bool masks; host
and device pointers and two calls return the same bytes; the erosion and the look-up at points are NumPy's."""
import importlib

import numpy as np
import pytest

import split_cases as cases
import split_ref as ref

pytestmark = pytest.mark.gpu

capi = importlib.import_module("3dsift_amd.capi")


def agree(got, want, what):
    assert got.dtype == np.int32 and got.shape == want.shape
    bad = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
    assert not len(bad), (what, len(bad), bad[:8].tolist(), got.reshape(-1)[bad[:8]].tolist(), want.reshape(-1)[bad[:8]].tolist())


@pytest.mark.parametrize("border", (0, 1))
@pytest.mark.parametrize("name", cases.edt_names())
def test_equals_restatement(name, border):
    got, seconds = capi.mask_distance(cases.edt_mask(name), border, with_seconds=True)
    assert seconds > 0
    agree(got, cases.edt_reference(name, border), (name, border))


def test_bool_masks_and_other_byte_values():
    m = cases.edt_mask("random-0.6")
    for border in (0, 1):
        want = cases.edt_reference("random-0.6", border)
        agree(capi.mask_distance(m.astype(bool), border), want, "bool")
        agree(capi.mask_distance((m * 200).astype(np.uint8), border), want, "200")
        agree(capi.mask_distance(np.where(m, np.arange(m.size).reshape(m.shape) % 255 + 1, 0).astype(np.uint8), border), want, "1..255")


DEVICE_CASES = ("all-out", "all-in", "one-out-corner", "long-y", "two-runs", "x-65", "random-0.6", "packing")


@pytest.mark.parametrize("border", (0, 1))
def test_device_pointers_repeatability_erosion_and_points(border):
    import torch

    for name in DEVICE_CASES:
        m = cases.edt_mask(name)
        want = cases.edt_reference(name, border)
        d = torch.from_numpy(np.array(m)).cuda()
        dist = capi.mask_distance(d, border)
        assert dist.is_cuda and dist.dtype == torch.int32 and tuple(dist.shape) == m.shape
        first = dist.cpu().numpy()
        agree(first, want, (name, border, "device"))
        assert first.tobytes() == capi.mask_distance(d, border).cpu().numpy().tobytes()
        assert first.tobytes() == capi.mask_distance(m, border).tobytes()
        for level2 in (1, 2, 9, ref.NONE):
            eroded = capi.mask_from_distance(dist, level2)
            assert eroded.is_cuda and eroded.dtype == torch.uint8
            assert np.array_equal(eroded.cpu().numpy(), ref.mask_from_distance(want, level2)), (name, level2)
            assert np.array_equal(capi.mask_from_distance(first, level2), ref.mask_from_distance(want, level2))
        assert np.array_equal(capi.mask_from_distance(first, 1), (m != 0).astype(np.uint8))   # erosion by nothing
        rng = np.random.default_rng(7)
        q = np.stack([rng.integers(-2, s + 2, 300) for s in m.shape[::-1]], 1).astype(np.int32)
        at = capi.distance_at(dist, torch.from_numpy(q).cuda())
        assert np.array_equal(at, ref.distance_at(want, q)) and np.array_equal(at, capi.distance_at(first, q))
