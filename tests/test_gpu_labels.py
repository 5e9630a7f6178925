"""GPU tests of the connected-component labels (sift3d_mask_label, sift3d_labels_at_points) against the NumPy restatement
(tests/label_ref.py) on the masks of tests/label_cases.py: labels and count are EQUAL on every mask at both connectivities and for
the min_voxels cuts, through host and through device pointers; two calls return the same bytes; a far-away component changes only
its own voxels and the numbers behind it.  The masks are placed by the extents of the kernel's LDS tile (every extent around it on
every axis, contacts through faces, edges and corners across the seams), and hold a path of 1500 voxels and masks at both
percolation thresholds, where a merge that stops after a fixed number of hops fails."""
import importlib

import numpy as np
import pytest

import label_cases as cases
import label_ref as ref

pytestmark = pytest.mark.gpu

capi = importlib.import_module("3dsift_amd.capi")
CONNECTIVITIES = (6, 26)


def agree(got, count, want, n, what):
    assert got.dtype == np.int32 and got.shape == want.shape
    assert count == n, (what, count, n)
    bad = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
    assert not len(bad), (what, len(bad), bad[:8].tolist(), got.reshape(-1)[bad[:8]].tolist(), want.reshape(-1)[bad[:8]].tolist())


@pytest.mark.parametrize("connectivity", CONNECTIVITIES)
@pytest.mark.parametrize("name", sorted(cases.MASKS))
def test_equals_restatement(name, connectivity):
    got, count, seconds = capi.mask_label(cases.get(name), connectivity, with_seconds=True)
    assert seconds > 0
    agree(got, count, *cases.reference(name, connectivity), (name, connectivity))


def test_min_voxels_cuts():
    for name, connectivity, cut in cases.size_cuts():
        got, count = capi.mask_label(cases.get(name), connectivity, min_voxels=cut)
        agree(got, count, *cases.reference(name, connectivity, cut), (name, connectivity, cut))
    # a cut above every size: nothing is kept
    got, count = capi.mask_label(cases.get("random-0.10"), 6, min_voxels=2 ** 31 - 1)
    assert count == 0 and not got.any()


def test_bool_masks_and_other_byte_values():
    m = cases.get("random-0.25")
    want = cases.reference("random-0.25", 26)
    agree(*capi.mask_label(m.astype(bool), 26), *want, "bool")
    agree(*capi.mask_label((m * 200).astype(np.uint8), 26), *want, "200")


DEVICE_CASES = ("zero", "full", "serpentine", "seam-corner", "u-shape", "extent-x-2T+1", "random-0.3116", "random-0.10")


@pytest.mark.parametrize("connectivity", CONNECTIVITIES)
def test_device_pointers_and_repeatability(connectivity):
    import torch

    for name in DEVICE_CASES:
        m = cases.get(name)
        want, n = cases.reference(name, connectivity)
        d = torch.from_numpy(np.array(m)).cuda()
        lab, count = capi.mask_label(d, connectivity)
        assert lab.is_cuda and lab.dtype == torch.int32 and tuple(lab.shape) == m.shape
        again, count2 = capi.mask_label(d, connectivity)
        first = lab.cpu().numpy()
        agree(first, count, want, n, (name, connectivity, "device"))
        assert count2 == count and first.tobytes() == again.cpu().numpy().tobytes()
        host, count3 = capi.mask_label(m, connectivity)
        assert count3 == count and host.tobytes() == first.tobytes()
        # the labels at points, on the device and on the host
        rng = np.random.default_rng(7)
        q = np.stack([rng.integers(-2, s + 2, 300) for s in m.shape[::-1]], 1).astype(np.int32)
        at = capi.labels_at(lab, torch.from_numpy(q).cuda())
        assert np.array_equal(at, ref.labels_at(want, q)) and np.array_equal(at, capi.labels_at(first, q))


def test_a_far_component_changes_only_its_own_voxels_and_the_numbers_behind_it():
    base = np.array(cases.get("random-0.3116"))
    nz, ny, nx = base.shape
    base[nz // 2 - 2:nz // 2 + 3, ny // 2 - 2:ny // 2 + 3, nx // 2 - 2:nx // 2 + 3] = 0   # a hole of 5^3 voxels ...
    more = base.copy()
    more[nz // 2, ny // 2, nx // 2] = 1                                                   # ... and a voxel in it that touches nothing
    for connectivity in CONNECTIVITIES:
        a, na = capi.mask_label(base, connectivity)
        b, nb = capi.mask_label(more, connectivity)
        k = int(b[nz // 2, ny // 2, nx // 2])
        assert nb == na + 1 and 1 < k < nb
        shifted = np.where(a >= k, a + 1, a)
        shifted[nz // 2, ny // 2, nx // 2] = k
        assert np.array_equal(b, shifted)
        agree(b, nb, *ref.label(more, connectivity), ("far", connectivity))
