"""-m gpu: the tail of the extrema stage (context.hip run_enqueue, kernels_detect.hip launch_detect_mark / launch_detect_emit_multi).

The candidate chains of octave 0, octave 1 and the octaves >= 2 run on three streams that the main stream joins (it waits for both
of the others itself), the candidate kernels' grids are sized to the octave, and ONE scan + ONE emit launch compact every octave
(octave 0 included) into the ordered extrema list.  None of this may change a result: extrema (order included), keypoints and
descriptors are compared with the CPU oracle field by field, as the detection tests of test_gpu_parity.py compare them, and run
against run byte for byte.

Shapes: 64^3 (4 octaves: the smallest volume whose octaves >= 2 take the third stream), 96 x 80 x 72 (non-cubic, not tile-aligned),
128^3 (5 octaves: the 16^3 and 8^3 octaves are single-workgroup launches of every detection kernel).

Not covered: a volume of more than eight octaves (2048 voxels along its shortest axis) keeps octave 0's own scan and emit launch in
front of the others'.  No test-sized volume reaches that branch, and nothing here pretends to."""
import importlib

import numpy as np
import pytest

from detect_full_ref import extrema_mask
from hipcheck import compare_keypoints, extrema_table

pytestmark = pytest.mark.gpu

SHAPES = {"64": ((64, 64, 64), 1234, 0.0), "96x80x72": ((96, 80, 72), 5, 0.02), "128": ((128, 128, 128), 21, 0.01)}


@pytest.fixture(scope="module")
def capi():
    m = importlib.import_module("3dsift_amd.capi")
    assert m.device_count() >= 1, "GPU tests need a visible MI355X (no CPU fallback exists)"
    return m


@pytest.fixture(scope="module")
def cases(orc, synth):
    """volume and oracle results per shape, computed once and only read by the tests"""
    out = {}

    def get(name):
        if name not in out:
            if name == "corner":
                # a 48^3 block of blobs in one corner of a constant 128^3 volume: what the block leaves in the 32^3, 16^3 and 8^3 octaves
                # passes the peak threshold nowhere on the last keypoint level, so these octaves park NOTHING (asserted below)
                vol = np.zeros((128, 128, 128), np.float32)
                vol[:48, :48, :48] = synth.blobs((48, 48, 48), seed=3, noise=0.02)
            else:
                shape, seed, noise = SHAPES[name]
                vol = synth.blobs(shape, seed=seed, noise=noise)
            vol.setflags(write=False)
            o = orc.extractor(vol).run(5)
            out[name] = (vol, o, extrema_table(o.extrema()), o.keypoints())
        return out[name]

    return get


def parked_per_octave(o, peak_thresh=0.1):
    """voxels of the last keypoint level that pass every test but the one against the level above (what k_mark parks for the lazy
    kernels), per octave, from the oracle's DoG levels"""
    out = []
    for oc in range(o.num_octaves):
        prev, cur = o.dog(oc, 2), o.dog(oc, 3)
        as_max = extrema_mask(prev, cur, np.full_like(cur, -np.inf), peak_thresh, 8)
        as_min = extrema_mask(prev, cur, np.full_like(cur, np.inf), peak_thresh, 8)
        out.append(int((as_max | as_min).sum()))
    return out


def check_against_oracle(g, case):
    _, _, oext, (okp, odesc) = case
    assert np.array_equal(extrema_table(g.extrema()), oext)
    kp, desc = g.GetKeypoints()
    compare_keypoints(kp, desc, okp, odesc)


def result_bytes(g):
    kp, desc = g.GetKeypoints()
    return g.extrema().tobytes(), kp.tobytes(), desc.tobytes()


@pytest.mark.parametrize("name", list(SHAPES))
def test_extrema_and_keypoints_equal_the_oracle(capi, cases, name):
    case = cases(name)
    g = capi.CreateCSIFT3D(case[0]).KpSiftAlgorithm()
    assert g.num_octaves == case[1].num_octaves == {"64": 4, "96x80x72": 4, "128": 5}[name]
    assert len(case[2]) > 20 and len(np.unique(case[2][:, 0])) >= 3, "extrema in at least three octaves"
    check_against_oracle(g, case)


def test_repeat_runs_with_a_second_handle_in_flight(capi, cases):
    """20 runs on one handle, 5 asynchronous runs on a second one in flight beside them: every run gives the first run's extrema list
    and descriptor bytes (a missing join between the detection streams lets the scan read counts that are still being written)"""
    case = cases("128")
    a, b = capi.CreateCSIFT3D(case[0]), capi.CreateCSIFT3D(case[0])
    first = None
    nb = 0
    for i in range(20):
        flying = i % 4 == 0 and nb < 5
        if flying:
            b.KpSiftAlgorithmAsync()
            nb += 1
        a.KpSiftAlgorithm()
        ra = result_bytes(a)
        if first is None:
            first = ra
            check_against_oracle(a, case)
        assert ra == first, ("first handle, run", i)
        if flying:
            b.Wait()
            assert result_bytes(b) == first, ("second handle, run", nb)
    assert nb == 5


def test_octaves_that_park_nothing(capi, cases):
    """an empty parked list under a reduced grid: the lazy kernels of the octaves >= 2 read a count of zero and leave"""
    case = cases("corner")
    parked = parked_per_octave(case[1])
    assert len(parked) == 5 and parked[0] > 0 and parked[1] > 0 and parked[2:] == [0, 0, 0], parked
    assert len(case[2]) > 20
    check_against_oracle(capi.CreateCSIFT3D(case[0]).KpSiftAlgorithm(), case)


@pytest.mark.parametrize("hook", ["lazy_generic", "one_stream"])
def test_hooks_equal_the_default(capi, cases, hook):
    """lazy_generic: every parked candidate down the workgroup form (its grid is sized to the octave too); one_stream: every chain on
    the handle's stream (no extra detection stream is created)"""
    case = cases("128")
    base = result_bytes(capi.CreateCSIFT3D(case[0]).KpSiftAlgorithm())
    with capi.hook(hook, 1):
        g = capi.CreateCSIFT3D(case[0]).KpSiftAlgorithm()
        got = result_bytes(g)
    assert got == base
    check_against_oracle(g, case)
