"""-m gpu: the schedule of a whole-volume run (context.hip plan_run -> RunPlan, read back through sift3d_test_run_plan) and its results.

Per case: (a) the plan equals the row of EXPECT below, (b) extrema, keypoint and descriptor bytes equal those of the same variant under
the one_stream hook (the serial schedule), (c) for the default variant the results equal the CPU oracle, compared as
test_detect_tail.py compares them.

Where EXPECT comes from: NOT from the code under test.  The stream of every head and tail, the moved tail, the small launch (first
octave, padded half width, level masks), the flags of the run and the detection values were printed by the commit BEFORE the RunPlan
existed, from the variables of its run_enqueue (prints added to a scratch copy, one run per case).  Wave priority and slot plan are
written out by hand from that commit's formula in smooth_level (octave 0: priority 0, no plan for the head, 512 slots for the tail;
octaves >= 1 of a volume with several octaves: priority 2, 256 slots): that commit never evaluated it for the octaves of the small launch.

Not covered: a volume of more than eight octaves (2048 voxels along its shortest axis) keeps octave 0's own scan and emit launch in
front of the others' (emit = 1), more than nine keep every octave's.  No test-sized volume reaches that, and nothing here pretends to."""
import contextlib
import importlib

import numpy as np
import pytest

from hipcheck import compare_keypoints, extrema_table

pytestmark = pytest.mark.gpu

SHAPES = {"16": (16, 16, 16), "32": (32, 32, 32), "64": (64, 64, 64), "96x80x72": (96, 80, 72), "128": (128, 128, 128), "168": (168, 168, 168)}
OCTAVES = {"16": 2, "32": 3, "64": 4, "96x80x72": 4, "128": 5, "168": 5}

# (shape, variant): (first octave of the small launch, chain stream, (padded half width, built levels, written DoG levels) of that launch,
#                    (dog_elide, g_last_elide, run_full, run_refine), (det_two, det_early, det_rest_stream, det_rest_own, emit),
#                    per octave (head stream, tail stream, tail moved)); stream -1 = the chain stream
EXPECT = {
    ("16", "default"): (0, 1, (6, 30, 14), (1, 1, 0, 0), (1, 1, 1, 0, 2), [(0, 0, 0), (-1, -1, 0)]),
    ("16", "one_stream"): (0, 0, (6, 30, 14), (1, 1, 0, 0), (0, 0, 0, 0, 0), [(0, 0, 0), (0, 0, 0)]),
    ("16", "det_serial"): (0, 1, (6, 30, 14), (1, 1, 0, 0), (0, 0, 0, 0, 0), [(0, 0, 0), (-1, -1, 0)]),
    ("16", "separable"): (-1, 1, (0, 0, 0), (1, 0, 0, 0), (1, 1, 1, 0, 2), [(0, 0, 0), (-1, 1, 0)]),
    ("16", "dog_eager"): (-1, 1, (0, 0, 0), (0, 0, 0, 0), (1, 1, 1, 0, 2), [(0, 0, 0), (-1, 1, 0)]),
    ("16", "glast_eager"): (-1, 1, (0, 0, 0), (1, 0, 0, 0), (1, 1, 1, 0, 2), [(0, 0, 0), (-1, 1, 0)]),
    ("32", "default"): (1, 1, (6, 30, 14), (1, 1, 0, 0), (1, 1, 2, 1, 2), [(0, 0, 0), (-1, -1, 0), (-1, -1, 0)]),
    ("32", "one_stream"): (1, 0, (6, 30, 14), (1, 1, 0, 0), (0, 0, 0, 0, 0), [(0, 0, 0), (1, 1, 0), (1, 1, 0)]),
    ("32", "det_serial"): (1, 1, (6, 30, 14), (1, 1, 0, 0), (0, 0, 0, 0, 0), [(0, 0, 0), (-1, -1, 0), (-1, -1, 0)]),
    ("32", "separable"): (-1, 1, (0, 0, 0), (1, 0, 0, 0), (1, 1, 2, 1, 2), [(0, 0, 0), (-1, 1, 0), (-1, 2, 0)]),
    ("32", "dog_eager"): (-1, 1, (0, 0, 0), (0, 0, 0, 0), (1, 1, 2, 1, 2), [(0, 0, 0), (-1, 1, 0), (-1, 2, 0)]),
    ("32", "glast_eager"): (-1, 1, (0, 0, 0), (1, 0, 0, 0), (1, 1, 2, 1, 2), [(0, 0, 0), (-1, 1, 0), (-1, 2, 0)]),
    ("64", "default"): (2, 1, (6, 30, 14), (1, 1, 0, 0), (1, 1, 2, 1, 2), [(0, 0, 0), (-1, 1, 0), (-1, -1, 0), (-1, -1, 0)]),
    ("64", "one_stream"): (2, 0, (6, 30, 14), (1, 1, 0, 0), (0, 0, 0, 0, 0), [(0, 0, 0), (1, 1, 0), (2, 2, 0), (2, 2, 0)]),
    ("64", "det_serial"): (2, 1, (6, 30, 14), (1, 1, 0, 0), (0, 0, 0, 0, 0), [(0, 0, 0), (-1, 1, 0), (-1, -1, 0), (-1, -1, 0)]),
    ("64", "separable"): (-1, 1, (0, 0, 0), (1, 0, 0, 0), (1, 1, 2, 1, 2), [(0, 0, 0), (-1, 1, 0), (-1, 2, 0), (-1, 3, 0)]),
    ("64", "dog_eager"): (-1, 1, (0, 0, 0), (0, 0, 0, 0), (1, 1, 2, 1, 2), [(0, 0, 0), (-1, 1, 0), (-1, 2, 0), (-1, 3, 0)]),
    ("64", "glast_eager"): (-1, 1, (0, 0, 0), (1, 0, 0, 0), (1, 1, 2, 1, 2), [(0, 0, 0), (-1, 1, 0), (-1, 2, 0), (-1, 3, 0)]),
    ("64", "neighbours80"): (-1, 1, (0, 0, 0), (0, 0, 1, 0), (1, 1, 2, 1, 2), [(0, 0, 0), (-1, 1, 0), (-1, 2, 0), (-1, 3, 0)]),
    ("64", "refine"): (-1, 1, (0, 0, 0), (0, 0, 1, 1), (1, 1, 2, 1, 2), [(0, 0, 0), (-1, 1, 0), (-1, 2, 0), (-1, 3, 0)]),
    ("64", "sigma1.7"): (-1, 1, (0, 0, 0), (1, 1, 0, 0), (1, 1, 2, 1, 2), [(0, 0, 0), (-1, 1, 0), (-1, 2, 0), (-1, 3, 0)]),
    ("64", "list_cap"): (2, 1, (6, 30, 14), (1, 1, 0, 0), (1, 1, 2, 1, 2), [(0, 0, 0), (-1, 1, 0), (-1, -1, 0), (-1, -1, 0)]),
    ("96x80x72", "default"): (3, 1, (6, 30, 14), (1, 1, 0, 0), (1, 1, 2, 1, 2), [(0, 0, 0), (-1, 1, 0), (-1, 2, 0), (-1, -1, 0)]),
    ("96x80x72", "one_stream"): (3, 0, (6, 30, 14), (1, 1, 0, 0), (0, 0, 0, 0, 0), [(0, 0, 0), (1, 1, 0), (2, 1, 1), (3, 3, 0)]),
    ("96x80x72", "det_serial"): (3, 1, (6, 30, 14), (1, 1, 0, 0), (0, 0, 0, 0, 0), [(0, 0, 0), (-1, 1, 0), (-1, 2, 0), (-1, -1, 0)]),
    ("96x80x72", "separable"): (-1, 1, (0, 0, 0), (1, 0, 0, 0), (1, 1, 2, 1, 2), [(0, 0, 0), (-1, 1, 0), (-1, 2, 0), (-1, 3, 0)]),
    ("96x80x72", "dog_eager"): (-1, 1, (0, 0, 0), (0, 0, 0, 0), (1, 1, 2, 1, 2), [(0, 0, 0), (-1, 1, 0), (-1, 2, 0), (-1, 3, 0)]),
    ("96x80x72", "glast_eager"): (-1, 1, (0, 0, 0), (1, 0, 0, 0), (1, 1, 2, 1, 2), [(0, 0, 0), (-1, 1, 0), (-1, 2, 0), (-1, 3, 0)]),
    ("128", "default"): (3, 1, (6, 30, 14), (1, 1, 0, 0), (1, 1, 2, 1, 2), [(0, 0, 0), (-1, 1, 0), (-1, 2, 0), (-1, -1, 0), (-1, -1, 0)]),
    ("128", "one_stream"): (3, 0, (6, 30, 14), (1, 1, 0, 0), (0, 0, 0, 0, 0), [(0, 0, 0), (1, 1, 0), (2, 1, 1), (3, 3, 0), (3, 3, 0)]),
    ("128", "det_serial"): (3, 1, (6, 30, 14), (1, 1, 0, 0), (0, 0, 0, 0, 0), [(0, 0, 0), (-1, 1, 0), (-1, 2, 0), (-1, -1, 0), (-1, -1, 0)]),
    ("128", "separable"): (-1, 1, (0, 0, 0), (1, 0, 0, 0), (1, 1, 2, 1, 2), [(0, 0, 0), (-1, 1, 0), (-1, 2, 0), (-1, 3, 0), (-1, 4, 0)]),
    ("128", "dog_eager"): (-1, 1, (0, 0, 0), (0, 0, 0, 0), (1, 1, 2, 1, 2), [(0, 0, 0), (-1, 1, 0), (-1, 2, 0), (-1, 3, 0), (-1, 4, 0)]),
    ("128", "glast_eager"): (-1, 1, (0, 0, 0), (1, 0, 0, 0), (1, 1, 2, 1, 2), [(0, 0, 0), (-1, 1, 0), (-1, 2, 0), (-1, 3, 0), (-1, 4, 0)]),
    ("128", "neighbours80"): (-1, 1, (0, 0, 0), (0, 0, 1, 0), (1, 1, 2, 1, 2), [(0, 0, 0), (-1, 1, 0), (-1, 2, 0), (-1, 3, 0), (-1, 4, 0)]),
    ("128", "refine"): (-1, 1, (0, 0, 0), (0, 0, 1, 1), (1, 1, 2, 1, 2), [(0, 0, 0), (-1, 1, 0), (-1, 2, 0), (-1, 3, 0), (-1, 4, 0)]),
    ("128", "sigma1.7"): (-1, 1, (0, 0, 0), (1, 1, 0, 0), (1, 1, 2, 1, 2), [(0, 0, 0), (-1, 1, 0), (-1, 2, 0), (-1, 3, 0), (-1, 4, 0)]),
    ("128", "list_cap"): (3, 1, (6, 30, 14), (1, 1, 0, 0), (1, 1, 2, 1, 2), [(0, 0, 0), (-1, 1, 0), (-1, 2, 0), (-1, -1, 0), (-1, -1, 0)]),
    ("168", "default"): (4, 0, (6, 30, 14), (1, 1, 0, 0), (1, 1, 2, 1, 2), [(0, 0, 0), (1, 1, 0), (2, 2, 0), (3, 2, 1), (4, 4, 0)]),
    ("168", "one_stream"): (4, 0, (6, 30, 14), (1, 1, 0, 0), (0, 0, 0, 0, 0), [(0, 0, 0), (1, 1, 0), (2, 2, 0), (3, 2, 1), (4, 4, 0)]),
    ("168", "det_serial"): (4, 0, (6, 30, 14), (1, 1, 0, 0), (0, 0, 0, 0, 0), [(0, 0, 0), (1, 1, 0), (2, 2, 0), (3, 2, 1), (4, 4, 0)]),
    ("168", "separable"): (-1, 0, (0, 0, 0), (1, 0, 0, 0), (1, 1, 2, 1, 2), [(0, 0, 0), (1, 1, 0), (2, 2, 0), (3, 3, 0), (4, 4, 0)]),
    ("168", "dog_eager"): (4, 0, (8, 62, 31), (0, 0, 0, 0), (1, 1, 2, 1, 2), [(0, 0, 0), (1, 1, 0), (2, 2, 0), (3, 2, 1), (4, 4, 0)]),
    ("168", "glast_eager"): (4, 0, (8, 62, 14), (1, 0, 0, 0), (1, 1, 2, 1, 2), [(0, 0, 0), (1, 1, 0), (2, 2, 0), (3, 2, 1), (4, 4, 0)]),
}
HOOK_VARIANTS = ("one_stream", "det_serial", "separable", "dog_eager", "glast_eager")
LIST_CAP = 48  # every list_cap shape has more extrema than this (asserted): the first enqueue overflows, the lists are regrown, the run enqueued again


def expected_plan(shape, variant):
    small_first, chain, small, flags, det, streams = EXPECT[(shape, variant)]
    n = OCTAVES[shape]
    assert len(streams) == n
    keys = ["noct", "small_first", "chain", "small_hwp", "small_build_mask", "small_dog_mask", "dog_elide", "g_last_elide", "run_full",
            "run_refine", "det_two", "det_early", "det_rest_stream", "det_rest_own", "emit"]
    plan = dict(zip(keys, (n, small_first, chain) + small + flags + det))
    # (every shape here has several octaves)
    plan["octaves"] = [(h, t, m, 0 if o == 0 else 2, 0 if o == 0 else 256, 512 if o == 0 else 256) for o, (h, t, m) in enumerate(streams)]
    return plan


@pytest.fixture(scope="module")
def capi():
    m = importlib.import_module("3dsift_amd.capi")
    assert m.device_count() >= 1, "GPU tests need a visible MI355X (no CPU fallback exists)"
    return m


@pytest.fixture(scope="module")
def volumes(synth):
    out = {}

    def get(shape):
        if shape not in out:
            out[shape] = synth.blobs(SHAPES[shape], seed=11, noise=0.02)
            out[shape].setflags(write=False)
        return out[shape]

    return get


def result_bytes(g):
    kp, desc = g.GetKeypoints()
    return g.extrema().tobytes(), kp.tobytes(), desc.tobytes()


def run_variant(capi, vol, variant, serial=False, cap=True):
    """the extractor of a variant after its run; serial: under the one_stream hook as well; cap=False: the list_cap variant without its cap"""
    with contextlib.ExitStack() as hooks:
        if serial:
            hooks.enter_context(capi.hook("one_stream", 1))
        if variant in HOOK_VARIANTS:
            hooks.enter_context(capi.hook(variant, 1))
        if variant == "list_cap" and cap:
            hooks.enter_context(capi.hook("list_cap", LIST_CAP))
        g = capi.CSIFT3D(vol, sigma_default=1.7) if variant == "sigma1.7" else capi.CSIFT3D(vol)
        if variant == "neighbours80":
            g.set_detect_options(neighbours=80)
        if variant == "refine":
            g.set_detect_options(refine=True)
        return g.KpSiftAlgorithm()


@pytest.mark.parametrize("shape,variant", list(EXPECT), ids=[f"{s}-{v}" for s, v in EXPECT])
def test_plan_and_results(capi, orc, volumes, shape, variant):
    vol = volumes(shape)
    g = run_variant(capi, vol, variant)
    assert g.num_octaves == OCTAVES[shape]
    assert g.run_plan() == expected_plan(shape, variant)  # (a)
    got = result_bytes(g)
    serial = run_variant(capi, vol, variant, serial=True)
    assert serial.run_plan()["det_two"] == 0 and serial.run_plan()["chain"] == 0
    assert got == result_bytes(serial)  # (b)
    if variant == "default":  # (c)
        o = orc.extractor(vol).run(5)
        assert o.num_octaves == OCTAVES[shape]
        assert np.array_equal(extrema_table(g.extrema()), extrema_table(o.extrema()))
        kp, desc = g.GetKeypoints()
        compare_keypoints(kp, desc, *o.keypoints())
    if variant == "list_cap":
        assert len(g.extrema()) > LIST_CAP and g.debug_counters()["list_regrows"] >= 1
        assert got == result_bytes(run_variant(capi, vol, variant, cap=False))


@pytest.mark.parametrize("shape", ["64", "128"])
def test_plan_is_unchanged_across_a_regrow(capi, volumes, shape):
    """the plan read between the first enqueue and the wait that finds the overflow, regrows the lists and enqueues again, and behind it"""
    with capi.hook("list_cap", LIST_CAP):
        g = capi.CSIFT3D(volumes(shape)).KpSiftAlgorithmAsync()
        before = g.run_plan()
        g.Wait()
    assert g.debug_counters()["list_regrows"] >= 1
    assert before == g.run_plan() == expected_plan(shape, "list_cap")


def test_cases_cover_every_situation():
    """the shape list cannot silently stop covering a branch of the planning (every row is asserted against the library above)"""
    rows = [expected_plan(s, v) for s, v in EXPECT]
    for s in SHAPES:
        assert {v for ss, v in EXPECT if ss == s} >= {"default", *HOOK_VARIANTS}
    for s in ("64", "128"):
        assert {v for ss, v in EXPECT if ss == s} >= {"neighbours80", "refine", "sigma1.7", "list_cap"}
    assert any(p["small_first"] == 0 for p in rows), "small launch starting at octave 0"
    assert any(p["small_first"] >= 1 for p in rows), "small launch starting at an octave >= 1"
    assert any(p["small_first"] == -1 for p in rows), "no small launch"
    assert any(p["chain"] == 1 and any(o[0] == -1 for o in p["octaves"]) for p in rows), "chain stream used"
    assert any(p["chain"] == 0 and p["det_two"] == 1 for p in rows), "chain stream absent (not by the one_stream hook)"
    assert any(o[2] == 1 and o[1] == i - 1 for p in rows if p["det_two"] for i, o in enumerate(p["octaves"])), "tail moved"
    assert any(p["det_early"] == 1 and p["det_rest_stream"] == 2 and p["det_rest_own"] == 1 for p in rows), "early masks with a third stream"
    assert any(p["det_two"] == 0 and p["det_rest_stream"] == 0 for p in rows), "single detection stream"
    assert expected_plan("64", "sigma1.7")["small_first"] == -1 and expected_plan("64", "default")["small_first"] == 2
    assert expected_plan("168", "default")["small_first"] >= 3 and expected_plan("168", "default")["chain"] == 0
