"""GPU tests of the cubic B-spline path where a subtle error would pass tests/test_gpu_bspline.py (the cases: tests/bspline_cases.py;
what they claim about themselves is asserted on the restatement in tests/test_bspline_cpu.py).
A. sift3d_bspline_prefilter returns the bytes of bspline_ref.prefilter(T, f32=True) -- no tolerance -- at every seam of
k_bspline_axis' 64 x 64 tiles along each axis, at partial and single-line tiles of lines, on every axis length from 1 to 17 (mirrors
folded repeatedly) and with all seams at once.
B. sift3d_icgn_bspline through the battery of tests/test_gpu_icgn_edges.py: radii up to 32 with a spike on a sentinel voxel of the
walk, volumes with pairwise different dimensions, T's exact domain edges, non-finite voxels at the prefilter's reach, every status
and their order, exact invariances, large offsets, convergent runs, 70 000 POIs and scratch regrowth.  In every "agrees" test the GPU
is given the restatement's coefficients and is compared with tests/bspline_ref.py on the same coefficient bits, to
test_gpu_icgn_edges' bound: statuses and iteration counts equal, |d displacement| <= 1e-4, |d gradient| <= 1e-5, |d zncc| <= 1e-5;
once per group the volume path (prefilter inside the call) must return the coefficient path's bytes."""
import importlib

import numpy as np
import pytest

import bspline_cases as bc
import bspline_ref as bref
import icgn_ref as ref
import test_gpu_icgn_edges as ke
from test_gpu_icgn_edges import odd_volumes, spike_volume, status_scene, value_scene  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

capi = importlib.import_module("3dsift_amd.capi")


def gpu(c, volume=False):
    """a case on the GPU: given the restatement's coefficients, or (volume) T itself, prefiltered inside the call"""
    return capi.icgn_bspline(c["R"], c["T"] if volume else c["C"], c["q"], init=c["init"], coefficients=not volume, **c["opts"])


# ---- A. the prefilter: the fp32 restatement's bits ------------------------------------------------------------------------------------

def first_wrong_pass(T):
    """where the bytes differ: each axis pass alone, on a volume that repeats one line of T along the other two axes (the other two
    passes return such a volume unchanged: every difference they weight is exactly 0)"""
    h = bref.taps().astype(np.float32)
    out = []
    for axis in (2, 1, 0):
        idx = [0, 0, 0]
        idx[axis] = slice(None)
        shape = [1, 1, 1]
        shape[axis] = T.shape[axis]
        V = np.ascontiguousarray(np.broadcast_to(T[tuple(idx)].reshape(shape), T.shape))
        out.append(f"{'zyx'[axis]} pass alone: {bc.first_difference(capi.bspline_prefilter(V), bref.prefilter_axis(V, axis, h))}")
    return "; ".join(out)


SHAPES = bc.prefilter_shapes()


@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_prefilter_has_the_restatements_bytes(shape):
    for kind in bc.KINDS:
        T = bc.volume(shape, kind)
        want = bref.prefilter(T, f32=True)
        got = capi.bspline_prefilter(T)
        assert got.dtype == want.dtype and got.shape == want.shape
        if got.tobytes() != want.tobytes():
            pytest.fail(f"{shape} {kind}: {bc.first_difference(got, want)}; {first_wrong_pass(T)}")


# ---- B1. radii with sentinel spikes ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("r", bc.SPIKE_R)
def test_every_radius_with_sentinel_spikes(spike_volume, r):
    """one call per sentinel (every sentinel up to r = 16, the Keys test's four beyond); the sensitivity of each, >= 100 tolerances,
    is asserted in tests/test_bspline_cpu.py"""
    for k, (name, c, _, _) in enumerate(bc.spike_cases(spike_volume, r)):
        want = bc.restate(c)
        assert want["status"][0] == 1 and want["iterations"][0] == 2, (name, want["status"])
        got = gpu(c)
        ke.assert_agree(got, want, f"r={r} {name}")
        if k == 0:
            ke.equal_results(gpu(c, volume=True), got)


# ---- B2. axes, strides, sizes ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("r", bc.ODD_R)
def test_axes_strides_and_sizes(odd_volumes, r):
    c = bc.odd_case(odd_volumes, r)
    want = bc.restate(c)
    assert list(want["status"]) == bc.ODD_STATUS and list(want["iterations"]) == bc.ODD_ITERATIONS, (want["status"], want["iterations"])
    assert ref.in_domain(c["T"].shape, c["init"][7], c["q"][7], r, True) and want["last_step"][7] > 0
    got = gpu(c)
    ke.assert_agree(got, want, f"odd r={r}", last_step=True)
    ke.equal_results(gpu(c, volume=True), got)


# ---- B3. T's edges --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("axis,side", bc.T_EDGES, ids=bc.T_EDGE_IDS)
def test_T_edges(axis, side):
    c = bc.t_edge_case(axis, side)
    want = bc.restate(c)
    assert list(want["status"]) == bc.T_EDGE_STATUS and list(want["iterations"]) == bc.T_EDGE_ITERATIONS, (want["status"], want["iterations"])
    got = gpu(c)
    ke.assert_init_returned(got, c["init"], 3, (1, 3))
    for i in (0, 2):
        print("row", i, "gaps", ke.gaps(got, want, [i]))
    ke.assert_agree(got, want, "T edge", last_step=True)
    ke.equal_results(gpu(c, volume=True), got)


def test_T_upper_edge_rotated():
    c = bc.rotated_edge_case()
    got = gpu(c)
    ke.assert_agree(got, bc.restate(c), "rotated edge", last_step=True)
    ke.equal_results(gpu(c, volume=True), got)


def test_status_3_after_a_step():
    c = bc.status_3_case()
    want = bc.restate(c)
    assert (want["status"] == 3).all() and (want["last_step"] > 0).all(), (want["status"], want["iterations"])
    got = gpu(c)
    ke.assert_agree(got, want, "status 3 after a step", last_step=True)
    for i in range(len(c["q"])):
        assert ref.in_domain(c["T"].shape, got["p"][i], c["q"][i], ke.EDGE_R, True)
        assert got["last_step"][i] > 0
        if got["iterations"][i] == 0:
            assert ke.same_bits(got["p"][i], c["init"][i])
    ke.equal_results(gpu(c, volume=True), got)


# ---- B4. non-finite T, statuses and their order ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("axis,side", bc.NF_SITES, ids=bc.NF_IDS)
def test_nonfinite_T_at_the_prefilters_reach(status_scene, axis, side):
    """through the volume path: the farthest voxel that changes the restatement gives the restatement's status, the next one the
    clean run's bytes, for NaN, +Inf and -Inf (tests/test_bspline_cpu.py asserts that the three share the pair of distances)"""
    R, T, _ = status_scene
    near, far, clean_want = bc.nf_straddle(R, T, axis, side)
    q = bc.nf_q(axis, side)

    def call(V):
        return capi.icgn_bspline(R, V, q, init=ke.ST_INIT, **ke.ST_OPTS)

    clean = call(T)
    ke.assert_agree(clean, clean_want, "clean", last_step=True)
    assert clean["status"][0] == 1 and clean["iterations"][0] == 3
    for v in bc.NF_VALUES:
        Tn = bc.nf_planted(T, axis, side, near, v)
        want = bc.nf_restate(R, Tn, axis, side)
        got = call(Tn)
        print(f"{v} at {near} voxels: status {want['status'].tolist()} iterations {want['iterations'].tolist()}; at {far}: the clean run")
        assert want["status"][0] != 1
        assert np.array_equal(got["status"], want["status"]) and np.array_equal(got["iterations"], want["iterations"]), (v, got["status"], want["status"])
        if want["iterations"][0] == 0:
            ke.assert_init_returned(got, ke.ST_INIT, want["status"][0], [0])
        ke.equal_results(call(bc.nf_planted(T, axis, side, far, v)), clean)


def test_status_order_in_one_call(status_scene):
    c, healthy = bc.status_order_case(status_scene)
    want = bc.restate(c)
    assert list(want["status"]) == bc.STATUS_ORDER, want["status"]
    got = gpu(c, volume=True)
    assert np.array_equal(got["status"], want["status"]), got["status"]
    for i, s in ((0, 5), (2, 2), (4, 4)):
        assert got["status"][i] == s and ke.same_bits(got["p"][i], c["init"][i]) and got["iterations"][i] == 0 and got["zncc"][i] == 0
    alone = gpu(healthy, volume=True)
    ke.equal_results(got, alone, [1, 3, 5], None)
    ke.assert_agree(alone, bc.restate(healthy), "healthy neighbours")
    ke.equal_results(gpu(healthy), alone)


# ---- B5. exact invariances ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(ke.SCALINGS))
def test_exact_invariances(value_scene, name):
    """the header's claim: a power-of-two scaling (of both volumes, or of T alone) and a negation return the unscaled call's bits,
    through the prefilter, the centring by a coefficient and the relative thresholds"""
    R, T, q, init, _ = value_scene
    a, b = ke.SCALINGS[name]
    opts = dict(subset_radius=6)
    base = capi.icgn_bspline(R, T, q[:16], init=init[:16], **opts)
    assert (base["status"] == 0).mean() >= 0.8
    got = capi.icgn_bspline(np.float32(a) * R, np.float32(b) * T, q[:16], init=init[:16], **opts)
    dp = np.abs(got["p"] - base["p"])
    print(name, "max |dp|", dp.max(), "rows that differ", int((dp.max(1) > 0).sum()), "status", list(got["status"]), list(base["status"]))
    for k in ("p", "zncc", "iterations", "status"):
        if base[k].dtype == np.float64:
            assert ke.same_bits(got[k], base[k]), (name, k)
        else:
            assert np.array_equal(got[k], base[k]), (name, k)


# ---- B6. offsets ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which,b,r", ke.OFFSETS, ids=[f"{m}-b{int(b)}-r{r}" for m, b, r in ke.OFFSETS])
def test_offsets(value_scene, which, b, r):
    """through the volume path.  The bound comes from the reference, as in the Keys test: e is the gap between the restatement with
    float32 per-voxel interpolation and the one that interpolates in fp64, both on the same fp32 coefficients; the GPU stays within
    the base tolerance + 4 e of the latter (fma and the tap order may each add about e).  A POI that the restatement calls flat
    (status 4: b = 32768 on one volume) is held to its status, which returns the init"""
    c = bc.offset_case(value_scene, which, b, r)
    w64, w32 = bc.restate(c), bc.restate(c, f32=True)
    assert np.array_equal(w32["status"], w64["status"]) and ((w64["status"] == 1).all() or (which != "both" and b == 32768.0)), (w32["status"], w64["status"])
    assert np.isin(w64["status"], (1, 4)).all(), w64["status"]
    ed, eg, ez = ke.gaps(w32, w64)
    got = gpu(c, volume=True)
    gd, gg, gz = ke.gaps(got, w64)
    print(f"offset {which} b={b} r={r}: status {w64['status'].tolist()}; e (f32 restatement - fp64) d/g/zncc {ed:.3e} {eg:.3e} {ez:.3e}; "
          f"GPU - fp64 {gd:.3e} {gg:.3e} {gz:.3e}")
    assert np.array_equal(got["status"], w64["status"]) and np.array_equal(got["iterations"], w64["iterations"]), (got["status"], w64["status"])
    ke.assert_init_returned(got, c["init"], 4, np.flatnonzero(w64["status"] == 4))
    assert gd <= ke.TOL_D + 4 * ed and gg <= ke.TOL_G + 4 * eg and gz <= ke.TOL_Z + 4 * ez, (gd, ed, gg, eg, gz, ez)


# ---- B7. convergent runs --------------------------------------------------------------------------------------------------------------

def test_convergent_runs(value_scene):
    """default tolerance: the iteration counts are the restatement's wherever no step of the restatement lies within 1 % of it"""
    c = bc.convergent_case(value_scene)
    want = bc.restate(c, tolerance=bc.CONVERGENT_TOL)
    near = bc.near_tolerance(want, bc.CONVERGENT_TOL)
    print("excluded", int(near.sum()), "of", len(near), "iterations", np.bincount(want["iterations"]), "status", np.bincount(want["status"]))
    assert near.mean() <= 0.10
    assert (want["status"] == 0).mean() >= 0.8
    got = gpu(c)
    keep = ~near
    assert np.array_equal(got["status"][keep], want["status"][keep]), (got["status"], want["status"])
    assert np.array_equal(got["iterations"][keep], want["iterations"][keep]), (got["iterations"], want["iterations"])
    dd = np.abs(got["p"][keep][:, ke.DISP] - want["p"][keep][:, ke.DISP]).max()
    print("convergent runs: max |d displacement|", dd)
    assert dd <= 1e-3, dd
    ke.equal_results(gpu(c, volume=True), got)


# ---- B8. many POIs, scratch growth and reuse ------------------------------------------------------------------------------------------

def test_many_pois_and_scratch_reuse(value_scene):
    """the volume path: every call also holds the coefficient volume and the prefilter's scratch"""
    R, T, q, init, _ = value_scene
    opts = dict(subset_radius=2, max_iterations=2, tolerance=0.0)
    small = capi.icgn_bspline(R, T, q[:7], init=init[:7], **opts)
    m, k = 70000, 50
    rep = -(-m // k)
    big = capi.icgn_bspline(R, T, np.tile(q[:k], (rep, 1))[:m], init=np.tile(init[:k], (rep, 1))[:m], **opts)
    after = capi.icgn_bspline(R, T, q[:7], init=init[:7], **opts)
    ke.equal_results(small, after)
    for f in ke.FIELDS:
        tiled = np.concatenate([big[f][:k]] * rep)[:m]
        if big[f].dtype == np.float64:
            assert ke.same_bits(big[f], tiled), f
        else:
            assert np.array_equal(big[f], tiled), f
    ke.equal_results(big, small, slice(0, 7), None)
    c = bc.case(R, T, q[:k], init[:k], **opts)
    ke.assert_agree({f: big[f][:k] for f in ke.FIELDS}, bc.restate(c), "50 distinct POIs")
    # a larger T between two calls on the 48^3 one: the coefficient volume and the prefilter's scratch regrow, then serve less again
    wide = ke.blobs((40, 52, 100), seed=61)
    between = capi.icgn_bspline(R, wide, q[:7], init=init[:7], **opts)
    again = capi.icgn_bspline(R, T, q[:7], init=init[:7], **opts)
    ke.equal_results(small, again)
    ke.equal_results(capi.icgn_bspline(R, wide, q[:7], init=init[:7], **opts), between)
