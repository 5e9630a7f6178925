"""CPU tests of the cubic B-spline interpolation's boundary and restatement (sift3d_bspline_prefilter, sift3d_icgn_bspline,
include/sift3d_hip.h; tests/bspline_ref.py): the library exports the entry points, bad arguments are refused before any device call,
the restated prefilter is scipy's exact filter to fp32 accuracy, reconstructs its input, keeps constants bit for bit and gives a NaN
the footprint the contract names, and on the restatement the B-spline mode recovers known deformations at least four times more
accurately than the Keys mode.  The last part asserts, on the restatement alone, what tests/test_gpu_bspline_edges.py relies on: the
kernel's way of forming the taps, inputs free of subnormal intermediates, two wrong prefilters that the tolerance could not see, and
the statuses, sensitivities and distances of the IC-GN cases (tests/bspline_cases.py)."""
import ctypes as C
import importlib
import os
import subprocess

import numpy as np
import pytest

import bspline_cases as bc
import bspline_ref as bref
import icgn_ref as ref
from test_gpu_icgn_edges import odd_volumes, spike_volume, status_scene, value_scene  # noqa: F401  (fixtures)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["sift3d_bspline_prefilter", "sift3d_icgn_bspline"]
ERR_ARG = 1
SHAPES = [(5, 1, 7), (2, 2, 2), (33, 17, 70), (3, 3, 300)]


@pytest.fixture(scope="module")
def capi():
    m = importlib.import_module("3dsift_amd.capi")
    if not os.path.exists(m.LIB_PATH):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "3dsift_amd", "csrc"), "-j8"])
    return m


def test_exports(capi):
    L = capi.lib()
    for n in NEW:
        assert hasattr(L, n), n
        assert n in capi.SYMBOLS


def _prefilter(capi, src=True, dst=True, same=False, dims=(4, 4, 4)):
    a, b = np.zeros((4, 4, 4), np.float32), np.zeros((4, 4, 4), np.float32)
    P = lambda v, on: v.ctypes.data_as(C.c_void_p) if on else None  # noqa: E731
    return capi.lib().sift3d_bspline_prefilter(P(a, src), dims[0], dims[1], dims[2], P(a if same else b, dst), 0, 0, None)


def test_prefilter_refusals(capi):
    assert _prefilter(capi, src=False) == ERR_ARG
    assert b"bad argument" in capi.lib().sift3d_last_error()
    assert _prefilter(capi, dst=False) == ERR_ARG
    assert _prefilter(capi, same=True) == ERR_ARG
    for k in range(3):
        for bad in (0, -1):
            dims = [4, 4, 4]
            dims[k] = bad
            assert _prefilter(capi, dims=tuple(dims)) == ERR_ARG, (k, bad)


def test_volumes_too_large_for_a_pass_are_refused(capi):
    # 4 x 4 x 2^25: 2^25 row tiles in the y pass, beyond the 2^24 - 1 workgroups of a launch; 1 x 65536 x 32768: ny * nz = 2^31
    for dims in ((4, 4, 1 << 25), (1, 1 << 16, 1 << 15), (0x7fffffff, 0x7fffffff, 0x7fffffff)):
        assert _prefilter(capi, dims=dims) == ERR_ARG, dims
        assert _icgn(capi, dims=(64, 64, 64) + dims, coef=0) == ERR_ARG, dims


def _opts(capi, **kw):
    o = capi.IcgnOptions()
    capi.lib().sift3d_default_icgn_options(C.byref(o))
    for k, v in kw.items():
        if k == "reserved":
            o.reserved[v] = 1
        else:
            setattr(o, k, v)
    return o


def _icgn(capi, o=None, ref=True, tar=True, pts=True, out=True, m=2, dims=(64, 64, 64, 64, 64, 64), coef=0):
    v = np.zeros((4, 4, 4), np.float32)
    q = np.zeros((2, 3), np.int32)
    res = np.zeros(2, capi.ICGN_DTYPE)
    P = lambda a, on: a.ctypes.data_as(C.c_void_p) if on else None  # noqa: E731
    return capi.lib().sift3d_icgn_bspline(P(v, ref), dims[0], dims[1], dims[2], P(v, tar), dims[3], dims[4], dims[5], P(q, pts), m, None,
                                          C.byref(o) if o is not None else None, coef, 0, 0, P(res, out), None)


BAD_OPTS = [dict(subset_radius=1), dict(subset_radius=33), dict(max_iterations=0), dict(max_iterations=101), dict(tolerance=-1e-3),
            dict(tolerance=float("nan")), dict(tolerance=float("inf")), dict(interpolation=1), dict(interpolation=2), dict(interpolation=-1),
            dict(reserved=0), dict(reserved=3)]


@pytest.mark.parametrize("bad", BAD_OPTS, ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))
@pytest.mark.parametrize("coef", [0, 1])
def test_icgn_bspline_bad_options_refused(capi, bad, coef):
    assert _icgn(capi, _opts(capi, **bad), coef=coef) == ERR_ARG
    assert b"sift3d_icgn_bspline: bad argument" in capi.lib().sift3d_last_error()


def test_icgn_bspline_bad_arguments_refused(capi):
    for coef in (2, -1, 3):
        assert _icgn(capi, coef=coef) == ERR_ARG, coef
    for coef in (0, 1):
        assert _icgn(capi, m=-1, coef=coef) == ERR_ARG
        for k in range(6):
            dims = [64] * 6
            dims[k] = 0
            assert _icgn(capi, dims=tuple(dims), coef=coef) == ERR_ARG, k
        assert _icgn(capi, ref=False, coef=coef) == ERR_ARG
        assert _icgn(capi, tar=False, coef=coef) == ERR_ARG
        assert _icgn(capi, out=False, coef=coef) == ERR_ARG
        assert _icgn(capi, out=False, m=0, coef=coef) == ERR_ARG
        assert _icgn(capi, pts=False, coef=coef) == ERR_ARG


def test_sift3d_icgn_still_refuses_interpolation_2(capi):
    v = np.zeros((4, 4, 4), np.float32)
    q = np.zeros((2, 3), np.int32)
    res = np.zeros(2, capi.ICGN_DTYPE)
    P = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    o = _opts(capi, interpolation=2)
    assert capi.lib().sift3d_icgn(P(v), 64, 64, 64, P(v), 64, 64, 64, P(q), 2, None, C.byref(o), 0, 0, P(res), None) == ERR_ARG


def _inputs(shape, seed):
    rng = np.random.default_rng(seed)
    n = rng.standard_normal(shape)
    return {"noise": rng.uniform(-1, 1, shape).astype(np.float32), "ct": np.round(30000 + 200 * n).astype(np.float32)}


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("kind", ["noise", "ct"])
def test_prefilter_is_scipys_filter(shape, kind):
    ndi = pytest.importorskip("scipy.ndimage")
    T = _inputs(shape, 1)[kind]
    want = ndi.spline_filter(T.astype(np.float64), order=3, mode="mirror", output=np.float64)
    got = bref.prefilter(T)
    err = np.abs(got - want).max()
    assert err <= 1e-7 * np.abs(T).max(), (err, np.abs(T).max())


def test_taps_sum_to_one():
    h = bref.taps()
    assert len(h) == bref.K and abs(h[0] / bref.Z1 * (1 + 2 * (bref.Z1 ** np.arange(1, 17)).sum()) - 1) < 1e-15
    assert abs(1 - 2 * h.sum() - h[0] / bref.Z1) < 1e-15   # the implied central weight is h_0 = h_1 / z1
    assert abs(bref.Z1) ** 17 < 2e-10


def test_mirror_map():
    assert list(bref.mirror(np.arange(-5, 9), 4)) == [1, 2, 3, 2, 1, 0, 1, 2, 3, 2, 1, 0, 1, 2]
    assert list(bref.mirror(np.arange(-3, 4), 1)) == [0] * 7
    assert list(bref.mirror(np.arange(-3, 5), 2)) == [1, 0, 1, 0, 1, 0, 1, 0]


@pytest.mark.parametrize("f32", [False, True])
def test_reconstruction(f32):
    T = _inputs((20, 24, 28), 2)["noise"]
    c = bref.prefilter(T, f32=f32).astype(np.float64)
    for axis in range(3):
        c = (np.roll(c, 1, axis) + 4 * c + np.roll(c, -1, axis)) / 6
    err = np.abs(c - T)[1:-1, 1:-1, 1:-1].max()
    # fp32: 3 axes x 34 roundings of 2^-24 on coefficients of magnitude up to sqrt(3)^3 max|T|; fp64: the truncated tail
    assert err <= (3 * 34 * 2.0 ** -24 * 3.0 ** 1.5 if f32 else 1e-7), err


def test_constants_bit_for_bit():
    for v in (0.0, 1.0, -3.7, 30123.0, 1e-30, 3e38):
        T = np.full((5, 3, 40), v, np.float32)
        assert np.array_equal(bref.prefilter(T, f32=True).view(np.uint32), T.view(np.uint32)), v
    T = np.full((1, 1, 1), 2.5, np.float32)
    assert bref.prefilter(T, f32=True)[0, 0, 0] == np.float32(2.5)


def test_axis_of_length_one_is_the_identity():
    T = _inputs((1, 9, 1), 3)["noise"]
    one = bref.prefilter(T[0, :, 0].reshape(1, 1, 9), f32=True).ravel()
    assert np.array_equal(bref.prefilter(T, f32=True).ravel(), one)


@pytest.mark.parametrize("f32", [False, True])
def test_nan_footprint(f32):
    T = _inputs((48, 48, 48), 4)["noise"]
    clean = bref.prefilter(T, f32=f32)
    T[24, 24, 24] = np.nan
    c = bref.prefilter(T, f32=f32)
    bad = ~np.isfinite(c)
    want = np.zeros_like(bad)
    want[8:41, 8:41, 8:41] = True
    assert np.array_equal(bad, want)
    assert np.array_equal(c[~want], clean[~want])


def test_weights_partition_unity_and_reproduce_a_line():
    t = np.linspace(0, 1, 33)[:-1]
    w = bref.weights(t)
    assert np.abs(w.sum(-1) - 1).max() < 1e-15 and (w >= 0).all()
    assert np.abs(w @ np.array([-1.0, 0.0, 1.0, 2.0]) - t).max() < 1e-15
    assert bref.weights(np.float32(0.25)).dtype == np.float32


def test_keys_weights_are_restored():
    keep = ref.keys_weights
    R, T, truth = ref.scene((40, 40, 40), tvec=(0.3, 0.0, 0.0))
    with pytest.raises(ValueError):
        bref.refine(R, T, (20, 20, 20), subset_radius=5, interpolation=1)
    with pytest.raises(IndexError):
        bref.icgn(R, T, [[20, 20, 20]], init=np.zeros((0, 12)), subset_radius=5)
    assert ref.keys_weights is keep
    assert bref.refine(R, T, (3, 20, 20), subset_radius=5)["status"] == 2
    assert ref.keys_weights is keep


# ---- the bias claim, on the restatement -------------------------------------------------------------------------------------------

RECOVER = [("translation", np.eye(3), (0.37, -0.52, 0.21), False), ("rotation", ref.rot(4.0, -3.0, 9.0), (3.0, -2.0, 1.0), True),
           ("dilation", 1.02 * np.eye(3), (0.0, 0.0, 0.0), True)]


def recover_case(L, t, guess):
    """the scene, the 27 POIs on {28, 48, 68}^3, the true parameters and the guesses of test_recovers_known_deformation"""
    R, T, truth = ref.scene((96, 96, 96), L, t, seed=11)
    g = np.array([28, 48, 68])
    q = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(np.int32)
    tr = truth(q)
    rng = np.random.default_rng(3)
    init = tr + np.where(np.arange(12) % 4 == 0, rng.uniform(-0.4, 0.4, tr.shape), rng.uniform(-0.01, 0.01, tr.shape)) if guess else None
    return R, T, q, tr, init


@pytest.mark.parametrize("name,L,t,guess", RECOVER, ids=[c[0] for c in RECOVER])
def test_bspline_bias_is_a_quarter_of_keys(name, L, t, guess):
    R, T, q, tr, init = recover_case(L, t, guess)
    keys = ref.icgn(R, T, q, init=init, subset_radius=12)
    bsp = bref.icgn(R, T, q, init=init, subset_radius=12, f32=True)
    assert (keys["status"] == 0).all() and (bsp["status"] == 0).all(), (keys["status"], bsp["status"])
    ek = np.abs(keys["p"] - tr)[:, [0, 4, 8]].max()
    eb = np.abs(bsp["p"] - tr)[:, [0, 4, 8]].max()
    print(f"{name}: max displacement error Keys {ek:.3e}, B-spline {eb:.3e}, ratio {ek / eb:.1f}")
    assert eb <= 0.25 * ek, (eb, ek)


# ---- what tests/test_gpu_bspline_edges.py relies on, asserted on the restatement alone (the cases: tests/bspline_cases.py) --------------

def test_kernel_taps_round_to_the_restatements():
    """repeated multiplication from the literal and bspline_ref's power function differ in fp64, not after the rounding to float32"""
    a, b = bc.kernel_taps(), bref.taps().astype(np.float32)
    assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), (a, b)
    assert len(bc.prefilter_shapes()) == len(set(bc.prefilter_shapes())) and bc.ALL_SEAMS in bc.prefilter_shapes()


@pytest.mark.parametrize("kind", bc.KINDS)
def test_prefilter_cases_have_no_subnormal(kind):
    """bit parity is asked only where it cannot hang on how a device treats subnormal numbers: every output and every per-axis
    intermediate of every case is zero or normal"""
    for shape in bc.prefilter_shapes():
        passes = []
        bref.prefilter(bc.volume(shape, kind), f32=True, passes=passes)
        assert len(passes) == 3 and all(bc.zero_or_normal(p) for p in passes), shape


def test_what_the_old_prefilter_bar_could_not_see():
    """two wrong restatements -- the taps accumulated k = 1 .. K, tap 16 dropped -- differ from the true one in bits and
    lie inside the bar 4 e + 1e-7 max|T| of test_prefilter_agrees_with_restatement; a byte comparison tells them apart"""
    T = bc.volume(bc.ALL_SEAMS, "noise")
    exact, true32 = bref.prefilter(T), bref.prefilter(T, f32=True)
    e = np.abs(true32 - exact).max()
    bar = 4 * e + 1e-7 * np.abs(T).max()
    for name, ks in bc.MUTANTS.items():
        wrong = bref.prefilter(T, f32=True, ks=ks)
        differ = int((wrong.view(np.uint32) != true32.view(np.uint32)).sum())
        gap, err = np.abs(wrong.astype(np.float64) - true32).max(), np.abs(wrong - exact).max()
        print(f"{name}: {differ} of {T.size} voxels differ in bits, max |wrong - true fp32| = {gap:.3e}, max |wrong - fp64| = {err:.3e}, "
              f"e = {e:.3e}, old bar {bar:.3e}: {'inside' if err <= bar else 'OUTSIDE'} the old bar")
        assert differ > 0, name
        assert err <= bar, (name, err, bar)


@pytest.mark.parametrize("r", [r for r in bc.SPIKE_R if r <= bc.SPIKE_ALL])
def test_spike_cases_on_the_restatement(spike_volume, r):
    """status 1 after 2 iterations for every sentinel, and zeroing the sentinel voxel in R alone moves p by >= 100 tolerances"""
    least = np.inf
    for name, c, at, amp in bc.spike_cases(spike_volume, r):
        want = bc.restate(c)
        assert want["status"][0] == 1 and want["iterations"][0] == 2, (name, want["status"], want["iterations"])
        sens = bc.spike_sensitivity(c, at, amp, want)
        least = min(least, sens)
        assert sens >= 100, (r, name, sens)
    print(f"r={r}: amplitude {amp:.1f}, smallest sensitivity over the sentinels {least:.0f} tolerances")


@pytest.mark.parametrize("r", bc.ODD_R)
def test_odd_volume_case_on_the_restatement(odd_volumes, r):
    c = bc.odd_case(odd_volumes, r)
    want = bc.restate(c)
    print(f"odd volumes r={r}: status {want['status'].tolist()} iterations {want['iterations'].tolist()} last_step[7] {want['last_step'][7]:.3e}")
    assert list(want["status"]) == bc.ODD_STATUS and list(want["iterations"]) == bc.ODD_ITERATIONS
    assert ref.in_domain(c["T"].shape, c["init"][7], c["q"][7], r, True) and want["last_step"][7] > 0  # 7 started inside T and left it


@pytest.mark.parametrize("axis,side", bc.T_EDGES, ids=bc.T_EDGE_IDS)
def test_T_edge_cases_on_the_restatement(axis, side):
    want = bc.restate(bc.t_edge_case(axis, side))
    print(f"T edge {'xyz'[axis]} side {side}: status {want['status'].tolist()} iterations {want['iterations'].tolist()}")
    assert list(want["status"]) == bc.T_EDGE_STATUS and list(want["iterations"]) == bc.T_EDGE_ITERATIONS


def test_status_3_case_on_the_restatement():
    """as under Keys weights, IC-GN's first step from within a voxel of the truth is nearly the whole error: every start leaves T
    with its first update"""
    c = bc.status_3_case()
    want = bc.restate(c)
    print("status 3 after a step: status", want["status"].tolist(), "iterations", want["iterations"].tolist(), "last_step", want["last_step"].round(3).tolist())
    assert (want["status"] == 3).all() and (want["last_step"] > 0).all(), (want["status"], want["iterations"])
    rot = bc.restate(bc.rotated_edge_case())
    print("rotated edge: status", rot["status"].tolist(), "iterations", rot["iterations"].tolist())
    assert (rot["status"] == 1).all() and (rot["iterations"] == 2).all()


@pytest.mark.parametrize("axis,side", bc.NF_SITES, ids=bc.NF_IDS)
def test_non_finite_reach_straddles(status_scene, axis, side):
    """the pair of distances that the GPU test plants at: the farthest voxel that changes the restatement and the next, which does
    not; the same pair for NaN, +Inf and -Inf, within the header's K + 2"""
    R, T, _ = status_scene
    pairs = [bc.nf_straddle(R, T, axis, side, v)[:2] for v in bc.NF_VALUES]
    clean = bc.nf_restate(R, T, axis, side)
    print(f"non-finite voxel {'xyz'[axis]} side {side}: changes the result up to {pairs[0][0]} voxels beyond the subset's face, "
          f"not at {pairs[0][1]} (K + 2 = {bref.K + 2}); clean status {clean['status'].tolist()}")
    assert pairs[0] == pairs[1] == pairs[2], pairs
    assert clean["status"][0] == 1 and clean["iterations"][0] == 3


def test_status_order_case_on_the_restatement(status_scene):
    c, healthy = bc.status_order_case(status_scene)
    assert list(bc.restate(c)["status"]) == bc.STATUS_ORDER


def test_convergent_case_on_the_restatement(value_scene):
    want = bc.restate(bc.convergent_case(value_scene), tolerance=bc.CONVERGENT_TOL)
    near = bc.near_tolerance(want, bc.CONVERGENT_TOL)
    print(f"convergent runs: {near.mean():.1%} left out ({int(near.sum())} of {len(near)}), {(want['status'] == 0).mean():.0%} end in status 0, "
          f"iterations {np.bincount(want['iterations'])}")
    assert near.mean() <= 0.10
    assert (want["status"] == 0).mean() >= 0.8
