"""GPU tests of sift3d_icgn2 where a subtle error would pass tests/test_gpu_icgn2.py: every legal subset radius with a spike on a
sentinel voxel of the walk (a missed or doubled voxel moves the result by >= 100 bars, asserted on the restatement), compositions
whose LU exchanges rows, volumes with pairwise different dimensions, R's and T's exact domain edges (reached through the first-order
and through the second-order terms), every status with its order and every source of status 4, non-finite voxels, offsets and exact
power-of-two scalings, convergent runs and 70 000 POIs in one call.  The cases come from tests/icgn2_cases.py, which the CPU
companion tests/test_icgn2_edges_cpu.py imports too; the reference is tests/icgn2_ref.py in fp64.

"Agrees" is test_agrees_with_restatement's bound everywhere: statuses and iteration counts equal, |d u| <= 1e-4, |d first
derivatives| <= 1e-5, |d second derivatives| <= 2e-5 / r, |d zncc| <= 1e-5, each widened to 4 x the gap between the restatement's fp32
and fp64 forms on the case (last_step, where named, within u's bar).  Every test prints the measured gaps and the bars.

Two things the file does not do.  Status 6 needs an exactly singular M(dp) or a non-finite dp out of finite sums; no construction
through the API reaches it, and none is contrived here.  No start within the domain made the LU exchange rows in a column of 4 or
higher: after the four eliminations of columns 0..3 the trailing 6 x 6 block is the symmetric square of the step's gradient
1 + grad dp, within a few 1e-2 of the identity for any step that stays in T, and an exchange there needs an off-diagonal term of
that gradient above the diagonal one.  The exchanges that do happen are in columns 0 to 3 (printed by the CPU file)."""
import importlib

import numpy as np
import pytest

import icgn2_cases as C
import icgn2_ref as ref2

pytestmark = pytest.mark.gpu

capi = importlib.import_module("3dsift_amd.capi")


def kid(k):
    return C.KINDS[k]


def gpu(c):
    return capi.icgn2(c["R"], c["T"], c["q"], init=c["init"], coefficients=c["coef"], **c["opts"])


# ---- 1. every radius, a spike on a sentinel voxel of the walk ------------------------------------------------------------------------

@pytest.fixture(scope="module")
def spike_volume():
    V = C.spike_volume()
    V.setflags(write=False)
    return V


@pytest.mark.parametrize("r,kind", C.SPIKE, ids=[f"r{r}-{kid(k)}" for r, k in C.SPIKE])
def test_every_radius_with_sentinel_spikes(spike_volume, r, kind):
    """one call per sentinel.  The spike is two voxels along x (the sentinel and its +x neighbour), so that the sentinel carries the
    spike's value and half of it as gradient; R and T differ by an integer shift, the init lies near the truth with small first-
    and second-order terms, two fixed iterations.  The sensitivity run zeroes the sentinel voxel in R alone and must move the
    restatement's p by >= 100 of the bars used (widened ones included).  The amplitude follows one rule in r and so does the
    init's spread, which is narrowed below r = 9 (icgn2_cases.spike_init says why): r = 2 keeps 6 % of it.  Trilinear at every
    radius and every sentinel; Keys and B-spline at r = 2, 3, 8, 17, 32 with four sentinels"""
    for name, (c, c0, i, d) in C.spike_cases(spike_volume, r, kind).items():
        what = f"r={r} {kid(kind)} {name} index {i} d={tuple(int(x) for x in d)}"
        want, w32, _ = C.spike_expected(c, c0, r, what)
        C.agree(gpu(c), want, w32, r, what)


# ---- 2. pivoted composition ------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def quad_scene():
    R, T, truth = ref2.quadratic_scene()
    R.setflags(write=False)
    T.setflags(write=False)
    return R, T, truth


@pytest.mark.parametrize("r,kind,it", C.PIVOT, ids=[f"r{r}-{kid(k)}-it{it}" for r, k, it in C.PIVOT])
def test_pivoted_composition(quad_scene, r, kind, it):
    """starts 0.6 to 1.4 voxel from the truth, along each axis in each sign and in two mixed directions: the LU of M(dp) exchanges
    rows in the first iteration of every POI (in column 0 too where the step exceeds 1 voxel), so the shuffled row swap, the perm
    exchange and the un-permutation decide the composed p.  One iteration returns that p itself; two add a second, small step"""
    c = C.pivot_case(quad_scene, r, kind, it)
    want, w32, first = C.pivot_expected(c)
    cols = [C.exchanged_columns(pm) for pm in first]
    print("columns that exchange rows, per POI:", cols)
    assert any(0 in cs for cs in cols)
    C.agree(gpu(c), want, w32, r, f"pivot r={r} {kid(kind)} it={it}", last_step=True)


# ---- 3. axes, strides and sizes ----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def odd_scene():
    return C.odd_scene()


@pytest.mark.parametrize("r,kind", C.ODD, ids=[f"r{r}-{kid(k)}" for r, k in C.ODD])
def test_axes_strides_and_sizes(odd_scene, r, kind):
    """R (40, 52, 46) and T (44, 38, 60) cropped from one quadratic scene with an asymmetric gradient and second-order terms that
    differ per component; the init is moved by the integer crop.  POI 6 is refused by T.ny where T.nz would accept it.  POI 7 starts
    beyond T.ny inside T's last z cell: it is accepted and computes a step, and as its init lies far from the truth the composed p
    leaves T (status 3, 0 iterations, the step's norm in last_step; a refusal at the start has last_step 0).  POIs 8 and 9 get to
    the same two places by a step from near the truth (status 3 with the step's norm; status 1 inside the last z cell)"""
    c = C.odd_case(odd_scene, r, kind)
    want, w32 = C.odd_expected(c, r, kind)
    got = gpu(c)
    C.agree(got, want, w32, r, f"odd r={r} {kid(kind)}", last_step=True)
    C.init_returned(got, c["init"], 3, [6])
    assert C.same_bits(got["p"][7], c["init"][7]) and got["last_step"][7] > 0  # accepted, stepped, left T: the start comes back
    assert C.same_bits(got["p"][8], c["init"][8])


# ---- 4. exact edges ----------------------------------------------------------------------------------------------------------------------

def test_R_edges():
    """q = r + 1 and q = n - 2 - r read R's outermost voxels and run; q = r and q = n - 1 - r are status 2 with the init's bits, on
    every axis and side"""
    c, r = C.R_edge_case()
    want, w32 = C.expected(c, [1] * 6 + [2] * 6)
    got = gpu(c)
    C.agree(got, want, w32, r, "R edges")
    C.init_returned(got, c["init"], 2, range(6, 12))


@pytest.mark.parametrize("axis,side,kind", C.T_EDGES, ids=[f"{'xyz'[a]}-{'upper' if s else 'lower'}-{kid(k)}" for a, s, k in C.T_EDGES])
def test_T_edges(axis, side, kind):
    """rows: 0 the extreme tap on T's first / last voxel (runs), 1 one voxel further (status 3, the init's bits), 2 2^-40 inside
    (upper: the fp32 fraction rounds to 1), 3 2^-40 outside"""
    c = C.T_edge_case(axis, side, kind)
    want, w32 = C.T_edge_expected(c)
    got = gpu(c)
    C.init_returned(got, c["init"], 3, (1, 3))
    C.agree(got, want, w32, C.T_EDGE_R, "T edge", last_step=True)


@pytest.mark.parametrize("axis,kind", C.QUAD_EDGES, ids=[f"{'xyz'[a]}-{kid(k)}" for a, k in C.QUAD_EDGES])
def test_T_edge_through_the_quadratic_part(axis, kind):
    """zero first-order terms; a mixed term (rows 0, 2) or a square (rows 1, 3) of the component carries a corner voxel to 2^-40
    below the first outside integer (rows 0, 1: in the domain, the fp32 fraction of o = cf + (lin + quad) rounds to 1 and the clamp
    of the sample takes it) or onto it (rows 2, 3: status 3)"""
    c, r = C.quad_edge_case(axis, kind)
    C.quad_edge_preconditions(c, r, kind, axis)
    want, w32 = C.expected(c)
    assert (want["last_step"][:2] > 0).all()
    got = gpu(c)
    C.init_returned(got, c["init"], 3, (2, 3))
    C.agree(got, want, w32, r, "quadratic edge", last_step=True)


@pytest.mark.parametrize("side,kind", C.WIDEN, ids=[kid(k) if s else f"lower-{kid(k)}" for s, k in C.WIDEN])
def test_widening_on_the_limit(side, kind):
    """each of the six second-order terms of u in turn.  Upper side: with B = 0.5 the widened corner is the last double below the
    limit (runs), with B = 0.5 + 2^-48 it is the limit (status 3).  Lower side: with B = 0.5 the widened corner is the last inside
    integer (runs), with B = 0.5 + 2^-48 it lies 2^-48 below it (status 3); without B every row is inside"""
    c, r = C.widen_case(kind, side)
    C.widen_preconditions(c, r, kind, side)
    want, w32 = C.expected(c)
    assert (want["last_step"][:6] > 0).all() and list(want["status"][6:]) == [3] * 6
    got = gpu(c)
    C.init_returned(got, c["init"], 3, range(6, 12))
    C.agree(got, want, w32, r, "widening", last_step=True)


# ---- 5. statuses ---------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def status_scene():
    return C.status_scene()


def check_status_4(c, what):
    want = C.restate(c)
    assert want["status"][0] == 4 and want["iterations"][0] == 0, (what, want["status"])
    got = gpu(c)
    assert got["status"][0] == 4, (what, got["status"])
    C.init_returned(got, c["init"], 4, [0])
    print(what, "-> status", int(got["status"][0]), "with the init's bits, as the restatement (no figure to compare)")


def test_status_order_in_one_call(status_scene):
    """5 before 2 before 4 before 3, each bad POI meeting the next condition as well, alternating with healthy POIs whose bits are
    those of a call of their own"""
    c, alone = C.order_case(status_scene)
    want, w32 = C.expected(c, C.ORDER_STATUS)
    got = gpu(c)
    C.agree(got, want, w32, c["opts"]["subset_radius"], "status order")
    for i, s in ((0, 5), (2, 2), (4, 4), (6, 3)):
        assert got["status"][i] == s and C.same_bits(got["p"][i], c["init"][i]), i
        assert got["iterations"][i] == 0 and got["zncc"][i] == 0 and got["last_step"][i] == 0, i
    C.equal_results(got, gpu(alone), [1, 3, 5, 7], None)


@pytest.mark.parametrize("kind", [0, 1, 2], ids=kid)
def test_status_4_from_R_and_constant_T(status_scene, kind):
    """a ramp of integers (an exactly zero pivot of the 30 x 30 Cholesky), constant T and T = (float)Rm (dT = 0), a NaN or +Inf in
    R's subset, a NaN in R's x margin only and in its z margin only"""
    check_status_4(C.status_case(status_scene, kind, R=C.ramp_R()), "ramp")
    for Tc in C.constant_targets(status_scene):
        check_status_4(C.status_case(status_scene, kind, T=Tc), f"T = {Tc[0, 0, 0]}")
    for what, Rb in C.nonfinite_R(status_scene).items():
        check_status_4(C.status_case(status_scene, kind, R=Rb), what)


@pytest.mark.parametrize("kind", [0, 1, 2], ids=kid)
def test_nonfinite_T(status_scene, kind):
    """a NaN, +Inf and -Inf under a tap of the centre voxel and of a corner voxel: status 4 at the start.  A NaN that no tap of any
    iteration touches leaves the clean call's bits.  (B-spline: planted in the coefficients, where a voxel stays a voxel)"""
    planted, coef = C.nonfinite_T(status_scene, kind)
    for what, (Tb, at) in planted.items():
        check_status_4(C.status_case(status_scene, kind, T=Tb, coef=coef), what)
    T, Tb, coef = C.untouched_T(status_scene, kind)
    clean = gpu(C.status_case(status_scene, kind, T=T, coef=coef))
    assert clean["status"][0] == 1 and clean["iterations"][0] == 3
    C.equal_results(gpu(C.status_case(status_scene, kind, T=Tb, coef=coef)), clean)


@pytest.mark.parametrize("kind", [0, 1, 2], ids=kid)
def test_status_4_after_a_step(status_scene, kind):
    """a NaN voxel that the start's taps miss and the second iteration's taps reach (found on the restatement): the p of the first
    iteration, iterations 1, that step's norm and zncc 0"""
    c, clean, at, first = C.late_nan_case(status_scene, kind)
    want, w32 = C.expected(c, [4])
    assert want["iterations"][0] == 1
    got = gpu(c)
    C.agree(got, want, w32, C.ST_R, f"late NaN at {tuple(int(v) for v in at)}", last_step=True)
    assert got["zncc"][0] == 0.0 and got["last_step"][0] > 0.5
    one = gpu(dict(clean, opts=dict(clean["opts"], max_iterations=1)))
    assert C.same_bits(got["p"], one["p"]) and C.same_bits(got["last_step"], one["last_step"])  # the clean first iteration's own bits


# ---- 6. values -----------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def value_scene():
    return C.value_scene()


@pytest.mark.parametrize("which,b,r", C.OFFSETS, ids=[f"{m}-b{int(b)}-r{r}" for m, b, r in C.OFFSETS])
def test_offsets(value_scene, which, b, r):
    """R + b and T + b, together and one at a time, one iteration: within the base bars + 4 e of the fp64 restatement, e the gap
    between the restatement's fp32 and fp64 forms, statuses equal (the fp32 form's too)"""
    c = C.offset_case(value_scene, which, b, r)
    want, w32 = C.expected(c)
    e = C.gaps(w32, want)
    got = gpu(c)
    g = C.gaps(got, want)
    base = C.base_bars(r)
    print(f"offset {which} b={b} r={r}: status {list(want['status'])}",
          " ".join(f"{k} GPU - fp64 {g[k]:.2e} (fp32 - fp64 {e[k]:.2e}, bar {base[k] + 4 * e[k]:.2e})" for k in base))
    assert np.array_equal(got["status"], want["status"]) and np.array_equal(got["iterations"], want["iterations"])
    for k in base:
        assert g[k] <= base[k] + 4 * e[k], (k, g[k], e[k])


@pytest.mark.parametrize("name", list(C.SCALINGS))
@pytest.mark.parametrize("kind", [0, 1, 2], ids=kid)
def test_exact_invariances(value_scene, name, kind):
    """every threshold is relative and every sum has a fixed order: a power-of-two scaling of both volumes, of T alone, or a
    negation of both returns the original call's bits in every field, last_step included (T alone: the kernel shifts T by a voxel
    of T, so T' scales exactly)"""
    base, scaled = C.scaling_case(value_scene, name, kind)
    a, b = gpu(base), gpu(scaled)
    dp = np.abs(a["p"] - b["p"])
    print(name, kid(kind), "max |dp|", dp.max(), "rows that differ", int((dp.max(1) > 0).sum()), "status", list(a["status"]), list(b["status"]))
    assert np.isin(a["status"], (0, 1)).all()
    print("  max |d last_step|", np.abs(a["last_step"] - b["last_step"]).max())
    C.equal_results(a, b)


def test_convergent_runs(value_scene):
    """default tolerance, 60 POIs at r = 6: iteration counts and statuses are the restatement's wherever no step of the restatement
    lies within 1 % of the tolerance, and |du| <= 1e-3 there"""
    c = C.convergent_case(value_scene)
    want, near = C.convergent_expected(c)
    got = capi.icgn2(c["R"], c["T"], c["q"], init=c["init"], subset_radius=6)  # the default options otherwise
    keep = ~near
    assert np.array_equal(got["status"][keep], want["status"][keep]), (got["status"], want["status"])
    assert np.array_equal(got["iterations"][keep], want["iterations"][keep]), (got["iterations"], want["iterations"])
    du = np.abs(got["p"][keep][:, ref2.DISP] - want["p"][keep][:, ref2.DISP]).max()
    print("convergent runs: max |du|", du)
    assert du <= 1e-3, du


# ---- 7. many POIs and scratch reuse --------------------------------------------------------------------------------------------------------

def test_many_pois_and_scratch_reuse(value_scene):
    """70 000 POIs (about 300 MB of per-POI state) tiled from 50: the tiled rows repeat the first 50 bit for bit, those agree with
    the restatement, and a 7-POI call gives the same bits before and after"""
    small, big, fifty = C.many_cases(value_scene)
    before = gpu(small)
    many = gpu(big)
    after = gpu(small)
    C.equal_results(before, after)
    k, rep = C.MANY_DISTINCT, -(-C.MANY // C.MANY_DISTINCT)
    for f in C.FIELDS:
        tiled = np.concatenate([many[f][:k]] * rep)[:C.MANY]
        if many[f].dtype == np.float64:
            assert C.same_bits(many[f], tiled), f
        else:
            assert np.array_equal(many[f], tiled), f
    C.equal_results(many, before, slice(0, 7), None)
    want, w32 = C.expected(fifty, [1] * k)
    C.agree({f: many[f][:k] for f in C.FIELDS}, want, w32, 2, "50 distinct POIs")
