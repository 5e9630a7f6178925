"""CPU companion of tests/test_gpu_icgn2_edges.py: on the restatement alone (tests/icgn2_ref.py) every precondition that file relies
on -- the statuses its cases are built to reach, the sensitivity of every spiked sentinel, the row permutations of the pivoted
compositions, the in-domain and outside flags at the exact edges -- with the cases taken from tests/icgn2_cases.py, which both files
import.  Each family prints the fp32-minus-fp64 gaps of the restatement (what widens the GPU file's bars), the sensitivities and the
permutations it found."""
import numpy as np
import pytest

import icgn2_cases as C
import icgn2_ref as ref2

IDENT = tuple(range(10))


def kid(k):
    return C.KINDS[k]


def show(what, want, w32, r):
    bars, e = C.bars_of(want, w32, r)
    print(what, "status", list(want["status"]), "iterations", list(want["iterations"]), "fp32 - fp64",
          " ".join(f"{k} {v:.2e}" for k, v in e.items()), "| bars", " ".join(f"{k} {v:.2e}" for k, v in bars.items()))


# ---- the restatement's own additions ---------------------------------------------------------------------------------------------------

def test_permutations_are_returned_and_replayed():
    rng = np.random.default_rng(0)
    assert C.exchanged_columns(IDENT) == []
    for _ in range(20):
        A = rng.standard_normal((10, 10))
        LU, perm = ref2.lu(A)
        L, U = np.tril(LU, -1) + np.eye(10), np.triu(LU)
        assert np.abs(L @ U - A[perm]).max() <= 1e-12
        assert sorted(perm) == list(range(10))
        assert (len(C.exchanged_columns(tuple(perm))) == 0) == (tuple(perm) == IDENT)
    p = np.zeros(30)
    dp = C.prow((1.3, 0.0, 0.0))
    f = ref2.lu(ref2.M_of(dp))
    assert 0 in C.exchanged_columns(tuple(f[1]))  # row 4 of column 0 is u^2, row 1 is u: u > 1 exchanges in column 0
    assert C.same_bits(ref2.compose(p, dp), ref2.compose(p, dp, f))
    assert 0 not in C.exchanged_columns(tuple(ref2.lu(ref2.M_of(C.prow((0.6, 0.0, 0.0))))[1]))


# ---- 1 -------------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def spike_volume():
    V = C.spike_volume()
    V.setflags(write=False)
    return V


def test_sentinels_cover_the_walk():
    for r in range(2, 33):
        s = C.sentinels(r)
        N = (2 * r + 1) ** 3
        assert len(s) >= 6 and len(set(s.values())) == len(s) and all(0 <= i < N for i in s.values())
        assert len(C.spike_sentinels(r, 0)) >= 4 and len(C.spike_sentinels(r, 1)) == len(s)
        if r >= 4:
            assert {"i255", "i256", "ycarry", "zcarry"} <= set(s), (r, s)
    assert {2, 3, 17, 32} <= set(C.CUBIC_RADII)
    assert {r for r, k in C.SPIKE if k == 1} == set(range(2, 33))


@pytest.mark.parametrize("r,kind", C.SPIKE, ids=[f"r{r}-{kid(k)}" for r, k in C.SPIKE])
def test_spiked_sentinels_are_sensitive(spike_volume, r, kind):
    """status 1 after two iterations, and zeroing the sentinel voxel in R alone moves p by >= 100 of the bars used"""
    for name, (c, c0, i, d) in C.spike_cases(spike_volume, r, kind).items():
        C.spike_expected(c, c0, r, f"r={r} {kid(kind)} {name} index {i} d={tuple(int(x) for x in d)}")


# ---- 2 -------------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def quad_scene():
    R, T, truth = ref2.quadratic_scene()
    R.setflags(write=False)
    T.setflags(write=False)
    return R, T, truth


def test_pivoted_compositions(quad_scene):
    """every first permutation differs from the identity, some exchange in column 0 (a step above 1 voxel); which columns exchange
    is printed.  No start of this family exchanges in a column of 4 or higher (see the GPU file's docstring)"""
    seen = set()
    for r, kind, it in C.PIVOT:
        c = C.pivot_case(quad_scene, r, kind, it)
        want, w32, first = C.pivot_expected(c)
        cols = [C.exchanged_columns(pm) for pm in first]
        show(f"pivot r={r} {kid(kind)} it={it}", want, w32, r)
        print("  first permutations", first, "columns", cols)
        seen.update(k for cs in cols for k in cs)
        assert any(0 in cs for cs in cols)
        assert (want["iterations"] == it).all()
    print("columns that exchange rows:", sorted(seen))
    assert not any(k >= 4 for k in seen)  # the docstring's claim


# ---- 3 -------------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def odd_scene():
    return C.odd_scene()


def test_odd_volumes_are_odd(odd_scene):
    R, T, truth = odd_scene
    assert len(set(R.shape)) == 3 and len(set(T.shape)) == 3 and T.shape[1] < T.shape[0] and R.shape != T.shape
    g = truth(C.ODD_MID[None])[0].reshape(3, 10)
    assert np.abs(g[:, 1:4] - g[:, 1:4].T).max() > 0.01           # an asymmetric gradient
    assert len({tuple(np.round(row, 9)) for row in g[:, 4:]}) == 3  # second-order terms that differ per component


@pytest.mark.parametrize("r,kind", C.ODD, ids=[f"r{r}-{kid(k)}" for r, k in C.ODD])
def test_axes_strides_and_sizes(odd_scene, r, kind):
    c = C.odd_case(odd_scene, r, kind)
    want, w32 = C.odd_expected(c, r, kind)
    show(f"odd r={r} {kid(kind)}", want, w32, r)
    tr = odd_scene[2](c["q"][:6])
    print("  |u - truth| after 3 iterations", np.abs(want["p"][:6] - tr)[:, ref2.DISP].max())
    assert np.abs(want["p"][:6] - tr)[:, ref2.DISP].max() < 0.5  # the crop's integer move of the init is right


# ---- 4 -------------------------------------------------------------------------------------------------------------------------------------

def test_R_edges():
    c, r = C.R_edge_case()
    want, w32 = C.expected(c, [1] * 6 + [2] * 6)
    show("R edges", want, w32, r)
    n = np.array(c["R"].shape)[::-1]
    lo, hi = c["q"][:6] - r - 1, c["q"][:6] + r + 1
    assert sorted(np.flatnonzero(lo.ravel() == 0)) == [0, 7, 14] and sorted(np.flatnonzero((hi == n - 1).ravel())) == [3, 10, 17]


@pytest.mark.parametrize("axis,side,kind", C.T_EDGES, ids=[f"{'xyz'[a]}-{'upper' if s else 'lower'}-{kid(k)}" for a, s, k in C.T_EDGES])
def test_T_edges(axis, side, kind):
    c = C.T_edge_case(axis, side, kind)
    want, w32 = C.T_edge_expected(c)
    show("T edge", want, w32, C.T_EDGE_R)
    for i, inside in enumerate((True, False, True, False)):
        assert ref2.in_domain(c["T"].shape, c["init"][i], c["q"][i], C.T_EDGE_R, kind != 1) == inside
    # the extreme tap of row 0 is T's first / last voxel
    pos = c["q"][0, axis] + c["init"][0, 10 * axis] + (C.T_EDGE_R if side else -C.T_EDGE_R)
    hi, lo = (1, 0) if kind == 1 else (2, 1)
    assert (pos + hi == c["T"].shape[2 - axis] - 1) if side else (pos - lo == 0)


@pytest.mark.parametrize("axis,kind", C.QUAD_EDGES, ids=[f"{'xyz'[a]}-{kid(k)}" for a, k in C.QUAD_EDGES])
def test_T_edge_through_the_quadratic_part(axis, kind):
    c, r = C.quad_edge_case(axis, kind)
    C.quad_edge_preconditions(c, r, kind, axis)
    want, w32 = C.expected(c)
    show("quadratic edge", want, w32, r)
    assert list(want["status"][2:]) == [3, 3] and (want["last_step"][:2] > 0).all() and (want["iterations"][2:] == 0).all()
    assert not c["init"][:, ref2.FIRST].any()


@pytest.mark.parametrize("side,kind", C.WIDEN, ids=[kid(k) if s else f"lower-{kid(k)}" for s, k in C.WIDEN])
def test_widening_on_the_limit(side, kind):
    c, r = C.widen_case(kind, side)
    C.widen_preconditions(c, r, kind, side)
    want, w32 = C.expected(c)
    show("widening", want, w32, r)
    assert (want["last_step"][:6] > 0).all() and list(want["status"][6:]) == [3] * 6 and (want["iterations"][6:] == 0).all()


# ---- 5 -------------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def status_scene():
    return C.status_scene()


def one(c):
    w = C.restate(c)
    return w["status"][0], w["iterations"][0], w["zncc"][0], w["last_step"][0]


def test_status_order(status_scene):
    c, alone = C.order_case(status_scene)
    want, w32 = C.expected(c, C.ORDER_STATUS)
    wa = C.restate(alone)
    C.equal_results(want, wa, [1, 3, 5, 7], None)
    R, q = c["R"], c["q"]
    r = c["opts"]["subset_radius"]
    assert q[0, 0] - r - 1 < 0 and q[2, 0] - r - 1 < 0                                        # rows 0, 2 lie outside R ...
    assert np.ptp(R[:, :, :q[2, 0] + r + 2]) == 0 and np.ptp(R[:, :, :q[4, 0] + r + 2]) == 0  # ... rows 2, 4 over constant R ...
    assert not ref2.in_domain(c["T"].shape, c["init"][4], q[4], r, True)                      # ... and row 4's init outside T
    assert not ref2.in_domain(c["T"].shape, c["init"][6], q[6], r, True)


def test_status_4_sources(status_scene):
    R, T, _ = status_scene
    for kind in (0, 1, 2):
        assert one(C.status_case(status_scene, kind))[:2] == (1, 3)
        assert one(C.status_case(status_scene, kind, R=C.ramp_R())) == (4, 0, 0.0, 0.0), "ramp"
        for Tc in C.constant_targets(status_scene):
            assert one(C.status_case(status_scene, kind, T=Tc)) == (4, 0, 0.0, 0.0), "constant T"
        for what, Rb in C.nonfinite_R(status_scene).items():
            assert one(C.status_case(status_scene, kind, R=Rb)) == (4, 0, 0.0, 0.0), what
        planted, coef = C.nonfinite_T(status_scene, kind)
        first = C.tap_voxels(T.shape, C.status_init(status_scene)[0], C.ST_Q[0], C.ST_R, kind)
        for what, (Tb, at) in planted.items():
            assert int(np.ravel_multi_index(at, T.shape)) in first, what
            assert one(C.status_case(status_scene, kind, T=Tb, coef=coef)) == (4, 0, 0.0, 0.0), what
    # the ramp's zero pivot is exact: H of R = x has a zero row and column for every term of v and w
    x, y, z = C.ST_Q[0]
    Rr = C.ramp_R()
    assert np.ptp(Rr[:, :, x]) == 0 and Rr[z, y, x + 1] - Rr[z, y, x - 1] == 2


@pytest.mark.parametrize("kind", [0, 1, 2], ids=kid)
def test_untouched_nan_and_late_nan(status_scene, kind):
    T, Tb, coef = C.untouched_T(status_scene, kind)
    clean, dirty = C.restate(C.status_case(status_scene, kind, T=T, coef=coef)), C.restate(C.status_case(status_scene, kind, T=Tb, coef=coef))
    assert clean["status"][0] == 1 and clean["iterations"][0] == 3
    C.equal_results(clean, dirty)
    c, cl, at, first = C.late_nan_case(status_scene, kind)
    want, w32 = C.expected(c, [4])
    print(f"late NaN {kid(kind)}: voxel {tuple(int(v) for v in at)}, first step {first['last_step'][0]:.3f}")
    assert want["iterations"][0] == 1 and want["zncc"][0] == 0.0
    assert C.same_bits(want["p"], first["p"]) and C.same_bits(want["last_step"], first["last_step"]) and want["last_step"][0] > 0.5
    assert C.restate(cl)["status"][0] == 1


# ---- 6 -------------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def value_scene():
    return C.value_scene()


@pytest.mark.parametrize("which,b,r", C.OFFSETS, ids=[f"{m}-b{int(b)}-r{r}" for m, b, r in C.OFFSETS])
def test_offsets_keep_their_status_in_fp32(value_scene, which, b, r):
    """every POI of every offset case ends with status 1 in both forms of the restatement, so that the GPU file compares figures in
    every row (a status-4 row would return the init and compare nothing)"""
    c = C.offset_case(value_scene, which, b, r)
    want, w32 = C.expected(c)
    show(f"offset {which} b={b} r={r}", want, w32, r)
    assert (want["status"] == 1).all() and (w32["status"] == 1).all(), (want["status"], w32["status"])


@pytest.mark.parametrize("name", list(C.SCALINGS))
def test_scalings_change_the_restatement_by_rounding_only(value_scene, name):
    """a precondition of test_exact_invariances, which compares the GPU with itself and needs no bar: each scaling is a symmetry of
    the operation, so the fp64 restatement of the scaled call is the original's up to its own rounding, statuses and iteration
    counts equal.  No bar of the GPU file is involved; "rounding only" is asserted as 1e-4 of each quantity's base bar (u 1e-8,
    first 1e-9, second 3.3e-10, zncc 1e-9), far above fp64 rounding through a 30 x 30 solve and far below anything the GPU file
    could take for agreement.  Measured: 0 for the three common scalings, 8e-15 for T alone by 2^7"""
    for kind in (0, 1, 2):
        base, scaled = C.scaling_case(value_scene, name, kind)
        base, scaled = dict(base, q=base["q"][:4], init=base["init"][:4]), dict(scaled, q=scaled["q"][:4], init=scaled["init"][:4])
        a, b = C.restate(base), C.restate(scaled)
        assert np.array_equal(a["status"], b["status"]) and np.array_equal(a["iterations"], b["iterations"])
        # B-spline: the restatement prefilters in float32 as the GPU does, exactly scale-free as well
        g = C.gaps(b, a)
        print(name, kid(kind), "restatement: scaled - original", " ".join(f"{k} {v:.2e}" for k, v in g.items()))
        for k, bar in C.base_bars(6).items():
            assert g[k] <= 1e-4 * bar, (name, kind, k, g[k])


def test_convergent_runs(value_scene):
    C.convergent_expected(C.convergent_case(value_scene))


# ---- 7 -------------------------------------------------------------------------------------------------------------------------------------

def test_many_pois_case(value_scene):
    small, big, fifty = C.many_cases(value_scene)
    assert len(big["q"]) == C.MANY and np.array_equal(big["q"][:50], fifty["q"]) and np.array_equal(big["q"][50:100], fifty["q"])
    assert C.same_bits(big["init"][69950:70000], fifty["init"])
    want, w32 = C.expected(fifty, [1] * 50)
    show("50 POIs r=2 trilinear", want, w32, 2)
