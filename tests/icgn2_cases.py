"""The cases of tests/test_gpu_icgn2_edges.py and tests/test_icgn2_edges_cpu.py, built in one place so that the two files cannot drift
apart: test infrastructure only.  A case is a dict (R, T, q, init, opts and, for a B-spline target given as coefficients, coef) that
`restate` hands to the NumPy restatement (tests/icgn2_ref.py) and the GPU file hands to capi.icgn2.  The CPU file asserts on the
restatement alone every precondition the GPU file relies on; the functions that compute such a precondition live here and are called
by both.  The bars are test_agrees_with_restatement's: 1e-4 for u, 1e-5 for the first derivatives, 2e-5 / r for the second
derivatives and 1e-5 for zncc, each widened to 4 x the gap between the restatement's fp32 and fp64 forms on the case."""
import numpy as np

import bspline_ref
import icgn2_ref as ref2
import icgn_ref as ref

KINDS = {0: "keys", 1: "linear", 2: "bspline"}
COLS = {"u": ref2.DISP, "first": ref2.FIRST, "second": ref2.SECOND}
FIELDS = ("p", "zncc", "last_step", "iterations", "status")
EPS = 2.0 ** -40


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.uint64), np.asarray(b, np.float64).view(np.uint64))


def case(R, T, q, init, r, kind, iterations=2, tolerance=0.0, coef=False):
    return dict(R=R, T=T, q=np.asarray(q, np.int32).reshape(-1, 3), init=None if init is None else np.asarray(init, np.float64).reshape(-1, 30),
                opts=dict(subset_radius=r, max_iterations=iterations, tolerance=tolerance, interpolation=kind), coef=coef)


def restate(c, f32=False):
    return ref2.icgn2(c["R"], c["T"], c["q"], init=c["init"], f32=f32, coefficients_given=c["coef"], **c["opts"])


def base_bars(r):
    return {"u": 1e-4, "first": 1e-5, "second": 2e-5 / r, "zncc": 1e-5}


def gaps(a, b, rows=None):
    """the largest |a - b| per quantity over the rows whose parameters are finite in b"""
    rows = np.arange(len(b["p"])) if rows is None else np.asarray(rows)
    rows = rows[np.isfinite(b["p"][rows]).all(1)] if len(rows) else rows
    out = {}
    for name, cols in COLS.items():
        out[name] = float(np.abs(a["p"][rows][:, cols] - b["p"][rows][:, cols]).max()) if len(rows) else 0.0
    for name in ("zncc", "last_step"):
        out[name] = float(np.abs(a[name][rows] - b[name][rows]).max()) if len(rows) else 0.0
    return out


def bars_of(want, w32, r, rows=None):
    """the bars of a case: (bars, e) with e the fp32-minus-fp64 restatement gaps; last_step takes u's bar"""
    e = gaps(w32, want, rows)
    b = {k: max(v, 4 * e[k]) for k, v in base_bars(r).items()}
    b["last_step"] = b["u"]
    return b, e


def agree(got, want, w32, r, what, rows=None, last_step=False):
    """statuses and iteration counts equal, non-finite parameter rows equal bit for bit, every gap within its bar; prints both"""
    assert np.array_equal(got["status"], want["status"]), (what, list(got["status"]), list(want["status"]))
    assert np.array_equal(got["iterations"], want["iterations"]), (what, list(got["iterations"]), list(want["iterations"]))
    for i in np.flatnonzero(~np.isfinite(want["p"]).all(1)):
        assert same_bits(got["p"][i], want["p"][i]), (what, i)
    bars, e = bars_of(want, w32, r, rows)
    g = gaps(got, want, rows)
    names = list(base_bars(r)) + (["last_step"] if last_step else [])
    print(what, "status", list(want["status"]), "| got - restatement",
          " ".join(f"{k} {g[k]:.2e} (fp32 - fp64 {e[k]:.2e}, bar {bars[k]:.2e})" for k in names))
    for k in names:
        assert g[k] <= bars[k], (what, k, g[k], bars[k])
    return g


def expected(c, status=None):
    """the fp64 and fp32 restatements of a case, with equal statuses and iteration counts (status: and these statuses)"""
    want, w32 = restate(c), restate(c, f32=True)
    assert np.array_equal(want["status"], w32["status"]) and np.array_equal(want["iterations"], w32["iterations"]), (want["status"], w32["status"])
    if status is not None:
        assert list(want["status"]) == list(status), (list(want["status"]), list(status))
    return want, w32


def init_returned(got, init, status, rows):
    for i in rows:
        assert got["status"][i] == status, (i, got["status"][i], status)
        assert same_bits(got["p"][i], init[i]), i
        assert got["iterations"][i] == 0 and got["zncc"][i] == 0 and got["last_step"][i] == 0, i


def equal_results(a, b, rows_a=None, rows_b=None):
    ra = slice(None) if rows_a is None else rows_a
    rb = slice(None) if rows_b is None else rows_b
    for k in FIELDS:
        if a[k].dtype == np.float64:
            assert same_bits(a[k][ra], b[k][rb]), k
        else:
            assert np.array_equal(a[k][ra], b[k][rb]), k


def blobs(shape, seed, per=512):
    nz, ny, nx = shape
    b = max(8, nz * ny * nx // per)
    rng = np.random.Generator(np.random.PCG64(seed))
    c = np.stack([rng.uniform(0, nx, b), rng.uniform(0, ny, b), rng.uniform(0, nz, b)], 1)
    return ref.render(shape, c, rng.uniform(1.5, 4.5, b), rng.uniform(0.3, 1.3, b))


def prow(u=(0.0, 0.0, 0.0), **terms):
    """30 parameters from (u, v, w) and named terms: ux, vy, wxx, uxy, ..."""
    names = ("", "x", "y", "z", "xx", "yy", "zz", "xy", "xz", "yz")
    p = np.zeros(30)
    p[ref2.DISP] = u
    for k, v in terms.items():
        p[10 * "uvw".index(k[0]) + names.index(k[1:])] = v
    return p


def perturbed(tr, rng, du=0.25, d1=0.005, d2=0.0005):
    k = np.arange(30) % 10
    return tr + rng.uniform(-1, 1, tr.shape) * np.where(k == 0, du, np.where(k < 4, d1, d2))


def coefficients(T):
    """the B-spline coefficients the GPU would make of T (float32 prefilter): a target to pass with coef=True"""
    return bspline_ref.prefilter(T, f32=True)


def tap_voxels(shape, p, q, r, kind):
    """the set of linear voxel indices of T under a tap of the subset at the parameters p"""
    pos = ref2.warp(p, np.asarray(q, np.float64), ref.offsets(r))
    fl = np.floor(pos).astype(np.int64)
    off = (0, 1) if kind == 1 else (-1, 0, 1, 2)
    nz, ny, nx = shape
    out = set()
    for oz in off:
        for oy in off:
            for ox in off:
                out.update((((fl[:, 2] + oz) * ny + fl[:, 1] + oy) * nx + fl[:, 0] + ox).tolist())
    return out


# ---- 1. every radius, a spike on a sentinel voxel of the walk ------------------------------------------------------------------------

PAD = 6             # voxels between the subset and the window's faces: R's margin (1), T's taps (2), the shift (1), its error and the steps (2)
SHIFT = (1, -1, 1)  # T(x + SHIFT) = R(x): the true displacement
SPIKE_N = 2 * 32 + 1 + 2 * PAD + 2
CUBIC_RADII = (2, 3, 8, 17, 32)
SPIKE = [(r, 1) for r in range(2, 33)] + [(r, k) for r in CUBIC_RADII for k in (0, 2)]


def spike_volume():
    return blobs((SPIKE_N,) * 3, seed=21)


sentinels = ref.sentinels  # the first-order file's: one walk, one definition


def spike_sentinels(r, kind):
    """every sentinel for the trilinear runs, four for the cubic ones (the restatement gathers 64 taps for each of up to 3e5 voxels)"""
    s = sentinels(r)
    if kind == 1:
        return s
    return {n: s[n] for n in [n for n in ("first", "last", "i256", "zcarry", "rand0", "rand1", "rand2", "rand3") if n in s][:4]}


def spike_amplitude(r):
    """one rule in r: several blob amplitudes (<= 1.3) at the small radii, growing with the subset, as one voxel's share of the sums
    falls as 1 / N"""
    return max(1.5, 5.0 * (r / 4.0) ** 1.5)


def spike_init(r, rng):
    """near the truth, by one rule in r: u within 0.2 s, the first-order terms within 0.05 s / r and the second-order ones within
    0.05 s / r^2 (each term moves a corner by at most 0.05 voxel), with s = min(1, 0.015 r^2): 1 from r = 9, 0.06 at r = 2.  The
    narrowing is what the smallest subsets need under a spike: a few hundred voxels do not hold 30 parameters against more (with
    s = 0.03 r^2 a first step of the restatement at r = 3 is 1.3 voxel and the second leaves the window, status 3; with
    s = 0.007 r^2 a sentinel of r = 2 moves p by 73 bars only)"""
    p = np.zeros(30)
    s = min(1.0, 0.015 * r * r)
    p[ref2.DISP] = np.array(SHIFT) + s * rng.uniform(-0.2, 0.2, 3)
    p[ref2.FIRST] = s * rng.uniform(-0.05, 0.05, 9) / r
    p[ref2.SECOND] = s * rng.uniform(-0.05, 0.05, 18) / (r * r)
    return p


def spike_cases(V, r, kind):
    """name -> (case, the same case with the sentinel voxel's spike zeroed in R alone, the subset index, the offset d)"""
    D = 2 * r + 1
    n = D + 2 * PAD
    o = V.shape[0] // 2 - n // 2
    q = np.array([[r + PAD] * 3], np.int32)
    amp = spike_amplitude(r)
    rng = np.random.default_rng(50 * r)
    inits = {name: spike_init(r, rng) for name in sentinels(r)}
    out = {}
    for name, i in spike_sentinels(r, kind).items():
        d = np.array([i % D - r, (i // D) % D - r, i // (D * D) - r])
        W = V.copy()
        s = o + q[0] + d
        W[s[2], s[1], s[0]:s[0] + 2] += amp
        R = W[o:o + n, o:o + n, o:o + n].copy()
        T = W[o - SHIFT[2]:o - SHIFT[2] + n, o - SHIFT[1]:o - SHIFT[1] + n, o - SHIFT[0]:o - SHIFT[0] + n].copy()
        at = (q[0, 2] + d[2], q[0, 1] + d[1], q[0, 0] + d[0])
        assert R[at] >= amp and T.max() >= amp
        R0 = R.copy()
        R0[at] -= np.float32(amp)
        c = case(R, T, q, inits[name], r, kind)
        out[name] = (c, dict(c, R=R0), i, d)
    return out


def spike_expected(c, c0, r, what):
    """the restatements of a spike case (status 1 after two iterations) and its sensitivity: zeroing the sentinel voxel in R alone
    moves the restatement's p by `sens` times the bar used for the case (the largest ratio over the parameter classes); >= 100"""
    want, w32 = expected(c, [1])
    assert want["iterations"][0] == 2
    bars, e = bars_of(want, w32, r)
    moved = gaps(restate(c0), want)
    sens = max(moved[k] / bars[k] for k in COLS)
    print(f"{what}: amplitude {spike_amplitude(r):.1f}, fp32 - fp64 u {e['u']:.2e} first {e['first']:.2e} second {e['second']:.2e}; zeroing the "
          f"sentinel in R moves p by {sens:.0f} bars")
    assert sens >= 100, (what, sens)
    return want, w32, sens


# ---- 2. pivoted composition ------------------------------------------------------------------------------------------------------------

# starts 0.6 to 1.5 voxel from the truth: each axis in each sign, and two mixed directions (|.| = 1.28, 1.39); one per POI of ref2.POIS
STARTS = np.array([(0.6, 0, 0), (-0.8, 0, 0), (0, 1.3, 0), (0, -0.6, 0), (0, 0, 0.8), (0, 0, -1.3), (0.7, -0.6, 0.9), (-1.1, 0.5, -0.7)])
PIVOT = [(r, k, it) for r in (5, 10) for k in (0, 1, 2) for it in (1, 2)]


def pivot_case(scene, r, kind, iterations):
    R, T, truth = scene
    init = truth(ref2.POIS)
    init[:, ref2.DISP] += STARTS
    return case(R, T, ref2.POIS, init, r, kind, iterations)


def pivot_expected(c):
    """every run ends with status 1 and the first iteration's permutation is the identity for no POI; returns the restatements and
    the first permutations"""
    want, w32 = expected(c, [1] * len(STARTS))
    first = [pm[0] for pm in want["perms"]]
    ident = tuple(range(10))
    assert all(pm is not None and pm != ident for pm in first), first
    assert [pm[0] for pm in w32["perms"]] == first
    return want, w32, first


def exchanged_columns(perm):
    """the columns k at which the LU that ended with `perm` exchanged rows (replayed: at step k the row that ends at k is fetched)"""
    cur, cols = list(range(10)), []
    for k in range(10):
        j = cur.index(perm[k])
        if j != k:
            cur[k], cur[j] = cur[j], cur[k]
            cols.append(k)
    return cols


# ---- 3. axes, strides and sizes ----------------------------------------------------------------------------------------------------------

ODD_SHAPE = (48, 52, 60)                       # the scene (nz, ny, nx)
ODD_R_AT, ODD_R_SHAPE = (6, 0, 3), (40, 52, 46)  # R = scene[6:46, 0:52, 3:49]
ODD_T_AT, ODD_T_SHAPE = (0, 7, 0), (44, 38, 60)  # T = scene[0:44, 7:45, 0:60]: T.ny < T.nz
ODD_G = ((0.01, 0.06, -0.02), (0.0, -0.03, 0.04), (0.03, 0.0, -0.05))  # asymmetric
ODD_Q = ((0.002, -0.001, 0.0015, 0.001, 0.0, 0.0005), (-0.0015, 0.001, -0.0005, 0.0, 0.002, 0.0), (0.0005, 0.002, -0.001, 0.001, 0.0, -0.002))
ODD_MID = np.array([25, 25, 17])  # in R's frame; in T's: (28, 18, 23)
ODD = [(r, k) for r in (4, 9) for k in (0, 1, 2)]


def odd_scene():
    R, T, truth = ref2.quadratic_scene(ODD_SHAPE, t=(0.37, -0.52, 0.21), G=ODD_G, Q=ODD_Q, seed=31)
    (rz, ry, rx), (tz, ty, tx) = ODD_R_AT, ODD_T_AT
    Rc = np.ascontiguousarray(R[rz:rz + ODD_R_SHAPE[0], ry:ry + ODD_R_SHAPE[1], rx:rx + ODD_R_SHAPE[2]])
    Tc = np.ascontiguousarray(T[tz:tz + ODD_T_SHAPE[0], ty:ty + ODD_T_SHAPE[1], tx:tx + ODD_T_SHAPE[2]])
    assert Rc.shape == ODD_R_SHAPE and Tc.shape == ODD_T_SHAPE
    move = np.array([rx - tx, ry - ty, rz - tz], np.float64)  # R's frame -> T's frame

    def truth_c(q):
        p = truth(np.asarray(q) + np.array([rx, ry, rz]))
        p[:, ref2.DISP] += move
        return p

    return Rc, Tc, truth_c


def widened_top(p, r):
    """per axis: how far above q + u the widened corner of the domain rule lies"""
    e = np.asarray(p).reshape(3, 10)
    F = e[:, 1:4] + np.eye(3)
    return np.abs(F).sum(1) * r + r * r * (0.5 * np.abs(e[:, 4:7]).sum(1) + np.abs(e[:, 7:]).sum(1))


def odd_stepper(scene, r, kind, hi, axis, cell):
    """a POI within 3 voxels of ODD_MID's line along `axis` whose true widened corner lies in the cell hi[axis] + cell of T, started 0.25 voxel
    below T's limit (cell 1: the truth is outside, the first step leaves T) or 0.15 voxel below the last admissible cell (cell 0: the
    truth is 0.1 to 0.6 voxel inside it, and the steps end there), for which the restatement does just that: (q, init row).  A subset of a few hundred voxels
    estimates its second-order terms, and with them the widening B, to a few tenths of a voxel, so not every candidate does"""
    R, T, truth = scene
    for v in range(r + 1, (ODD_R_SHAPE[2 - axis] - 2 - r) + 1):
        for o in range(49):
            q = ODD_MID.copy()
            q[axis] = v
            q[(axis + 1) % 3] += o % 7 - 3
            q[(axis + 2) % 3] += o // 7 - 3
            p = truth(q[None])[0]
            frac = q[axis] + p[10 * axis] + widened_top(p, r)[axis] - (hi[axis] + cell)
            if not (0.1 <= frac <= (0.9 if cell else 0.6)):
                continue
            p[10 * axis] -= frac + (0.25 if cell else 0.15)
            w = ref2.refine(R, T, q, init=p, subset_radius=r, max_iterations=3, tolerance=0.0, interpolation=kind)
            top = q[axis] + w["p"][10 * axis] + widened_top(w["p"], r)[axis]
            left = w["status"] == 3 and w["iterations"] == 0 and w["last_step"] > 0.3
            if left if cell else (w["status"] == 1 and np.floor(top) == hi[axis]):
                return q, p
    raise AssertionError("no such POI")


def odd_case(scene, r, kind):
    """10 POIs; 0..7 lie about ODD_MID and start near the truth.  POI 6's widened corner passes T's last admissible y by half a
    voxel (status 3 at the start; T.nz as the y limit would accept it); POI 7's ends half a voxel inside T's last admissible z cell,
    beyond T.ny (T.ny as the z limit would refuse it): it passes the start's domain test and computes a step.  Its init is placed by
    the edge, some 15 voxels from the truth, so that step is no refinement: the composed p leaves T and the POI ends with status 3,
    0 iterations and the step's norm in last_step, which a refusal at the start (last_step 0) would not give.  POIs 8 and 9 reach
    the same two places by a step from near the truth (odd_stepper): 8 leaves T's y range, 9 ends with status 1 inside the last z
    cell"""
    R, T, truth = scene
    rng = np.random.default_rng(7 * r + kind)
    q = np.concatenate([ODD_MID + rng.integers(-3, 4, (8, 3)), np.zeros((2, 3), np.int64)])
    hi = np.array([ODD_T_SHAPE[2], ODD_T_SHAPE[1], ODD_T_SHAPE[0]]) - 1 - (1 if kind == 1 else 2)  # the largest admissible floor
    q[8], p8 = odd_stepper(scene, r, kind, hi, 1, 1)
    q[9], p9 = odd_stepper(scene, r, kind, hi, 2, 0)
    init = perturbed(truth(q), rng, 0.25, 0.003, 0.0003)
    init[6, 10] = hi[1] + 1.5 - q[6, 1] - widened_top(init[6], r)[1]
    init[7, 20] = hi[2] + 0.5 - q[7, 2] - widened_top(init[7], r)[2]
    init[8], init[9] = p8, p9
    assert hi[2] - 1 > ODD_T_SHAPE[1] - 1 and hi[1] + 1 < hi[2]
    return case(R, T, q, init, r, kind, iterations=3)


def odd_expected(c, r, kind):
    want, w32 = expected(c)
    cubic = kind != 1
    hi = np.array([ODD_T_SHAPE[2], ODD_T_SHAPE[1], ODD_T_SHAPE[0]]) - 1 - (2 if cubic else 1)
    assert want["status"][6] == 3 and want["iterations"][6] == 0
    swapped = (ODD_T_SHAPE[1], ODD_T_SHAPE[0], ODD_T_SHAPE[2])  # ny and nz exchanged
    assert ref2.in_domain(swapped, c["init"][6], c["q"][6], r, cubic) and not ref2.in_domain(swapped, c["init"][7], c["q"][7], r, cubic)
    for i in (7, 8, 9):
        assert ref2.in_domain(ODD_T_SHAPE, c["init"][i], c["q"][i], r, cubic), i
    # 7: accepted at the start (a step was computed), then the composed p leaves T: not a refusal, whose last_step is 0
    assert (want["status"][:6] == 1).all() and want["last_step"][7] > 0, (want["status"], want["last_step"])
    assert want["status"][7] == 3 and want["iterations"][7] == 0, (want["status"][7], want["iterations"][7])
    assert same_bits(want["p"][7], c["init"][7])
    # 8: the first step leaves T's y range (the start comes back with the step's norm); it would not with T.nz as the y limit
    assert want["status"][8] == 3 and want["iterations"][8] == 0 and want["last_step"][8] > 0.3, (want["status"][8], want["last_step"][8])
    # 9: the steps end inside T's last admissible z cell, beyond T.ny
    p9 = want["p"][9]
    top = c["q"][9, 2] + p9[20] + widened_top(p9, r)[2]
    assert want["status"][9] == 1 and np.floor(top) == hi[2] and top > ODD_T_SHAPE[1], (want["status"][9], top)
    assert not ref2.in_domain(swapped, p9, c["q"][9], r, cubic)
    return want, w32


# ---- 4. exact edges ----------------------------------------------------------------------------------------------------------------------

EDGE_Q = np.array([23, 26, 20])
EDGE_SHAPE = (40, 52, 46)
EDGE_FRAC = 0.45  # the true displacement lies this far inside the edge position


def R_edge_case(kind=0):
    """q = r + 1 and q = n - 2 - r (rows 0..5: they read R's outermost voxels) and q = r, q = n - 1 - r (rows 6..11: status 2), every
    axis and side"""
    r, pad = 4, 4
    nz, ny, nx = EDGE_SHAPE
    V = blobs((nz + 2 * pad, ny + 2 * pad, nx + 2 * pad), seed=33)
    R, T = V[pad:pad + nz, pad:pad + ny, pad:pad + nx].copy(), V  # R(x) = T(x + pad)
    n = np.array([nx, ny, nz])
    runs, outside = [], []
    for a in range(3):
        for inner, outer in ((r + 1, r), (n[a] - 2 - r, n[a] - 1 - r)):
            for lst, v in ((runs, inner), (outside, outer)):
                q = n // 2
                q[a] = v
                lst.append(q)
    rng = np.random.default_rng(5)
    init = perturbed(np.tile(prow((pad, pad, pad)), (12, 1)), rng, 0.2, 0.003, 0.0003)
    return case(R, T, np.array(runs + outside), init, r, kind), r


def edge_volumes(axis, side, kind, r, frac=EDGE_FRAC):
    """R, T and the integer displacement k_in along `axis` whose extreme tap is T's last (side 1) or first (side 0) voxel; the true
    displacement is k_in -+ frac (towards T's inside), zero along the other axes"""
    t = np.zeros(3)
    t[axis] = -frac if side else frac
    R, T, _ = ref.scene(EDGE_SHAPE, tvec=t, seed=34, per=128)  # a dense texture: see T_edge_expected
    taps_hi, taps_lo = (1, 0) if kind == 1 else (2, 1)
    cut = [slice(None)] * 3
    if side:
        n = EDGE_Q[axis] + r + 1 + taps_hi  # floor(q + r + 0) + taps_hi = n - 1
        cut[2 - axis] = slice(0, n)
        k_in = 0
    else:
        x0 = EDGE_Q[axis] - r - taps_lo  # floor(q - r - x0) - taps_lo = 0
        cut[2 - axis] = slice(x0, None)
        k_in = -x0
    return R, np.ascontiguousarray(T[tuple(cut)]), k_in


T_EDGES = [(a, s, k) for a in range(3) for s in (0, 1) for k in (0, 1, 2)]
T_EDGE_R = 5


def T_edge_case(axis, side, kind):
    """rows: 0 the extreme tap on T's first / last voxel (runs), 1 one voxel further (status 3), 2 just inside (upper: 2^-40 below
    the first outside integer, whose fp32 fraction rounds to 1; lower: 2^-40 above k_in), 3 just outside"""
    R, T, k_in = edge_volumes(axis, side, kind, T_EDGE_R)
    out = k_in + 1 if side else k_in - 1
    init = np.zeros((4, 30))
    init[:, 10 * axis] = [k_in, out, out - EPS if side else k_in + EPS, out if side else k_in - EPS]
    return case(R, T, np.tile(EDGE_Q, (4, 1)), init, T_EDGE_R, kind)


def T_edge_expected(c):
    """rows 1 and 3 are refused at the start; rows 0 and 2 run from taps on T's outermost voxels and stay inside: status 1 after two
    iterations.  That needs the dense texture of edge_volumes: a step's second-order terms widen the corner by B, and on one
    blob per 512 voxels a subset of r = 5 estimates them to a few tenths of a voxel, more than the 0.45 voxel between the truth
    and the edge, so that most composed p left T again (status 3)"""
    want, w32 = expected(c, [1, 3, 1, 3])
    assert list(want["iterations"]) == [2, 0, 2, 0] and not want["last_step"][[1, 3]].any()
    return want, w32


QUAD_EDGE_R, QUAD_EDGE_B = 4, 0.25
QUAD_EDGES = [(a, k) for a in range(3) for k in (0, 1, 2)]


def quad_edge_case(axis, kind):
    """T's upper edge reached through the quadratic part alone: zero first-order terms and one second-order term of component `axis`
    whose widening is B = 0.25 (r = 4: r^2 c is exact), u = 1 - 2^-40 - B, so that the widened corner, which is the true position
    of a corner voxel of the subset, ends 2^-40 below the first outside integer.  Rows: 0 a mixed term (xy on the x axis, yz on y,
    xz on z) inside, 1 the square of another axis (zz; yy on the z axis) inside, 2 and 3 the same two with u = 1 - B: on the
    integer, status 3"""
    r = QUAD_EDGE_R
    R, T, _ = edge_volumes(axis, 1, kind, r, frac=0.2)
    mixed = {0: 7, 1: 9, 2: 8}[axis]
    square = 6 if axis != 2 else 5
    init = np.zeros((4, 30))
    for i, (k, c) in enumerate(((mixed, QUAD_EDGE_B / (r * r)), (square, 2 * QUAD_EDGE_B / (r * r))) * 2):
        init[i, 10 * axis + k] = c
        init[i, 10 * axis] = 1.0 - QUAD_EDGE_B - (EPS if i < 2 else 0.0)
    return case(R, T, np.tile(EDGE_Q, (4, 1)), init, r, kind), r


def quad_edge_preconditions(c, r, kind, axis):
    """rows 0, 1: inside the domain, and a corner voxel's true position lies within 2^-39 of the end of the last admissible cell (its fp32
    fraction rounds to 1); rows 2, 3: outside"""
    cubic = kind != 1
    n = c["T"].shape[2 - axis]
    for i in range(4):
        assert ref2.in_domain(c["T"].shape, c["init"][i], c["q"][i], r, cubic) == (i < 2), i
    corners = np.array([[sx, sy, sz] for sz in (-r, r) for sy in (-r, r) for sx in (-r, r)], np.float64)
    for i in range(2):
        top = ref2.warp(c["init"][i], c["q"][i].astype(np.float64), corners)[:, axis].max()
        end = n - (2 if cubic else 1)
        assert 0 < end - top <= 2 * EPS, (i, end - top)
        assert np.float32(top - np.floor(top)) == np.float32(1.0)


WIDEN_R = 4
ULP48 = 2.0 ** -48  # the spacing of the doubles in [16, 32): T's limit here


WIDEN = [(s, k) for s in (1, 0) for k in (0, 1, 2)]


def widen_case(kind, side=1):
    """the widening B on the x axis, each of the six second-order terms of u in turn, r = 4 (r^2 = 16: B is exact).  Upper side:
    B = 0.5 and u = 0.5 - 2^-48, so that q + r + u + B is the last double below the first outside integer (rows 0..5: inside); the
    same with B = 0.5 + 2^-48: on the integer (rows 6..11: status 3).  Lower side: u = k_in + 0.5, so that q - r + u - B is the
    last inside integer itself with B = 0.5 (rows 0..5: inside, floor(mn - B) on the limit) and 2^-48 below it with
    B = 0.5 + 2^-48 (rows 6..11: status 3); a dropped B or a wrong sign in floor(mn - B) accepts rows 6..11 or refuses rows 0..5"""
    r = WIDEN_R
    R, T, k_in = edge_volumes(0, side, kind, r)
    init = np.zeros((12, 30))
    for i in range(12):
        k = 4 + i % 6
        B = 0.5 + (ULP48 if i >= 6 else 0.0)
        init[i, k] = B / (r * r) * (2.0 if k < 7 else 1.0)
        init[i, 0] = 0.5 - ULP48 if side else k_in + 0.5
    return case(R, T, np.tile(EDGE_Q, (12, 1)), init, r, kind), r


def widen_preconditions(c, r, kind, side=1):
    cubic = kind != 1
    lim = float(c["T"].shape[2] - (2 if cubic else 1)) if side else (1.0 if cubic else 0.0)  # upper: the first outside integer; lower: the last inside one
    assert 16 <= lim < 32 or not side
    for i in range(12):
        e = c["init"][i].reshape(3, 10)
        B = r * r * (0.5 * np.abs(e[0, 4:7]).sum() + np.abs(e[0, 7:]).sum())
        assert B == 0.5 + (ULP48 if i >= 6 else 0.0)
        if side:
            top = (float(c["q"][i, 0]) + r) + e[0, 0] + B
            assert top == (lim if i >= 6 else np.nextafter(lim, 0.0)), (i, top, lim)
        else:
            bottom = (float(c["q"][i, 0]) - r) + e[0, 0] - B
            assert bottom == (lim - ULP48 if i >= 6 else lim), (i, bottom, lim)
            assert ref2.in_domain(c["T"].shape, np.where(np.arange(30) < 4, c["init"][i], 0.0), c["q"][i], r, cubic)  # without B: inside
        assert ref2.in_domain(c["T"].shape, c["init"][i], c["q"][i], r, cubic) == (i < 6), i


# ---- 5. statuses ---------------------------------------------------------------------------------------------------------------------------

ST_R, ST_Q = 5, np.array([[20, 20, 20]], np.int32)
ST_SHAPE = (40, 40, 40)


def status_scene():
    return ref2.quadratic_scene(ST_SHAPE, seed=41)


def status_init(scene, q=ST_Q, seed=3):
    return perturbed(scene[2](q), np.random.default_rng(seed), 0.2, 0.003, 0.0003)


def status_case(scene, kind, R=None, T=None, coef=False, init=None, iterations=3):
    return case(scene[0] if R is None else R, scene[1] if T is None else T, ST_Q, status_init(scene) if init is None else init, ST_R, kind,
                iterations, coef=coef)


def ramp_R():
    """R = x, integers: dR > 0, the ten monomials of the x component are independent, and the pivot of v is exactly 0"""
    return np.broadcast_to(np.arange(ST_SHAPE[2], dtype=np.float32), ST_SHAPE).copy()


def constant_targets(scene):
    """T constant, and T = (float)Rm of the POI's subset"""
    R = scene[0]
    w = ref.offsets(ST_R).astype(int) + ST_Q[0]
    rm = np.float32(R[w[:, 2], w[:, 1], w[:, 0]].astype(np.float64).mean())
    return [np.full(ST_SHAPE, c, np.float32) for c in (np.float32(0.75), rm)]


def nonfinite_R(scene):
    R = scene[0]
    x, y, z = ST_Q[0]
    out = {}
    for what, at, v in (("NaN in the subset", (z + 2, y - 1, x + ST_R), np.nan), ("+Inf in the subset", (z, y + 3, x - 2), np.inf),
                        ("NaN in the x margin only", (z, y, x + ST_R + 1), np.nan), ("NaN in the z margin only", (z - ST_R - 1, y + 1, x), np.nan)):
        Rb = R.copy()
        Rb[at] = v
        out[what] = Rb
    return out


def target_of(scene, kind):
    """(T, coef): the volume itself, or for the B-spline its coefficients, in which a planted voxel stays one voxel"""
    return (coefficients(scene[1]), True) if kind == 2 else (scene[1], False)


def nonfinite_T(scene, kind):
    """a NaN, +Inf and -Inf under a tap of the centre voxel and of a corner voxel (B-spline: planted in the coefficients)"""
    T, coef = target_of(scene, kind)
    x, y, z = ST_Q[0]
    out = {}
    for v in (np.nan, np.inf, -np.inf):
        for where, at in (("centre", (z, y, x)), ("corner", (z + ST_R, y - ST_R, x + ST_R))):
            Tb = T.copy()
            Tb[at] = v
            out[f"{v} under the {where} voxel"] = (Tb, at)
    return out, coef


def untouched_T(scene, kind):
    """(clean T, T with two NaN voxels that no tap of any iteration touches, coef)"""
    T, coef = target_of(scene, kind)
    x, y, z = ST_Q[0]
    Tb = T.copy()
    Tb[1, 2, 3] = np.nan
    Tb[z + ST_R + 6, y, x] = np.nan
    return T, Tb, coef


LATE_START = (0.8, -0.7, 0.75)  # the start's distance from the truth: the first step moves the taps by most of a voxel


def late_nan_case(scene, kind):
    """status 4 after a step: (case, the clean case, the NaN voxel): a voxel of T that the start's taps miss and the taps of the
    restatement's second iteration reach"""
    T, coef = target_of(scene, kind)
    init = scene[2](ST_Q)
    init[:, ref2.DISP] += LATE_START
    clean = status_case(scene, kind, T=T, coef=coef, init=init, iterations=2)
    one = restate(dict(clean, opts=dict(clean["opts"], max_iterations=1)))
    assert one["status"][0] == 1 and one["iterations"][0] == 1
    first, second = (tap_voxels(T.shape, p, ST_Q[0], ST_R, kind) for p in (init[0], one["p"][0]))
    new = sorted(second - first)
    assert new, "the second iteration reaches no new voxel"
    at = np.unravel_index(new[len(new) // 2], T.shape)
    Tb = T.copy()
    Tb[at] = np.nan
    return dict(clean, T=Tb), clean, at, one


def order_case(scene, kind=0):
    """5 before 2 before 4 before 3 in one call, alternating with healthy POIs: rows 0 (a NaN init, outside R: 5), 2 (outside R, over
    constant R: 2), 4 (constant R, the init outside T: 4), 6 (the init outside T: 3); rows 1, 3, 5, 7 healthy"""
    R, T, truth = scene
    R = R.copy()
    R[:, :, :14] = 0.5  # a constant slab at the low x end, wide enough for a subset and its margin (2 r + 3 = 9 voxels)
    r = 3
    healthy = np.array([[24, 20, 20], [26, 24, 18], [22, 17, 25], [25, 22, 21]], np.int32)
    hinit = status_init(scene, healthy, seed=4)
    bad = np.array([[1, 20, 20], [r, 20, 20], [6, 20, 20], [23, 21, 19]], np.int32)
    binit = np.zeros((4, 30))
    binit[0, 16] = np.nan   # a NaN init outside R: 5 before 2
    binit[1, 0] = 0.25      # outside R, over constant R: 2 before 4
    binit[2, 20] = 100.0    # constant R, outside T: 4 before 3
    binit[3, 10] = -100.0   # outside T
    order = [0, 4, 1, 5, 2, 6, 3, 7]
    c = case(R, T, np.concatenate([bad, healthy])[order], np.concatenate([binit, hinit])[order], r, kind, iterations=3)
    return c, case(R, T, healthy, hinit, r, kind, iterations=3)


ORDER_STATUS = [5, 1, 2, 1, 4, 1, 3, 1]


# ---- 6. values -----------------------------------------------------------------------------------------------------------------------------

def value_scene():
    R, T, truth = ref2.quadratic_scene((48, 48, 48), seed=51, per=128)  # a dense texture: a 13^3 subset converges within 20 iterations
    rng = np.random.default_rng(52)
    q = rng.integers(16, 32, (60, 3)).astype(np.int32)
    init = perturbed(truth(q), rng, 0.3, 0.004, 0.0004)
    return R, T, q, init, truth


OFFSETS = [(m, b, r) for m in ("both", "T", "R") for b in (-1024.0, 1000.0, 32768.0) for r in (5, 16)]
SCALINGS = {"both_2^-10": (2.0 ** -10, 2.0 ** -10), "both_2^13": (2.0 ** 13, 2.0 ** 13), "T_2^7": (1.0, 2.0 ** 7), "negated": (-1.0, -1.0)}


def offset_case(vs, which, b, r):
    R, T, q, _, truth = vs
    Rb = (R + np.float32(b)).astype(np.float32) if which in ("both", "R") else R
    Tb = (T + np.float32(b)).astype(np.float32) if which in ("both", "T") else T
    q = q[(q >= r + 3).all(1) & (q <= 44 - r).all(1)][:5]
    assert len(q) == 5
    init = perturbed(truth(q), np.random.default_rng(int(abs(b)) + r), 0.2, 0.002, 0.0002)
    return case(Rb, Tb, q, init, r, 0, iterations=1)


def scaling_case(vs, name, kind):
    R, T, q, init, _ = vs
    a, b = SCALINGS[name]
    base = case(R, T, q[:16], init[:16], 6, kind, iterations=20, tolerance=1e-3)
    return base, dict(base, R=np.float32(a) * R, T=np.float32(b) * T)


CONV_TOL = float(np.float32(1e-3))


def convergent_case(vs):
    R, T, q, init, _ = vs
    return case(R, T, q, init, 6, 0, iterations=20, tolerance=CONV_TOL)


def convergent_expected(c):
    """the restatement's run, and the POIs with a step within 1 % of the tolerance (at most 10 %; at least 80 % reach status 0)"""
    want = restate(c)
    near = np.array([any(abs(s - CONV_TOL) <= 0.01 * CONV_TOL for s in st) for st in want["steps"]])
    print("convergent runs: excluded", int(near.sum()), "of", len(near), "iterations", np.bincount(want["iterations"]), "status",
          np.bincount(want["status"]))
    assert near.mean() <= 0.10
    assert (want["status"] == 0).mean() >= 0.8
    return want, near


# ---- 7. many POIs --------------------------------------------------------------------------------------------------------------------------

MANY, MANY_DISTINCT = 70000, 50


def many_cases(vs):
    """(the 7-POI case, the 70 000-POI case tiled from 50, the 50-POI case)"""
    R, T, q, init, _ = vs
    k = MANY_DISTINCT
    rep = -(-MANY // k)
    small = case(R, T, q[:7], init[:7], 2, 1)
    big = case(R, T, np.tile(q[:k], (rep, 1))[:MANY], np.tile(init[:k], (rep, 1))[:MANY], 2, 1)
    return small, big, case(R, T, q[:k], init[:k], 2, 1)
