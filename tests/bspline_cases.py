"""The cases of tests/test_gpu_bspline_edges.py and of the edge part of tests/test_bspline_cpu.py, built in one place so that the two
files cannot drift apart: test infrastructure only.  Part A: the shapes at which sift3d_bspline_prefilter must return the bytes of
bspline_ref.prefilter(T, f32=True) -- every seam of k_bspline_axis' 64 x 64 tiles -- and the two deliberately wrong restatements
the old tolerance could not tell from the right one.  Part B: the battery of tests/test_gpu_icgn_edges.py for sift3d_icgn_bspline.
The builders, tables and bars of that file are imported, not copied; what it builds inside a test function is rebuilt here with the
same seeds and the same draws.  A case is a dict (R, T, C, q, init, opts): C = bspline_ref.prefilter(T, f32=True) is what the GPU is
given with coefficients=True and what `restate` interpolates, so the IC-GN kernel is judged on identical coefficient bits."""
import numpy as np

import bspline_ref as bref
import icgn_ref as ref
import test_gpu_bspline as tgb
import test_gpu_icgn_edges as ke

DISP, GRAD = ke.DISP, ke.GRAD
FIELDS = ke.FIELDS


# ---- A. the prefilter ---------------------------------------------------------------------------------------------------------------

KINDS = ("noise", "ct")
ALL_SEAMS = (65, 66, 130)


volume = tgb.volume  # the inputs of test_gpu_bspline: uniform noise in [-1, 1), CT-like integers around 30000


def prefilter_shapes():
    """(nz, ny, nx), the smallest that reach each path of k_bspline_axis (a workgroup: 64 outputs along the axis by 64 lines; the
    lines are the ny * nz rows in the x pass, 64 consecutive x in the y and z passes), each shape once"""
    out = []

    def add(*s):
        if s not in out:
            out.append(s)

    for n in (63, 64, 65, 128, 129):  # a seam of the 64-output tiles along each axis in turn
        add(3, 5, n), add(3, n, 5), add(n, 3, 5)
    add(3, 5, 65), add(3, 5, 130)     # a second and a third, partial tile of lines (x) in the y and z passes
    add(13, 5, 7), add(8, 8, 7)       # 65 rows: the x pass's second row tile holds one row; exactly 64 rows
    for n in range(1, 18):            # mirrors folded repeatedly (n <= K) and the first n that needs no fold
        add(3, 3, n), add(3, n, 3), add(n, 3, 3)
    add(*ALL_SEAMS)
    return out


def kernel_taps():
    """h_1 .. h_K the way make_taps() of kernels_bspline.hip forms them: powers by repeated multiplication in fp64 from the literal
    1.7320508075688772 - 2.0, their sum in index order, one rounding to float32"""
    z1 = 1.7320508075688772 - 2.0
    pw, s = [1.0], 0.0
    for k in range(1, bref.K + 1):
        pw.append(pw[-1] * z1)
        s += pw[k]
    return np.array([np.float32(pw[k] / (1.0 + 2.0 * s)) for k in range(1, bref.K + 1)], np.float32)


MUTANTS = {"ascending k": range(1, bref.K + 1), "tap 16 dropped": range(bref.K - 1, 0, -1)}


def zero_or_normal(a):
    a = np.abs(np.asarray(a, np.float32))
    return bool(np.all((a == 0) | ((a >= np.finfo(np.float32).tiny) & np.isfinite(a))))


def first_difference(got, want):
    """a line for an assertion message: how many voxels differ in bits and the first of them"""
    ne = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    if not len(ne):
        return "same bytes"
    z, y, x = ne[0]
    return f"{len(ne)} of {got.size} voxels differ, the first at (z, y, x) = {(int(z), int(y), int(x))}: {got[z, y, x]!r} against {want[z, y, x]!r}"


# ---- B. first-order IC-GN on the coefficients ---------------------------------------------------------------------------------------

def case(R, T, q, init, **opts):
    T = np.ascontiguousarray(T, np.float32)
    return dict(R=np.ascontiguousarray(R, np.float32), T=T, C=bref.prefilter(T, f32=True), q=np.asarray(q, np.int32).reshape(-1, 3),
                init=None if init is None else np.asarray(init, np.float64).reshape(-1, 12), opts=opts)


def restate(c, f32=False, **more):
    """the restatement of a case on its coefficients; f32: with float32 per-voxel interpolation; more: options over the case's"""
    return bref.icgn(c["R"], c["C"], c["q"], init=c["init"], coefficients_given=True, f32=f32, **dict(c["opts"], **more))


def same_results(a, b):
    """every field of two results (one POI or many) has the same bits"""
    for k in FIELDS:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        if not (np.array_equal(x, y) if x.dtype.kind in "iu" else ke.same_bits(x, y)):
            return False
    return True


# 1. every radius class, a spike on one sentinel voxel of the walk

SPIKE_R = (2, 3, 5, 8, 12, 16, 17, 24, 32)
SPIKE_ALL = 16  # up to this radius every sentinel is used and the sensitivity is asserted; above it, the Keys test's BIG_CUBIC


def spike_cases(volume73, r):
    """test_every_radius_with_sentinel_spikes' construction, window and inits (the same generator, the same draws, one per sentinel
    in the sentinels' order): yields (name, case, at, amp), at the sentinel voxel's (z, y, x) in R"""
    PAD, SHIFT = ke.PAD, ke.SHIFT
    D = 2 * r + 1
    n = D + 2 * PAD
    c = volume73.shape[0] // 2
    o = c - n // 2
    q = np.array([[r + PAD] * 3], np.int32)
    rng = np.random.default_rng(50 * r)
    amp = ke.spike_amplitude(r)
    sent = ke.sentinels(r)
    assert len(sent) >= 6
    e = min(0.2, 0.05 * r)
    inits = {name: np.concatenate([np.array(SHIFT) + rng.uniform(-e, e, 3), rng.uniform(-0.002, 0.002, 9)])[[0, 3, 4, 5, 1, 6, 7, 8, 2, 9, 10, 11]][None]
             for name in sent}
    if r > SPIKE_ALL:
        sent = {name: sent[name] for name in ke.BIG_CUBIC}
    for name, i in sent.items():
        d = np.array([i % D - r, (i // D) % D - r, i // (D * D) - r])
        V = volume73.copy()
        s = o + q[0] + d
        V[s[2], s[1], s[0]:s[0] + 2] += amp
        R = V[o:o + n, o:o + n, o:o + n].copy()
        T = V[o - SHIFT[2]:o - SHIFT[2] + n, o - SHIFT[1]:o - SHIFT[1] + n, o - SHIFT[0]:o - SHIFT[0] + n].copy()
        at = (int(q[0, 2] + d[2]), int(q[0, 1] + d[1]), int(q[0, 0] + d[0]))
        assert R[at] >= amp and T.max() >= amp
        yield name, case(R, T, q, inits[name], subset_radius=r, max_iterations=2, tolerance=0.0), at, amp


def spike_sensitivity(c, at, amp, want):
    """how far, in tolerances, the restatement's p moves when the sentinel voxel's spike is zeroed in R only"""
    R0 = c["R"].copy()
    R0[at] -= np.float32(amp)
    moved = np.abs(bref.refine(R0, c["C"], c["q"][0], init=c["init"][0], coefficients_given=True, **c["opts"])["p"] - want["p"][0])
    return max(moved[DISP].max() / ke.TOL_D, moved[GRAD].max() / ke.TOL_G)


# 2. axes, strides, sizes

ODD_R = (4, 9)
ODD_STATUS, ODD_ITERATIONS = [1, 1, 1, 1, 1, 1, 3, 3], [3, 3, 3, 3, 3, 3, 0, 0]


def odd_case(odd_volumes, r):
    """test_axes_strides_and_sizes' POIs and inits in their tricubic form (the B-spline taps are the tricubic taps), with its two
    rows at T's y and z limits"""
    R, T = odd_volumes
    rng = np.random.default_rng(7 * r)
    q = ke.ODD_Q0 + rng.integers(-3, 4, (8, 3))
    init = np.tile(ke.row(**ke.ODD_P), (8, 1))
    init[:, DISP] += (q - ke.ODD_Q0) @ (ref.F_of(init[0]) - np.eye(3)).T + rng.uniform(-0.3, 0.3, (8, 3))
    F = ref.F_of(init[0])
    top = np.abs(F).sum(1) * r
    hi = np.array([ke.T_SHAPE[2], ke.T_SHAPE[1], ke.T_SHAPE[0]]) - 1 - 2
    init[6, 4] = hi[1] + 1.5 - q[6, 1] - top[1]
    init[7, 8] = hi[2] + 0.5 - q[7, 2] - top[2]
    assert hi[2] - 1 > ke.T_SHAPE[1] - 1 and hi[1] + 1 < hi[2]
    return case(R, T, q, init, subset_radius=r, max_iterations=3, tolerance=0.0)


# 3. T's edges

T_EDGES = [(a, s) for a in range(3) for s in (0, 1)]
T_EDGE_IDS = [f"{'xyz'[a]}-{'upper' if s else 'lower'}" for a, s in T_EDGES]
T_EDGE_STATUS, T_EDGE_ITERATIONS = [1, 3, 1, 3], [2, 0, 2, 0]


def t_edge_case(axis, side):
    """test_T_edges' four rows: 0 the extreme tap on T's first / last voxel, 1 one voxel further, 2 2^-40 inside (upper: the fp32
    fraction rounds to 1), 3 just outside"""
    R, T, k_in = ke.edge_case(axis, side, 0)
    out = k_in + 1 if side else k_in - 1
    u = [k_in, out, out - ke.EPS if side else k_in + ke.EPS, out if side else k_in - ke.EPS]
    init = np.zeros((4, 12))
    init[:, 4 * axis] = u
    return case(R, T, np.tile(ke.EDGE_Q, (4, 1)), init, subset_radius=ke.EDGE_R, max_iterations=2, tolerance=0.0)


def rotated_edge_case():
    """test_T_upper_edge_rotated: only a corner voxel of the subset reaches T's last admissible position, 2^-30 below the first
    outside one"""
    r = ke.EDGE_R
    R, T, _ = ke.edge_case(0, 1, 0)
    rots = (ref.rot(1.5, -2.0, 2.5), ref.rot(-2.0, 1.0, -1.5))
    init = np.zeros((len(rots), 12))
    q = np.tile(ke.EDGE_Q, (len(rots), 1)).astype(np.int32)
    corners = np.array([[s0, s1, s2] for s0 in (-r, r) for s1 in (-r, r) for s2 in (-r, r)], np.float64)
    for i, F in enumerate(rots):
        init[i, GRAD] = (F - np.eye(3)).ravel()
        init[i, 4], init[i, 8] = 0.1, -0.15
        top = (corners @ F.T)[:, 0].max()
        init[i, 0] = (T.shape[2] - 2) - 2.0 ** -30 - (q[i, 0] + top)
        c = ref.warp(init[i], q[i].astype(np.float64), corners)[:, 0]
        assert ref.in_domain(T.shape, init[i], q[i], r, True)
        assert c.max() - np.floor(c.max()) > 1 - 1e-6 and np.sort(c)[-2] < c.max() - 0.1
    return case(R, T, q, init, subset_radius=r, max_iterations=2, tolerance=0.0)


def status_3_case():
    """test_status_3_after_a_step: the true displacement lies 1.7 voxels outside T's domain"""
    R, T, k_in = ke.edge_case(0, 0, 0)
    starts = (0.1, 0.7, 1.4, 2.2)
    q = np.tile(ke.EDGE_Q - np.array([2, 0, 0]), (len(starts), 1))
    init = np.zeros((len(starts), 12))
    init[:, 0] = k_in + 2 + np.array(starts)
    return case(R, T, q, init, subset_radius=ke.EDGE_R, max_iterations=20, tolerance=1e-3)


# 4. non-finite T and the prefilter's reach

NF_VALUES = (np.nan, np.inf, -np.inf)
NF_SITES = [(a, s) for a in range(3) for s in (0, 1)]
NF_IDS = [f"{'xyz'[a]}-{'above' if s else 'below'}" for a, s in NF_SITES]
NF_D = range(bref.K - 1, bref.K + 5)  # the distances tried: the header's reach K + 2 with room on both sides


def nf_q(axis, side):
    """the POI of a site: 7 voxels from the face opposite the planted voxel, so that the reach r + K + 2 stays inside the 40^3
    volume (at ST_Q = 20 every voxel of the axis would lie within it)"""
    q = ke.ST_Q[0].copy()
    q[axis] = 7 if side else 40 - 1 - 7
    return q[None]


def nf_planted(T, axis, side, d, v):
    """T with the value v at the voxel d voxels beyond the subset's face along the axis (the POI's other coordinates)"""
    at = nf_q(axis, side)[0].copy()
    at[axis] += (ke.ST_R + d) * (1 if side else -1)
    Tb = T.copy()
    Tb[at[2], at[1], at[0]] = v
    return Tb


def nf_restate(R, T, axis, side):
    with np.errstate(invalid="ignore"):
        return bref.icgn(R, T, nf_q(axis, side), init=ke.ST_INIT, **ke.ST_OPTS)


def nf_straddle(R, T, axis, side, v=np.nan):
    """(near, far, clean): near the largest distance at which planting v changes the restatement's result, far = near + 1; asserts
    that every tried distance up to near changes it and every one beyond does not"""
    clean = nf_restate(R, T, axis, side)
    changed = [not same_results(nf_restate(R, nf_planted(T, axis, side, d, v), axis, side), clean) for d in NF_D]
    k = sum(changed)
    assert 0 < k < len(changed) and changed == [True] * k + [False] * (len(changed) - k), (axis, side, v, changed)
    near = NF_D[k - 1]
    assert near <= bref.K + 2, near  # the header: within K + 2 voxels of the warped subset and no further
    return near, near + 1, clean


def status_order_case(status_scene):
    """test_status_order_in_one_call's call: bad and healthy POIs alternate; returns the case, the healthy rows' case and the bad rows"""
    R, T, _ = status_scene
    R = R.copy()
    R[:, :, :14] = 0.5
    r = 3
    healthy = np.array([[24, 20, 20], [26, 24, 18], [22, 17, 25]], np.int32)
    hinit = np.tile(ke.ST_INIT, (3, 1))
    bad = np.array([[1, 20, 20], [r, 20, 20], [6, 20, 20]], np.int32)
    binit = np.zeros((3, 12))
    binit[0, 6] = np.inf   # a non-finite init outside R: 5 before 2
    binit[1, 0] = 0.25     # outside R, over constant R: 2 before 4
    binit[2, 8] = 100.0    # constant R, outside T: 4 before 3
    order = [0, 3, 1, 4, 2, 5]
    q, init = np.concatenate([bad, healthy])[order], np.concatenate([binit, hinit])[order]
    opts = dict(subset_radius=r, max_iterations=3, tolerance=0.0)
    return case(R, T, q, init, **opts), case(R, T, healthy, hinit, **opts)


STATUS_ORDER = [5, 1, 2, 1, 4, 1]


# 6. offsets

def offset_case(value_scene, which, b, r):
    """test_offsets' volumes, POIs and inits"""
    R, T, q, _, truth = value_scene
    Rb = (R + np.float32(b)).astype(np.float32) if which in ("both", "R") else R
    Tb = (T + np.float32(b)).astype(np.float32) if which in ("both", "T") else T
    q = q[(q >= r + 3).all(1) & (q <= 44 - r).all(1)][:5]
    init = truth(q) + np.random.default_rng(int(abs(b)) + r).uniform(-0.2, 0.2, (len(q), 12)) * np.where(np.arange(12) % 4 == 0, 1.0, 0.01)
    assert len(q) == 5
    return case(Rb, Tb, q, init, subset_radius=r, max_iterations=1, tolerance=0.0)


# 7. convergent runs

CONVERGENT_TOL = float(np.float32(1e-3))  # the default tolerance as the library holds it


def convergent_case(value_scene):
    """test_convergent_runs' call: the default tolerance and iteration limit (the restatement is handed CONVERGENT_TOL)"""
    R, T, q, init, _ = value_scene
    return case(R, T, q, init, subset_radius=6)


def near_tolerance(want, tol):
    """the POIs with a restatement step within 1 % of the tolerance: their iteration count may differ by rounding alone"""
    return np.array([any(abs(s - tol) <= 0.01 * tol for s in st) for st in want["steps"]])
