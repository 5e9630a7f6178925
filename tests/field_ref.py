"""NumPy fp64 restatement of the field evaluation's contract (sift3d_field_eval and its host helpers, include/sift3d_hip.h): the
members of a real-valued query by the rounded offsets, the weights in the header's association, the weighted plane fit once from the
normal equations as the header writes them (solve="normal") and once from numpy.linalg.lstsq on the rows sqrt(w) [1, d]
(solve="lstsq").  Also the inputs of the GPU parity test, parity_error(): e, the largest absolute difference between the two solves
over every field of every status-0 query of those inputs, and the sliding query of the continuity test."""
import functools

import numpy as np

COORD_MAX = 2 ** 24
PIVOT_REL = 1e-9
FLOATS = ("disp", "G", "rms", "wsum")
INTS = ("neighbours", "sides", "status")
PARITY_RADII = (1, 2, 5, 16, 40)
PARITY_MIN_NEIGHBOURS = 6
WEIGHTINGS = (0, 1)


def contributes(points, disp, valid=None):
    q = np.asarray(points, np.int64).reshape(-1, 3)
    u = np.asarray(disp, np.float64).reshape(-1, 3)
    ok = np.isfinite(u).all(1) & (np.abs(q) <= COORD_MAX).all(1)
    if valid is not None:
        ok &= np.asarray(valid).reshape(-1) != 0
    return ok


def weights(d, radius, weighting):
    """the weights of the offsets d (n, 3), all of them members: 1, or the tensor biweight in the header's association"""
    if not weighting:
        return np.ones(len(d))
    t = d / float(radius)
    f = 1.0 - t * t
    g = f * f
    return (g[:, 0] * g[:, 1]) * g[:, 2]


def fit(d, u, w, solve="normal"):
    """the weighted plane through the counted members' displacements u (n, 3) at the offsets d (n, 3), u[0] the lowest index's:
    status (0 or 4), disp (3,), G (3, 3), rms, W"""
    a = u - u[0]
    W = w.sum()
    wd = w[:, None] * d
    S1, S2 = wd.sum(0), wd.T @ d
    C = S2 - np.outer(S1, S1) / W
    floor = PIVOT_REL * max(C[0, 0], C[1, 1], C[2, 2])
    with np.errstate(invalid="ignore", divide="ignore"):
        l00 = np.sqrt(C[0, 0]); l10 = C[0, 1] / l00; l20 = C[0, 2] / l00
        p1 = C[1, 1] - l10 * l10
        l11 = np.sqrt(p1); l21 = (C[1, 2] - l20 * l10) / l11
        p2 = (C[2, 2] - l20 * l20) - l21 * l21
    if not (C[0, 0] > floor and p1 > floor and p2 > floor):
        return 4, np.zeros(3), np.zeros((3, 3)), 0.0, 0.0
    if solve == "normal":
        l22 = np.sqrt(p2)
        wa = w[:, None] * a
        U, P = wa.sum(0), wa.T @ d
        B = P - np.outer(U, S1) / W
        G = np.zeros((3, 3))
        for c in range(3):
            y0 = B[c, 0] / l00; y1 = (B[c, 1] - l10 * y0) / l11; y2 = ((B[c, 2] - l20 * y0) - l21 * y1) / l22
            G[c, 2] = y2 / l22
            G[c, 1] = (y1 - l21 * G[c, 2]) / l11
            G[c, 0] = ((y0 - l10 * G[c, 1]) - l20 * G[c, 2]) / l00
        disp = (u[0] + U / W) - (G @ S1) / W
    else:
        s = np.sqrt(w)[:, None]
        coef = np.linalg.lstsq(s * np.concatenate([np.ones((len(d), 1)), d], 1), s * u, rcond=None)[0]
        disp, G = coef[0].copy(), coef[1:].T.copy()
    res = (u - disp) - d @ G.T
    return 0, disp, G, float(np.sqrt((w * (res * res).sum(1)).sum() / (3.0 * W))), float(W)


def evaluate(points, disp, valid, queries, radius=16, min_neighbours=10, weighting=1, require_enclosed=1, solve="normal"):
    """every query: arrays like capi.field_eval's (without the records and the seconds)"""
    q = np.asarray(points, np.int64).reshape(-1, 3)
    u = np.asarray(disp, np.float64).reshape(-1, 3)
    xs = np.asarray(queries, np.float64).reshape(-1, 3)
    on = np.flatnonzero(contributes(q, u, valid))   # ascending index
    qn, un = q[on].astype(np.float64), u[on]
    nq = len(xs)
    out = {"disp": np.zeros((nq, 3)), "G": np.zeros((nq, 3, 3)), "rms": np.zeros(nq), "wsum": np.zeros(nq),
           "neighbours": np.zeros(nq, np.int32), "sides": np.zeros(nq, np.int32), "status": np.zeros(nq, np.int32)}
    rad = float(radius)
    for i, x in enumerate(xs):
        if not (np.abs(x) <= COORD_MAX).all():   # false for NaN
            out["status"][i] = 2
            continue
        d = qn - x
        mem = np.flatnonzero((np.abs(d) <= rad).all(1))
        d = d[mem]
        w = weights(d, radius, weighting)
        keep = w > 0
        mem, d, w = mem[keep], d[keep], w[keep]
        out["neighbours"][i] = len(mem)
        sides = 0
        for a in range(3):
            sides |= (1 << (2 * a) if (d[:, a] <= 0).any() else 0) | (2 << (2 * a) if (d[:, a] >= 0).any() else 0)
        out["sides"][i] = sides
        if len(mem) < min_neighbours:
            out["status"][i] = 1
            continue
        if require_enclosed and sides != 63:
            out["status"][i] = 5
            continue
        st, d0, G, rms, W = fit(d, un[mem], w, solve)
        out["status"][i] = st
        if st == 0:
            out["disp"][i], out["G"][i], out["rms"][i], out["wsum"][i] = d0, G, rms, W
    return out


def enclosed(res):
    """the result of require_enclosed = 1 from that of require_enclosed = 0 on the same input"""
    out = {k: v.copy() for k, v in res.items()}
    hit = ((res["status"] == 0) | (res["status"] == 4)) & (res["sides"] != 63)
    out["status"][hit] = 5
    for k in FLOATS:
        out[k][hit] = 0.0
    return out


# ---- the host helpers ------------------------------------------------------------------------------------------------------------
def queries(points, disp):
    return np.asarray(points, np.int32).astype(np.float64) + np.asarray(disp, np.float64)


def unpack(res):
    return res["disp"].copy(), res["G"].reshape(-1, 9).copy(), (res["status"] == 0).astype(np.uint8)


def compose(dispA, gradA, validA, atB):
    """disp, grad (None without gradA), valid of sift3d_compose_displacements"""
    uA = np.asarray(dispA, np.float64).reshape(-1, 3)
    ok = atB["status"] == 0
    if validA is not None:
        ok = ok & (np.asarray(validA).reshape(-1) != 0)
    disp = np.where(ok[:, None], uA + atB["disp"], 0.0)
    grad = None
    if gradA is not None:
        GA = np.asarray(gradA, np.float64).reshape(-1, 3, 3)
        GB = atB["G"].reshape(-1, 3, 3)
        grad = np.zeros_like(GA)
        for r in range(3):
            for c in range(3):
                prod = (GB[:, r, 0] * GA[:, 0, c] + GB[:, r, 1] * GA[:, 1, c]) + GB[:, r, 2] * GA[:, 2, c]
                grad[:, r, c] = (GA[:, r, c] + GB[:, r, c]) + prod
        grad = np.where(ok[:, None], grad.reshape(-1, 9), 0.0)
    return disp, grad, ok.astype(np.uint8)


def init_from_field(disp, grad, valid, only_valid, init):
    """(init12, count) of sift3d_icgn_init_from_field"""
    out = np.array(init, np.float64).reshape(-1, 12).copy()
    u = np.asarray(disp, np.float64).reshape(-1, 3)
    g = np.zeros((len(u), 9)) if grad is None else np.asarray(grad, np.float64).reshape(-1, 9)
    rows = np.ones(len(u), bool) if not only_valid or valid is None else np.asarray(valid).reshape(-1) != 0
    full = np.concatenate([u[:, 0:1], g[:, 0:3], u[:, 1:2], g[:, 3:6], u[:, 2:3], g[:, 6:9]], 1)
    out[rows] = full[rows]
    return out, int(rows.sum())


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def bar(e, umax):
    """the bar of every fp64 field of a case whose largest |u| is umax"""
    return max(4.0 * e, 1e-12) * max(1.0, umax)


def largest_u(disp):
    u = np.asarray(disp, np.float64)
    u = u[np.isfinite(u)]
    return float(np.abs(u).max()) if u.size else 0.0


def smooth_field(q):
    x, y, z = (np.asarray(q, np.float64)[:, k] for k in range(3))
    return np.stack([6.0 * np.sin(x / 17.0) + 0.04 * y - 1.5, 5.0 * np.cos(y / 13.0 + z / 29.0) + 0.03 * x, 0.002 * x * z - 0.05 * y + 2.0], 1)


def jittered_lattice(rng, counts=(15, 13, 11), step=4, origin=2):
    """a lattice of the given step whose POIs are moved by -1, 0 or 1 voxel per axis: counts = (15, 13, 11) fills 60 x 52 x 44 voxels"""
    g = [origin + step * np.arange(n) for n in counts]
    q = np.stack(np.meshgrid(*g, indexing="ij"), -1).reshape(-1, 3)
    return (q + rng.integers(-1, 2, q.shape)).astype(np.int32)


@functools.lru_cache(maxsize=None)
def parity_inputs():
    """2145 POIs on a jittered lattice in a 62 x 54 x 46 box plus a cluster of 300 in 6^3 voxels of it (duplicates among them), a
    smooth field plus noise with |u| up to 10, 10 % invalid; 1500 queries: anywhere in the box, in the cluster, exact POI positions,
    half-integers, and positions outside the POIs' bounding box by 0.25 .. 50 voxels (less and more than every radius).  Only the
    cluster is dense enough for windows of radius 1 and 2, and its queries lie on a quarter-voxel grid: a real-valued query there has
    members next to the window's faces whose biweight is as small as one likes, the weighted normal equations of radius 1 are then
    ill-conditioned (the two solves differ by 1e-8 instead of 1e-14) and e would say nothing about the well-posed windows."""
    rng = np.random.default_rng(2025)
    q = np.concatenate([jittered_lattice(rng), rng.integers(20, 26, (300, 3)).astype(np.int32)])
    u = np.clip(smooth_field(q) + rng.normal(0.0, 0.3, (len(q), 3)), -10.0, 10.0)
    valid = (rng.random(len(q)) >= 0.1).astype(np.uint8)
    lo, hi = q.min(0).astype(np.float64), q.max(0).astype(np.float64)
    anywhere = lo + rng.random((500, 3)) * (hi - lo)
    cluster = 19.5 + 0.25 * rng.integers(0, 25, (300, 3))
    exact = q[rng.choice(len(q), 200, replace=False)].astype(np.float64)
    half = np.floor(lo + rng.random((200, 3)) * (hi - lo)) + 0.5 * rng.integers(0, 2, (200, 3))
    outside = lo + rng.random((300, 3)) * (hi - lo)
    margin = rng.choice([0.25, 0.5, 1.5, 3.0, 10.0, 30.0, 50.0], 300)
    axis, top = rng.integers(0, 3, 300), rng.integers(0, 2, 300)
    for k in range(300):
        outside[k, axis[k]] = hi[axis[k]] + margin[k] if top[k] else lo[axis[k]] - margin[k]
    return q, u, valid, np.concatenate([anywhere, cluster, exact, half, outside])


@functools.lru_cache(maxsize=None)
def parity_reference(radius, weighting, solve="normal"):
    """require_enclosed = 0; enclosed() gives the other"""
    q, u, valid, xs = parity_inputs()
    return evaluate(q, u, valid, xs, radius=radius, min_neighbours=PARITY_MIN_NEIGHBOURS, weighting=weighting, require_enclosed=0, solve=solve)


@functools.lru_cache(maxsize=None)
def parity_error():
    e = 0.0
    for r in PARITY_RADII:
        for wt in WEIGHTINGS:
            a, b = parity_reference(r, wt), parity_reference(r, wt, "lstsq")
            ok = a["status"] == 0
            for k in FLOATS:
                if ok.any():
                    e = max(e, float(np.abs(a[k][ok] - b[k][ok]).max()))
    return e


def solve_gap(a, b):
    """the largest absolute difference between two results of evaluate() over every field of the queries with status 0 in a"""
    ok = a["status"] == 0
    return max(float(np.abs(a[k][ok] - b[k][ok]).max()) for k in FLOATS) if ok.any() else 0.0


@functools.lru_cache(maxsize=None)
def cell_inputs():
    """1500 POIs at random in [-12, 12)^3 (some 37 to a window of radius 3, whose cells have side 4 from the box's corner) and 2000
    queries: 1700 real-valued ones in [-10, 10]^3, whose windows have members on both sides, and 300 anywhere in [-16, 16)^3 whose
    fractions are 0, 0.5, 2^-30 and 1 - 2^-30.  What is kept out is a real-valued query outside the POIs: under the biweight its
    window can hang on one plane of POIs next to a face, whose weight of 1e-9 .. 1e-4 of the others' passes the pivot rule and leaves
    normal equations that the two solves of this file already answer 1e-9 apart.  The fractions above give such a plane a weight of
    0.09 at least or of 1e-18 at most: well posed, or degenerate by the pivot rule."""
    rng = np.random.default_rng(8)
    q = rng.integers(-12, 12, (1500, 3)).astype(np.int32)
    u = smooth_field(q) + rng.normal(0, 0.1, (1500, 3))
    xs = rng.random((2000, 3)) * 20.0 - 10.0
    xs[:300] = rng.integers(-16, 16, (300, 3)) + rng.choice([0.0, 0.5, 1.0 - 2.0 ** -30, 2.0 ** -30], (300, 3))
    return q, u, xs


CELL_OPTIONS = dict(radius=3, min_neighbours=4)


@functools.lru_cache(maxsize=None)
def continuity_inputs():
    """a 7 x 7 x 7 lattice of step 3 with a smooth field, and one outlying POI 1 voxel off that field at x = 30, beyond the lattice's
    last plane x = 18; the query slides in 200 steps of 0.01 along x across 30 - radius = 22, where the outlier enters the window of
    radius 8 (a face at x - 8, members on both sides of the query on every axis)"""
    g = 3 * np.arange(7)
    q = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    q = np.concatenate([q, [[30, 9, 9]]]).astype(np.int32)
    u = 0.1 * smooth_field(q)
    u[-1] += 1.0
    xs = np.stack([21.0 + 0.01 * np.arange(200), np.full(200, 9.3), np.full(200, 8.6)], 1)
    return q, u, xs


CONTINUITY_OPTIONS = dict(radius=8, min_neighbours=10, require_enclosed=0)


def largest_step(disp):
    """the largest step-to-step change of any component along the slide"""
    return float(np.abs(np.diff(disp, axis=0)).max())
