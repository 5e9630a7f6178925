"""Inputs of the displacement validation's tests (tests/test_validate_cpu.py, tests/test_gpu_validate.py): each case is a dict with
points (m, 3) int32, disp (m, 3) float64, grad (m, 9) float64 or None, valid (m,) uint8 or None and opts, plus what the case claims
about itself.  reference(name) is the restatement's answer (tests/validate_ref.py), computed once per process."""
import functools

import numpy as np

import validate_ref as ref


def grid(n, spacing=1, origin=0):
    g = np.arange(n) * spacing + origin
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(np.int32)


def case(points, disp, grad=None, valid=None, **opts):
    return dict(points=np.ascontiguousarray(points, np.int32), disp=np.ascontiguousarray(disp, np.float64),
                grad=None if grad is None else np.ascontiguousarray(grad, np.float64).reshape(-1, 9),
                valid=None if valid is None else np.ascontiguousarray(valid, np.uint8), opts=opts)


# ---- planted outliers: 9^3 POIs at spacing 4, a quadratic field about the grid's centre, 36 vectors off by 3 voxels -----------------
H = np.array([[[1.0, 0.3, -0.2], [0.3, -0.8, 0.4], [-0.2, 0.4, 0.6]],
              [[-0.7, 0.2, 0.5], [0.2, 1.0, -0.3], [0.5, -0.3, 0.4]],
              [[0.5, -0.4, 0.1], [-0.4, 0.6, 0.2], [0.1, 0.2, -1.0]]])   # symmetric, entries of magnitude <= 1: the curvature's shape
LIN = np.array([[0.004, -0.002, 0.001], [0.001, 0.003, -0.002], [-0.003, 0.001, 0.002]])
B0 = np.array([1.25, -2.5, 0.75])


def quadratic(q, curvature):
    """u_c = b_c + LIN_c . d + curvature / 2 d^T H_c d about the centre of the 9^3 grid, and its exact gradient"""
    d = q.astype(np.float64) - 16.0
    u = B0 + d @ LIN.T + 0.5 * curvature * np.einsum("na,cab,nb->nc", d, H, d)
    g = LIN[None] + curvature * np.einsum("cab,nb->nca", H, d)
    return u, g


def planted(curvature, noise, with_grad):
    rng = np.random.default_rng(2005)
    q = grid(9, 4)
    u, g = quadratic(q, curvature)
    if noise:
        u = u + rng.normal(0, noise, u.shape)
    rows = np.sort(rng.choice(len(q), 36, replace=False))
    u[rows, rng.integers(0, 3, 36)] += rng.choice([-3.0, 3.0], 36)
    c = case(q, u, g if with_grad else None, radius=8)
    c["planted"] = rows
    return c


# ---- passes: the 3 x 3 x 3 block at 12..20 shifted by 5 voxels in a linear field ------------------------------------------------------
def block(passes):
    q = grid(9, 4)
    u = B0 + q.astype(np.float64) @ (0.5 * LIN.T)
    inside = ((q >= 12) & (q <= 20)).all(1)
    u[inside] += 5.0
    c = case(q, u, radius=4, min_neighbours=6, passes=passes)
    c["block"], c["centre"] = inside, int(np.flatnonzero((q == 16).all(1))[0])
    return c


# ---- counts ---------------------------------------------------------------------------------------------------------------------------
def hostile_values(rng, m):
    """heavy ties (quantised to 0.25), negative values, both zeros, subnormals"""
    u = np.round(rng.normal(0, 1.0, (m, 3)) * 4) / 4
    u[rng.random((m, 3)) < 0.05] = -0.0
    u[rng.random((m, 3)) < 0.05] = 0.0
    sub = rng.random((m, 3)) < 0.05
    u[sub] = rng.integers(-5, 6, int(sub.sum())) * 5e-324
    return u


def cluster(m, **opts):
    """m POIs within one window of each other: every POI has n = m - 1"""
    rng = np.random.default_rng(100 + m)
    q = rng.permutation(grid(3))[:m] if m <= 27 else grid(4)[:m]
    return case(q, hostile_values(rng, m), radius=3, **opts)


def dense(side, radius, n_centre, with_grad, seed, passes=2):
    """a spacing-1 grid of side^3 POIs whose centre POI has exactly n_centre neighbours (None: all): contributors around the centre are
    switched off by valid bytes until the count is met.  One POI beside the centre holds magnitudes up to 1e300: the first pass flags
    it, so the centre has n_centre neighbours in the first pass and n_centre - 1 from then on."""
    rng = np.random.default_rng(seed)
    q = grid(side)
    m = len(q)
    u = hostile_values(rng, m)
    centre = int(np.flatnonzero((q == side // 2).all(1))[0])
    big = (centre + 3) % m
    u[big] = [1e300, -1e300, 3e299]
    valid = np.ones(m, np.uint8)
    if n_centre is not None:
        near = np.flatnonzero((np.abs(q - q[centre]) <= radius).all(1) & (np.arange(m) != centre) & (np.arange(m) != big))
        off = len(near) + 1 - n_centre
        assert 0 <= off < len(near)
        valid[rng.permutation(near)[:off]] = 0
    g = None
    if with_grad:
        g = np.round(rng.normal(0, 0.05, (m, 9)) * 64) / 64
    c = case(q, u, g, valid, radius=radius, passes=passes, threshold=1e3)   # the threshold: only the huge POI is flagged
    c["centre"], c["big"] = centre, big
    return c


# ---- contribution rules -------------------------------------------------------------------------------------------------------------
def rules():
    """two clusters 2^25 apart (the cell grid's side is enlarged), negative coordinates, a coordinate at 2^24 and one past it, valid
    bytes of 0, NaN / Inf in disp and in grad, duplicate points"""
    rng = np.random.default_rng(77)
    a = grid(5, 2, -2 ** 24)                      # x, y, z from -2^24
    b = grid(5, 2, 2 ** 24 - 8)                   # up to 2^24
    b[:, 1:] -= 2 ** 24                           # only x is far away
    extra = np.array([[2 ** 24 + 1, -8, -8], [2 ** 24, -8, -8], [-2 ** 24 - 1, -2 ** 24, -2 ** 24], [2 ** 24 - 4, -6, -6], [2 ** 24 - 4, -6, -6],
                      [-2 ** 24 + 3, -2 ** 24 + 3, -2 ** 24 + 3], [-2 ** 24 + 3, -2 ** 24 + 3, -2 ** 24 + 3]], np.int32)
    q = np.concatenate([a, b, extra])
    m = len(q)
    u = hostile_values(rng, m) + q[:, :1] * 1e-9
    g = np.round(rng.normal(0, 0.05, (m, 9)) * 64) / 64
    valid = np.ones(m, np.uint8)
    valid[[3, 40, 130, 131]] = 0
    valid[7] = 255
    u[10, 1] = np.nan
    u[60, 0] = np.inf
    u[140, 2] = -np.inf
    g[20, 4] = np.nan
    g[150, 8] = np.inf
    c = case(q, u, g, valid, radius=4, min_neighbours=6, passes=3)
    c["out_of_range"] = [250, 252]
    return c


# ---- invariances --------------------------------------------------------------------------------------------------------------------
def linear(with_grad):
    """a strongly linear field with its exact gradients: the gradient form scores 0 to rounding everywhere, the plain form does not at
    the domain's corners"""
    q = grid(6, 4, -10)
    G = np.array([[0.10, 0.11, 0.12], [-0.08, 0.12, 0.09], [0.11, -0.07, 0.10]])
    u = B0 + q.astype(np.float64) @ G.T
    return case(q, u, np.tile(G.reshape(1, 9), (len(q), 1)) if with_grad else None, radius=4, min_neighbours=6, eps=0.07)


CASES = {f"planted-k{k:g}-n{n:g}-{'grad' if g else 'plain'}": functools.partial(planted, k, n, g)
         for k in (2e-4, 2e-3) for n in (0.0, 0.02) for g in (False, True)}
CASES.update({f"block-p{p}": functools.partial(block, p) for p in (1, 2, 3, 4)})
CASES.update({"m1": functools.partial(cluster, 1), "m2": functools.partial(cluster, 2),
              # a threshold out of reach: nothing is flagged and the report holds the medians of exactly these counts
              "n-min-minus-1": functools.partial(cluster, 6, min_neighbours=6, threshold=1e3),
              "n-min-even": functools.partial(cluster, 7, min_neighbours=6, threshold=1e3),
              "n-odd": functools.partial(cluster, 8, min_neighbours=6, threshold=1e3),
              "n-min-3": functools.partial(cluster, 4, min_neighbours=3, threshold=1e3),
              "n-odd-flags": functools.partial(cluster, 22, min_neighbours=6, passes=4),
              "all-invalid": lambda: dict(cluster(12), valid=np.zeros(12, np.uint8)),
              "rules": rules, "linear-grad": functools.partial(linear, True), "linear-plain": functools.partial(linear, False)})


def capacity_cases(cap):
    """dense grids whose centre POI has cap - 1 ... cap + 2 neighbours in the first pass (one fewer in the report) and several times cap"""
    side = 3
    while side ** 3 - 1 < cap + 1:
        side += 2
    big = side
    while big ** 3 - 1 < 3 * cap:
        big += 2
    return {"cap-minus-1": functools.partial(dense, side, side // 2, cap - 1, False, 1), "cap": functools.partial(dense, side, side // 2, cap, True, 2),
            "cap-plus-1": functools.partial(dense, side, side // 2, cap + 1, False, 3), "cap-plus-2": functools.partial(dense, side, side // 2, cap + 2, True, 5),
            "cap-times-3": functools.partial(dense, big, big // 2, None, True, 4, passes=1)}


@functools.lru_cache(maxsize=None)
def get(name, cap=None):
    table = CASES if cap is None else capacity_cases(cap)
    return table[name]()


@functools.lru_cache(maxsize=None)
def reference(name, cap=None):
    """(the records, the trace of every pass's scores); shared by the tests and never modified"""
    c = get(name, cap)
    trace = []
    rec = ref.validate(c["points"], c["disp"], c["grad"], c["valid"], trace=trace, **c["opts"])
    rec.setflags(write=False)
    return rec, trace
