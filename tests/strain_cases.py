"""Inputs of the strain fields' edge battery (tests/test_strain_cases_cpu.py, tests/test_gpu_strain_edges.py): each case is a dict with
points (m, 3) int32, disp (m, 3) float64, valid (m,) uint8 or None and opts, plus what the case claims about itself.  The CPU test
checks every claim against the restatement (tests/strain_ref.py) and exact rational arithmetic; the GPU test runs the cases.

The families: windows on both sides of the degeneracy rule's floor (pivot <= 1e-9 x the largest diagonal entry of C), exactly
degenerate windows, a constant added to every displacement, boxes whose extents sit on the cell grid's seams, stars at the smallest
and the largest radius, grids the cell cap coarsens, POIs outside the box of the contributing ones, the invariances of the parity
inputs (translation, order, signed axis permutations) and affine fields with known strains."""
import functools
import itertools

import numpy as np

import strain_ref as ref

G0 = np.array([[0.010, -0.004, 0.002], [0.003, -0.020, 0.001], [-0.002, 0.005, 0.015]])
B0 = np.array([1.25, -2.5, 0.75])
MAX_CELLS = 2 ** 24


def case(points, disp, valid=None, **opts):
    return dict(points=np.ascontiguousarray(points, np.int32), disp=np.ascontiguousarray(disp, np.float64),
                valid=None if valid is None else np.ascontiguousarray(valid, np.uint8), opts=opts)


def reference(c, **more):
    return ref.strain(c["points"], c["disp"], c["valid"], **dict(c["opts"], **more))


def umax(c):
    return ref.largest_u(c["disp"])


# ---- windows at the pivot floor ------------------------------------------------------------------------------------------------------
# The POI in question is row 0: it sits at the window's origin and does not contribute (valid byte 0), so the contract's count n is
# the number of planted neighbours.  c["offsets"] are their integer offsets from it, c["rho"] the smallest exact pivot ratio.
SIGNS = ((1, 1), (1, -1), (-1, 1), (-1, -1))


def _window(d, radius, origin, seed):
    rng = np.random.default_rng(seed)
    d = np.asarray(d, np.int64)
    q = np.concatenate([np.zeros((1, 3), np.int64), d]) + np.asarray(origin)
    u = np.concatenate([np.zeros((1, 3), np.int64), d]) @ G0.T + 1.0 + rng.normal(0.0, 0.01, (len(d) + 1, 3))
    valid = np.ones(len(q), np.uint8)
    valid[0] = 0
    c = case(q, u, valid, radius=radius, min_neighbours=4)
    c["offsets"], c["n"], c["rho"] = d, len(d), ref.smallest_pivot_ratio(d)
    c["status"] = 0 if c["rho"] > ref.PIVOT_REL else 4
    return c


def thin_axis(axis, n):
    """n neighbours at the four corners (+-4096, +-4096) of the plane normal to `axis`, in turn, the last one a voxel off the plane"""
    d = np.zeros((n, 3), np.int64)
    others = [a for a in range(3) if a != axis]
    for j in range(n):
        d[j, others] = 4096 * np.array(SIGNS[j % 4])
    d[n - 1, axis] = 1
    c = _window(d, 4096, (100000 * (axis + 1), -70000, 30000 + n), 500 + 10 * axis + n)
    c["deciding"] = axis   # c00, p1 or p2: the pivot the thin axis leaves small
    return c


def tilted(h, n):
    """n neighbours at (a, b, -a - b), a, b = +-h in turn: the plane x + y + z = 0; one of those at z = 0 has z raised by 1"""
    d = np.zeros((n, 3), np.int64)
    for j in range(n):
        a, b = h * np.array(SIGNS[j % 4])
        d[j] = (a, b, -a - b)
    d[n - 2, 2] += 1   # (-h, h, 0): the window's half width is 2 h, so a POI at z = 2 h could not be raised
    c = _window(d, 2 * h, (-50000 - h, 20000 + n, 7000), 700 + h + n)
    c["deciding"] = 2
    return c


THIN = {f"thin-{'xyz'[a]}-n{n}": functools.partial(thin_axis, a, n) for a in range(3) for n in (48, 64)}
TILTED = {f"tilted-h{h}-n{n}": functools.partial(tilted, h, n) for h, n in ((2048, 64), (2048, 128), (64, 64))}
# what the cases state about themselves, checked on the CPU: (lowest, highest) rho x 1e9 and the status of row 0
STATED = {"thin-n48": (1.155, 1.225, 0), "thin-n64": (0.885, 0.925, 4), "tilted-h2048-n64": (1.77, 1.79, 0), "tilted-h2048-n128": (0.90, 0.92, 4),
          "tilted-h64-n64": (1.7e3, 1.9e3, 0)}


def stated(name):
    return STATED[name if name in STATED else name[:5] + name[7:]]


@functools.lru_cache(maxsize=None)
def pivot_case(name):
    return (THIN if name in THIN else TILTED)[name]()


@functools.lru_cache(maxsize=None)
def e_case(name):
    """the measured error of a tilted case: the largest absolute difference, over every fp64 field of every status-0 POI, between the
    restatement's normal solve and (a) its lstsq solve, (b) its normal solve on 16 seeded permutations of the POI order"""
    c = pivot_case(name)
    base = reference(c)
    ok = base["status"] == 0
    worst = 0.0

    def widen(other, rows):
        nonlocal worst
        for k in ref.FLOATS:
            if ok.any():
                worst = max(worst, float(np.abs(other[k][rows][ok] - base[k][ok]).max()))

    widen(reference(c, solve="lstsq"), np.arange(len(ok)))
    rng = np.random.default_rng(16)
    for _ in range(16):
        p = rng.permutation(len(ok))
        got = ref.strain(c["points"][p], c["disp"][p], c["valid"][p], **c["opts"])
        back = np.argsort(p)
        assert np.array_equal(got["status"][back], base["status"]) and np.array_equal(got["neighbours"][back], base["neighbours"])
        widen(got, back)
    return worst


def tilted_bar(name):
    return ref.bar(2.0 * e_case(name), umax(pivot_case(name)))


def _degenerate(d, seed):
    rng = np.random.default_rng(seed)
    d = np.asarray(d, np.int64).reshape(-1, 3)
    q = d + np.array([17, -5, 40])
    u = q @ G0.T + B0 + rng.normal(0.0, 0.01, (len(q), 3))
    c = case(q, u, radius=40, min_neighbours=4)
    c["offsets"] = d
    return c


def _plane(axis):
    g = np.stack(np.meshgrid(np.arange(4) * 2, np.arange(4) * 3, indexing="ij"), -1).reshape(-1, 2)
    d = np.zeros((len(g), 3), np.int64)
    d[:, [a for a in range(3) if a != axis]] = g
    d[:, axis] = 5
    return d


DEGENERATE = {
    "plane-x": lambda: _degenerate(_plane(0), 41), "plane-y": lambda: _degenerate(_plane(1), 42), "plane-z": lambda: _degenerate(_plane(2), 43),
    "plane-111": lambda: _degenerate([(a, b, 3 - a - b) for a in range(-2, 3) for b in range(-2, 3)], 44),
    "line-111": lambda: _degenerate([(t, t, t) for t in range(-4, 5)], 45),
    "line-1-20": lambda: _degenerate([(t, -2 * t, 0) for t in range(-4, 5)], 46),
    "coincident": lambda: _degenerate([(3, 1, 4)] * 12, 47),
    "two-sites": lambda: _degenerate([(3, 1, 4), (-2, 7, 0)] * 6, 48)}


# ---- sums on u - u0 ------------------------------------------------------------------------------------------------------------------
SHIFT = 2.0 ** 20
SHIFT_RADII = (7, 20)


@functools.lru_cache(maxsize=None)
def dyadic_parity_inputs():
    """the parity inputs with u rounded to multiples of 2^-20: u + 2^20 is exact"""
    q, u, valid = ref.parity_inputs()
    u = np.round(u * SHIFT) / SHIFT
    assert np.array_equal((u + SHIFT) - SHIFT, u)
    u.setflags(write=False)
    return q, u, valid


def shift_disagreement(a, b, e):
    """a: the results on u, b: on u + 2^20.  Empty when the claim holds: status, neighbours, G, E, principal and equivalent the same
    bytes; over status-0 rows disp - 2^20 within bar(e, 2^20) and rms within bar(e, 10)"""
    bad = [k for k in ("status", "neighbours", "G", "E", "principal", "equivalent") if a[k].tobytes() != b[k].tobytes()]
    ok = a["status"] == 0
    dd, dr = float(np.abs((b["disp"][ok] - SHIFT) - a["disp"][ok]).max()), float(np.abs(b["rms"][ok] - a["rms"][ok]).max())
    print(f"shift by 2^20: max |disp - K - disp0| = {dd:.2e} (bar {ref.bar(e, SHIFT):.2e}), max |rms - rms0| = {dr:.2e} (bar {ref.bar(e, 10.0):.2e})")
    if not dd <= ref.bar(e, SHIFT):
        bad.append(("disp", dd))
    if not dr <= ref.bar(e, 10.0):
        bad.append(("rms", dr))
    if b["disp"][~ok].any() or b["rms"][~ok].any():
        bad.append("non-zero fields of a failed POI")
    return bad


# ---- the cell grid -------------------------------------------------------------------------------------------------------------------
def choose_grid(extent, radius):
    """poi_choose_grid restated: (side, (nx, ny, nz)) for a box of the given extents (max - min per axis).  The side is the radius
    and grows by (side + 3) / 4 (integer division) until nx * ny and nx * ny * nz are at most 2^24"""
    side = int(radius)
    while True:
        nx, ny, nz = (int(e) // side + 1 for e in extent)
        if nx * ny <= MAX_CELLS and nx * ny * nz <= MAX_CELLS:
            return side, (nx, ny, nz)
        side += (side + 3) // 4


def box_of(c):
    """(low corner, extent) of the contributing POIs of a case"""
    on = ref.contributes(c["points"], c["disp"], c["valid"])
    q = c["points"][on].astype(np.int64)
    return q.min(0), q.max(0) - q.min(0)


def grid_of(c):
    lo, extent = box_of(c)
    return (lo,) + choose_grid(extent, c["opts"]["radius"])


def corners_of(lo, hi):
    return np.array([[(lo, hi)[b][a] for a, b in enumerate(bits)] for bits in np.ndindex(2, 2, 2)], np.int64)


EXTENT_RADII = (1, 2, 7)
EXTENT_CASES = [(r, axis, delta) for r in EXTENT_RADII for axis in range(3) for delta in (-1, 0, 1)]


@functools.lru_cache(maxsize=None)
def extents(r, axis, delta):
    """a box of extent 5 r + delta on `axis` and 3 r on the other two, filled at random at about 12 POIs per window, with POIs on both
    faces of `axis` and at the eight corners; one POI in twelve does not contribute (the planted ones all do)"""
    rng = np.random.default_rng(1000 * r + 10 * axis + delta + 1)
    ext = np.full(3, 3 * r, np.int64)
    ext[axis] = 5 * r + delta
    lo = np.array([-7, 11, -3 * r - 1], np.int64)   # the box straddles 0 on x and ends at -1 on z
    m = int(min(400 - 16, np.ceil(12.0 * np.prod(ext + 1) / (2 * r + 1) ** 3)))
    fill = rng.integers(0, ext + 1, (m, 3))
    faces = rng.integers(0, ext + 1, (8, 3))
    faces[:4, axis], faces[4:, axis] = 0, ext[axis]
    q = np.concatenate([fill, faces, corners_of(np.zeros(3, np.int64), ext)]) + lo
    u = q @ G0.T + B0 + rng.normal(0.0, 0.01, (len(q), 3))
    valid = np.ones(len(q), np.uint8)
    valid[:m][rng.random(m) < 1.0 / 12.0] = 0
    c = case(q, u, valid, radius=r, min_neighbours=4)
    c["extent"], c["axis"], c["planted"] = ext, axis, np.arange(m, len(q))
    return c


STAR_RADII = (1, 2, 4096)


def star_offsets(r):
    """the offsets 0 .. r - 1 of a star from the cell borders; of a large radius the ends and the middle"""
    return list(range(r)) if r <= 8 else [0, 1, 2, r // 2 - 1, r // 2, r - 2, r - 1]


@functools.lru_cache(maxsize=None)
def stars(r, centres_contribute=True):
    """stars: a centre, and on each axis and side one POI at distance r (counted) and one at r + 1 (not counted).  The cells have
    side r from the box's lowest corner, and the stars sit at the offsets star_offsets(r) from it on x (twice and three times the
    offset, modulo r, on y and z), so the two POIs of a side fall into the same cell, into neighbouring cells and across the last
    cell the window touches.  POIs at the eight corners of the box."""
    q = []
    for i, k in enumerate(star_offsets(r)):
        c = np.array([8 * r * (i + 1) + k, 8 * r + (2 * k) % r, 8 * r + (3 * k) % r], np.int64)
        q.append(c)
        for ax in range(3):
            for sg in (-1, 1):
                for dist in (r, r + 1):
                    p = c.copy()
                    p[ax] += sg * dist
                    q.append(p)
    q = np.array(q)
    assert q.min() > 0   # the box's low corner is the origin, so a centre's offset from the cell borders is its coordinate modulo r
    q = np.concatenate([q, corners_of(np.zeros(3, np.int64), q.max(0) + 3)]) - np.array([5, 0, 2 * r])   # the low corner at (-5, 0, -2 r)
    rng = np.random.default_rng(3 + r)
    u = q @ G0.T + rng.normal(0, 0.01, (len(q), 3))
    centres = np.arange(len(star_offsets(r))) * 13
    valid = np.ones(len(q), np.uint8)
    if not centres_contribute:
        valid[centres] = 0
    c = case(q, u, valid, radius=r, min_neighbours=4)
    c["centres"], c["corners"] = centres, np.arange(len(q) - 8, len(q))
    return c


BIG = 2 ** 25   # the extent of a box from -2^24 to 2^24
BOXES = {"cube": (3000, 3000, 3000), "needle-x": (BIG, 39, 39), "needle-y": (39, BIG, 39), "needle-z": (39, 39, BIG),
         "sheet-xy": (BIG, BIG, 39), "sheet-yz": (39, BIG, BIG), "sheet-zx": (BIG, 39, BIG)}
COARSE_RADII = (1, 3)
COARSE_CASES = [(b, r) for b in BOXES for r in COARSE_RADII] + [("cube", 5)]   # the cube's side is 12: no multiple of 5
BLOCK = np.stack(np.meshgrid(*[np.arange(-1, 2)] * 3, indexing="ij"), -1).reshape(-1, 3)


@functools.lru_cache(maxsize=None)
def coarsened(box, r):
    """3 x 3 x 3 blocks of POIs around the voxels lo + c side - 1 and lo + c side of the coarsened grid, c the first, the middle and
    the last interior border of an axis: across a border in x, in y, in z (where the axis has more than one cell) and across all the
    borders at once (a cell corner).  Two POIs at opposite corners span the box."""
    extent = np.array(BOXES[box], np.int64)
    lo = np.where(extent == BIG, -2 ** 24, np.array([-11, 5, -39]))
    side, n = choose_grid(extent, r)
    # the interior borders c of each axis whose block stays inside the box; none where the axis has one cell
    picks = [[c for c in sorted({1, n[a] // 2, n[a] - 1}) if 0 < c < n[a] and c * side + 1 <= extent[a]] for a in range(3)]
    inside = lo + np.minimum(extent // 2, 17)   # where a block sits on the axes it does not straddle
    wanted = [(a,) for a in range(3) if picks[a]] + [tuple(a for a in range(3) if picks[a])]
    blocks = set()
    for axes in wanted:
        for t in range(3):
            at = inside.copy()
            for a in axes:
                at[a] = lo[a] + picks[a][min(t, len(picks[a]) - 1)] * side
            blocks.add((tuple(int(v) for v in at), tuple(int(a in axes) for a in range(3))))
    blocks = sorted(blocks)
    centres, spans = np.array([k[0] for k in blocks], np.int64), np.array([k[1] for k in blocks])
    q = np.concatenate([ctr + BLOCK for ctr in centres] + [np.stack([lo, lo + extent])])
    rng = np.random.default_rng(90 + r + sum(map(ord, box)))
    u = (q / 2.0 ** 24) @ G0.T + B0 + rng.normal(0.0, 0.05, (len(q), 3))
    c = case(q, u, radius=r, min_neighbours=4)
    c["extent"], c["lo"], c["block_centres"], c["block_spans"], c["grid"] = extent, lo, centres, spans, (side, n)
    return c


OUTSIDE_RADII = (4, 7)


@functools.lru_cache(maxsize=None)
def outside(r):
    """a contributing 5 x 5 x 5 grid at spacing 3 (voxels 0 .. 12) with a linear field plus noise, shifted off the origin, and POIs that
    do not contribute (in turn a valid byte of 0, a NaN and an infinite displacement under a byte of 1) outside its box: beyond each
    face at distance 1 (a fit), r - 1, r (one plane is in reach: degenerate) and r + 1 (nothing), beyond an edge and a corner
    diagonally at the same distances, and 10001 voxels beyond the low and 10000 beyond the high face of each axis"""
    rng = np.random.default_rng(60 + r)
    g = np.arange(5) * 3
    grid = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    out, kinds = [], []
    for dist in (1, r - 1, r, r + 1):
        for a in range(3):
            for low in (True, False):
                p = np.array([6, 7, 5])
                p[a] = -dist if low else 12 + dist
                out.append(p), kinds.append("face")
        for low in (True, False):
            e = -dist if low else 12 + dist
            out += [np.array([e, e, 6]), np.array([6, e, e]), np.array([e, 6, 12 - e]), np.array([e, e, e]), np.array([e, 12 - e, e])]
            kinds += ["edge"] * 3 + ["corner"] * 2
    for a in range(3):
        for far in (-10001, 12 + 10000):
            p = np.array([6, 7, 5])
            p[a] = far
            out.append(p), kinds.append("far")
    q = np.concatenate([grid, np.array(out)]) + np.array([-2, 30, -40])
    u = q @ G0.T + B0 + rng.normal(0.0, 0.01, (len(q), 3))
    valid = np.ones(len(q), np.uint8)
    for k in range(len(out)):
        row = len(grid) + k
        if k % 3 == 0:
            valid[row] = 0
        else:
            u[row, k % 3] = (np.nan, np.inf, -np.inf)[k % 3]
    c = case(q, u, valid, radius=r, min_neighbours=4)
    c["outsiders"], c["kinds"] = np.arange(len(grid), len(q)), kinds
    return c


# ---- invariances of the parity inputs ------------------------------------------------------------------------------------------------
INVARIANCE_RADII = (7, 20)
OUTSIDERS = np.array([[-3, 20, 21], [62, 51, 43]])   # beyond the low x face and beyond the high corner of the 60 x 50 x 40 box


@functools.lru_cache(maxsize=None)
def parity_with_outsiders():
    """the parity inputs and two POIs just outside their box that do not contribute (a byte of 0, a NaN under a byte of 1)"""
    q, u, valid = ref.parity_inputs()
    q = np.concatenate([q, OUTSIDERS]).astype(np.int32)
    u = np.concatenate([u, [[0.5, -0.25, 1.0], [np.nan, 0.0, 0.0]]])
    valid = np.concatenate([valid, [0, 1]]).astype(np.uint8)
    for a in (q, u, valid):
        a.setflags(write=False)
    return q, u, valid


def translations():
    q, u, valid = ref.parity_inputs()
    on = ref.contributes(q, u, valid)
    lo, hi = q[on].min(0).astype(np.int64), q[on].max(0).astype(np.int64)
    return {"straddle": np.array([-30, -25, -20]), "minus-1000": np.array([-1000] * 3), "low-corner": -2 ** 24 - lo, "high-corner": 2 ** 24 - hi}


@functools.lru_cache(maxsize=None)
def translated(name, r):
    """the parity inputs with their outsiders, every point moved by translations()[name].  c["out_of_range"]: the outsiders the move
    takes past 2^24 (status 2, every field 0); every other record is claimed to equal the unmoved one byte for byte"""
    q, u, valid = parity_with_outsiders()
    moved = q.astype(np.int64) + (translations()[name] if name != "none" else 0)
    c = case(moved, u, valid, radius=r, min_neighbours=ref.PARITY_MIN_NEIGHBOURS)
    c["out_of_range"] = np.flatnonzero((np.abs(moved) > ref.COORD_MAX).any(1))
    return c


def translation_disagreement(base, got, out_of_range):
    """the fields of `got` (a moved case) that are not the bytes of `base` (the unmoved one) outside the rows out of range, and what is
    wrong with those rows"""
    rows = np.ones(len(base["status"]), bool)
    rows[out_of_range] = False
    bad = [k for k in ref.FLOATS + ("neighbours", "status") if got[k][rows].tobytes() != base[k][rows].tobytes()]
    if not (got["status"][out_of_range] == 2).all() or any(got[k][out_of_range].any() for k in ref.FLOATS + ("neighbours",)):
        bad.append("out of range")
    return bad


AXIS_MAPS = [(p, s) for p, s in zip(itertools.permutations(range(3)), ((-1, 1, 1), (1, -1, 1), (1, 1, -1), (-1, -1, 1), (1, -1, -1), (-1, -1, -1)))]


def axis_matrix(perm, signs):
    """Q with (Q q)_a = signs[a] q[perm[a]]"""
    Q = np.zeros((3, 3), np.int64)
    for a in range(3):
        Q[a, perm[a]] = signs[a]
    return Q


def sym_of(E):
    """(m, 6) xx yy zz xy yz zx -> (m, 3, 3)"""
    return E[:, [0, 3, 5, 3, 1, 4, 5, 4, 2]].reshape(-1, 3, 3)


def six_of(S):
    return np.stack([S[:, 0, 0], S[:, 1, 1], S[:, 2, 2], S[:, 0, 1], S[:, 1, 2], S[:, 2, 0]], 1)


def mapped_result(res, Q):
    """what the results `res` become when every point and displacement is multiplied by Q"""
    Qf = Q.astype(np.float64)
    out = {k: res[k].copy() for k in ("principal", "equivalent", "rms", "neighbours", "status")}
    out["disp"] = res["disp"] @ Qf.T
    out["G"] = np.einsum("ab,nbc,dc->nad", Qf, res["G"], Qf)
    out["E"] = six_of(np.einsum("ab,nbc,dc->nad", Qf, sym_of(res["E"]), Qf))
    return out


# ---- affine fields with known strains ------------------------------------------------------------------------------------------------
def _dyadic(G, bits=10):
    return np.round(np.asarray(G, np.float64) * 2.0 ** bits) / 2.0 ** bits


def _rotation(axis, angle):
    k = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


def known_fields():
    """name -> (G, constant): G's entries are multiples of 2^-10 (the rotation's of 2^-30, the graded one's of 2^-40), so u = G q + b is exact"""
    R = _dyadic(_rotation((1, 2, 2), np.pi / 6), 30)
    V = _rotation((2, -1, 3), 0.7)
    graded = _dyadic(V @ np.diag([1e-1, 1e-6, 1e-11]) @ V.T, 40)   # symmetric: with measure 1, E = G
    return {"dilation": (_dyadic(0.02 * np.eye(3)), B0), "uniaxial": (_dyadic(np.diag([0.03125, 0, 0])), B0),
            "shear": (_dyadic([[0, 0.0625, 0], [0, 0, 0], [0, 0, 0]]), B0), "rotation": (R - np.eye(3), B0),
            "large": (_dyadic([[1.5, -2.25, 0.75], [0.5, 2.0, -1.25], [-1.75, 0.25, 1.0]]), B0), "graded": (graded, B0),
            "constant": (np.zeros((3, 3)), np.array([3.0, -1.5, 0.25]))}


@functools.lru_cache(maxsize=None)
def known(name):
    """a 7 x 7 x 7 grid at spacing 3 about the origin, radius 6, under the exactly affine field known_fields()[name]"""
    G, b = known_fields()[name]
    g = np.arange(-3, 4) * 3
    q = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    u = q @ G.T + b
    c = case(q, u, radius=6)
    c["G"], c["b"] = G, b
    return c
