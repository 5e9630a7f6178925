"""Inputs of the guided matcher's tests (tests/test_match_guided_cpu.py, tests/test_gpu_match_guided.py).  Plain NumPy, no GPU.

A case is a dict: a, ax, b, bx, pred (float32), radius, and what it was built for, which the CPU module checks on the restatement
(tests/match_guided_ref.py) before the GPU module compares the kernel with it:
  sizes   {row: the number of targets in its gate}
  best    {row: (gIdx, sIdx) of the forward pass before any filter}
  in_gate / not_in_gate   lists of (row, column)
Rows are of 768 floats, n and m stay below about 700.  The kernel walks a row's window in chunks of 64 entries and scores the gated
columns 64 at a time: the gate sizes sit on those edges.  The index's cells have the side ceil(radius) + 1 (SIDE) and start at the
least floor of the targets' coordinates; a window is walked cell row by cell row (z, then y, x ascending), a cell's targets in
ascending column.
"""
import functools

import numpy as np

import match_cases as mc

F32 = np.float32
KD = mc.KD
THRESH = mc.THRESH
RADII = (0.5, 2.5, 16.0, 4096.0)
GATE_SIZES = (0, 1, 2, 63, 64, 65, 128, 129)
DENSE = 400
ALL_GATE = 4096.0   # holds every target of every case whose coordinates stay within +-2000


def side(radius):
    return int(np.ceil(radius)) + 1


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def _unit(rng, n):
    return mc.unit_rows(rng, n, True)


def _noisy(rng, rows, amount=0.3):
    c = rows + amount * _unit(rng, len(rows))
    return c / np.linalg.norm(c, axis=1, keepdims=True)


def _case(a, ax, b, bx, pred, radius, **extra):
    f = lambda v, w: np.ascontiguousarray(v, F32).reshape(-1, w)
    return dict(a=f(a, KD), ax=f(ax, 3), b=f(b, KD), bx=f(bx, 3), pred=f(pred, 3), radius=float(radius), **extra)


def scene(seed, n, m, box, radius, lo=0.0, jitter=0.25, share=3):
    """m targets scattered in [lo, lo + box)^3; reference row i is a noisy copy of target t_i and is expected jitter away from it
    (uniform per axis, in units of the radius); every `share`-th row shares its target with the row before it (mode 3 masks those)"""
    rng = _rng(seed)
    b = _unit(rng, m)
    bx = lo + rng.uniform(0, box, (m, 3))
    t = rng.integers(0, m, n)
    for k in range(share, n, share):
        t[k] = t[k - 1]
    a = _noisy(rng, b[t])
    pred = bx[t] + rng.uniform(-jitter, jitter, (n, 3)) * radius
    ax = pred - np.array([3.0, -2.0, 1.0])
    return _case(a, ax, b, bx, pred, radius, target=t)


def gate_sizes():
    """row i < 8: a cluster of GATE_SIZES[i] targets strictly inside the gate of its prediction, clusters 200 apart; 40 more rows
    look at the clusters from the side and hold a part of one"""
    rng = _rng(11)
    r = 16.0
    centres = np.array([[200.0 * i + 0.37, 50.21, -30.6] for i in range(len(GATE_SIZES))])
    bx = np.concatenate([centres[i] + rng.uniform(-15.5, 15.5, (k, 3)) for i, k in enumerate(GATE_SIZES)])
    m = len(bx)
    b = _unit(rng, m)
    first = np.concatenate([[0], np.cumsum(GATE_SIZES)])
    pred = [c for c in centres]
    a = []
    for i, k in enumerate(GATE_SIZES):   # the best is the LAST column of the cluster, the second its first
        a.append(b[first[i + 1] - 1] + (0.6 * b[first[i]] if k > 1 else 0) if k else _unit(rng, 1)[0])
    for q in range(40):
        i = 3 + q % 5
        pred.append(centres[i] + rng.uniform(-20, 20, 3))
        a.append(b[rng.integers(first[i], first[i + 1])])
    a = np.array(a)
    a /= np.linalg.norm(a, axis=1, keepdims=True)
    best = {i: (int(first[i + 1] - 1) if k else -1, int(first[i]) if k > 1 else -1) for i, k in enumerate(GATE_SIZES)}
    return _case(a, np.array(pred) + 1.5, b, bx, pred, r, sizes=dict(enumerate(GATE_SIZES)), best=best)


def dense():
    """one cluster of DENSE targets: row 0 holds all of them, 60 more rows hold some hundreds; 150 targets lie scattered around"""
    rng = _rng(12)
    r = 16.0
    c = np.array([40.5, 41.25, 39.75])
    bx = np.concatenate([c + rng.uniform(-15.9, 15.9, (DENSE, 3)), c + rng.uniform(-120, 120, (150, 3))])
    far = np.abs(bx[DENSE:] - c).max(1) > 16.5
    bx = np.concatenate([bx[:DENSE], bx[DENSE:][far]])
    m = len(bx)
    b = _unit(rng, m)
    t = np.concatenate([[DENSE - 1], rng.integers(0, DENSE, 60)])
    pred = np.concatenate([[c], bx[t[1:]] + rng.uniform(-6, 6, (60, 3))])
    return _case(_noisy(rng, b[t]), pred - 2.0, b, bx, pred, r, sizes={0: DENSE}, target=t)


def edges(radius):
    """a target exactly `radius` from the prediction on one axis (in the gate) and one at the next float beyond (out), on each axis and
    with both signs; radius 16 adds the rounding case: prediction 0.99999994f, target 17 -- the exact difference 16.00000006 rounds
    to 16.0f (in) while the floors differ by 17 -- and its mirror image, prediction 1, target -15.00000095f (the difference is half
    an ulp beyond -16 and the tie rounds to it; floors 1 and -16).  Every row also holds a decoy 0.25 away.  The row's descriptor is the edge
    target's, so the edge target is the best wherever it is in the gate."""
    rng = _rng(13)
    r = F32(radius)
    step = max(1024.0, 8.0 * float(r))   # between the rows, along the axis after the tested one
    kinds = ["exact", "beyond"] + (["rounding"] if radius == 16.0 else [])
    bx, pred, in_gate, out_gate, best, rounding = [], [], [], [], {}, []
    for axis in range(3):
        for sign in (1.0, -1.0):
            for kind in kinds:
                row = len(pred)
                p = np.zeros(3, F32)
                p[(axis + 1) % 3] = F32(step * (row + 1))
                p[(axis + 2) % 3] = F32(77.0)
                t = p.copy()
                if kind == "rounding":
                    rounding.append(row)
                    p[axis] = np.nextafter(F32(1), F32(0)) if sign > 0 else F32(1)
                    t[axis] = F32(17) if sign > 0 else np.nextafter(F32(-15), F32(-np.inf))
                else:
                    p[axis] = F32(sign * 1024.0)
                    t[axis] = p[axis] + F32(sign) * r
                    assert float(t[axis]) == float(p[axis]) + sign * float(r)   # representable
                    if kind == "beyond":
                        t[axis] = np.nextafter(t[axis], F32(sign * np.inf))
                decoy = p.copy()
                decoy[(axis + 2) % 3] += F32(0.25)
                pred.append(p)
                bx += [decoy, t]   # columns 2 row, 2 row + 1
                (out_gate if kind == "beyond" else in_gate).append((row, 2 * row + 1))
                in_gate.append((row, 2 * row))
                best[row] = (2 * row, -1) if kind == "beyond" else (2 * row + 1, 2 * row)
    b = _unit(rng, len(bx))
    a = b[1::2] + 0.5 * b[0::2]
    a /= np.linalg.norm(a, axis=1, keepdims=True)
    return _case(a, np.array(pred), b, np.array(bx), np.array(pred), radius, in_gate=in_gate, not_in_gate=out_gate, best=best, rounding=rounding,
                 sizes={row: 1 + ((row, 2 * row + 1) in in_gate) for row in range(len(pred))})


def all_cells():
    """600 targets in exactly 3 x 3 x 3 cells, 27 of them planted one per cell 14 from the middle; the rows are expected near the
    middle, so their gates reach into all 27"""
    rng = _rng(14)
    r, s = 16.0, side(16.0)
    bx = rng.uniform(0, 3 * s, (600, 3))
    bx[0] = 0.5   # the grid starts at floor 0
    bx[1:28] = 1.5 * s + 14.0 * (np.stack(np.meshgrid(*[np.arange(3)] * 3, indexing="ij"), -1).reshape(-1, 3) - 1)
    b = _unit(rng, 600)
    pred = 1.5 * s + rng.uniform(-1, 1, (30, 3))
    t = np.array([np.flatnonzero(np.abs(bx - p).max(1) < 15)[k % 7] for k, p in enumerate(pred)])
    return _case(_noisy(rng, b[t]), pred + 0.5, b, bx, pred, r, target=t, cells27=list(range(30)))


def outside_box():
    """targets in [0, 50)^3; predictions beyond each face of their bounding box: far away (the window misses the grid) and close
    enough for the gate to reach back in"""
    rng = _rng(15)
    bx = rng.uniform(0, 50, (400, 3))
    b = _unit(rng, 400)
    pred, sizes = [], {}
    for axis in range(3):
        for sign in (-1, 1):
            for dist in (100.0, 17.5, 10.0):
                p = np.array([25.3, 24.6, 25.9])
                p[axis] = (50.0 + dist) if sign > 0 else -dist
                if dist > 16.0:
                    sizes[len(pred)] = 0
                pred.append(p)
    pred.append(np.array([-500.0, 700.0, 1e6]))
    sizes[len(pred) - 1] = 0
    pred = np.array(pred)
    t = np.array([int(np.argmin(np.abs(bx - p).max(1))) for p in pred])
    return _case(_noisy(rng, b[t]), pred, b, bx, pred, 16.0, sizes=sizes, target=t)


def one_cell():
    """every target in one cell of the index (their floors span less than the cell side)"""
    rng = _rng(16)
    bx = 100.0 + rng.uniform(0, 10, (300, 3))
    b = _unit(rng, 300)
    t = rng.integers(0, 300, 50)
    pred = bx[t] + rng.uniform(-12, 12, (50, 3))
    return _case(_noisy(rng, b[t]), pred, b, bx, pred, 16.0, target=t, one_cell=True)


def order():
    """Targets in 3 x 3 x 3 cells.  Rows 0..19: the row's best descriptor sits on two targets, the LOWER column in the last cell of the
    walk and the higher column in the first -- the lower column must win and the other be second.  Rows 20..29 / 30..39: the best is
    the first / the last gated entry of the walk (those rows are expected where the doubled targets are outside their gates)."""
    rng = _rng(17)
    r, s = 16.0, side(16.0)
    m = 500
    bx = rng.uniform(0, 3 * s, (m, 3))
    bx[m - 1] = 0.25
    b = _unit(rng, m)
    c = 1.5 * s
    pred = c + rng.uniform(-0.4, 0.4, (40, 3))
    pred[20:] += [-3.0, 4.0, 0.0]
    a = np.zeros((40, KD))
    best = {}
    for i in range(20):
        lo, hi = i, m - 2 - i                                   # lo < hi
        bx[lo] = [c + 14.0, c + 13.0, c + 15.0 - 0.01 * i]      # cell (2, 2, 2): walked last
        bx[hi] = [c - 14.0, c - 13.0, c - 15.0 + 0.01 * i]      # cell (0, 0, 0): walked first
        b[hi] = b[lo]
        a[i] = b[lo]
        best[i] = (lo, hi)
    key = lambda j: (int(bx[j, 2]) // s, int(bx[j, 1]) // s, int(bx[j, 0]) // s, j)
    F = lambda v: np.asarray(v, F32)
    for i in range(20, 40):
        inside = [j for j in range(m) if (np.abs(F(bx[j]) - F(pred[i])) <= F32(r)).all()]
        walk = sorted(inside, key=key)
        j = walk[0] if i < 30 else walk[-1]
        a[i] = b[j]
        best[i] = (j, None)
    a /= np.linalg.norm(a, axis=1, keepdims=True)
    return _case(a, pred, b, bx, pred, r, best=best, walk_key=key)


def negative():
    """negative and non-integer coordinates on both sides of zero: the cell of a target is the FLOOR of its coordinate"""
    c = scene(18, 300, 500, 90.0, 16.0, lo=-60.3)
    c["mixed_signs"] = True
    return c


def bad_positions():
    """NaN prediction rows, NaN and +-inf target coordinates, coordinates beyond 2^24 (in no gate, whatever the difference says) and at
    2^24 exactly (the last that are in)"""
    rng = _rng(19)
    big = 2.0 ** 24
    m, n = 120, 60
    bx = np.zeros((m, 3)); bx[:, 0] = rng.uniform(-30, 30, m); bx[:, 1:] = rng.uniform(0, 9, (m, 2))
    t = rng.integers(20, m, n)
    pred = bx[t] + rng.uniform(-2, 2, (n, 3))
    for j, (ax_, v) in enumerate([(0, np.nan), (1, np.inf), (2, -np.inf), (0, -np.inf), (2, np.nan)]):
        bx[j, ax_] = v
    bx[5, 0], bx[6, 0], bx[7, 0], bx[8, 0] = big, big + 2, -big, -big - 2
    bx[9] = [big, 4.0, 4.0]
    pred[0] = np.nan
    pred[1] = [bx[21, 0], np.nan, bx[21, 2]]
    pred[2] = [np.inf, 4.0, 4.0]
    pred[3] = [big - 3, bx[5, 1], bx[5, 2]]      # holds the targets 5 and 9 if they are near in y and z
    pred[4] = [big + 2, bx[6, 1], bx[6, 2]]      # beyond the bound itself: empty
    pred[5] = [-big, bx[7, 1], bx[7, 2]]
    pred[6] = [-big - 2, bx[8, 1], bx[8, 2]]
    b = _unit(rng, m)
    a = _noisy(rng, b[t])
    a[3], a[5] = b[5], b[7]
    return _case(a, np.nan_to_num(pred, nan=1.0, posinf=2.0), b, bx, pred, 16.0,
                 sizes={0: 0, 1: 0, 2: 0, 4: 0, 6: 0}, in_gate=[(3, 5), (5, 7)], not_in_gate=[(4, 6), (6, 8), (3, 6), (5, 8)],
                 dead_targets=[0, 1, 2, 3, 4, 6, 8])


def hostile(name):
    """a hostile descriptor class of tests/match_cases.py (zero rows, negative scores, NaN / inf components) with positions: row i is
    expected near the target planted as its best"""
    src = mc.CASES[name]()
    rng = _rng(20)
    n, m = len(src["a"]), len(src["b"])
    pred = src["bx"][np.arange(n) % m] + rng.uniform(-4, 4, (n, 3))
    return _case(src["a"], src["ax"], src["b"], src["bx"], pred, 16.0)


HOSTILE = ["zero_ref_rows", "zero_tar_rows", "negative_only", "one_hot", "dup_7", "nonfinite_nan_tar5", "nonfinite_pinf_tar5",
           "nonfinite_ninf_tar21", "nonfinite_nan_ref0", "nonfinite_pinf_ref127", "nonfinite_ninf_ref199"]
PURPOSE_ROWS = 150


def purpose():
    """What the gate is for: every target descriptor is present twice, once where the reference keypoint lands and once 300 voxels
    away.  The two score alike, so sift3d_match's ratio test (mode 1) rejects every row; at radius 8 the far copy is in no gate and
    every row is accepted with the near copy.  Even rows have the near copy in the lower column, odd rows in the higher; column 0 is
    an unrelated target (a rejected index 0 would stay 0 by the reference's sign flip)."""
    rng = _rng(21)
    k = PURPOSE_ROWS
    grid = np.stack(np.meshgrid(*[np.arange(6)] * 3, indexing="ij"), -1).reshape(-1, 3)[:k] * 30.0   # 30 apart: one per gate
    ax = grid + rng.uniform(0, 5, (k, 3))
    move = lambda x: x * 1.01 + np.array([2.5, -1.5, 0.75])
    d = _unit(rng, k)
    near, far = move(ax), move(ax) + np.array([300.0, 0.0, 0.0])
    low_is_near = (np.arange(k) % 2 == 0)[:, None]
    bx = np.concatenate([[[-500.0, -500.0, -500.0]], np.where(low_is_near, near, far), np.where(low_is_near, far, near)])
    b = np.concatenate([_unit(rng, 1), d, d])
    want = np.where(low_is_near[:, 0], 1 + np.arange(k), 1 + k + np.arange(k))
    return _case(_noisy(rng, d, 0.2), ax, b, bx, move(ax), 8.0, want=want, best={i: (int(want[i]), -1) for i in range(k)})


def random_big():
    """700 x 650 planted descriptors with scattered positions: the case of the all-holding gate"""
    c = mc.planted(700, 650, 250, 4242, False)
    rng = _rng(22)
    return _case(c["a"], c["ax"], c["b"], c["bx"], rng.uniform(0, 100, (700, 3)), ALL_GATE)


def empty(n, m):
    rng = _rng(23)
    return _case(_unit(rng, n), rng.uniform(0, 50, (n, 3)), _unit(rng, m), rng.uniform(0, 50, (m, 3)), rng.uniform(0, 50, (n, 3)), 16.0,
                 sizes={i: 0 for i in range(n)})


def _build():
    cases = {}

    def add(name, fn, *args):
        cases[name] = functools.lru_cache(maxsize=None)(functools.partial(fn, *args))

    add("gate_sizes", gate_sizes)
    add("dense", dense)
    for r in RADII:
        add(f"edges_r{r:g}", edges, r)
        add(f"scene_r{r:g}", scene, 100 + int(r), 400, 600, 60.0 * max(1.0, r / 4.0) if r < 100 else 100.0, r)
    add("all_cells", all_cells)
    add("outside_box", outside_box)
    add("one_cell", one_cell)
    add("order", order)
    add("negative", negative)
    add("bad_positions", bad_positions)
    for h in HOSTILE:
        add(f"hostile_{h}", hostile, h)
    add("purpose", purpose)
    add("random_big", random_big)
    add("empty_m0", empty, 40, 0)
    add("empty_n0", empty, 0, 40)
    return cases


CASES = _build()
NAMES = list(CASES)
MODES = (1, 2, 3)

_want = {}


def restated(orc, name, mode, radius=None):
    """match_guided_ref.match_guided of a case (at its own radius, or at another), computed once per process and shared; the forward
    rows are shared between the modes.  Never modified by the tests."""
    import match_guided_ref as ref

    c = CASES[name]()
    radius = c["radius"] if radius is None else radius
    if (name, mode, radius) not in _want:
        fwd = _want.get((name, "forward", radius))
        w = ref.match_guided(orc, c["a"], c["ax"], c["b"], c["bx"], c["pred"], radius, THRESH, mode, forward=fwd)
        _want[(name, "forward", radius)] = w.pop("forward")
        for v in w.values():
            v.setflags(write=False)
        _want[(name, mode, radius)] = w
    return _want[(name, mode, radius)]


FIELDS = ("gIdx", "sIdx", "gDist", "sDist", "candidates", "pairs")


def same(x, y):
    """exact equality of two result arrays: floats by bits"""
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    if x.shape != y.shape or x.dtype != y.dtype:
        return False
    if x.dtype == np.float32:
        return np.array_equal(x.view(np.uint32), y.view(np.uint32))
    return np.array_equal(x, y)
