"""NumPy restatement of the ZNCC integer search's contract (sift3d_zncc_search, include/sift3d_hip.h): test infrastructure only.
fp64 by default; f32=True forms R - (float)Rm, T - Tc, every product and every sum over the subset in float32, which is what measures
how far a float32 evaluation may lie from the fp64 one.  A loop over (ez, ey) with ex vectorised (a matrix product per step).
Also the scenes and POIs that tests/test_gpu_search.py and tests/test_gpu_search_plans.py compare with the GPU, so that
tests/test_search_cpu.py can check their margins without one."""
import functools

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

import icgn_ref

MAX_GUESS = 1 << 24


def admissible(q, g, r, s, n):
    """inclusive range (lo, hi) of e + s on one axis, in Python integers: q + g + e - r >= 0 and q + g + e + r <= n - 1"""
    q, g, n = int(q), int(g), int(n)
    if abs(g) > MAX_GUESS:
        return 0, -1
    return max(0, r - q - g + s), min(2 * s, n - 1 - r - q - g + s)


def centre(T, c, r):
    """Tc, the level the sums are centred on: over the subset of T at c = q + g clamped to [r, n - 1 - r] on every axis (the subset of
    the admissible candidate nearest to e = 0), the finite voxel nearest to the fp64 mean of the finite voxels, the lowest index
    (dz, dy, dx) among equals; 0 when no voxel is finite.  A voxel of T, so T - Tc is exact on integer data and 0 on a constant T;
    within one standard deviation of the subset's mean, so that no single voxel sets the level."""
    tz, ty, tx = T.shape
    cx, cy, cz = (min(max(int(v), r), n - 1 - r) for v, n in zip(c, (tx, ty, tz)))
    sub = T[cz - r:cz + r + 1, cy - r:cy + r + 1, cx - r:cx + r + 1].astype(np.float64).ravel()
    fin = np.isfinite(sub)
    if not fin.any():
        return np.float32(0.0)
    mean = sub[fin].sum() / float(fin.sum())
    return np.float32(sub[np.argmin(np.where(fin, np.abs(np.where(fin, sub, 0.0) - mean), np.inf))])


def scores(R, T, q, g=(0, 0, 0), subset_radius=8, search_radius=8, f32=False):
    """(status, table): table[ez, ey, ex] is the score of candidate e = (ex, ey, ez) - s, NaN where it was not scored"""
    r, s = int(subset_radius), int(search_radius)
    D, E = 2 * r + 1, 2 * s + 1
    tab = np.full((E, E, E), np.nan)
    x, y, z = (int(v) for v in q)
    nz, ny, nx = R.shape
    if x < r or x > nx - 1 - r or y < r or y > ny - 1 - r or z < r or z > nz - 1 - r:
        return 2, tab
    sub = R[z - r:z + r + 1, y - r:y + r + 1, x - r:x + r + 1]
    N = float(D ** 3)
    with np.errstate(invalid="ignore"):
        Rm = sub.astype(np.float64).sum() / N
        dR = np.sqrt(((sub.astype(np.float64) - Rm) ** 2).sum())
    if not (dR > 0.0) or not np.isfinite(dR):
        return 4, tab
    tz, ty, tx = T.shape
    (xl, xh), (yl, yh), (zl, zh) = (admissible(a, b, r, s, n) for a, b, n in zip((x, y, z), g, (tx, ty, tz)))
    if xl > xh or yl > yh or zl > zh:
        return 3, tab
    Tc = centre(T, [a + int(b) for a, b in zip((x, y, z), g)], r)
    ft = np.float32 if f32 else np.float64
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        rm = ft(Rm)
        Rp = sub.astype(ft) - rm
        sr = Rp.astype(np.float64).sum()
        sh = float(Tc) - float(rm)
        x0 = x + int(g[0]) - s - r + xl  # T coordinate of the first voxel that an admissible candidate reads
        y0 = y + int(g[1]) - s - r + yl
        z0 = z + int(g[2]) - s - r + zl
        nex, ney, nez = xh - xl + 1, yh - yl + 1, zh - zl + 1
        Tp = T[z0:z0 + nez + D - 1, y0:y0 + ney + D - 1, x0:x0 + nex + D - 1].astype(ft) - ft(Tc)

        def box(v):  # sums over every D^3 box: along x, then y, then z
            for ax in (2, 1, 0):
                v = sliding_window_view(v, D, axis=ax).sum(-1, dtype=ft)
            return v.astype(np.float64)

        S1, S2 = box(Tp), box(Tp * Tp)
        Rk = np.ascontiguousarray(Rp.reshape(D * D, D).T)  # [dx, (dz, dy)]
        diag = (np.arange(D)[:, None], np.arange(nex)[None, :] + np.arange(D)[:, None])
        S3 = np.zeros((nez, ney, nex))
        for ez in range(nez):
            for ey in range(ney):
                M = Rk @ Tp[ez:ez + D, ey:ey + D, :].reshape(D * D, -1)  # [dx, x']: sum over (dz, dy) of R'[dz, dy, dx] T'[dz, dy, x']
                S3[ez, ey] = M[diag].sum(0, dtype=ft)                   # sum over dx of M[dx, ex + dx]
        tm = S1 / N
        dt2 = S2 - S1 * tm
        ttm = (S2 + 2.0 * sh * S1) + (N * sh) * sh
        zn = (S3 - tm * sr) / (dR * np.sqrt(dt2))
        ok = (dt2 > 1e-10 * ttm) & np.isfinite(zn)
        tab[zl:zh + 1, yl:yh + 1, xl:xh + 1] = np.where(ok, zn, np.nan)
    return (0 if np.isfinite(tab).any() else 3), tab


def pick(status, tab, g, s):
    """the record of one POI from its status and score table"""
    g = [int(v) for v in g]
    if status != 0:
        return {"d": g, "status": status, "zncc": 0.0, "zncc_second": -2.0, "candidates": 0}
    E = 2 * s + 1
    best = int(np.nanargmax(tab))  # the first of equal maxima: the lowest (ez, ey, ex)
    bz, by, bx = best // (E * E), best // E % E, best % E
    iz, iy, ix = np.meshgrid(np.arange(E), np.arange(E), np.arange(E), indexing="ij")
    far = np.isfinite(tab) & (np.maximum(np.maximum(abs(iz - bz), abs(iy - by)), abs(ix - bx)) > 1)
    return {"d": [g[0] + bx - s, g[1] + by - s, g[2] + bz - s], "status": 0, "zncc": float(tab[bz, by, bx]),
            "zncc_second": float(tab[far].max()) if far.any() else -2.0, "candidates": int(np.isfinite(tab).sum())}


def search(R, T, points, guess=None, subset_radius=8, search_radius=8, f32=False, tables=False):
    """the restatement of zncc_search over m POIs: arrays d (m, 3), status, zncc, zncc_second, candidates (and the score tables)"""
    pts = np.asarray(points).reshape(-1, 3)
    gs = np.zeros_like(pts) if guess is None else np.asarray(guess).reshape(-1, 3)
    recs, tabs = [], []
    for q, g in zip(pts, gs):
        st, tab = scores(R, T, q, g, subset_radius, search_radius, f32)
        recs.append(pick(st, tab, g, int(search_radius)))
        tabs.append(tab)
    out = {"d": np.array([a["d"] for a in recs], np.int64).reshape(-1, 3), "status": np.array([a["status"] for a in recs], np.int32),
           "zncc": np.array([a["zncc"] for a in recs]), "zncc_second": np.array([a["zncc_second"] for a in recs]),
           "candidates": np.array([a["candidates"] for a in recs], np.int32)}
    if tables:
        out["tables"] = tabs
    return out


def init_from_search(res, init, only_missing=True):
    out = np.array(init, np.float64).reshape(-1, 12).copy()
    for i, (d, st) in enumerate(zip(res["d"], res["status"])):
        if st == 0 and (not only_missing or not np.isfinite(out[i]).all()):
            out[i] = [d[0], 0, 0, 0, d[1], 0, 0, 0, d[2], 0, 0, 0]
    return out


# ---- the inputs of the GPU parity test --------------------------------------------------------------------------------------------
# (r, s) -> POIs: 27 candidates on 125 voxels (less than a workgroup), odd sizes, the whole window in LDS, and the slab path in an 80^3
# target.  The pair is non-cubic with R and T of different sizes: T is the scene's target with a border of (3, 1, 4) voxels cut off
# in (x, y, z), which shifts the truth by that much.
SHIFT = (4, -1, 3)             # the scene's integer move (x, y, z) ...
FRACTION = (0.06, -0.04, 0.05)  # ... and its fraction: the best integer is SHIFT
CUT = (3, 0, 4)                # voxels cut from T's low faces (x, y, z)
PARITY = {(2, 1): 40, (5, 7): 24, (8, 8): 12, (16, 16): 2}


def scene(shape, tvec, seed, per=24, sigma=(0.7, 1.2)):
    """R and T = R moved by tvec (x, y, z): narrow dense blobs (about one per `per` voxels), so that a subset of 5^3 voxels has texture
    and one voxel of misplacement costs its score far more than rounding does"""
    nz, ny, nx = shape
    b = max(8, nz * ny * nx // per)
    rng = np.random.Generator(np.random.PCG64(seed))
    c = np.stack([rng.uniform(0, nx, b), rng.uniform(0, ny, b), rng.uniform(0, nz, b)], 1)
    sg, am = rng.uniform(sigma[0], sigma[1], b), rng.uniform(0.3, 1.3, b)
    return icgn_ref.render(shape, c, sg, am), icgn_ref.render(shape, c + np.asarray(tvec, np.float64), sg, am)


@functools.lru_cache(maxsize=None)
def parity_scene(r, s):
    """R (nz, ny, nx), T, the true integer displacement (x, y, z) in T's frame"""
    if (r, s) == (16, 16):
        R, T = scene((80, 80, 80), np.add(SHIFT, FRACTION), seed=21)
        return R, T, np.array(SHIFT)
    R, T = scene((64, 56, 48), np.add(SHIFT, FRACTION), seed=22)  # nz, ny, nx = 64, 56, 48
    T = np.ascontiguousarray(T[CUT[2]:60, CUT[1]:, CUT[0]:46])   # 56 x 56 x 43
    return R, T, np.array(SHIFT) - np.array(CUT)


def parity_case(r, s, edge):
    """R, T, POIs and guesses of one parity case.  edge = 0: zero guess; edge = +1 / -1: a guess that puts the truth at e = (+s, ., .)
    or (-s, ., .), the edge of the search range.  Every POI keeps the subset at the truth inside T."""
    R, T, d = parity_scene(r, s)
    m = PARITY[(r, s)]
    rng = np.random.default_rng(1000 * r + 10 * s)
    nz, ny, nx = R.shape
    tz, ty, tx = T.shape
    lo = [max(r, r - int(d[a])) for a in range(3)]
    hi = [min(n - 1 - r, t - 1 - r - int(d[a])) for a, (n, t) in enumerate(zip((nx, ny, nz), (tx, ty, tz)))]
    q = np.stack([rng.integers(lo[a], hi[a] + 1, m) for a in range(3)], 1).astype(np.int32)
    g = np.zeros((m, 3), np.int32)
    if edge:
        g[:, 0] = d[0] - edge * s
        g[:, 1] = d[1] + rng.integers(-1, 2, m)
        g[:, 2] = d[2] + rng.integers(-1, 2, m)
    else:
        assert np.abs(d).max() <= s
    return R, T, q, g, d


@functools.lru_cache(maxsize=None)
def parity_reference(r, s, edge, f32=False):
    R, T, q, g, d = parity_case(r, s, edge)
    return search(R, T, q, g if edge else None, subset_radius=r, search_radius=s, f32=f32, tables=True)


EDGES = (0, 1, -1)


@functools.lru_cache(maxsize=None)
def parity_error():
    """e: the largest |zncc(f32 mode) - zncc(fp64 mode)| over every scored candidate of every parity input"""
    e = 0.0
    for (r, s) in PARITY:
        for edge in EDGES:
            a, b = parity_reference(r, s, edge), parity_reference(r, s, edge, True)
            for ta, tb in zip(a["tables"], b["tables"]):
                assert np.array_equal(np.isfinite(ta), np.isfinite(tb))
                e = max(e, float(np.nanmax(np.abs(ta - tb))))
    return e


def parity_bar():
    """the bar on |zncc(GPU) - zncc(fp64 restatement)|: 4 e, not below 1e-6"""
    return max(4.0 * parity_error(), 1e-6)


# ---- the inputs of tests/test_gpu_search_plans.py ---------------------------------------------------------------------------------
K_THREADS, K_CAND, LDS_FLOATS, MAX_GROUPS = 256, 5, 16128, 512


def search_plan(r, s):
    """(ec, zs) of kernels_search.hip's search_plan: the candidate planes per chunk and the subset planes per slab"""
    D, E = 2 * r + 1, 2 * s + 1
    W = D + 2 * s
    ec = min(max(K_THREADS * K_CAND // (E * E), 1), E)
    while ec > 1 and ec * W * W + D * D > LDS_FLOATS:
        ec -= 1
    return ec, min((LDS_FLOATS - (ec - 1) * W * W) // (W * W + D * D), D)


PAIRS = [(r, s) for r in range(2, 17) for s in range(1, 17)]
PLAN_SHAPE = (68, 70, 72)       # nz, ny, nx: the interior POI of r = s = 16 needs sides of at least 65
PLAN_MOVE = (-0.94, 0.96, 0.05)  # the best integer (-1, 1, 0) lies within s = 1, also where a face halves the range of e
PLAN_D = (-1, 1, 0)


@functools.lru_cache(maxsize=None)
def plan_scene():
    return scene(PLAN_SHAPE, PLAN_MOVE, seed=52)


def plan_case(r, s):
    """R, T and the three POIs of one (r, s): (a) interior, every candidate admissible; (b) the window clipped at T's low z face
    (lo[2] > 0, the number of admissible ez no multiple of ec where s allows it) and its high x face; (c) clipped at the high z and
    the low y face.  The truth PLAN_D is admissible for each."""
    R, T = plan_scene()
    nz, ny, nx = R.shape
    ec, _ = search_plan(r, s)
    k = next((k for k in range(s) if (s + 1 + k) % ec), 0)  # qz = r + k: s + 1 + k admissible planes of ez
    q = np.array([[nx // 2, ny // 2, nz // 2], [nx - 1 - r, ny // 2, r + k], [nx // 2 + 3, r, nz - 1 - r]], np.int32)
    return R, T, q


@functools.lru_cache(maxsize=None)
def plan_reference(r, s, f32=False):
    R, T, q = plan_case(r, s)
    return search(R, T, q, None, subset_radius=r, search_radius=s, f32=f32, tables=True)


# one call of more POIs than a launch has workgroups: workgroup j walks POIs j, j + 512 and j + 1024, whose kinds differ
LONG_M, LONG_R, LONG_S = 2 * MAX_GROUPS + 37, 2, 2
LONG_MOVE, LONG_D = (1.06, 0.96, 1.05), (1, 1, 1)
LONG_KINDS = ("full", "clipped", "st2", "full", "st4", "clipped", "st3")  # cyclically, no kind follows itself


@functools.lru_cache(maxsize=None)
def long_case():
    """R, T, POIs, guesses and kinds.  POI i = 512 p + j has kind LONG_KINDS[(j + p) % 7]: in a workgroup a full window (125 scored
    candidates) is followed by a heavily clipped one (stale slots in its score table), and the statuses 2, 4, 3 and 0 alternate.
    Status 4: a constant block set into R; status 3: a far guess."""
    r, s = LONG_R, LONG_S
    R, T = scene((40, 44, 48), LONG_MOVE, seed=61)
    R = R.copy()
    nz, ny, nx = R.shape
    R[nz - 9:, ny - 9:, nx - 9:] = np.float32(0.75)
    rng = np.random.default_rng(62)
    q, g, kinds = np.zeros((LONG_M, 3), np.int32), np.zeros((LONG_M, 3), np.int32), []
    for i in range(LONG_M):
        kind = LONG_KINDS[(i % MAX_GROUPS + i // MAX_GROUPS) % len(LONG_KINDS)]
        kinds.append(kind)
        inner = [int(rng.integers(r + s, n - 9 - r - s)) for n in (nx, ny, nz)]
        if kind == "full":
            q[i] = inner
        elif kind == "clipped":  # two or three low faces: (1 + s + j)^k candidates with j = 0 or 1
            q[i] = [r + int(rng.integers(0, 2)), r + int(rng.integers(0, 2)), r + int(rng.integers(0, 2)) if i % 2 else inner[2]]
        elif kind == "st2":
            q[i] = inner
            q[i][i % 3] = (r - 1, (nx, ny, nz)[i % 3] - r)[(i // 3) % 2]
        elif kind == "st4":
            q[i] = [n - 9 + r + int(rng.integers(0, 5)) for n in (nx, ny, nz)]
        else:
            q[i] = inner
            g[i][i % 3] = (60, -60, 1 << 25, -(1 << 30))[(i // 3) % 4]
    return R, T, q, g, tuple(kinds)


@functools.lru_cache(maxsize=None)
def long_reference(f32=False):
    R, T, q, g, _ = long_case()
    return search(R, T, q, g, subset_radius=LONG_R, search_radius=LONG_S, f32=f32, tables=True)


# voxel classes (named as in tests/input_classes.py) at (r, s) = (3, 8): a pair of the same class, 7 POIs further than r + s apart
# (no POI's planted voxel lies in another's window), the last with its window over T's high x face.  The move exceeds r along x, so
# the subset of the best candidate does not hold the voxel planted at q + g.
CLASS_R, CLASS_S = 3, 8
CLASS_MOVE, CLASS_D = (5.06, -1.04, 2.05), (5, -1, 2)
CLASS_POIS = ((12, 12, 12), (30, 12, 38), (48, 30, 12), (12, 43, 38), (30, 43, 12), (48, 43, 38), (51, 28, 40))
CLASSES = ("plain", "negated", "negdom", "quantised1000", "quantised30000", "offset32768", "nan_corner", "inf_corner", "nan_subset",
           "inf_subset", "nan_tc", "huge", "outlier0", "outlier65535", "outlier0_amp20", "outlier65535_amp20")


def quantise(v, base, amp):
    return np.round(np.float32(base) + np.float32(amp) * v).astype(np.float32)


@functools.lru_cache(maxsize=None)
def class_case(name):
    """R, T and the POIs (zero guess) of one voxel class"""
    R, T = scene((52, 56, 60), CLASS_MOVE, seed=71)
    q = np.array(CLASS_POIS, np.int32)
    w = CLASS_R + CLASS_S

    def plant(V, at, value):
        V = V.copy()
        for x, y, z in at:
            V[z, y, x] = value
        return V

    if name == "negated":
        R, T = -R, -T
    elif name == "negdom":
        R, T = R - np.float32(3.0), T - np.float32(3.0)
    elif name == "quantised1000":
        R, T = quantise(R, 1000, 200), quantise(T, 1000, 200)
    elif name == "quantised30000":
        R, T = quantise(R, 30000, 200), quantise(T, 30000, 200)
    elif name == "offset32768":
        R, T = R + np.float32(32768.0), T + np.float32(32768.0)
    elif name in ("nan_corner", "inf_corner"):  # the low corner of the window: candidate e = (-s, -s, -s) alone sees it
        T = plant(T, q[:6] - w, np.nan if name == "nan_corner" else np.inf)
    elif name in ("nan_subset", "inf_subset"):
        R = plant(R, q + np.array([1, -2, 3]), np.nan if name == "nan_subset" else -np.inf)
    elif name == "nan_tc":
        T = plant(T, q, np.nan)
    elif name == "huge":
        T = T * np.float32(2.0 ** 70)
    elif name.startswith("outlier"):
        amp = 20 if name.endswith("amp20") else 200
        R, T = quantise(R, 30000, amp), quantise(T, 30000, amp)
        T = plant(T, q, 0.0 if name.startswith("outlier0") else 65535.0)
    else:
        assert name == "plain", name
    return R, T, q


@functools.lru_cache(maxsize=None)
def class_reference(name, f32=False):
    R, T, q = class_case(name)
    return search(R, T, q, None, subset_radius=CLASS_R, search_radius=CLASS_S, f32=f32, tables=True)


def table_error(a, b):
    """the largest |zncc(a) - zncc(b)| over the candidates that both references scored, and whether they scored the same ones"""
    e, same = 0.0, True
    for ta, tb in zip(a["tables"], b["tables"]):
        fa, fb = np.isfinite(ta), np.isfinite(tb)
        same = same and bool(np.array_equal(fa, fb))
        if (fa & fb).any():
            e = max(e, float(np.abs(ta - tb)[fa & fb].max()))
    return e, same


@functools.lru_cache(maxsize=None)
def class_error(name):
    """e of one class: the largest |zncc(f32 mode) - zncc(fp64 mode)| over its scored candidates"""
    return table_error(class_reference(name), class_reference(name, True))


def class_bar(name):
    return max(4.0 * class_error(name)[0], 1e-6)


@functools.lru_cache(maxsize=None)
def plan_error():
    """e over every scored candidate of the 240 plan inputs and of the long call"""
    e = table_error(long_reference(), long_reference(True))[0]
    for r, s in PAIRS:
        e = max(e, table_error(plan_reference(r, s), plan_reference(r, s, True))[0])
    return e


def plan_bar():
    return max(4.0 * plan_error(), 1e-6)


# exact invariances: an integer-quantised pair at (r, s) = (3, 3), whose products neither underflow nor overflow under the scalings
INV_R, INV_S = 3, 3
INV_POIS = ((20, 22, 18), (4, 30, 25), (40, 4, 30), (25, 25, 4), (42, 38, 33), (12, 9, 33))  # four with a clipped window
INV_D = (1, -1, 2)
INV_R_OFFSET = 4097.0
INV_T_OFFSETS = (4097.0, -500.0, 30000.0)  # small enough for the rule dT^2 > 1e-10 sum (T - Rm)^2 to skip no candidate


@functools.lru_cache(maxsize=None)
def invariance_case():
    R, T = scene((40, 44, 48), (1.06, -1.04, 2.05), seed=81)
    return quantise(R, 1000, 200), quantise(T, 1000, 200), np.array(INV_POIS, np.int32)


@functools.lru_cache(maxsize=None)
def invariance_reference(offset=False, f32=False):
    """the pair as it is, or with INV_R_OFFSET added to R (not an exact invariance: Rm is rounded to float32)"""
    R, T, q = invariance_case()
    return search(R + np.float32(INV_R_OFFSET) if offset else R, T, q, None, subset_radius=INV_R, search_radius=INV_S, f32=f32, tables=True)


def invariance_error():
    return max(table_error(invariance_reference(o), invariance_reference(o, True))[0] for o in (False, True))


def invariance_bar():
    return max(4.0 * invariance_error(), 1e-6)
