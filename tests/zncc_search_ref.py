"""NumPy restatement of the ZNCC integer search's contract (sift3d_zncc_search, include/sift3d_hip.h): test infrastructure only.
fp64 by default; f32=True forms R - (float)Rm, T - Tc, every product and every sum over the subset in float32, which is what measures
how far a float32 evaluation may lie from the fp64 one.  A loop over (ez, ey) with ex vectorised (a matrix product per step).
Also the scenes and POIs that tests/test_gpu_search.py compares with the GPU, so that tests/test_search_cpu.py can check their margins
without one."""
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
    Rm = sub.astype(np.float64).sum() / N
    dR = np.sqrt(((sub.astype(np.float64) - Rm) ** 2).sum())
    if not (dR > 0.0) or not np.isfinite(dR):
        return 4, tab
    tz, ty, tx = T.shape
    (xl, xh), (yl, yh), (zl, zh) = (admissible(a, b, r, s, n) for a, b, n in zip((x, y, z), g, (tx, ty, tz)))
    if xl > xh or yl > yh or zl > zh:
        return 3, tab
    c = [min(max(a + int(b), 0), n - 1) for a, b, n in zip((x, y, z), g, (tx, ty, tz))]
    Tc = T[c[2], c[1], c[0]]
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
