"""Planted keypoints for the two one-keypoint entries (sift3d_orient_keypoint / sift3d_describe_keypoint): the cases, shared by
tests/test_kp_cases_cpu.py (the cases do what they claim, asserted on the oracle alone) and tests/test_gpu_orient_edges.py /
tests/test_gpu_describe_edges.py (the HIP path against the oracle on every one of them).  Pure NumPy plus the oracle, no GPU.

A case is ``Case(name, level, unit, rec, args)``: a level [z, y, x] (shared between the cases that use it: never written to), the
level's unit, a KP_DTYPE record and, for the orientation, ``(sigma, max_eig_ratio, corner_thresh)``.

ORIENTATION WINDOW PATHS.  k_orient (kernels_orient.hip) takes one of three paths.  With (x0..x1, y0..y1) the window clipped to
[1, n - 2], tw = x1 - x0 + 3, th = y1 - y0 + 3 (footprint plus the central-difference border), len = floor(r^2 / u^2) + 2 the length
of the weight table and nin the largest squared offset inside the sphere:

    lds_list   tw <= 28 and th <= 27 and len <= 256, and the lattice list exists (append_lut: floor(sqrt(nin)) <= 127, nin < 65536)
               and its central plane #{(dx, dy): dx^2 + dy^2 <= nin} holds at most 512 entries (8 per lane)
    lds_box    tw <= 28 and th <= 27 and len <= 256, central plane above 512 entries: box scan over the LDS tiles
    global     everything else: box scan with six global loads per voxel

At unit 1 a whole window of radius r has tw = th = 2 ceil(r) + 3: whole windows up to r = 12 are lds_list, from r > 12 global; the
central plane passes 512 entries at nin = 161 (r = 12.69), so lds_box needs 12.69 <= r < 15.94 AND a border that clips the window to
26 x 25.  SIZE_PATHS below states the path of every case of the size family, TILE_PATHS of the tile-limit cases;
tests/test_kp_cases_cpu.py recomputes tw, th, len and the central plane and asserts both tables.
"""
import collections
import ctypes
import ctypes.util
import functools

import numpy as np

import oracle_lib as ol

KP_DTYPE = ol.KP_DTYPE
Case = collections.namedtuple("Case", "name level unit rec args")
f32 = np.float32
UNITS = (1.0, 2.0, 4.0, 16.0)
PLANT_VALUES = (("nan", np.float32(np.nan)), ("inf", np.float32(np.inf)), ("3e38", np.float32(3e38)))
AMPLITUDE_EXPONENTS = tuple(range(-24, 0)) + (-126, -60, -40, 4, 10, 20, 40, 60)

# |sum - fp64 sum| / sum |term| of the ORACLE's sequential fp32 window sums, largest over every orientation case of this module
# (measured and asserted by tests/test_kp_cases_cpu.py::test_fp64_bar_of_the_sequential_sums, which prints it); the GPU's parallel sums
# of rejected keypoints get 4x this (tests/test_gpu_orient_edges.py)
ORACLE_SEQ_RATIO = 4.17e-5   # 4.162e-5, at the radius-20 window (33 000 terms one after the other)
FP64_BAR = 4.0 * ORACLE_SEQ_RATIO

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.expf.restype = ctypes.c_float
_libm.expf.argtypes = [ctypes.c_float]


def rec_at(x, y, z, scale, rotation=None, str_tensor=None):
    r = np.zeros(1, KP_DTYPE)
    r["x"], r["y"], r["z"], r["scale"] = x, y, z, scale
    r["rx"] = r["ry"] = r["rz"] = -1.0
    if rotation is not None:
        r["Rotation"][0] = np.asarray(rotation, np.float32).reshape(9)
    if str_tensor is not None:
        r["str_tensor"][0] = np.asarray(str_tensor, np.float32).reshape(9)
    return r[0]


# ---- window geometry, restated from win_bounds / append_lut / k_orient ---------------------------------------------------------
def win_bounds(c, rad, u, n):
    q = f32(rad) / f32(u)
    s, e = int(np.floor(f32(c) - q)), int(np.ceil(f32(c) + q))
    return max(s, 1), min(e, n - 2)


def ori_radius(sigma):
    return f32(sigma) * f32(3.0)


def desc_radius(scale):
    return f32(2.0) * (f32(scale) * f32(7.071067812))


def lut_len_nin(radius, u):
    r2, uu = f32(radius) * f32(radius), f32(u) * f32(u)
    n_len = int(np.floor(float(r2) / float(uu))) + 2
    nin = -1
    for n in range(n_len):
        if not f32(n) * uu > r2:
            nin = n
    return n_len, nin


def central_plane(nin):
    r = int(np.floor(np.sqrt(max(nin, 0))))
    d = np.arange(-r, r + 1)
    return int(((d[:, None] ** 2 + d[None, :] ** 2) <= nin).sum())


def orient_path(shape, unit, rec, sigma):
    """(path, tw, th, len, central plane entries) of k_orient for this window"""
    nz, ny, nx = shape
    rad = ori_radius(sigma)
    x0, x1 = win_bounds(rec["x"], rad, unit, nx)
    y0, y1 = win_bounds(rec["y"], rad, unit, ny)
    z0, z1 = win_bounds(rec["z"], rad, unit, nz)
    tw, th = x1 - x0 + 3, y1 - y0 + 3
    n_len, nin = lut_len_nin(rad, unit)
    cp = central_plane(nin)
    if x1 < x0 or y1 < y0 or z1 < z0:
        return "empty", tw, th, n_len, cp
    if tw <= 28 and th <= 27 and n_len <= 256:
        has_list = int(np.floor(np.sqrt(max(nin, 0)))) <= 127 and nin < 65536
        return ("lds_list" if has_list and cp <= 512 else "lds_box"), tw, th, n_len, cp
    return "global", tw, th, n_len, cp


def clipped(shape, unit, rec, radius):
    """does the level's border cut the window's box?"""
    nz, ny, nx = shape
    q = f32(radius) / f32(unit)
    for c, n in ((rec["x"], nx), (rec["y"], ny), (rec["z"], nz)):
        if int(np.floor(f32(c) - q)) < 1 or int(np.ceil(f32(c) + q)) > n - 2:
            return True
    return False


# ---- fp64 sums of the orientation window's fp32 terms ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ori_weights(sigma, unit):
    sigma, u = f32(sigma), f32(unit)
    rad = ori_radius(sigma)
    r2, uu, s2 = rad * rad, u * u, sigma * sigma
    n_len = int(np.floor(float(r2) / float(uu))) + 2
    w = np.full(n_len, -1.0, np.float32)
    for n in range(n_len):
        sq = f32(n) * uu
        if not sq > r2:
            w[n] = _libm.expf(f32(-0.5 * float(sq) / float(s2)))  # the reference's expf((float)(-0.5 * (double)sq / (double)(sigma * sigma)))
    return w


def orient_sums(level, unit, rec, sigma):
    """Assign_Orientation_Imp's window sums with the reference's fp32 terms (weights from expf in fp32, central differences in fp32,
    products in fp32) ACCUMULATED IN FP64: (sums[9], sum of |term| [9]) in the order t00 t01 t02 t11 t12 t22 g0 g1 g2"""
    nz, ny, nx = level.shape
    cx, cy, cz = int(rec["x"]), int(rec["y"]), int(rec["z"])
    rad = ori_radius(sigma)
    x0, x1 = win_bounds(cx, rad, unit, nx)
    y0, y1 = win_bounds(cy, rad, unit, ny)
    z0, z1 = win_bounds(cz, rad, unit, nz)
    w = _ori_weights(float(f32(sigma)), float(unit))
    dz, dy, dx = np.meshgrid(np.arange(z0, z1 + 1) - cz, np.arange(y0, y1 + 1) - cy, np.arange(x0, x1 + 1) - cx, indexing="ij")
    n = dx * dx + dy * dy + dz * dz
    ww = np.where(n < len(w), w[np.minimum(n, len(w) - 1)], f32(-1.0)).astype(np.float32)
    ok = ww >= 0
    inv_u = f32(1.0) / f32(unit)
    zs, ys, xs = slice(z0, z1 + 1), slice(y0, y1 + 1), slice(x0, x1 + 1)
    with np.errstate(all="ignore"):
        def half(a, b):
            return (0.5 * (a - b).astype(np.float64)).astype(np.float32) * inv_u
        vx = half(level[zs, ys, x0 + 1:x1 + 2], level[zs, ys, x0 - 1:x1])
        vy = half(level[zs, y0 + 1:y1 + 2, xs], level[zs, y0 - 1:y1, xs])
        vz = half(level[z0 + 1:z1 + 2, ys, xs], level[z0 - 1:z1, ys, xs])
        terms = (vx * vx * ww, vx * vy * ww, vx * vz * ww, vy * vy * ww, vy * vz * ww, vz * vz * ww, vx * ww, vy * ww, vz * ww)
        sums = np.array([t[ok].astype(np.float64).sum() for t in terms])
        mags = np.array([np.abs(t[ok].astype(np.float64)).sum() for t in terms])
    return sums, mags


def record_sums(rec):
    st = rec["str_tensor"]
    return np.array([st[0], st[1], st[2], st[4], st[5], st[8], rec["win"][0], rec["win"][1], rec["win"][2]], np.float32)


def sum_ratio(rec, sums, mags):
    """largest |component - fp64 sum| / sum |term| of a record's window sums; None when a sum is not finite (poisoned window)"""
    got = record_sums(rec).astype(np.float64)
    if not (np.isfinite(got).all() and np.isfinite(sums).all() and np.isfinite(mags).all()):
        return None
    err = np.abs(got - sums)
    if (err[mags == 0] != 0).any():
        return np.inf
    nz = mags > 0
    return float((err[nz] / mags[nz]).max()) if nz.any() else 0.0


# ---- thresholds, as finish_orientation forms them in fp32 --------------------------------------------------------------------
def _dot3(a, b):
    return f32(f32(f32(a[0]) * f32(b[0])) + f32(f32(a[1]) * f32(b[1]))) + f32(f32(a[2]) * f32(b[2]))


def eig_ratio_f32(rec):
    ev = rec["eigvalue"].astype(np.float32)
    return max(abs(f32(ev[0] / ev[1])), abs(f32(ev[1] / ev[2])))


def corner_f32(rec):
    w3 = rec["win"].astype(np.float32)
    dn = np.sqrt(_dot3(w3, w3))
    corner = f32(np.finfo(np.float32).max)
    for i in (2, 1):
        v = rec["eigvector"][3 * i:3 * i + 3].astype(np.float32)
        a = abs(f32(_dot3(v, w3) / f32(dn * np.sqrt(_dot3(v, v)))))
        corner = min(corner, a)
    return f32(corner)


# ---- levels ---------------------------------------------------------------------------------------------------------------------
_levels = {}


def levels(orc):
    """L0: the oracle's gss(0, 2) of blobs((48, 44, 52), seed 11); L1: the same of an odd (41, 37, 45) volume (rows of 45 and 37).  On the
    device the 16-byte pieces start at the alignment of the BOX the entry cuts out, not of the level's rows: the border sweeps give box
    widths 11 .. 21 (orientation) and 17 .. 33 (descriptor), every residue modulo 4.  Built once."""
    if not _levels:
        import importlib
        synth = importlib.import_module("3dsift_amd.synth")
        _levels["L0"] = orc.extractor(synth.blobs((48, 44, 52), seed=11, noise=0.01)).run(1).gss(0, 2)
        _levels["L1"] = orc.extractor(synth.blobs((41, 37, 45), seed=12, noise=0.01)).run(1).gss(0, 2)
        for a in _levels.values():
            a.setflags(write=False)
    return _levels


_big = {}


def big_level(orc):
    """120^3 blobs smoothed with sigma 2: the only level the radius-55 descriptor windows fit in (one test only)"""
    if not _big:
        import importlib
        synth = importlib.import_module("3dsift_amd.synth")
        _big["L"] = orc.gaussian_smooth(synth.blobs((120, 120, 120), seed=13, noise=0.01), 2.0)
        _big["L"].setflags(write=False)
    return _big["L"]


def border_positions(shape, R):
    """(tag, x, y, z): distance d = 0 .. R + 1 from each of the 6 faces (the other coordinates central), the 8 corners and the 12
    edge midpoints at d = 1 and d = R // 2"""
    nz, ny, nx = shape
    dims, mid = (nx, ny, nz), (nx // 2, ny // 2, nz // 2)
    out = []
    for a in range(3):
        for far in (0, 1):
            for d in range(R + 2):
                p = list(mid)
                p[a] = dims[a] - 1 - d if far else d
                out.append(("face%s%s_d%d" % ("xyz"[a], "+-"[1 - far], d), *p))
    for d in sorted({1, max(R // 2, 1)}):
        for sx in (0, 1, 2):       # 0: near face, 1: far face, 2: central
            for sy in (0, 1, 2):
                for sz in (0, 1, 2):
                    k = (sx == 2) + (sy == 2) + (sz == 2)
                    if k > 1:
                        continue   # corners (no central coordinate) and edge midpoints (one)
                    p = [(d, dims[i] - 1 - d, mid[i])[s] for i, s in enumerate((sx, sy, sz))]
                    out.append(("%s%d%d%d_d%d" % ("corner" if k == 0 else "edge", sx, sy, sz, d), *p))
    return out


# ---- orientation families ----------------------------------------------------------------------------------------------------------
ORI_BORDER = dict(scale=2.0, sigma=3.0)   # radius 9


def orient_border(orc, unit=1.0):
    out = []
    for ln, L in levels(orc).items():
        R = int(np.ceil(float(ori_radius(ORI_BORDER["sigma"])) / unit))
        for tag, x, y, z in border_positions(L.shape, R):
            out.append(Case("oborder_%s_u%g_%s" % (ln, unit, tag), L, unit, rec_at(x, y, z, ORI_BORDER["scale"]), (ORI_BORDER["sigma"], 0.9, 0.4)))
    return out


def size_sigmas():
    """(R, side, sigma): 3 sigma just under and just over every integer radius 1 .. 20"""
    return [(R, side, float(f32((R + eps) / 3.0))) for R in range(1, 21) for side, eps in (("under", -0.01), ("over", 0.01))]


def size_positions(shape):
    nz, ny, nx = shape
    return (("c", nx // 2, ny // 2, nz // 2), ("x2", 2, ny // 2, nz // 2), ("y2", nx // 2, 2, nz // 2), ("z2", nx // 2, ny // 2, 2))


def orient_sizes(orc, unit=1.0):
    L = levels(orc)["L0"]
    return [Case("osize_R%d_%s_%s_u%g" % (R, side, tag, unit), L, unit, rec_at(x, y, z, 2.0), (sigma, 0.9, 0.4))
            for R, side, sigma in size_sigmas() for tag, x, y, z in size_positions(L.shape)]


# the path of every (R, side) of the size family at unit 1 on L0 (52 x 44 x 48), positions c / x2 / y2 / z2: L = lds_list, B = lds_box,
# G = global.  A whole window is 2 ceil(r) + 3 wide: R "over" is one voxel wider than R "under".  d = 2 from the x face clips the
# window to x1 = 2 + ceil(r) columns (tw = ceil(r) + 4 <= 28), which leaves th = 2 ceil(r) + 3 <= 27 in charge: r <= 12; the y face
# likewise.  (44 rows: the y-central window of r > 20 is clipped at both ends, still far above 27.)
SIZE_PATHS = {
    **{(R, "under"): "LLLL" for R in range(1, 13)},
    **{(R, "over"): "LLLL" for R in range(1, 12)},
    (12, "over"): "GGGG",   # ceil(12.01) = 13: tw = 29 whole; x2: th = 29; y2: tw = 29
    **{(R, s): "GGGG" for R in range(13, 21) for s in ("under", "over")},
}
_LETTER = {"lds_list": "L", "lds_box": "B", "global": "G"}

# windows whose clipped footprint sits exactly on and around the tile limits (kTileW = 28, kTileH = 27), sigma 4.2 (r = 12.6, len 160,
# central plane 489 <= 512: the list) and 4.5 (r = 13.5, len 184, central plane 577: the box scan); and one window small enough for
# the tile whose table is too long for its LDS copy (r = 16.2: len 264 > 256), clipped on x and y by a corner position
TILE_PATHS = (
    # name, sigma, (tw, th), path
    ("tile_28x27_list", 4.2, (28, 27), "lds_list"),
    ("tile_29x27", 4.2, (29, 27), "global"),
    ("tile_28x28", 4.2, (28, 28), "global"),
    ("tile_27x28", 4.2, (27, 28), "global"),
    ("tile_28x27_box", 4.5, (28, 27), "lds_box"),
    ("tile_27x26_box", 4.5, (27, 26), "lds_box"),
    ("tile_24x23_longlut", 5.4, (24, 23), "global"),
)


def _coord_for_width(n, rad, want, far=False):
    """the coordinate nearest the low (far: high) face whose clipped window is `want` voxels wide"""
    for c in (range(n - 1, -1, -1) if far else range(0, n)):
        lo, hi = win_bounds(c, rad, 1.0, n)
        if hi - lo + 1 == want:
            return c
    raise AssertionError((n, rad, want))


def orient_tiles(orc):
    L = levels(orc)["L0"]
    nz, ny, nx = L.shape
    out = []
    for name, sigma, (tw, th), _ in TILE_PATHS:
        rad = ori_radius(sigma)
        # clipped by the low faces (the tile's LAST row and column lie outside the sphere: ceil(r) > r) and by the high faces (its last row and
        # column carry window voxels, and their central differences read the row / column behind them: tile row th - 1, tile column tw - 1)
        for side, far in (("lo", False), ("hi", True)):
            x, y = _coord_for_width(nx, rad, tw - 2, far), _coord_for_width(ny, rad, th - 2, far)
            for tag, z in (("zc", nz // 2), ("z3", 3)):
                out.append(Case("%s_%s_%s" % (name, side, tag), L, 1.0, rec_at(x, y, z, 2.0), (sigma, 0.9, 0.4)))
    return out


def _probe_grid(shape, step=4, margin=4):
    nz, ny, nx = shape
    return [(x, y, z) for z in range(margin, nz - margin, step) for y in range(margin, ny - margin, step) for x in range(margin, nx - margin, step)]


_accepted = {}


def accepted_keypoints(orc, count=24):
    """voxels of L0 the oracle ACCEPTS with the border family's (scale, sigma): clipped windows of the border family first, then a grid"""
    if "k" not in _accepted:
        L = levels(orc)["L0"]
        pos = [(x, y, z) for c in orient_border(orc) if c.level is L and clipped(L.shape, 1.0, c.rec, 9.0) for x, y, z in [(int(c.rec["x"]), int(c.rec["y"]), int(c.rec["z"]))]]
        got = []
        for x, y, z in pos + _probe_grid(L.shape):
            if orc.orient_one(rec_at(x, y, z, 2.0), L, 1.0, 3.0)[0] == 1 and (x, y, z) not in got:
                got.append((x, y, z))
        _accepted["k"] = got
    return _accepted["k"][:count]


def interior_accepted(orc, count=4):
    """accepted voxels of L0 whose orientation AND descriptor (scale 1) windows are whole, with room for three floats behind the tile row"""
    if "i" not in _accepted:
        L = levels(orc)["L0"]
        nz, ny, nx = L.shape
        got = []
        for z in range(17, nz - 17, 2):
            for y in range(17, ny - 17, 2):
                for x in range(17, nx - 17, 2):
                    if orc.orient_one(rec_at(x, y, z, 2.0), L, 1.0, 3.0)[0] == 1 and orc.orient_one(rec_at(x, y, z, 1.0), L, 1.0, 1.5)[0] == 1:
                        got.append((x, y, z))
        _accepted["i"] = got
    return _accepted["i"][:count]


def amplitude_keypoints(orc):
    return accepted_keypoints(orc)[:2] + interior_accepted(orc, 2)


def ramp(shape, g, offset=0.25):
    nz, ny, nx = shape
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    return (offset + g[0] * (x - nx // 2) + g[1] * (y - ny // 2) + g[2] * (z - nz // 2)).astype(np.float32)


RAMP_DIRECTIONS = ((0.01, 0.0, 0.0), (0.0, 0.0, 0.0125), (0.004, 0.003, 0.002), (0.01, 0.01, 0.01), (-0.007, 0.002, 0.0051), (0.0031, -0.0092, 0.0017))


def orient_codes(orc):
    """every code: -1 on a constant level, -2 on pure ramps (a rank-one tensor: the ratio test runs on rounding noise of either sign)
    and on the near-isotropic neighbourhood of a blob, -3 and 1 from L0"""
    shape = (37, 35, 39)
    out = [Case("code_constant", np.full(shape, 0.5, np.float32), 1.0, rec_at(19, 17, 18, 2.0), (3.0, 0.9, 0.4))]
    for i, g in enumerate(RAMP_DIRECTIONS):
        for sigma in (3.0, 2.2):
            out.append(Case("code_ramp%d_s%g" % (i, sigma), ramp(shape, g), 1.0, rec_at(19, 17, 18, 2.0), (sigma, 0.9, 0.4)))
    nz, ny, nx = shape
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    for i, (ox, oy, oz) in enumerate(((0.3, 0.2, 0.1), (0.5, 0.5, 0.5), (0.05, -0.4, 0.25))):
        blob = np.exp(-0.5 * ((x - 19 - ox) ** 2 + (y - 17 - oy) ** 2 + (z - 18 - oz) ** 2) / 6.0 ** 2).astype(np.float32)
        out.append(Case("code_blob%d" % i, blob, 1.0, rec_at(19, 17, 18, 2.0), (3.0, 0.9, 0.4)))
    L = levels(orc)["L0"]
    for x, y, z in _probe_grid(L.shape, step=6):
        out.append(Case("code_L0_%d_%d_%d" % (x, y, z), L, 1.0, rec_at(x, y, z, 2.0), (3.0, 0.9, 0.4)))
    return out


def orient_straddles(orc):
    """(ratio triples, corner triples): for every accepted keypoint three calls with max_eig_ratio at nextafter(m, 0), m, nextafter(m, 2)
    (m = max(r01, r12) in fp32, corner_thresh 0: the oracle's codes are -2, 1, 1) and three with corner_thresh at nextafter(c, 0), c,
    nextafter(c, 2) (c = the corner cosine in fp32, max_eig_ratio 0.9: 1, 1, -3)"""
    L = levels(orc)["L0"]
    ratio, corner = [], []
    for x, y, z in accepted_keypoints(orc)[:20] + interior_accepted(orc, 4):
        rec = rec_at(x, y, z, 2.0)
        code, k = orc.orient_one(rec, L, 1.0, 3.0)
        assert code == 1
        m, c = eig_ratio_f32(k), corner_f32(k)
        for tag, v in (("below", np.nextafter(m, f32(0))), ("at", m), ("above", np.nextafter(m, f32(2)))):
            ratio.append(Case("ratio_%d_%d_%d_%s" % (x, y, z, tag), L, 1.0, rec, (3.0, float(v), 0.0)))
        for tag, v in (("below", np.nextafter(c, f32(0))), ("at", c), ("above", np.nextafter(c, f32(2)))):
            corner.append(Case("corner_%d_%d_%d_%s" % (x, y, z, tag), L, 1.0, rec, (3.0, 0.9, float(v))))
    return ratio, corner


_gg = {}


def orient_gg_straddles(orc, count=6):
    """pairs (weak, strong): s L0 at two ADJACENT fp32 factors s between which the oracle's code turns from -1 (|mean gradient|^2 <
    1e-10) to something else, found by bisection; for `count` keypoints"""
    if "c" not in _gg:
        L = levels(orc)["L0"]
        out = []
        for x, y, z in [(26, 22, 24)] + accepted_keypoints(orc)[:count - 1]:
            rec = rec_at(x, y, z, 2.0)
            code = lambda s: orc.orient_one(rec, L * f32(s), 1.0, 3.0)[0]
            lo, hi = f32(1e-9), f32(1.0)
            assert code(lo) == -1 and code(hi) != -1
            while np.nextafter(lo, f32(2)) < hi:
                mid = f32(np.sqrt(float(lo) * float(hi)))
                if not lo < mid < hi:
                    mid = np.nextafter(lo, f32(2))
                if code(mid) == -1:
                    lo = mid
                else:
                    hi = mid
            out.append((Case("gg_%d_%d_%d_weak" % (x, y, z), L * lo, 1.0, rec, (3.0, 0.9, 0.4)),
                        Case("gg_%d_%d_%d_strong" % (x, y, z), L * hi, 1.0, rec, (3.0, 0.9, 0.4)), float(lo), float(hi)))
        _gg["c"] = out
    return _gg["c"]


def _plant(L, x, y, z, v):
    a = L.copy()
    a[z, y, x] = v
    return a


def orient_plants(orc):
    """[(kind, case, unplanted case)]: a NaN, a +Inf and a 3e38 at (a) the corner of the window's box (outside the sphere, no in-sphere
    voxel beside it), (b) the voxel just outside the sphere that the central difference of the sphere's +x pole reads, (c) the centre,
    (d) the three floats behind column tw - 1 of a tile row.  The entry does not run k_orient on the caller's level: it copies the BOX the
    window reaches, [x - 10, x + 10]^3 for this whole radius-9 window, and passes its dimensions as the level's.  A tile row is then a
    whole box row (tw = 21), and what its sixth 16-byte piece reads behind column 20 are box columns 0 .. 2 of the NEXT row -- or, behind
    the last row of a plane, of row 0 of the next plane.  Planted there, at places nothing legitimate reads: row y + 9 (the only
    in-sphere voxel of that row is dx = 0; read behind row y + 8), column 0 of row y + 1 (its x-neighbour x - 9 has n = 82 > nin = 81),
    and row y - 10 of plane z + 1 (the border row; read behind the last row of plane z)"""
    L = levels(orc)["L0"]
    out = []
    for x, y, z in interior_accepted(orc, 2) + [(26, 22, 24)]:
        rec = rec_at(x, y, z, 2.0)
        base = Case("oplant_%d_%d_%d_none" % (x, y, z), L, 1.0, rec, (3.0, 0.9, 0.4))
        assert not clipped(L.shape, 1.0, rec, 9.0)
        places = (("a", (x - 9, y - 9, z - 9)), ("a", (x + 9, y + 9, z - 9)), ("b", (x + 10, y, z)), ("b", (x, y, z - 10)), ("c", (x, y, z)),
                  ("d", (x - 10, y + 9, z)), ("d", (x - 9, y + 9, z)), ("d", (x - 8, y + 9, z)), ("d", (x - 10, y + 1, z)),
                  ("d", (x - 10, y - 10, z + 1)), ("d", (x - 9, y - 10, z + 1)), ("d", (x - 8, y - 10, z + 1)))
        for kind, (px, py, pz) in places:
            for vn, v in PLANT_VALUES:
                out.append((kind, Case("oplant_%d_%d_%d_%s_%d_%d_%d_%s" % (x, y, z, kind, px - x, py - y, pz - z, vn), _plant(L, px, py, pz, v), 1.0, rec,
                                       (3.0, 0.9, 0.4)), base))
    return out


_scaled = {}


def scaled_level(orc, e):
    if e not in _scaled:
        _scaled[e] = (levels(orc)["L0"].astype(np.float64) * 2.0 ** e).astype(np.float32)
    return _scaled[e]


def orient_amplitude(orc):
    return [Case("oamp_%d_%d_%d_e%d" % (x, y, z, e), scaled_level(orc, e), 1.0, rec_at(x, y, z, 2.0), (3.0, 0.9, 0.4))
            for e in AMPLITUDE_EXPONENTS for x, y, z in amplitude_keypoints(orc)]


# ---- descriptor families -----------------------------------------------------------------------------------------------------------
IDENTITY = np.eye(3, dtype=np.float32)


def oriented_record(orc, L, unit, x, y, z, scale):
    """the record the orientation stage would hand the descriptor: the oracle's orient_one with the pipeline's sigma = 1.5 scale; its
    rotation when accepted, else the identity; its structure tensor either way"""
    code, k = orc.orient_one(rec_at(x, y, z, scale), L, unit, f32(1.5) * f32(scale))
    st = k["str_tensor"] if np.isfinite(k["str_tensor"]).all() else np.zeros(9, np.float32)
    return rec_at(x, y, z, scale, k["Rotation"].reshape(3, 3) if code == 1 else IDENTITY, st)


def describe_border(orc, unit=1.0):
    out = []
    for ln, L in levels(orc).items():
        R = int(np.ceil(float(desc_radius(1.0)) / unit))
        for tag, x, y, z in border_positions(L.shape, R):
            out.append(Case("dborder_%s_u%g_%s" % (ln, unit, tag), L, unit, oriented_record(orc, L, unit, x, y, z, 1.0), ()))
    return out


def rotations():
    """the 24 proper signed permutations, the identity first (voxel offsets land exactly on cell faces and centres), 45 degrees about
    each axis, 8 seeded random rotations: 35"""
    import itertools
    out = []
    for p in itertools.permutations(range(3)):
        for s in itertools.product((1.0, -1.0), repeat=3):
            m = np.zeros((3, 3))
            for i in range(3):
                m[i, p[i]] = s[i]
            if np.linalg.det(m) > 0:
                out.append(("perm%d%d%d_%s" % (*p, "".join("+" if v > 0 else "-" for v in s)), m))
    assert len(out) == 24 and np.array_equal(out[0][1], np.eye(3))
    c = np.sqrt(0.5)
    out.append(("x45", np.array([[1, 0, 0], [0, c, -c], [0, c, c]])))
    out.append(("y45", np.array([[c, 0, c], [0, 1, 0], [-c, 0, c]])))
    out.append(("z45", np.array([[c, -c, 0], [c, c, 0], [0, 0, 1]])))
    rng = np.random.default_rng(31)
    for i in range(8):
        q, r = np.linalg.qr(rng.standard_normal((3, 3)))
        q = q * np.sign(np.diag(r))
        if np.linalg.det(q) < 0:
            q[:, 2] = -q[:, 2]
        out.append(("rand%d" % i, q))
    return [(n, m.astype(np.float32)) for n, m in out]


def describe_rotations(orc):
    L = levels(orc)["L0"]
    nz, ny, nx = L.shape
    out = []
    for tag, (x, y, z) in (("c", (nx // 2, ny // 2, nz // 2)), ("corner3", (3, ny - 4, 3))):
        st = oriented_record(orc, L, 1.0, x, y, z, 1.0)["str_tensor"]
        for rn, m in rotations():
            out.append(Case("drot_%s_%s" % (tag, rn), L, 1.0, rec_at(x, y, z, 1.0, m, st), ()))
    return out


def mesh_directions(orc):
    """unit vectors: the 12 vertices, 30 edge midpoints and 20 face centres of the oracle's icosahedron"""
    v, _ = orc.mesh()
    v = v.astype(np.float64)
    key = lambda p: tuple(int(t) for t in np.round(p * 1000))
    verts, edges, faces = {}, {}, []
    for f in range(20):
        for j in range(3):
            verts[key(v[f, j])] = v[f, j]
        for a, b in ((0, 1), (1, 2), (0, 2)):
            edges[key(v[f, a] + v[f, b])] = v[f, a] + v[f, b]
        faces.append(v[f].sum(axis=0))
    assert len(verts) == 12 and len(edges) == 30
    out = [("vertex%d" % i, d) for i, (_, d) in enumerate(sorted(verts.items()))] + [("edge%d" % i, d) for i, (_, d) in enumerate(sorted(edges.items()))] + \
          [("face%d" % f, d) for f, d in enumerate(faces)]
    return [(n, d / np.linalg.norm(d)) for n, d in out]


def describe_icosahedron(orc):
    """level = a ramp along d plus 1e-3 of a smooth seeded perturbation, d over the icosahedron's vertices, edge midpoints and face
    centres turned by the case's rotation: the rotated gradients of the window scatter around a place where two, three or five faces
    meet -- the symmetry lookup, its 6e-6 margin and the ordered scan behind it, through the real march"""
    shape = (37, 35, 39)
    nz, ny, nx = shape
    z, y, x = np.meshgrid(np.arange(nz, dtype=np.float64), np.arange(ny, dtype=np.float64), np.arange(nx, dtype=np.float64), indexing="ij")
    rng = np.random.default_rng(41)
    pert = np.zeros(shape)
    for _ in range(6):
        k, ph = rng.uniform(-0.35, 0.35, 3), rng.uniform(0, 2 * np.pi)
        pert += np.sin(k[0] * x + k[1] * y + k[2] * z + ph) / max(np.linalg.norm(k), 0.1)
    pert /= 6.0
    rots = rotations()
    out = []
    for rn, m in (rots[0], rots[-1]):
        for dn, d in mesh_directions(orc):
            g = m.astype(np.float64) @ d   # the descriptor turns the gradient by Rotation^T: Rotation^T (Rotation d) = d
            L = (0.5 + 0.02 * (g[0] * (x - 19) + g[1] * (y - 17) + g[2] * (z - 18) + 1e-3 * pert)).astype(np.float32)
            st = np.zeros(9, np.float32)
            st[[0, 4, 8]] = (0.02 * g) ** 2 * 50.0
            out.append(Case("dico_%s_%s" % (rn, dn), L, 1.0, rec_at(19, 17, 18, 1.0, m, st), ()))
    return out


def first_guess_tensors(true_st):
    t = np.asarray(true_st, np.float32)
    return (("zero", np.zeros(9, np.float32)), ("2^-40", t * f32(2.0 ** -40)), ("true", t), ("2^40", t * f32(2.0 ** 40)),
            ("inf", np.full(9, np.inf, np.float32)), ("nan", np.full(9, np.nan, np.float32)))


def describe_first_guess(orc):
    """[(case, shift)]: the same record with str_tensor set to zero, true x 2^-40, true, true x 2^40, +Inf and NaN, each under
    hook("desc_mass_shift", s) for s in (0, 20, 40); the oracle ignores str_tensor: one expected row per keypoint"""
    L = levels(orc)["L0"]
    out = []
    for x, y, z in accepted_keypoints(orc)[:1] + interior_accepted(orc, 2):
        base = oriented_record(orc, L, 1.0, x, y, z, 1.0)
        for tn, t in first_guess_tensors(base["str_tensor"]):
            for shift in (0, 20, 40):
                out.append((Case("dguess_%d_%d_%d_%s_s%d" % (x, y, z, tn, shift), L, 1.0, rec_at(x, y, z, 1.0, base["Rotation"].reshape(3, 3), t), ()), shift))
    return out


DESC_SCALES = (0.3, 1.0, 2.7, 2.8, 3.9)   # table lengths 20, 201, 1459, 1570 (> kMaxDescLut = 1536: table in global memory), 3043 (radius 55)


def describe_sizes(orc):
    """descriptor windows of scale 0.3 .. 3.9 at unit 1, central in the 120^3 level and clipped at d = 5 from a corner; and flat windows"""
    L = big_level(orc)
    out = []
    for scale in DESC_SCALES:
        for tag, (x, y, z) in (("c", (60, 60, 60)), ("corner5", (5, 114, 5))):
            out.append(Case("dsize_s%g_%s" % (scale, tag), L, 1.0, oriented_record(orc, L, 1.0, x, y, z, scale), ()))
    flat = np.full((37, 35, 39), 0.25, np.float32)
    for scale in (0.3, 1.0):
        out.append(Case("dsize_flat_s%g" % scale, flat, 1.0, rec_at(19, 17, 18, scale, IDENTITY), ()))
    return out


def describe_amplitude(orc):
    """L0 2^e: the record (rotation, structure tensor) is the UNSCALED level's -- the first guess of the unit is off by 2^e; the oracle
    runs on each scaled level"""
    L = levels(orc)["L0"]
    out = []
    for x, y, z in amplitude_keypoints(orc):
        rec = oriented_record(orc, L, 1.0, x, y, z, 1.0)
        for e in AMPLITUDE_EXPONENTS:
            out.append(Case("damp_%d_%d_%d_e%d" % (x, y, z, e), scaled_level(orc, e), 1.0, rec, ()))
    return out


# x axis -> the cube's diagonal: the sphere's +x pole (14 voxels out) lies inside the rotated 4x4x4 cube (half width 10 per axis)
_DIAG = np.array([[1, 1, 1], [1, -1, 0], [1, 1, -2]], np.float64)
DIAG_ROTATION = (_DIAG / np.linalg.norm(_DIAG, axis=1, keepdims=True)).astype(np.float32)
assert np.linalg.det(DIAG_ROTATION.astype(np.float64)) > 0


def describe_plants(orc):
    """[(kind, case, unplanted case)]: (a) the corner of the window's box, (b) the voxel behind the sphere's +x pole (read by the pole's
    central difference; Rotation^T turns the x axis onto the cube's diagonal, so the pole is inside the cube), (c) the centre"""
    L = levels(orc)["L0"]
    out = []
    for x, y, z in interior_accepted(orc, 2):
        st = oriented_record(orc, L, 1.0, x, y, z, 1.0)["str_tensor"]
        rec = rec_at(x, y, z, 1.0, DIAG_ROTATION, st)
        assert not clipped(L.shape, 1.0, rec, desc_radius(1.0))
        base = Case("dplant_%d_%d_%d_none" % (x, y, z), L, 1.0, rec, ())
        for kind, (px, py, pz) in (("a", (x - 15, y - 15, z - 15)), ("a", (x + 15, y - 15, z + 15)), ("b", (x + 15, y, z)), ("c", (x, y, z))):
            for vn, v in PLANT_VALUES:
                out.append((kind, Case("dplant_%d_%d_%d_%s_%d_%d_%d_%s" % (x, y, z, kind, px - x, py - y, pz - z, vn), _plant(L, px, py, pz, v), 1.0, rec, ()), base))
    return out


# ---- the oracle on a case ---------------------------------------------------------------------------------------------------------
def oracle_orient(orc, c):
    sigma, mer, ct = c.args
    return orc.orient_one(c.rec, c.level, c.unit, sigma, mer, ct)


def oracle_describe(orc, c):
    """(record with the rotation transposed, row): describe_one takes the rotation as the orientation stage left it"""
    return orc.describe_one(c.rec, c.level, c.unit)


def by_tables(cases):
    """order of the GPU calls: onekp_prepare rebuilds its tables when (sigma, scale) change and its context when the unit does"""
    return sorted(cases, key=lambda c: (c.unit, float(c.rec["scale"]), c.args[0] if c.args else 0.0))
