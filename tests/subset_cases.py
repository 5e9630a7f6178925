"""The inputs of the subset-screening tests (tests/test_subset_cpu.py, tests/test_gpu_subset.py, tests/test_gpu_subset_edges.py): the
parity volumes and POIs, thresholds with a checked margin, the edge volume, and the walk order of k_subset_quality restated for the
seam tests (3dsift_amd/csrc/kernels_subset.hip: the cube of r_min in linear order, then each Chebyshev shell as face dz = -k, face
dz = +k, then per plane the ring: row dy = -k, row dy = +k, then the columns dx = -k / +k in pairs)."""
import functools

import numpy as np

import icgn_ref
import subset_ref as ref

SHAPE = (44, 46, 48)          # nz, ny, nx of the parity volumes
R_MIN, R_MAX = 4, 16          # the parity plan
MARGIN = 1e-6                 # relative distance of every threshold from every c(rho) it is compared with
EDGE_SHAPE = (68, 70, 72)     # nz, ny, nx of the edge volume (a 72 x 70 x 68 volume)


def _profile1d(n, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64)
    return sum(a * np.sin(w * t + p) for a, w, p in zip(rng.uniform(0.3, 1.0, 4), rng.uniform(0.2, 1.3, 4), rng.uniform(0, 6, 4)))


@functools.lru_cache(maxsize=None)
def volumes():
    """the parity volumes by name (float32, read-only)"""
    nz, ny, nx = SHAPE
    scene = icgn_ref.scene(SHAPE, seed=77)[0]
    half = scene.copy()
    half[:, :, :nx // 2] = 0.0  # the "air" half: x < nx / 2
    fz = _profile1d(nz, 1).astype(np.float32)
    fd = _profile1d(nx + ny, 2).astype(np.float32)
    x, y = np.arange(nx), np.arange(ny)
    diag = np.broadcast_to(fd[y[:, None] + x[None, :]][None], SHAPE)
    out = {"scene": scene, "half_flat": half, "layered": np.ascontiguousarray(np.broadcast_to(fz[:, None, None], SHAPE)),
           "diagonal": np.ascontiguousarray(diag), "diagonal_z": (diag + fz[:, None, None]).astype(np.float32)}
    rng = np.random.default_rng(5)
    out["uint8"] = rng.integers(0, 256, SHAPE).astype(np.float32)
    out["uint16"] = rng.integers(0, 65536, SHAPE).astype(np.float32)
    for v in out.values():
        v.setflags(write=False)
    return out


INTEGER = ("uint8", "uint16")
FLOAT = ("scene", "half_flat", "layered", "diagonal", "diagonal_z")


def pois(shape=SHAPE):
    """an interior grid (every radius of the plan feasible), per face two POIs whose feasible radius that face cuts (to 4 .. 13), and
    three POIs with no feasible cube"""
    nz, ny, nx = shape
    cx, cy, cz = nx // 2, ny // 2, nz // 2
    g = [[x, y, z] for z in (17, cz, nz - 18) for y in (17, cy, ny - 18) for x in (17, cx, nx - 18)]
    g += [[5, cy, cz], [12, cy, cz], [nx - 7, cy, cz], [nx - 15, cy, cz], [cx, 6, cz], [cx, 11, cz], [cx, ny - 8, cz], [cx, ny - 13, cz],
          [cx, cy, 9], [cx, cy, 14], [cx, cy, nz - 6], [cx, cy, nz - 12]]
    return np.array(g + [[0, 0, 0], [nx - 1, cy, cz], [cx, R_MIN, cz]], np.int32)


def clear_of(t, values, margin=MARGIN):
    """True when t is at least `margin` (relative) away from every finite value"""
    v = np.asarray([c for c in values if np.isfinite(c)], np.float64)
    return bool(np.all(np.abs(v - t) >= margin * np.maximum(np.abs(v), abs(t))))


def pick_threshold(values, target):
    """the threshold nearest above `target` that is clear of every value"""
    t = float(target)
    while not clear_of(t, values):
        t *= 1.0 + 1e-3
    return t


@functools.lru_cache(maxsize=None)
def all_criteria(name, criterion, r_min=R_MIN, r_max=R_MAX):
    """c(rho) of every POI and feasible radius of a parity volume: a list (per POI) of lists"""
    R = volumes()[name]
    return [ref.criteria(R, q, r_min, r_max, criterion)[1] for q in pois()]


@functools.lru_cache(maxsize=None)
def threshold(name, criterion):
    """the parity threshold of a volume: the median c(8) of the scene's POIs (of the volume's own POIs for the integer volumes), so
    the reported radii spread over the plan; moved clear of every c(rho) of the volume's POIs"""
    src = name if name in INTEGER else "scene"
    at = [c[8 - R_MIN] for c in all_criteria(src, criterion) if len(c) > 8 - R_MIN]
    flat = [v for c in all_criteria(name, criterion) for v in c]
    return pick_threshold(flat, float(np.median(at)))


@functools.lru_cache(maxsize=None)
def parity_reference(name, criterion):
    return ref.quality(volumes()[name], pois(), r_min=R_MIN, r_max=R_MAX, criterion=criterion, threshold=threshold(name, criterion))


# ---- the kernel's walk ---------------------------------------------------------------------------------------------------------------

THREADS = 256


def block_order(r):
    """offsets (dx, dy, dz) of the cube of radius r in the kernel's order: linear, dx fastest"""
    d = np.arange(-r, r + 1)
    dz, dy, dx = np.meshgrid(d, d, d, indexing="ij")
    return np.stack([dx.ravel(), dy.ravel(), dz.ravel()], 1)


def shell_order(k):
    """offsets (dx, dy, dz) of Chebyshev shell k in the kernel's order"""
    D = 2 * k + 1
    d = np.arange(-k, k + 1)
    fy, fx = np.meshgrid(d, d, indexing="ij")
    face = np.stack([fx.ravel(), fy.ravel()], 1)
    out = [np.concatenate([face, np.full((D * D, 1), -k)], 1), np.concatenate([face, np.full((D * D, 1), k)], 1)]
    ring = [[x, -k] for x in d] + [[x, k] for x in d]
    for y in range(-k + 1, k):
        ring += [[-k, y], [k, y]]
    ring = np.array(ring)
    assert len(ring) == 8 * k
    for z in range(-k + 1, k):
        out.append(np.concatenate([ring, np.full((8 * k, 1), z)], 1))
    out = np.concatenate(out)
    assert len(out) == 24 * k * k + 2
    return out


def seams(r_min, r_max):
    """offsets worth a spike for a walk r_min .. r_max: the first and the last voxel of the block and of every shell, and in each the
    last voxel of the workgroup's first round and the first of its second (indices 255 and 256), where it has that many"""
    out = {}

    def add(tag, order):
        idx = {"first": 0, "last": len(order) - 1}
        if len(order) > THREADS:
            idx.update(i255=THREADS - 1, i256=THREADS)
        for k, i in idx.items():
            out[f"{tag}-{k}"] = tuple(int(v) for v in order[i])

    add(f"block{r_min}", block_order(r_min))
    for k in range(r_min + 1, r_max + 1):
        add(f"shell{k}", shell_order(k))
    return out


# ---- the edge volume -------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def edge_volume():
    """integer-valued (12-bit) noise: every sum is exact, so every field but eig is compared bit for bit"""
    v = np.random.default_rng(11).integers(0, 4096, EDGE_SHAPE).astype(np.float32)
    v.setflags(write=False)
    return v


EDGE_CENTRE = (36, 35, 34)  # x, y, z: the cube of radius 32 plus its margin fits (z: 34 +- 33 = 1 .. 67)


def face_pois(rho, shape=EDGE_SHAPE):
    """for a forced radius rho: the central POI, then per face a POI whose cube + margin touches it exactly (feasible) and the POI one
    voxel further out (status 2): (points (13, 3), expected feasibility (13,))"""
    nz, ny, nx = shape
    pts, ok = [list(EDGE_CENTRE)], [True]
    for ax, n in enumerate((nx, ny, nz)):
        for v, good in ((rho + 1, True), (rho, False), (n - 2 - rho, True), (n - 1 - rho, False)):
            p = list(EDGE_CENTRE)
            p[ax] = v
            pts.append(p)
            ok.append(good)
    return np.array(pts, np.int32), np.array(ok)


@functools.lru_cache(maxsize=None)
def centre_criteria(criterion):
    """c(rho) for rho = 2 .. 32 at the centre of the edge volume"""
    rr, cc = ref.criteria(edge_volume(), EDGE_CENTRE, 2, 32, criterion)
    assert rr == list(range(2, 33))
    return cc


def selection_plan(criterion):
    """(rho, threshold) for rho = 2 .. 32: with that threshold a walk 2 .. 32 at the centre reports rho -- the geometric mean of
    c(rho - 1) and c(rho) (half of c(2) for rho = 2)"""
    c = centre_criteria(criterion)
    return [(2, float(c[0]) / 2)] + [(rho, float(np.sqrt(c[rho - 3] * c[rho - 2]))) for rho in range(3, 33)]


def cut_pois(shape=EDGE_SHAPE):
    """POIs whose feasible radius (r_max = 32) is cut by each of the six faces in turn: (points (6, 3), feasible (6,))"""
    nz, ny, nx = shape
    pts, f = [], []
    for ax, n, lo, rho in ((0, nx, True, 3), (0, nx, False, 9), (1, ny, True, 14), (1, ny, False, 20), (2, nz, True, 26), (2, nz, False, 31)):
        p = list(EDGE_CENTRE)
        p[ax] = rho + 1 if lo else n - 2 - rho
        pts.append(p)
        f.append(rho)
    return np.array(pts, np.int32), np.array(f, np.int32)


MATERIAL_RADIUS = 5


def material_cases():
    """(level, material count, fraction_min below, fraction_min above) at the centre of the edge volume and radius MATERIAL_RADIUS:
    the level at a voxel value of the cube, one float below it and one float above it; the fractions half a voxel either side of
    material / N"""
    R = edge_volume()
    x, y, z = EDGE_CENTRE
    r = MATERIAL_RADIUS
    cube = R[z - r:z + r + 1, y - r:y + r + 1, x - r:x + r + 1]
    v = np.float32(np.sort(cube.ravel())[cube.size // 2])  # a value the cube holds
    N = float(cube.size)
    out = []
    for level in (v, np.nextafter(v, np.float32(-np.inf)), np.nextafter(v, np.float32(np.inf))):
        m = int(np.count_nonzero(cube.astype(np.float64) >= np.float64(level)))
        out.append((float(level), m, (m - 0.5) / N, (m + 0.5) / N))
    return out


# ---- the chain ---------------------------------------------------------------------------------------------------------------------------

CHAIN_SHAPE = (44, 44, 72)    # nz, ny, nx: blobs only in x >= 36, the half x < 36 is exactly 0 ("air")
CHAIN_SCALE, CHAIN_SHIFT = 1.01, (0.3, -0.2, 0.1)


@functools.lru_cache(maxsize=None)
def chain_case():
    """R, T = R dilated by 1 % about the middle and shifted (narrow blobs rendered at the moved centres: exact), 30 POIs across both
    halves, and the true displacement at each"""
    nz, ny, nx = CHAIN_SHAPE
    rng = np.random.default_rng(21)
    b = nz * ny * (nx // 2) // 40
    c = np.stack([rng.uniform(nx // 2 + 8, nx + 6, b), rng.uniform(-6, ny + 6, b), rng.uniform(-6, nz + 6, b)], 1)
    sg, am = rng.uniform(1.2, 1.6, b), rng.uniform(0.3, 1.3, b)
    mid = (np.array([nx, ny, nz], np.float64) - 1) / 2
    c2 = (c - mid) * CHAIN_SCALE + mid + np.array(CHAIN_SHIFT)
    R, T = icgn_ref.render(CHAIN_SHAPE, c, sg, am), icgn_ref.render(CHAIN_SHAPE, c2, sg * CHAIN_SCALE, am)
    assert not R[:, :, :nx // 2].any()
    pts = np.array([[x, y, z] for z in (20, 23) for y in (19, 22, 24) for x in (18, 30, 42, 48, 54)], np.int32)
    u = (pts - mid) * CHAIN_SCALE + mid + np.array(CHAIN_SHIFT) - pts
    R.setflags(write=False)
    T.setflags(write=False)
    return R, T, pts, u


CHAIN_R_MIN, CHAIN_R_MAX = 4, 16


@functools.lru_cache(maxsize=None)
def chain_threshold():
    """the median c(7) of the POIs in the textured half, moved clear of every c(rho) of the chain's POIs"""
    R, _, pts, _ = chain_case()
    cc = [ref.criteria(R, q, CHAIN_R_MIN, CHAIN_R_MAX, 0)[1] for q in pts]
    at = [c[7 - CHAIN_R_MIN] for c, q in zip(cc, pts) if q[0] >= 42]
    return pick_threshold([v for c in cc for v in c], float(np.median(at)))


@functools.lru_cache(maxsize=None)
def chain_reference():
    R, _, pts, _ = chain_case()
    return ref.quality(R, pts, r_min=CHAIN_R_MIN, r_max=CHAIN_R_MAX, threshold=chain_threshold())
