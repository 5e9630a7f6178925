"""GPU tests of sift3d_icgn where a subtle error would pass tests/test_gpu_icgn.py: every legal subset radius with a spike on one
sentinel voxel of the walk (a missed or doubled voxel moves the result by >= 100 tolerances, asserted on the restatement), volumes
with pairwise different dimensions and an asymmetric deformation gradient, R's and T's exact domain edges (the positions just inside
T's upper edge included), every status with its order, non-finite voxels, exact invariances under power-of-two scalings and a
negation, large offsets against a bound measured on the restatement, convergent runs, and 70 000 POIs in one call.  Unless a test
says otherwise "agrees" is test_agrees_with_restatement's bound against tests/icgn_ref.py: statuses and iteration counts equal,
|d displacement| <= 1e-4, |d gradient| <= 1e-5, |d zncc| <= 1e-5."""
import importlib

import numpy as np
import pytest

import icgn_ref as ref

pytestmark = pytest.mark.gpu

capi = importlib.import_module("3dsift_amd.capi")
GRAD = [k for k in range(12) if k % 4]
DISP = [0, 4, 8]
TOL_D, TOL_G, TOL_Z = 1e-4, 1e-5, 1e-5
EPS = 2.0 ** -40
FIELDS = ("p", "zncc", "last_step", "iterations", "status")


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.uint64), np.asarray(b, np.float64).view(np.uint64))


def gaps(got, want, rows=None):
    rows = slice(None) if rows is None else rows
    dp = np.abs(got["p"][rows] - want["p"][rows])
    return float(dp[:, DISP].max()), float(dp[:, GRAD].max()), float(np.abs(got["zncc"][rows] - want["zncc"][rows]).max())


def assert_agree(got, want, what="", last_step=False):
    print(what, "status", list(want["status"]), "iterations", list(want["iterations"]))
    assert np.array_equal(got["status"], want["status"]), (what, got["status"], want["status"])
    assert np.array_equal(got["iterations"], want["iterations"]), (what, got["iterations"], want["iterations"])
    dd, dg, dz = gaps(got, want)
    print(what, "gaps d/g/zncc", dd, dg, dz)
    assert dd <= TOL_D and dg <= TOL_G and dz <= TOL_Z, (what, dd, dg, dz)
    if last_step:
        ls = np.abs(got["last_step"] - want["last_step"]).max()
        assert ls <= TOL_D, (what, ls)


def assert_init_returned(got, init, status, rows):
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
    """a blob volume of any shape (ref.scene's texture without a second volume)"""
    nz, ny, nx = shape
    b = max(8, nz * ny * nx // per)
    rng = np.random.Generator(np.random.PCG64(seed))
    c = np.stack([rng.uniform(0, nx, b), rng.uniform(0, ny, b), rng.uniform(0, nz, b)], 1)
    return ref.render(shape, c, rng.uniform(1.5, 4.5, b), rng.uniform(0.3, 1.3, b))


def row(u=0.0, v=0.0, w=0.0, **g):
    names = ("u", "ux", "uy", "uz", "v", "vx", "vy", "vz", "w", "wx", "wy", "wz")
    p = np.zeros(12)
    p[[0, 4, 8]] = u, v, w
    for k, x in g.items():
        p[names.index(k)] = x
    return p


# ---- 1. every radius, a spike on one sentinel voxel of the walk --------------------------------------------------------------------

PAD = 4          # voxels between the subset and the window's faces: R's margin (1), T's taps (2) and the shift plus its error (1)
SHIFT = (1, -1, 1)  # T(x + SHIFT) = R(x): the true displacement


@pytest.fixture(scope="module")
def spike_volume():
    n = 2 * 32 + 1 + 2 * PAD + 2
    return blobs((n, n, n), seed=21)


sentinels = ref.sentinels  # one definition for both orders: the walk is shared


def spike_amplitude(r):
    """several blob amplitudes (<= 1.3) at the small radii, growing with the subset: one voxel's share of the sums falls as 1 / N"""
    return max(1.5, 5.0 * (r / 4.0) ** 1.5)


SPIKE = [(r, 1) for r in range(2, 33)] + [(r, 0) for r in (3, 7, 8, 12, 24, 32)]


SENS_BIG = ("first", "last", "i255")  # r > 16: the sentinels whose sensitivity is asserted
BIG_CUBIC = ("first", "last", "i256", "zcarry")  # r >= 24, tricubic: the restatement costs 64 gathers for each of 10^5 voxels


@pytest.mark.parametrize("r,interp", SPIKE, ids=[f"r{r}-{'cubic' if i == 0 else 'linear'}" for r, i in SPIKE])
def test_every_radius_with_sentinel_spikes(spike_volume, r, interp):
    """one call per sentinel.  The spike is two voxels along x (the sentinel and its +x neighbour), so that the sentinel carries the
    spike's value and half of it as gradient; the sensitivity run zeroes the sentinel voxel alone, in R only.  To keep the
    restatement's time down the sensitivity is asserted for every sentinel up to r = 16 and for three of them beyond (the amplitude
    follows one rule for all), and the tricubic cases of r >= 24 take four sentinels and leave the sensitivity to the trilinear
    case of their radius (same volumes, same inits)"""
    D = 2 * r + 1
    n = D + 2 * PAD
    c = spike_volume.shape[0] // 2
    o = c - n // 2  # the window's origin in the volume (a centred window for every radius)
    q = np.array([[r + PAD] * 3], np.int32)
    opts = dict(subset_radius=r, max_iterations=2, tolerance=0.0, interpolation=interp)
    rng = np.random.default_rng(50 * r)
    amp = spike_amplitude(r)
    sent = sentinels(r)
    assert len(sent) >= 6
    big = interp == 0 and r >= 24
    e = min(0.2, 0.05 * r)  # 125 voxels under a spike do not hold 12 parameters against more
    inits = {name: np.concatenate([np.array(SHIFT) + rng.uniform(-e, e, 3), rng.uniform(-0.002, 0.002, 9)])[[0, 3, 4, 5, 1, 6, 7, 8, 2, 9, 10, 11]][None]
             for name in sent}
    if big:
        sent = {name: sent[name] for name in BIG_CUBIC}

    def cpu(item):
        name, i = item
        d = np.array([i % D - r, (i // D) % D - r, i // (D * D) - r])
        V = spike_volume.copy()
        s = o + q[0] + d
        V[s[2], s[1], s[0]:s[0] + 2] += amp
        R = V[o:o + n, o:o + n, o:o + n].copy()
        T = V[o - SHIFT[2]:o - SHIFT[2] + n, o - SHIFT[1]:o - SHIFT[1] + n, o - SHIFT[0]:o - SHIFT[0] + n].copy()
        at = (q[0, 2] + d[2], q[0, 1] + d[1], q[0, 0] + d[0])
        assert R[at] >= amp and T.max() >= amp
        want = ref.icgn(R, T, q, init=inits[name], **opts)
        sens = None
        if not big and (r <= 16 or name in SENS_BIG):  # sensitivity (CPU): the same run with the sentinel voxel's spike zeroed in R only
            R0 = R.copy()
            R0[at] -= np.float32(amp)
            moved = np.abs(ref.refine(R0, T, q[0], init=inits[name][0], **opts)["p"] - want["p"][0])
            sens = max(moved[DISP].max() / TOL_D, moved[GRAD].max() / TOL_G)
        return name, i, d, R, T, want, sens

    for name, i, d, R, T, want, sens in map(cpu, sent.items()):
        assert want["status"][0] == 1 and want["iterations"][0] == 2, (name, want["status"])
        if sens is not None:
            print(f"r={r} {name} index {i} d={tuple(int(x) for x in d)} amplitude {amp:.1f}: zeroing it in R moves p by {sens:.0f} tolerances")
            assert sens >= 100, (name, i, sens)
        got = capi.icgn(R, T, q, init=inits[name], **opts)
        assert_agree(got, want, f"r={r} {name}")


# ---- 2. axes, strides, different sizes ---------------------------------------------------------------------------------------------

R_SHAPE, T_SHAPE = (40, 52, 46), (44, 38, 60)  # (nz, ny, nx), pairwise different


ODD_Q0 = np.array([23, 26, 20])
ODD_P = dict(u=7.3, v=-7.4, w=2.15, ux=0.01, uy=0.08, uz=-0.02, vx=0.0, vy=-0.03, vz=0.04, wx=0.03, wy=0.0, wz=-0.05)  # asymmetric


@pytest.fixture(scope="module")
def odd_volumes():
    """the same blobs in both volumes, their centres mapped by x -> q0 + F (x - q0) + (u, v, w) (widths kept: a texture, not a truth)"""
    rng = np.random.Generator(np.random.PCG64(31))
    b = 400
    c = np.stack([rng.uniform(-8, 54, b), rng.uniform(-8, 60, b), rng.uniform(-8, 48, b)], 1)
    sg, am = rng.uniform(1.5, 4.0, b), rng.uniform(0.3, 1.3, b)
    p = row(**ODD_P)
    c2 = ODD_Q0 + (c - ODD_Q0) @ ref.F_of(p).T + p[DISP]
    return ref.render(R_SHAPE, c, sg, am), ref.render(T_SHAPE, c2, sg, am)


@pytest.mark.parametrize("r", [4, 9])
@pytest.mark.parametrize("interp", [0, 1], ids=["cubic", "linear"])
def test_axes_strides_and_sizes(odd_volumes, r, interp):
    R, T = odd_volumes
    rng = np.random.default_rng(7 * r + interp)
    q = ODD_Q0 + rng.integers(-3, 4, (8, 3))
    init = np.tile(row(**ODD_P), (8, 1))
    init[:, DISP] += (q - ODD_Q0) @ (ref.F_of(init[0]) - np.eye(3)).T + rng.uniform(-0.3, 0.3, (8, 3))
    # T.ny < T.nz: POI 6's subset passes T's last admissible y by half a voxel (status 3; T.nz as the y limit would accept it),
    # POI 7's ends half a voxel inside T's last admissible z cell, beyond T.ny (T.ny as the z limit would refuse it)
    F = ref.F_of(init[0])
    top = np.abs(F).sum(1) * r  # the largest corner offset per axis
    hi = np.array([T_SHAPE[2], T_SHAPE[1], T_SHAPE[0]]) - 1 - (2 if interp == 0 else 1)  # the largest admissible floor per axis
    init[6, 4] = hi[1] + 1.5 - q[6, 1] - top[1]
    init[7, 8] = hi[2] + 0.5 - q[7, 2] - top[2]
    assert hi[2] - 1 > T_SHAPE[1] - 1 and hi[1] + 1 < hi[2]
    opts = dict(subset_radius=r, max_iterations=3, tolerance=0.0, interpolation=interp)
    want = ref.icgn(R, T, q, init=init, **opts)
    assert want["status"][6] == 3 and want["iterations"][6] == 0
    assert ref.in_domain(T.shape, init[7], q[7], r, interp == 0)
    assert (want["status"][:6] == 1).all() and want["last_step"][7] > 0, (want["status"], want["last_step"])  # 7 started inside T
    got = capi.icgn(R, T, q.astype(np.int32), init=init, **opts)
    assert_agree(got, want, f"odd r={r}", last_step=True)


# ---- 3. exact edges ----------------------------------------------------------------------------------------------------------------

def test_R_edges():
    """q = r + 1 and q = n - 2 - r read R's outermost voxels and run; q = r and q = n - 1 - r are status 2, on every axis and side"""
    r, pad = 4, 4
    nz, ny, nx = R_SHAPE
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
    q = np.array(runs + outside, np.int32)
    rng = np.random.default_rng(5)
    init = np.zeros((12, 12))
    init[:, DISP] = pad + rng.uniform(-0.2, 0.2, (12, 3))
    opts = dict(subset_radius=r, max_iterations=2, tolerance=0.0)
    got = capi.icgn(R, T, q, init=init, **opts)
    want = ref.icgn(R, T, q, init=init, **opts)
    assert (want["status"][:6] == 1).all() and (want["status"][6:] == 2).all(), want["status"]
    assert_agree(got, want, "R edges")
    assert_init_returned(got, init, 2, range(6, 12))


EDGE_R, EDGE_Q = 5, np.array([23, 26, 20])
EDGE_FRAC = 0.3  # the true displacement lies this far inside the edge position


def edge_case(axis, side, interp, frac=EDGE_FRAC):
    """R, T and the integer displacement k_in along `axis` whose extreme tap is T's last (side 1) or first (side 0) voxel; the true
    displacement is k_in -+ frac (towards T's inside), zero along the other axes"""
    t = np.zeros(3)
    t[axis] = -frac if side else frac
    R, T, _ = ref.scene(R_SHAPE, tvec=t, seed=34)
    taps_hi, taps_lo = (2, 1) if interp == 0 else (1, 0)
    cut = [slice(None)] * 3
    if side:
        n = EDGE_Q[axis] + EDGE_R + 1 + taps_hi  # floor(q + r + 0) + taps_hi = n - 1
        cut[2 - axis] = slice(0, n)
        k_in = 0
    else:
        x0 = EDGE_Q[axis] - EDGE_R - taps_lo  # floor(q - r - x0) - taps_lo = 0
        cut[2 - axis] = slice(x0, None)
        k_in = -x0
    return R, np.ascontiguousarray(T[tuple(cut)]), k_in


EDGES = [(a, s, i) for a in range(3) for s in (0, 1) for i in (0, 1)]


@pytest.mark.parametrize("axis,side,interp", EDGES, ids=[f"{'xyz'[a]}-{'upper' if s else 'lower'}-{'cubic' if i == 0 else 'linear'}" for a, s, i in EDGES])
def test_T_edges(axis, side, interp):
    """rows: 0 the extreme tap on T's first / last voxel (in the domain), 1 one voxel further (status 3), 2 just inside (upper:
    2^-40 below the first outside integer, whose fp32 fraction rounds to 1; lower: 2^-40 above k_in), 3 just outside"""
    R, T, k_in = edge_case(axis, side, interp)
    out = k_in + 1 if side else k_in - 1
    u = [k_in, out, out - EPS if side else k_in + EPS, out if side else k_in - EPS]
    init = np.zeros((4, 12))
    init[:, 4 * axis] = u
    q = np.tile(EDGE_Q, (4, 1)).astype(np.int32)
    opts = dict(subset_radius=EDGE_R, max_iterations=2, tolerance=0.0, interpolation=interp)
    want = ref.icgn(R, T, q, init=init, **opts)
    assert list(want["status"]) == [1, 3, 1, 3] and list(want["iterations"]) == [2, 0, 2, 0], (want["status"], want["iterations"])
    got = capi.icgn(R, T, q, init=init, **opts)
    assert_init_returned(got, init, 3, (1, 3))
    for i in (0, 2):
        print("row", i, "gaps", gaps(got, want, [i]))
    assert_agree(got, want, "T edge", last_step=True)


@pytest.mark.parametrize("interp", [0, 1], ids=["cubic", "linear"])
def test_T_upper_edge_rotated(interp):
    """a small rotation in F: only the subset's corner voxels reach T's last admissible position, 2^-30 below the first outside one"""
    R, T, _ = edge_case(0, 1, interp)
    rots = (ref.rot(1.5, -2.0, 2.5), ref.rot(-2.0, 1.0, -1.5))
    init = np.zeros((len(rots), 12))
    q = np.tile(EDGE_Q, (len(rots), 1)).astype(np.int32)
    corners = np.array([[s0, s1, s2] for s0 in (-EDGE_R, EDGE_R) for s1 in (-EDGE_R, EDGE_R) for s2 in (-EDGE_R, EDGE_R)], np.float64)
    for i, F in enumerate(rots):
        init[i, GRAD] = (F - np.eye(3)).ravel()
        init[i, 4], init[i, 8] = 0.1, -0.15
        top = (corners @ F.T)[:, 0].max()
        init[i, 0] = (T.shape[2] - (2 if interp == 0 else 1)) - 2.0 ** -30 - (q[i, 0] + top)  # the end of the last admissible cell
        c = ref.warp(init[i], q[i].astype(np.float64), corners)[:, 0]
        assert ref.in_domain(T.shape, init[i], q[i], EDGE_R, interp == 0)
        assert c.max() - np.floor(c.max()) > 1 - 1e-6 and np.sort(c)[-2] < c.max() - 0.1  # one corner alone, at the cell's very end
    opts = dict(subset_radius=EDGE_R, max_iterations=2, tolerance=0.0, interpolation=interp)
    want = ref.icgn(R, T, q, init=init, **opts)
    got = capi.icgn(R, T, q, init=init, **opts)
    assert_agree(got, want, "rotated edge", last_step=True)


@pytest.mark.parametrize("interp", [0, 1], ids=["cubic", "linear"])
def test_status_3_after_a_step(interp):
    """the true displacement lies outside T's domain: an update leaves T, and the last in-domain p comes back"""
    R, T, k_in = edge_case(0, 0, interp)  # lower x edge: the truth is k_in + EDGE_FRAC; shifting q by +2 puts it 1.7 voxels outside
    starts = (0.1, 0.7, 1.4, 2.2)
    q = np.tile(EDGE_Q - np.array([2, 0, 0]), (len(starts), 1)).astype(np.int32)
    init = np.zeros((len(starts), 12))
    init[:, 0] = k_in + 2 + np.array(starts)
    opts = dict(subset_radius=EDGE_R, max_iterations=20, tolerance=1e-3, interpolation=interp)
    want = ref.icgn(R, T, q, init=init, **opts)
    # IC-GN's first step from within a voxel of the truth is nearly the whole error: every start leaves T with its first update
    assert (want["status"] == 3).all() and (want["last_step"] > 0).all(), (want["status"], want["iterations"])
    got = capi.icgn(R, T, q, init=init, **opts)
    assert_agree(got, want, "status 3 after a step", last_step=True)
    for i in range(len(starts)):
        assert ref.in_domain(T.shape, got["p"][i], q[i], EDGE_R, interp == 0)
        assert got["last_step"][i] > 0
        if got["iterations"][i] == 0:
            assert same_bits(got["p"][i], init[i])


# ---- 4. statuses and their order ---------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def status_scene():
    return ref.scene((40, 40, 40), tvec=(0.3, -0.2, 0.1), seed=41)


ST_R, ST_Q = 5, np.array([[20, 20, 20]], np.int32)
ST_OPTS = dict(subset_radius=ST_R, max_iterations=3, tolerance=0.0)
ST_INIT = row(0.2, -0.1, 0.15, ux=0.003, vz=-0.002)[None]


def check_status_4(R, T, what, init=ST_INIT, **more):
    opts = dict(ST_OPTS, **more)
    got = capi.icgn(R, T, ST_Q, init=init, **opts)
    want = ref.icgn(R, T, ST_Q, init=init, **opts)
    assert want["status"][0] == 4, (what, want["status"])
    assert np.array_equal(got["status"], want["status"]), (what, got["status"])
    assert_init_returned(got, init, 4, [0])


def test_status_4_ramp(status_scene):
    """R = x (integers: every pivot is exact), so dR > 0 and H[4][4] = sum Ry^2 = 0"""
    _, T, _ = status_scene
    R = np.broadcast_to(np.arange(40, dtype=np.float32), (40, 40, 40)).copy()
    check_status_4(R, T, "ramp")


@pytest.mark.parametrize("interp", [0, 1], ids=["cubic", "linear"])
def test_status_4_constant_T(status_scene, interp):
    """T constant over every tap: dT = 0.  With T = (float)Rm the flatness test has nothing but rounding to compare: 64 fp32 products
    of the constant do not sum to it, so the kernel weights the taps' differences from a voxel of T, which are exactly 0 here
    (weighting the taps themselves ran on to status 3 with a step of 5.4 voxels)"""
    R, _, _ = status_scene
    w = ref.offsets(ST_R).astype(int) + ST_Q[0]
    rm = np.float32(R[w[:, 2], w[:, 1], w[:, 0]].astype(np.float64).mean())
    for c in (np.float32(0.75), rm):
        check_status_4(R, np.full((40, 40, 40), c, np.float32), f"T = {c}", interpolation=interp)


def test_status_4_nonfinite_R(status_scene):
    R, T, _ = status_scene
    x, y, z = ST_Q[0]
    for what, at, v in (("NaN in the subset", (z + 2, y - 1, x + ST_R), np.nan), ("NaN in the margin only", (z, y, x + ST_R + 1), np.nan),
                        ("NaN in the z margin only", (z - ST_R - 1, y + 1, x), np.nan), ("+Inf in the subset", (z, y + 3, x - 2), np.inf)):
        Rb = R.copy()
        Rb[at] = v
        check_status_4(Rb, T, what)


@pytest.mark.parametrize("interp", [0, 1], ids=["cubic", "linear"])
def test_nonfinite_T(status_scene, interp):
    R, T, _ = status_scene
    x, y, z = ST_Q[0]
    for v in (np.nan, np.inf, -np.inf):
        for at in ((z, y, x), (z + ST_R, y - ST_R, x + ST_R)):  # under a tap of the centre voxel, of a corner voxel
            Tb = T.copy()
            Tb[at] = v
            check_status_4(R, Tb, f"{v} at {at}", interpolation=interp)
    # a NaN that no tap of any iteration touches: the clean volume's bits
    Tb = T.copy()
    Tb[1, 2, 3] = np.nan
    Tb[z + ST_R + 6, y, x] = np.nan
    opts = dict(ST_OPTS, interpolation=interp)
    clean = capi.icgn(R, T, ST_Q, init=ST_INIT, **opts)
    assert clean["status"][0] == 1 and clean["iterations"][0] == 3
    equal_results(capi.icgn(R, Tb, ST_Q, init=ST_INIT, **opts), clean)


def test_status_order_in_one_call(status_scene):
    R, T, _ = status_scene
    R = R.copy()
    R[:, :, :14] = 0.5  # a constant slab at the low x end, wide enough for a subset and its margin (2 r + 3 = 9 voxels)
    r = 3
    healthy = np.array([[24, 20, 20], [26, 24, 18], [22, 17, 25]], np.int32)
    hinit = np.tile(ST_INIT, (3, 1))
    bad = np.array([[1, 20, 20], [r, 20, 20], [6, 20, 20]], np.int32)
    binit = np.zeros((3, 12))
    binit[0, 6] = np.inf   # a non-finite init outside R: 5 before 2
    binit[1, 0] = 0.25     # outside R, over constant R: 2 before 4
    binit[2, 8] = 100.0    # constant R, outside T: 4 before 3
    order = [0, 3, 1, 4, 2, 5]  # bad and healthy POIs alternate
    q, init = np.concatenate([bad, healthy])[order], np.concatenate([binit, hinit])[order]
    opts = dict(subset_radius=r, max_iterations=3, tolerance=0.0)
    got = capi.icgn(R, T, q, init=init, **opts)
    want = ref.icgn(R, T, q, init=init, **opts)
    assert list(want["status"]) == [5, 1, 2, 1, 4, 1], want["status"]
    assert np.array_equal(got["status"], want["status"]), got["status"]
    for i, s in ((0, 5), (2, 2), (4, 4)):
        assert got["status"][i] == s and same_bits(got["p"][i], init[i]) and got["iterations"][i] == 0 and got["zncc"][i] == 0
    alone = capi.icgn(R, T, healthy, init=hinit, **opts)
    equal_results(got, alone, [1, 3, 5], None)
    ok = [1, 3, 5]
    sub = {k: want[k][ok] for k in FIELDS}
    assert_agree(alone, sub, "healthy neighbours")


# ---- 5. voxel values ---------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def value_scene():
    R, T, truth = ref.scene((48, 48, 48), ref.rot(1.5, -1.0, 2.0), (0.3, -0.25, 0.2), seed=51)
    rng = np.random.default_rng(52)
    q = rng.integers(16, 32, (60, 3)).astype(np.int32)
    tr = truth(q)
    init = tr + np.where(np.arange(12) % 4 == 0, rng.uniform(-0.3, 0.3, tr.shape), rng.uniform(-0.004, 0.004, tr.shape))
    return R, T, q, init, truth


SCALINGS = {"both_2^-10": (2.0 ** -10, 2.0 ** -10), "both_2^13": (2.0 ** 13, 2.0 ** 13), "T_2^7": (1.0, 2.0 ** 7), "negated": (-1.0, -1.0)}


@pytest.mark.parametrize("name", list(SCALINGS))
@pytest.mark.parametrize("interp", [0, 1], ids=["cubic", "linear"])
def test_exact_invariances(value_scene, name, interp):
    """every threshold of the contract is relative: a power-of-two scaling or a negation returns the original call's bits.
    T_2^7 holds because the kernel shifts T by a voxel of T (with a shift by Rm, T' = T(W) - Rm is no exact multiple when T alone
    is scaled: the restatement's float32 form differs by about 1e-9 there)"""
    R, T, q, init, _ = value_scene
    a, b = SCALINGS[name]
    opts = dict(subset_radius=6, interpolation=interp)
    base = capi.icgn(R, T, q[:16], init=init[:16], **opts)
    assert (base["status"] == 0).mean() >= 0.8
    got = capi.icgn(np.float32(a) * R, np.float32(b) * T, q[:16], init=init[:16], **opts)
    dp = np.abs(got["p"] - base["p"])
    print(name, "max |dp|", dp.max(), "rows that differ", int((dp.max(1) > 0).sum()), "status", list(got["status"]), list(base["status"]))
    for k in ("p", "zncc", "iterations", "status"):
        if base[k].dtype == np.float64:
            assert same_bits(got[k], base[k]), (name, k)
        else:
            assert np.array_equal(got[k], base[k]), (name, k)


OFFSETS = [("both", b, r) for b in (-1024.0, 1000.0, 32768.0) for r in (5, 16)] + [(m, b, 5) for m in "TR" for b in (-1024.0, 1000.0, 32768.0)]


@pytest.mark.parametrize("which,b,r", OFFSETS, ids=[f"{m}-b{int(b)}-r{r}" for m, b, r in OFFSETS])
def test_offsets(value_scene, which, b, r):
    """R + b and T + b, together and one at a time (unit-amplitude texture, one iteration).  The bound comes from the reference: e is the gap between the
    restatement with float32 per-voxel interpolation and the fp64 restatement; the GPU stays within the base tolerance + 4 e of the
    fp64 restatement (fma and the tap order may each add about e)"""
    R, T, q, _, truth = value_scene
    Rb = (R + np.float32(b)).astype(np.float32) if which in ("both", "R") else R
    Tb = (T + np.float32(b)).astype(np.float32) if which in ("both", "T") else T
    q = q[(q >= r + 3).all(1) & (q <= 44 - r).all(1)][:5]
    init = truth(q) + np.random.default_rng(int(abs(b)) + r).uniform(-0.2, 0.2, (len(q), 12)) * np.where(np.arange(12) % 4 == 0, 1.0, 0.01)
    assert len(q) == 5
    opts = dict(subset_radius=r, max_iterations=1, tolerance=0.0)
    w64 = ref.icgn(Rb, Tb, q, init=init, **opts)
    w32 = ref.icgn(Rb, Tb, q, init=init, f32=True, **opts)
    # b = 32768 on one volume alone: dT^2 <= 1e-10 sum (T - Rm)^2 holds for some POIs, which the contract calls flat (status 4)
    assert np.array_equal(w32["status"], w64["status"]) and ((w64["status"] == 1).all() or (which != "both" and b == 32768.0))
    ed, eg, ez = gaps(w32, w64)
    got = capi.icgn(Rb, Tb, q, init=init, **opts)
    gd, gg, gz = gaps(got, w64)
    print(f"offset {which} b={b} r={r}: e (f32 restatement - fp64) d/g/zncc {ed:.3e} {eg:.3e} {ez:.3e}; GPU - fp64 {gd:.3e} {gg:.3e} {gz:.3e}")
    assert np.array_equal(got["status"], w64["status"]) and np.array_equal(got["iterations"], w64["iterations"])
    assert gd <= TOL_D + 4 * ed and gg <= TOL_G + 4 * eg and gz <= TOL_Z + 4 * ez, (gd, ed, gg, eg, gz, ez)


def test_convergent_runs(value_scene):
    """default tolerance: the iteration counts are the restatement's wherever no step of the restatement lies within 1 % of it"""
    R, T, q, init, _ = value_scene
    tol = float(np.float32(1e-3))
    opts = dict(subset_radius=6)
    want = ref.icgn(R, T, q, init=init, tolerance=tol, **opts)
    near = np.array([any(abs(s - tol) <= 0.01 * tol for s in st) for st in want["steps"]])
    print("excluded", int(near.sum()), "of", len(q), "iterations", np.bincount(want["iterations"]), "status", np.bincount(want["status"]))
    assert near.mean() <= 0.10
    assert (want["status"] == 0).mean() >= 0.8
    got = capi.icgn(R, T, q, init=init, **opts)
    keep = ~near
    assert np.array_equal(got["status"][keep], want["status"][keep]), (got["status"], want["status"])
    assert np.array_equal(got["iterations"][keep], want["iterations"][keep]), (got["iterations"], want["iterations"])
    dd = np.abs(got["p"][keep][:, DISP] - want["p"][keep][:, DISP]).max()
    print("convergent runs: max |d displacement|", dd)
    assert dd <= 1e-3, dd


# ---- 6. many POIs, scratch growth and reuse ----------------------------------------------------------------------------------------

def test_many_pois_and_scratch_reuse(value_scene):
    R, T, q, init, _ = value_scene
    opts = dict(subset_radius=2, interpolation=1, max_iterations=2, tolerance=0.0)
    small = capi.icgn(R, T, q[:7], init=init[:7], **opts)
    m, k = 70000, 50
    rep = -(-m // k)
    big = capi.icgn(R, T, np.tile(q[:k], (rep, 1))[:m], init=np.tile(init[:k], (rep, 1))[:m], **opts)
    after = capi.icgn(R, T, q[:7], init=init[:7], **opts)
    equal_results(small, after)
    for f in FIELDS:
        first = big[f][:k]
        tiled = np.concatenate([first] * rep)[:m]
        if big[f].dtype == np.float64:
            assert same_bits(big[f], tiled), f
        else:
            assert np.array_equal(big[f], tiled), f
    equal_results(big, small, slice(0, 7), None)
    want = ref.icgn(R, T, q[:k], init=init[:k], **opts)
    assert_agree({f: big[f][:k] for f in FIELDS}, want, "50 distinct POIs")
