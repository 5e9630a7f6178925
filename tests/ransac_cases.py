"""Inputs and assertions of the RANSAC edge tests (tests/test_gpu_ransac_edges.py), shared with tests/test_ransac_cpu.py.

Test infrastructure only.  Every check_* function takes an engine: an object with fit(pairs, **opts), fit_local(pairs, points, k=,
radius=, **opts) and device(array), returning what capi.fit_affine / capi.fit_affine_local return.  The GPU module passes the binding,
the CPU module passes RefEngine (the restatement of tests/ransac_ref.py in the kernel's place), which proves every assertion here
satisfiable without a GPU; the CPU module also checks that each input has the property it was built for.

What is compared, and how (the header's contract): neighbours, status, candidates, best_hypothesis, best_count exactly; hyp bit for
bit (a NaN's sign and payload are unspecified: NaN at the same positions, equal bits elsewhere); with refine = 0 also mask, inliers
and A bit for bit.  With refine > 0 the sums' order is free: A to rtol = atol = 1e-9, inliers, mask and status exactly -- a fair
demand only where no decision of the refit sits on a rounding error, which refit_margins() measures on the restatement:
  * no candidate with |d2 - tau2| <= 1e-6 tau2 in any round (tau = 0: none with 0 < d2 <= 1e-18 in any round after a refit; the
    first scoring uses hyp, which the GPU gives bit for bit, so its d2 are the restatement's bits and need no margin),
  * no |det Cov| within a relative 1e-6 of min_det."""
import hashlib
import itertools

import numpy as np

import ransac_ref as ref

F32 = np.float32
A_ERR = [0.0]  # the largest |A - ref| seen by check_records with refine > 0


def same_bits_or_nan(a, b):
    """NaN at the same positions, equal bits everywhere else"""
    a = np.ascontiguousarray(a, np.float64).ravel()
    b = np.ascontiguousarray(b, np.float64).ravel()
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint64)[~na], b.view(np.uint64)[~na]))


# ---- the restatement, shaped like the binding ------------------------------------------------------------------------------------

_CACHE = {}


def _digest(*arrays):
    h = hashlib.sha1()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def _opts(opts, local):
    o = dict(iterations=256 if local else 4096, inlier_thresh=3.0, seed=1, refine=1, min_det=1.0)
    o.update(opts)
    if not o["iterations"]:
        o["iterations"] = 256 if local else 4096
    return o


def want_global(pairs, **opts):
    """the restatement's global fit (computed once per input)"""
    pairs = np.ascontiguousarray(pairs, F32).reshape(-1, 6)
    o = _opts(opts, False)
    key = ("g", _digest(pairs), tuple(sorted(o.items())))
    if key not in _CACHE:
        _CACHE[key] = ref.fit(pairs, **o)
    return _CACHE[key]


def want_local(pairs, points, k, radius, which=None, **opts):
    """the restatement's local fits of the points listed (each computed once per input)"""
    pairs = np.ascontiguousarray(pairs, F32).reshape(-1, 6)
    points = np.ascontiguousarray(points, F32).reshape(-1, 3)
    o = _opts(opts, True)
    dp = _digest(pairs)
    res = []
    for p in (range(len(points)) if which is None else which):
        key = ("l", dp, int(p), points[p].tobytes(), int(k), float(radius), tuple(sorted(o.items())))
        if key not in _CACHE:
            _CACHE[key] = ref.fit_local(pairs, points, k=k, radius=radius, which=[int(p)], **o)[0]
        res.append(_CACHE[key])
    return res


class RefEngine:
    """tests/ransac_ref.py behind the binding's interface"""

    @staticmethod
    def device(a):
        return a

    @staticmethod
    def fit(pairs, **opts):
        w = want_global(pairs, **opts)
        n = len(np.asarray(pairs).reshape(-1, 6))
        return {"A": w["A"].reshape(3, 4).copy(), "hyp": w["hyp"].reshape(3, 4).copy(), "status": w["status"], "candidates": n,
                "best_hypothesis": w["best_hypothesis"], "best_count": w["best_count"], "inliers": w["inliers"], "rms": float(F32(w["rms"])),
                "mask": np.asarray(w["mask"], bool).copy(), "seconds": 0.0}

    @staticmethod
    def fit_local(pairs, points, k=32, radius=0.0, **opts):
        w = want_local(pairs, points, k, radius, **opts)
        m = len(w)
        return {"A": np.array([x["A"] for x in w]).reshape(m, 3, 4), "hyp": np.array([x["hyp"] for x in w]).reshape(m, 3, 4),
                "status": np.array([x["status"] for x in w], np.int32), "candidates": np.array([x["candidates"] for x in w], np.int32),
                "best_hypothesis": np.array([x["best_hypothesis"] for x in w], np.int32),
                "best_count": np.array([x["best_count"] for x in w], np.int32), "inliers": np.array([x["inliers"] for x in w], np.int32),
                "rms": np.array([x["rms"] for x in w], F32), "neighbours": np.array([x["neighbours"] for x in w], np.int32).reshape(m, k),
                "seconds": 0.0}


# ---- comparisons -----------------------------------------------------------------------------------------------------------------

def check_global(engine, pairs, **opts):
    """one global fit against the restatement; returns (got, want)"""
    pairs = np.ascontiguousarray(pairs, F32).reshape(-1, 6)
    got = engine.fit(pairs, **opts)
    w = want_global(pairs, **opts)
    what = (len(pairs), opts)
    assert got["status"] == w["status"], what
    assert got["candidates"] == len(pairs), what
    assert got["best_hypothesis"] == w["best_hypothesis"], what
    assert got["best_count"] == w["best_count"], what
    assert same_bits_or_nan(got["hyp"], w["hyp"]), what
    assert got["inliers"] == w["inliers"], what
    assert np.array_equal(got["mask"], w["mask"]), what
    if _opts(opts, False)["refine"] == 0:
        assert same_bits_or_nan(got["A"], w["A"]), what
    else:
        err = float(np.abs(got["A"].ravel() - w["A"]).max())
        A_ERR[0] = max(A_ERR[0], err)
        print(f"global n={len(pairs)} {opts}: |A - ref| = {err:.3e}")
        np.testing.assert_allclose(got["A"].ravel(), w["A"], rtol=1e-9, atol=1e-9)
    return got, w


def check_records(got, want, which, refine, what=""):
    """local records `which` of got against the restatement's dicts"""
    err = 0.0
    for p, w in zip(which, want):
        at = (what, int(p))
        assert np.array_equal(got["neighbours"][p], w["neighbours"]), at
        assert got["status"][p] == w["status"], at
        assert got["candidates"][p] == w["candidates"], at
        assert got["best_hypothesis"][p] == w["best_hypothesis"], at
        assert got["best_count"][p] == w["best_count"], at
        assert same_bits_or_nan(got["hyp"][p], w["hyp"]), at
        assert got["inliers"][p] == w["inliers"], at
        if refine == 0:
            assert same_bits_or_nan(got["A"][p], w["A"]), at
        else:
            err = max(err, float(np.abs(got["A"][p].ravel() - w["A"]).max()))
    if refine:
        A_ERR[0] = max(A_ERR[0], err)
        print(f"{what}: largest |A - ref| = {err:.3e} (bar 1e-9)")
        for p, w in zip(which, want):
            np.testing.assert_allclose(got["A"][p].ravel(), w["A"], rtol=1e-9, atol=1e-9, err_msg=str((what, int(p))))


def check_local(engine, pairs, points, k, radius, which=None, what="", **opts):
    """one local call against the restatement on the points listed (default: all); returns (got, want)"""
    pairs = np.ascontiguousarray(pairs, F32).reshape(-1, 6)
    points = np.ascontiguousarray(points, F32).reshape(-1, 3)
    which = list(range(len(points))) if which is None else list(which)
    got = engine.fit_local(pairs, points, k=k, radius=radius, **opts)
    assert got["neighbours"].shape == (len(points), k) and got["A"].shape == (len(points), 3, 4)
    want = want_local(pairs, points, k, radius, which, **opts)
    check_records(got, want, which, _opts(opts, True)["refine"], what or f"k={k} radius={radius} {opts}")
    return got, want


def refit_margins(pairs, p=0, **o):
    """the smallest margins of one fit's refit decisions in the restatement: (relative distance of any d2 from tau2 (tau = 0: the
    smallest non-zero d2 after a refit), relative distance of any |det Cov| from min_det, the trace)"""
    trace = []
    ref.fit(pairs, p=p, trace=trace, **o)
    tau2 = ref.tau2_of(o["inlier_thresh"])
    md = float(F32(o["min_det"]))
    m_d2 = m_det = np.inf
    for t in trace:
        d2 = t["d2"][np.isfinite(t["d2"])]
        if tau2 > 0:
            if len(d2):
                m_d2 = min(m_d2, float(np.abs(d2 - tau2).min() / tau2))
        elif t["round"] > 0 and (d2 > 0).any():
            m_d2 = min(m_d2, float(d2[d2 > 0].min()))
        if t["det"] is not None and md > 0:
            m_det = min(m_det, abs(abs(t["det"]) - md) / md)
    return m_d2, m_det, trace


def local_margins(pairs, points, k, radius, which=None, **opts):
    """refit_margins over the local problems of a call: (min d2 margin, min det margin, list of traces)"""
    pairs = np.ascontiguousarray(pairs, F32).reshape(-1, 6)
    points = np.ascontiguousarray(points, F32).reshape(-1, 3)
    o = _opts(opts, True)
    a = b = np.inf
    traces = []
    for p in (range(len(points)) if which is None else which):
        nb = ref.neighbours(pairs, points[p], k, radius)
        if len(nb) < 4:
            traces.append([])
            continue
        x, y, tr = refit_margins(pairs[nb], p=int(p), **o)
        a, b = min(a, x), min(b, y)
        traces.append(tr)
    return a, b, traces


def margins_ok(tau, m_d2, m_det):
    return (m_d2 > 1e-6 if tau > 0 else m_d2 > 1e-18) and m_det > 1e-6


def _affine_targets(r, rng, noise):
    th = 0.2
    R = np.array([[np.cos(th), -np.sin(th), 0], [np.sin(th), np.cos(th), 0], [0, 0, 1]])
    L = R @ np.diag([1.05, 0.97, 1.02])
    b = np.array([7.5, -3.25, 11.0])
    return np.asarray(r, np.float64) @ L.T + b + rng.normal(0, noise, np.shape(r))


def _pairs(r, rng, noise=0.2):
    return np.concatenate([np.asarray(r, np.float64), _affine_targets(r, rng, noise)], 1).astype(F32)


# ---- 1. every k ------------------------------------------------------------------------------------------------------------------

EVERY_K = list(range(4, 65))
EVERY_K_RADIUS = 20.0


def every_k_inputs():
    """700 pairs (not a multiple of 64): a third uniform over an extent of 64, two thirds on an integer lattice of step 8 (ties);
    24 query points, half on lattice sites, some outside the cloud"""
    rng = np.random.default_rng(1001)
    a = ref.synth_pairs(234, rng, noise=0.3, outliers=0.3, extent=64.0)[0]
    sites = rng.integers(0, 9, (466, 3)) * 8.0
    b = _pairs(sites, rng, 0.3)
    pairs = np.concatenate([a, b])[rng.permutation(700)]
    pts = np.concatenate([rng.integers(0, 9, (12, 3)) * 8.0, rng.uniform(-20, 84, (12, 3))])[rng.permutation(24)].astype(F32)
    return np.ascontiguousarray(pairs), pts


def check_every_k(engine, k):
    pairs, pts = every_k_inputs()
    out = []
    for radius in (0.0, EVERY_K_RADIUS):
        got, want = check_local(engine, pairs, pts, k, radius, iterations=64, seed=k, refine=0)
        out.append(got)
    assert (out[0]["candidates"] == k).all() and (out[0]["neighbours"] >= 0).all()
    return out


# ---- 2. hostile orders -----------------------------------------------------------------------------------------------------------

HOSTILE_Q = np.array([3.5, -2.25, 7.0], F32)
HOSTILE_N = [63, 64, 65, 127, 128, 129, 191, 192, 193, 1000]
HOSTILE_K = [4, 5, 63, 64]
HOSTILE_ORDERS = ["descending", "ascending", "blocks"]


def hostile_pairs(n, order):
    """n pairs at strictly increasing distances 2 + 0.05 i from HOSTILE_Q in random directions, listed nearest-last (every insertion
    goes to position 0), farthest-last (everything after the first k is skipped) or ascending in blocks of 64, each block reversed"""
    rng = np.random.default_rng(2000 + n)
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    r = HOSTILE_Q.astype(np.float64) + u * (2.0 + 0.05 * np.arange(n))[:, None]
    pairs = _pairs(r, rng)
    if order == "descending":
        return np.ascontiguousarray(pairs[::-1])
    if order == "blocks":
        idx = np.concatenate([np.arange(b, min(b + 64, n))[::-1] for b in range(0, n, 64)])
        return np.ascontiguousarray(pairs[idx])
    return pairs


def check_hostile(engine, n, order):
    pairs = hostile_pairs(n, order)
    for k in HOSTILE_K:
        got, want = check_local(engine, pairs, HOSTILE_Q[None], k, 0.0, iterations=64, refine=0, what=f"{order} n={n} k={k}")
        c = min(n, k)
        if order == "ascending":
            assert np.array_equal(got["neighbours"][0, :c], np.arange(c))
        if order == "descending":
            assert np.array_equal(got["neighbours"][0, :c], n - 1 - np.arange(c))
        assert got["candidates"][0] == c and got["status"][0] == 0


SPHERE_Q = np.array([10.0, -7.0, 5.0], F32)
SPHERE_N = [144, 200]


def sphere_pairs(n):
    """pairs at the same fp32 distance 21 from SPHERE_Q: the sign and permutation images of the Pythagorean quadruples
    (4, 5, 20, 21), (4, 8, 19, 21), (8, 11, 16, 21), 48 each, 144 distinct positions; n = 200 repeats the first 56"""
    v = []
    for t in ((4, 5, 20), (4, 8, 19), (8, 11, 16)):
        for perm in itertools.permutations(t):
            for sg in itertools.product((1, -1), repeat=3):
                v.append([a * b for a, b in zip(perm, sg)])
    v = np.array(v, np.float64)
    v = v[np.arange(n) % len(v)]
    rng = np.random.default_rng(2100 + n)
    return _pairs(SPHERE_Q.astype(np.float64) + v, rng)


def check_sphere(engine, n):
    pairs = sphere_pairs(n)
    for k in HOSTILE_K:
        got, want = check_local(engine, pairs, SPHERE_Q[None], k, 0.0, iterations=64, refine=0, what=f"sphere n={n} k={k}")
        assert np.array_equal(got["neighbours"][0], np.arange(k))  # equal distances: index order, and a full list rejects the rest
        got, want = check_local(engine, pairs, SPHERE_Q[None], k, 21.0, iterations=64, refine=0, what=f"sphere n={n} k={k} radius 21")
        assert np.array_equal(got["neighbours"][0], np.arange(k))
        got, want = check_local(engine, pairs, SPHERE_Q[None], k, 20.999, iterations=64, refine=0, what=f"sphere n={n} k={k} radius < 21")
        assert got["candidates"][0] == 0 and got["status"][0] == 1


RIM_Q = np.array([16.0, 32.0, -8.0], F32)
RIM_RADIUS = 8.0
RIM_OUTSIDE = 320


def rim_pairs(c):
    """c pairs within RIM_RADIUS of RIM_Q (one of them exactly on it) spread through RIM_OUTSIDE pairs whose fp32 d2 is one ulp above
    radius * radius: 8 along one axis and e along another, with e * e between half an ulp and one and a half"""
    rng = np.random.default_rng(2200 + c)
    r2 = ref.radius2(RIM_RADIUS)
    up = np.nextafter(r2, F32(np.inf))
    ulp = float(up) - float(r2)
    out = []
    while len(out) < RIM_OUTSIDE:
        e = rng.uniform(np.sqrt(0.6 * ulp), np.sqrt(1.4 * ulp)) * rng.choice([-1.0, 1.0])
        v = np.zeros(3)
        a, b = rng.choice(3, 2, replace=False)
        v[a], v[b] = RIM_RADIUS * rng.choice([-1.0, 1.0]), e
        r = (RIM_Q.astype(np.float64) + v).astype(F32)
        if ref.distances(np.concatenate([r, r])[None], RIM_Q)[0] == up:
            out.append(r.astype(np.float64))
    inside = RIM_Q.astype(np.float64) + rng.uniform(-4.5, 4.5, (c, 3))
    inside[0] = RIM_Q.astype(np.float64) + [0.0, -RIM_RADIUS, 0.0]
    r = np.concatenate([np.array(out), inside])
    slot = np.sort(rng.choice(len(r), c, replace=False))  # the inside pairs' places in the list
    order = np.empty(len(r), np.int64)
    order[slot] = RIM_OUTSIDE + np.arange(c)
    order[np.setdiff1d(np.arange(len(r)), slot)] = np.arange(RIM_OUTSIDE)
    return _pairs(r[order], rng), slot


def check_rim(engine, k):
    for c in (k - 1, k, k + 1):
        pairs, slot = rim_pairs(c)
        got, want = check_local(engine, pairs, RIM_Q[None], k, RIM_RADIUS, iterations=64, refine=0, what=f"rim k={k} c={c}")
        assert got["candidates"][0] == min(c, k)
        assert set(got["neighbours"][0, :min(c, k)].tolist()) <= set(slot.tolist())
        assert got["status"][0] == (1 if c < 4 else 0)


# ---- 3. statuses and mixed workgroups --------------------------------------------------------------------------------------------

STATUS_M = 4 * 24 + 1
STATUS_OPTS = dict(iterations=64, inlier_thresh=3.0, min_det=0.5, refine=1, seed=3)
STATUS_K, STATUS_RADIUS = 8, 5.0


def status_kinds():
    """the status each point is built for: the 24 orders of (1, 2, 3, 0), one per workgroup of four waves, and one more point"""
    return np.array([s for perm in itertools.permutations((1, 2, 3, 0)) for s in perm] + [0])


def coplanar_cluster(centre, rng):
    """10 pairs in the plane z = centre z, on a quarter-voxel lattice: every sample's det is exactly 0"""
    xy = rng.permutation(25 * 25)[:10]
    r = np.stack([(xy % 25 - 12) * 0.25, (xy // 25 - 12) * 0.25, np.zeros(10)], 1) + centre
    return _pairs(r, rng)


def tetrahedron(centre):
    """the unit tetrahedron moved by (1, 1, 1): |det| of the sample 1, det of the four inliers' covariance 0.25"""
    four = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float64) + centre
    return np.concatenate([four, four + 1], 1).astype(F32)


def status_inputs():
    """clusters 100 apart, one per point, of the kind status_kinds() lists: nothing or three pairs (1), a coplanar cluster (2), a
    unit tetrahedron with min_det = 0.5 (3), twelve healthy pairs (0)"""
    rng = np.random.default_rng(3001)
    kinds = status_kinds()
    pairs, pts = [], []
    for p, s in enumerate(kinds):
        centre = 100.0 * np.array([p % 5, (p // 5) % 5, p // 25], np.float64) + 10
        pts.append(centre + (0.25 if s != 3 else 0.0))
        if s == 1 and p % 8 < 4:
            pairs.append(_pairs(centre + rng.uniform(-2, 2, (3, 3)), rng))
        elif s == 2:
            pairs.append(coplanar_cluster(centre, rng))
        elif s == 3:
            pairs.append(tetrahedron(centre))
        elif s == 0:
            pairs.append(_pairs(centre + rng.uniform(-2.5, 2.5, (12, 3)), rng, noise=0.05))
    pairs = np.concatenate(pairs)
    return np.ascontiguousarray(pairs[rng.permutation(len(pairs))]), np.array(pts, F32), kinds


def check_statuses(engine):
    pairs, pts, kinds = status_inputs()
    got, want = check_local(engine, pairs, pts, STATUS_K, STATUS_RADIUS, what="statuses", **STATUS_OPTS)
    assert np.array_equal(got["status"], kinds)
    for p, s in enumerate(kinds):
        if s in (1, 2):
            assert not got["A"][p].any() and not got["hyp"][p].any() and got["best_hypothesis"][p] == -1 and got["inliers"][p] == 0, p
        if s == 3:
            assert same_bits_or_nan(got["A"][p], got["hyp"][p]) and got["best_hypothesis"][p] >= 0 and got["inliers"][p] == 4, p
        if s == 0:
            assert got["inliers"][p] >= 4 and got["candidates"][p] == STATUS_K, p
    rng = np.random.default_rng(3002)
    g, w = check_global(engine, coplanar_cluster(np.array([40.0, 50.0, 60.0]), rng), **STATUS_OPTS)
    assert g["status"] == 2 and g["best_hypothesis"] == -1 and not g["A"].any() and not g["hyp"].any() and not g["mask"].any()
    g, w = check_global(engine, tetrahedron(np.array([10.0, 10.0, 10.0])), **STATUS_OPTS)
    assert g["status"] == 3 and same_bits_or_nan(g["A"], g["hyp"]) and g["inliers"] == 4 and g["mask"].all()


# ---- 4. tails of the launches ----------------------------------------------------------------------------------------------------

GLOBAL_TAILS = [(255, 1), (256, 2), (257, 255), (511, 257), (513, 300), (255, 300), (257, 1), (513, 255), (256, 257), (511, 2), (513, 1),
                (255, 257)]
LOCAL_TAIL_H = [1, 63, 65, 100, 129]
LOCAL_TAIL_M = [2, 3, 5]


def check_global_tail(engine, n, H):
    rng = np.random.default_rng(4000 + 7 * n + H)
    pairs = ref.synth_pairs(n, rng, noise=0.3, outliers=0.4)[0]
    got, want = check_global(engine, pairs, iterations=H, seed=H, refine=0)
    assert got["status"] == 0 and 0 <= got["best_hypothesis"] < H


def local_tail_inputs():
    rng = np.random.default_rng(4100)
    pairs = ref.synth_pairs(600, rng, noise=0.3, outliers=0.3, extent=64.0)[0]
    return pairs, rng.uniform(0, 64, (40, 3)).astype(F32)


def check_local_tail_h(engine, H):
    pairs, pts = local_tail_inputs()
    got, want = check_local(engine, pairs, pts, 16, 0.0, iterations=H, seed=H, refine=0)
    assert (got["best_hypothesis"] < H).all()


def check_local_tail_m(engine, m):
    pairs, pts = local_tail_inputs()
    check_local(engine, pairs, pts[:m], 16, 0.0, iterations=64, seed=m, refine=0)


# ---- 5. refit rounds, locally ----------------------------------------------------------------------------------------------------

REFIT_K = [8, 32, 64]
REFIT_TAU = [0.0, 0.5, 3.0]
REFIT_ROUNDS = [0, 1, 2, 3, 4]
REFIT_MIN_DET = 1.0


def refit_inputs():
    """30 % outliers; a dense quarter of the volume (inliers few voxels apart: small covariances, where min_det bites) and a
    sparse rest; 20 points, half in each part"""
    rng = np.random.default_rng(5003)
    dense = ref.synth_pairs(1500, rng, noise=0.3, outliers=0.3, extent=8.0)[0]
    sparse = ref.synth_pairs(1500, rng, noise=0.3, outliers=0.3, extent=64.0)[0]
    pairs = np.concatenate([dense, sparse])[rng.permutation(3000)]
    pts = np.concatenate([rng.uniform(0, 8, (10, 3)), rng.uniform(8, 64, (10, 3))]).astype(F32)
    return np.ascontiguousarray(pairs), pts


# tau = 0: a hypothesis often fits its own four samples with d2 == 0 exactly, and a refit of those four would leave d2 ~ 1e-29 on
# them: inliers by rounding error, which the contract does not fix.  Four of the points and, per k, the first seed (searched once,
# upwards from 1) with which the bit-exact scoring counts fewer than 4 for each of them; test_ransac_cpu.py checks that it does.
REFIT_TAU0_POINTS = [3, 9, 12, 17]
REFIT_TAU0_SEED = {8: 36, 32: 84, 64: 312}


def refit_case(k, tau, refine):
    """(pairs, points, options) of one refit call"""
    pairs, pts = refit_inputs()
    o = dict(iterations=64, inlier_thresh=tau, refine=refine, min_det=REFIT_MIN_DET, seed=11)
    if tau == 0:
        pts = np.ascontiguousarray(pts[REFIT_TAU0_POINTS])
        o["seed"] = REFIT_TAU0_SEED[k]
    return pairs, pts, o


def check_refit(engine, k, tau):
    for refine in REFIT_ROUNDS:
        pairs, pts, o = refit_case(k, tau, refine)
        got, want = check_local(engine, pairs, pts, k, 0.0, what=f"refit k={k} tau={tau} refine={refine}", **o)
        if tau == 0:  # whatever the bit-exact scoring counts, it is fewer than 4: the refit stops there
            assert np.isin(got["status"], (0, 2)).all() and (got["inliers"] < 4).all() and (got["inliers"] == got["best_count"]).all()
            assert same_bits_or_nan(got["A"], got["hyp"])


# ---- 6. values -------------------------------------------------------------------------------------------------------------------

VALUE_K = 16
VALUE_CLASSES = ["nan_ref", "nan_tar", "inf_ref", "inf_tar", "huge_ref", "huge_ref_radius", "nan_query", "huge_query", "offset_2p20",
                 "tiny_extent", "duplicates", "all_nan"]
HUGE = 3e19


def value_inputs(name):
    """(pairs, points, local radius, options) of a value class, from a 600-pair base and 30 points"""
    rng = np.random.default_rng(6000)
    pairs = ref.synth_pairs(600, rng, noise=0.3, outliers=0.3, extent=64.0)[0]
    pts = rng.uniform(0, 64, (30, 3)).astype(F32)
    rng = np.random.default_rng(6001 + VALUE_CLASSES.index(name))
    radius, opts = 0.0, dict(iterations=64, refine=0, seed=5)
    some = rng.choice(600, 30, replace=False)  # 5 %
    col = rng.integers(0, 3, 30)
    if name == "nan_ref":
        pairs[some, col] = np.nan
    elif name == "nan_tar":
        pairs[some, 3 + col] = np.nan
    elif name == "inf_ref":
        pairs[some, col] = np.where(rng.random(30) < 0.5, np.inf, -np.inf)
    elif name == "inf_tar":
        pairs[some, 3 + col] = np.where(rng.random(30) < 0.5, np.inf, -np.inf)
    elif name in ("huge_ref", "huge_ref_radius"):
        pairs = pairs[:18].copy()  # fewer finite pairs than k: the pairs at +inf distance follow them, in index order
        far = np.array([1, 4, 5, 9, 12, 13, 16, 17])
        pairs[far, rng.integers(0, 3, 8)] = np.where(rng.random(8) < 0.5, HUGE, -HUGE)
        radius = 1000.0 if name == "huge_ref_radius" else 0.0
    elif name == "nan_query":
        pts[np.arange(0, 30, 3), rng.integers(0, 3, 10)] = np.nan
    elif name == "huge_query":
        pts[np.arange(0, 30, 3), rng.integers(0, 3, 10)] = HUGE
    elif name == "offset_2p20":
        pairs = (pairs.astype(np.float64) + 2.0 ** 20).astype(F32)
        pts = (pts.astype(np.float64) + 2.0 ** 20).astype(F32)
    elif name == "tiny_extent":
        sc = 1e-2 / 64.0
        pairs, pts = (pairs * F32(sc)).astype(F32), (pts * F32(sc)).astype(F32)
        opts.update(min_det=0.0, inlier_thresh=3.0 * sc)
    elif name == "duplicates":
        src = rng.choice(600, 3, replace=False)
        dup = np.setdiff1d(rng.permutation(600)[:123], src)[:120]  # 20 %: 40 copies of each of three pairs
        pairs[dup] = pairs[src][np.arange(120) % 3]
        pts[:3] = pairs[src, :3]  # these points see copies of one pair only
        opts.update(min_det=0.0)
    elif name == "all_nan":
        pairs[:] = np.nan
    return np.ascontiguousarray(pairs), pts, radius, opts


def check_values(engine, name):
    pairs, pts, radius, opts = value_inputs(name)
    g, gw = check_global(engine, pairs, **opts)
    got, want = check_local(engine, pairs, pts, VALUE_K, radius, what=name, **opts)
    nb = got["neighbours"]
    if name in ("nan_ref", "inf_ref", "nan_tar", "inf_tar"):
        assert g["status"] == 0
    if name == "nan_ref":
        bad = np.nonzero(np.isnan(pairs[:, :3]).any(1))[0]
        assert not np.isin(nb, bad).any() and (got["candidates"] == VALUE_K).all()
    if name == "huge_ref":
        assert (nb[:, :10] < 18).all() and np.array_equal(nb[:, 10:], np.tile([1, 4, 5, 9, 12, 13], (30, 1)))
    if name == "huge_ref_radius":
        assert (got["candidates"] == 10).all() and (nb[:, 10:] == -1).all()
    if name == "nan_query":
        assert (got["status"][::3] == 1).all() and (got["candidates"][::3] == 0).all() and (nb[::3] == -1).all()
        assert (got["status"][1::3] == 0).all()
    if name == "huge_query":
        assert np.array_equal(nb[::3], np.tile(np.arange(VALUE_K), (10, 1)))
    if name == "duplicates":
        assert not np.isfinite(got["hyp"][:3]).all(axis=(1, 2)).any() and (got["status"][:3] == 0).all()
    if name == "all_nan":
        assert g["status"] == 2 and (got["status"] == 1).all() and (got["candidates"] == 0).all()


# ---- 7. independence and repeatability -------------------------------------------------------------------------------------------

INDEP_K, INDEP_M = 24, 203
INDEP_FIELDS = ("A", "hyp", "status", "candidates", "best_hypothesis", "best_count", "inliers", "rms", "neighbours")


def indep_inputs():
    """5000 pairs (five dense clusters among them), 203 points, and the same points with all but the indices = 1 (mod 4) replaced by
    NaN points, far points and points inside the dense clusters"""
    rng = np.random.default_rng(7001)
    pairs = ref.synth_pairs(4000, rng, noise=0.3, outliers=0.3, extent=128.0)[0]
    centres = rng.uniform(20, 108, (5, 3))
    dense = _pairs(np.repeat(centres, 200, 0) + rng.normal(0, 0.5, (1000, 3)), rng)
    pairs = np.ascontiguousarray(np.concatenate([pairs, dense])[rng.permutation(5000)])
    pts = rng.uniform(0, 128, (INDEP_M, 3)).astype(F32)
    other = pts.copy()
    for p in range(INDEP_M):
        if p % 4 == 1:
            continue
        kind = (p // 4 + p) % 3
        if kind == 0:
            other[p, rng.integers(0, 3)] = np.nan
        elif kind == 1:
            other[p] = [HUGE, -1e6, 5e5][p % 3]
        else:
            other[p] = centres[p % 5] + rng.normal(0, 0.3, 3)
    return pairs, pts, other


def check_independence(engine):
    pairs, pts, other = indep_inputs()
    kept = np.arange(1, INDEP_M, 4)
    o = dict(iterations=64, seed=9)
    a = engine.fit_local(pairs, pts, k=INDEP_K, **o)
    b = engine.fit_local(pairs, other, k=INDEP_K, **o)
    dp = engine.device(pairs)
    da = engine.fit_local(dp, engine.device(pts), k=INDEP_K, **o)
    db = engine.fit_local(dp, engine.device(other), k=INDEP_K, **o)
    for f in INDEP_FIELDS:
        assert a[f][kept].tobytes() == b[f][kept].tobytes(), f
        assert a[f].tobytes() == da[f].tobytes(), f
        assert b[f].tobytes() == db[f].tobytes(), f
    which = kept[::2]
    check_records(a, want_local(pairs, pts, INDEP_K, 0.0, which, **o), which, 1, "independence")
    which = np.arange(0, INDEP_M, 5)
    check_records(b, want_local(pairs, other, INDEP_K, 0.0, which, **o), which, 1, "independence, replaced points")
