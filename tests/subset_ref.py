"""NumPy fp64 restatement of the subset-screening contract of include/sift3d_hip.h (sift3d_subset_quality,
sift3d_subset_group_by_radius): test infrastructure only.  Two forms of the sums: `direct` sums the cube of one radius in linear order,
`profile` sums the cube of r_min as one block and then the Chebyshev shells outward, adding each to the running totals (the order of
the contract's Determinism paragraph).  Every sum is a plain sequential fp64 sum (np.bincount adds its weights in index order).  On
integer-valued volumes every order gives the same bits; elsewhere the forms, and the GPU, agree within the bar of `bar_rel`."""
import math

import numpy as np

FIELDS = ("mean", "dR", "G", "eig", "radius", "status", "feasible", "material")
PAIRS = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))  # G: xx yy zz xy xz yz
_ERR = dict(invalid="ignore", over="ignore", divide="ignore")


def feasible(shape, q, r_max):
    """the largest rho <= r_max whose cube plus a 1-voxel margin lies in R (may be negative: no cube does)"""
    nz, ny, nx = shape
    room = int(r_max)
    for c, n in zip(q, (nx, ny, nz)):
        room = min(room, int(c) - 1, n - 2 - int(c))
    return room


def terms(R, q, rho):
    """the per-voxel terms of the cube of radius rho at q, in linear order (dz, dy, dx), dx fastest: a dict of flat arrays -- a (fp64),
    the three gradients (fp32 central differences widened to fp64), the voxels (fp32) and the Chebyshev shell index"""
    Rf = np.asarray(R, np.float32)
    x, y, z = int(q[0]), int(q[1]), int(q[2])
    s = lambda c, o=0: slice(c - rho + o, c + rho + 1 + o)  # noqa: E731
    half = np.float32(0.5)
    with np.errstate(**_ERR):
        g = [(half * (Rf[s(z), s(y), s(x, 1)] - Rf[s(z), s(y), s(x, -1)])).astype(np.float64).ravel(),
             (half * (Rf[s(z), s(y, 1), s(x)] - Rf[s(z), s(y, -1), s(x)])).astype(np.float64).ravel(),
             (half * (Rf[s(z, 1), s(y), s(x)] - Rf[s(z, -1), s(y), s(x)])).astype(np.float64).ravel()]
        v = Rf[s(z), s(y), s(x)].ravel()
        a = v.astype(np.float64) - np.float64(Rf[z, y, x])
    d = np.abs(np.arange(-rho, rho + 1))
    k = np.maximum(np.maximum(d[:, None, None], d[None, :, None]), d[None, None, :]).ravel()
    return {"a": a, "g": g, "v": v, "k": k}


def summands(t):
    """the eight summands per voxel: a, a^2 and the six gradient products, (8, n)"""
    with np.errstate(**_ERR):
        return np.stack([t["a"], t["a"] * t["a"]] + [t["g"][i] * t["g"][j] for i, j in PAIRS])


def plain_sum(x, label=None, n=1):
    """sequential fp64 sums of x by label (None: one sum), in index order"""
    if label is None:
        label = np.zeros(len(x), np.int64)
    with np.errstate(**_ERR):
        return np.bincount(label, weights=x, minlength=n)


def jacobi_eig(G):
    """eigenvalues of G (xx yy zz xy xz yz), descending: cyclic Jacobi, 8 sweeps over the planes (0,1) (0,2) (1,2), the operations of
    the kernel one by one; three NaN where an entry is not finite"""
    G = np.asarray(G, np.float64)
    if not np.all(np.isfinite(G)):
        return np.full(3, np.nan)
    a = {(0, 0): G[0], (1, 1): G[1], (2, 2): G[2], (0, 1): G[3], (0, 2): G[4], (1, 2): G[5]}
    one = np.float64(1.0)

    def rotate(p, q, r):
        pq, rp, rq = tuple(sorted((p, q))), tuple(sorted((r, p))), tuple(sorted((r, q)))
        apq = a[pq]
        if apq == 0.0:
            return
        theta = (a[(q, q)] - a[(p, p)]) / (np.float64(2.0) * apq)
        t = (one if theta >= 0.0 else -one) / (abs(theta) + np.sqrt(theta * theta + one))
        c = one / np.sqrt(t * t + one)
        s = t * c
        a[(p, p)] = a[(p, p)] - t * apq
        a[(q, q)] = a[(q, q)] + t * apq
        a[pq] = np.float64(0.0)
        a[rp], a[rq] = c * a[rp] - s * a[rq], s * a[rp] + c * a[rq]

    with np.errstate(**_ERR):
        for _ in range(8):
            rotate(0, 1, 2)
            rotate(0, 2, 1)
            rotate(1, 2, 0)
        hi = max(a[(0, 0)], max(a[(1, 1)], a[(2, 2)]))
        lo = min(a[(0, 0)], min(a[(1, 1)], a[(2, 2)]))
        mid = ((a[(0, 0)] + a[(1, 1)]) + a[(2, 2)]) - hi - lo
    return np.array([hi, mid, lo], np.float64)


def criterion_value(G, eig, criterion):
    """c(rho): NaN where an entry of G is not finite"""
    if not np.all(np.isfinite(G)):
        return np.float64(np.nan)
    return np.float64(min(G[0], G[1], G[2])) if criterion == 0 else np.float64(eig[2])


def record(sums, material, rho, rc):
    """mean, dR, G, eig of a cube from its eight sums (S, Q, G), its material count, its radius and the shift Rc"""
    N = np.float64((2 * rho + 1) ** 3)
    S, Q = np.float64(sums[0]), np.float64(sums[1])
    with np.errstate(**_ERR):
        var = Q - S * S / N
        if var < 0.0:
            var = np.float64(0.0)
        out = {"mean": np.float64(rc) + S / N, "dR": np.sqrt(var)}
    out["G"] = np.array(sums[2:8], np.float64)
    out["eig"] = jacobi_eig(out["G"])
    out["radius"], out["material"] = int(rho), int(material)
    return out


def direct(R, q, rho, level=-np.inf):
    """the record of the cube of radius rho at q (which must be feasible), summed in linear order"""
    t = terms(R, q, rho)
    sums = np.array([plain_sum(row)[0] for row in summands(t)])
    return record(sums, int(np.count_nonzero(t["v"].astype(np.float64) >= level)), rho, np.asarray(R, np.float32)[q[2], q[1], q[0]])


def profile(R, q, r_min, r_top, level=-np.inf):
    """the records of the cubes of radius r_min .. r_top at q (r_top feasible) by shell prefix sums: the cube of r_min as one block,
    then shell after shell added to the running totals"""
    t = terms(R, q, r_top)
    label = np.maximum(t["k"], r_min) - r_min
    n = r_top - r_min + 1
    per = np.stack([plain_sum(row, label, n) for row in summands(t)])            # (8, n): the block, then each shell
    mat = np.bincount(label, weights=(t["v"].astype(np.float64) >= level).astype(np.float64), minlength=n)
    with np.errstate(**_ERR):
        tot = np.add.accumulate(per, axis=1)                                         # running totals, in shell order
    mat = np.cumsum(mat)
    rc = np.asarray(R, np.float32)[q[2], q[1], q[0]]
    return [record(tot[:, i], int(mat[i]), r_min + i, rc) for i in range(n)]


DEFAULTS = dict(r_min=8, r_max=16, criterion=0, threshold=0.0, level=-np.inf, fraction_min=0.0)


def screen(R, q, **opts):
    """one POI: the record sift3d_subset_quality reports, and the list of c(rho) of every radius walked before the decision"""
    o = dict(DEFAULTS, **opts)
    rf = feasible(np.shape(R), q, o["r_max"])
    if rf < o["r_min"]:
        return dict(mean=0.0, dR=0.0, G=np.zeros(6), eig=np.zeros(3), radius=0, status=2, feasible=0, material=0), []
    cs = []
    for rec in profile(R, q, o["r_min"], rf, o["level"]):
        c = criterion_value(rec["G"], rec["eig"], o["criterion"])
        cs.append(c)
        if np.isfinite(c) and c >= o["threshold"]:
            N = float((2 * rec["radius"] + 1) ** 3)
            rec["status"] = 3 if float(rec["material"]) < o["fraction_min"] * N else 0
            break
    else:
        rec["status"] = 1
    rec["feasible"] = rf
    return rec, cs


def quality(R, points, **opts):
    """every POI of points ((m, 3) x, y, z): arrays like capi.subset_quality's"""
    pts = np.asarray(points, np.int64).reshape(-1, 3)
    rows = [screen(R, q, **opts)[0] for q in pts]
    out = {k: np.array([w[k] for w in rows]) for k in FIELDS}
    out["G"] = out["G"].reshape(-1, 6)
    out["eig"] = out["eig"].reshape(-1, 3)
    for k in ("radius", "status", "feasible", "material"):
        out[k] = out[k].astype(np.int32)
    return out


def criteria(R, q, r_min, r_max, criterion):
    """c(rho) of every feasible radius of r_min .. r_max at q: (radii, values)"""
    rf = feasible(np.shape(R), q, r_max)
    recs = profile(R, q, r_min, rf) if rf >= r_min else []
    return [w["radius"] for w in recs], [criterion_value(w["G"], w["eig"], criterion) for w in recs]


def group_by_radius(radius, status, r_min, r_max):
    """sift3d_subset_group_by_radius: [(radius, indices)] of the non-empty groups"""
    radius, status = np.asarray(radius), np.asarray(status)
    out = []
    for r in range(r_min, r_max + 1):
        idx = np.flatnonzero((status == 0) & (radius == r)).astype(np.int32)
        if len(idx):
            out.append((r, idx))
    return out


# ---- the bars ----------------------------------------------------------------------------------------------------------------------

def abs_sums(R, q, rho):
    """sum |term| of the eight sums of the cube of radius rho at q"""
    with np.errstate(**_ERR):
        return np.abs(summands(terms(R, q, rho))).sum(axis=1)


def summation_error(R, q, rho, orders=16, seed=0):
    """the largest |plain fp64 sum - exact sum| / sum |term| over the eight sums of a cube: the linear order and `orders` seeded
    permutations of it.  The exact sum is math.fsum's (correctly rounded, whatever the order)."""
    rows = summands(terms(R, q, rho))
    rng = np.random.default_rng(seed)
    perms = [np.arange(rows.shape[1])] + [rng.permutation(rows.shape[1]) for _ in range(orders)]
    e = 0.0
    for row in rows:
        scale = float(np.abs(row).sum())
        if scale == 0.0:
            continue
        exact = math.fsum(row.tolist())
        for p in perms:
            e = max(e, abs(float(plain_sum(row[p])[0]) - exact) / scale)
    return e


def jacobi_error(Gs):
    """the largest |jacobi_eig - numpy.linalg.eigvalsh| / trace over the matrices Gs ((n, 6), finite, positive trace)"""
    e = 0.0
    for G in np.asarray(Gs, np.float64).reshape(-1, 6):
        M = np.array([[G[0], G[3], G[4]], [G[3], G[1], G[5]], [G[4], G[5], G[2]]])
        tr = G[0] + G[1] + G[2]
        if not np.isfinite(tr) or tr <= 0:
            continue
        e = max(e, float(np.abs(jacobi_eig(G) - np.linalg.eigvalsh(M)[::-1]).max() / tr))
    return e


def bar_rel(e):
    """the GPU's bar relative to sum |term|: the kernel's order is another sample of the same rounding, hence the factor 4"""
    return max(4.0 * e, 1e-13)


def field_bars(R, q, rho, rel, jac_rel):
    """absolute bars of one record (the cube of radius rho at q) for a relative bar `rel` on the sums and `jac_rel` on the Jacobi
    solve (relative to the trace).  The last operations of mean and dR are the same in both forms and their inputs differ by at most
    the sums' bars, so each adds the propagated bar and a few ulp of the value.  dR is compared on its square, v = Q - S^2 / N:
    |dv| <= bar(Q) + 2 |S| bar(S) / N.  An eigenvalue moves by at most the 2-norm of the change of G (Weyl), bounded here by the sum
    of the bars of its nine entries."""
    A = abs_sums(R, q, rho)
    N = float((2 * rho + 1) ** 3)
    t = terms(R, q, rho)
    S = abs(float(plain_sum(t["a"])[0]))
    gb = rel * A[2:8]
    rec = direct(R, q, rho)
    tr = float(rec["G"][0] + rec["G"][1] + rec["G"][2])
    return {"mean": rel * A[0] / N + 4 * np.spacing(abs(rec["mean"])),
            "dR2": rel * (A[1] + 2 * S * A[0] / N) + 8 * np.spacing(rec["dR"] ** 2),
            "G": gb + 2 * np.spacing(np.abs(rec["G"])),
            "eig": float(gb[:3].sum() + 2 * gb[3:].sum()) + 4 * jac_rel * tr + 4 * np.spacing(tr)}
