"""NumPy fp64 restatement of the second-order IC-GN contract of include/sift3d_hip.h (sift3d_icgn2, sift3d_icgn2_init_from_icgn):
test infrastructure only.  Everything the contract shares with sift3d_icgn comes from icgn_ref (interp, offsets, positive_definite)
and, for the B-spline interpolation, from bspline_ref; what is restated here is the 30-parameter shape function, its 10 x 10 warp
matrix and composition, the stopping norm and the conservative domain rule.  Also the quadratic scene: blobs evaluated at arbitrary
points, deformed by a globally quadratic map whose expansion about a point gives the true 30 parameters there."""
import numpy as np

import bspline_ref
import icgn_ref

# exponents (of dx, dy, dz) of the ten terms (c, cx, cy, cz, cxx, cyy, czz, cxy, cxz, cyz) and the factor of each in the shape function
EXP = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [2, 0, 0], [0, 2, 0], [0, 0, 2], [1, 1, 0], [1, 0, 1], [0, 1, 1]])
HALF = np.array([1, 1, 1, 1, 0.5, 0.5, 0.5, 1, 1, 1])
DISP = [0, 10, 20]
FIRST = [k for k in range(30) if k % 10 in (1, 2, 3)]
SECOND = [k for k in range(30) if k % 10 >= 4]
PAIRS = [(0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2)]  # rows 4..9 of M: the products of the position polynomials


def xi(d):
    """(N, 10): 1, dx, dy, dz, dx^2, dy^2, dz^2, dx dy, dx dz, dy dz"""
    d = np.asarray(d, np.float64).reshape(-1, 3)
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    return np.stack([np.ones(len(d)), x, y, z, x * x, y * y, z * z, x * y, x * z, y * z], 1)


def xip(d):
    """xi', the steepest-descent monomials: the squares carry their 1/2"""
    return xi(d) * HALF


def from_first_order(p12):
    """(..., 12) first-order parameters -> (..., 30) with zero second derivatives"""
    p12 = np.asarray(p12, np.float64)
    out = np.zeros(p12.shape[:-1] + (30,))
    for a in range(3):
        out[..., 10 * a:10 * a + 4] = p12[..., 4 * a:4 * a + 4]
    return out


def first_order_of(p30):
    p30 = np.asarray(p30, np.float64)
    return np.concatenate([p30[..., 10 * a:10 * a + 4] for a in range(3)], -1)


def warp(p, q, d):
    """positions (N, 3) of the subset offsets d under p at the POI q"""
    return (np.asarray(q, np.float64) + d) + xip(d) @ np.asarray(p, np.float64).reshape(3, 10).T


def coefficient_rows(p):
    """(3, 10): the position polynomials W(d) - q in the basis xi"""
    c = np.asarray(p, np.float64).reshape(3, 10) * HALF
    for a in range(3):
        c[a, 1 + a] += 1.0
    return c


def truncated_product(A, B):
    """the product of two polynomials in the basis xi, terms of degree 3 and 4 dropped"""
    o = np.zeros(10)
    o[0] = A[0] * B[0]
    for k in (1, 2, 3):
        o[k] = A[0] * B[k] + A[k] * B[0]
        o[3 + k] = (A[0] * B[3 + k] + A[3 + k] * B[0]) + A[k] * B[k]
    for n, (i, j) in zip((7, 8, 9), ((1, 2), (1, 3), (2, 3))):
        o[n] = (A[0] * B[n] + A[n] * B[0]) + (A[i] * B[j] + A[j] * B[i])
    return o


def M_of(p):
    c = coefficient_rows(p)
    M = np.zeros((10, 10))
    M[0, 0] = 1.0
    M[1:4] = c
    for n, (a, b) in enumerate(PAIRS):
        M[4 + n] = truncated_product(c[a], c[b])
    return M


def p_of(M):
    c = np.array(M[1:4], np.float64)
    for a in range(3):
        c[a, 1 + a] -= 1.0
    return (c / HALF).reshape(30)


def lu(A):
    """P A = L U with partial pivoting (the first entry of largest magnitude; a NaN is never larger): (LU, perm), or None when a pivot
    is 0 or not finite"""
    A = np.array(A, np.float64)
    n = len(A)
    perm = np.arange(n)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for k in range(n):
            best, bi = -1.0, k
            for i in range(k, n):
                v = abs(A[i, k])
                if v > best:
                    best, bi = v, i
            if bi != k:
                A[[k, bi]] = A[[bi, k]]
                perm[[k, bi]] = perm[[bi, k]]
            pv = A[k, k]
            if not pv != 0 or not np.isfinite(pv):
                return None
            A[k + 1:, k] = A[k + 1:, k] / pv
            A[k + 1:, k + 1:] = A[k + 1:, k + 1:] - np.outer(A[k + 1:, k], A[k, k + 1:])
    return A, perm


def solve_rows(f, B):
    """X with X A = B from the factors of A"""
    LU, perm = f
    n = len(LU)
    B = np.atleast_2d(np.asarray(B, np.float64))
    X = np.zeros_like(B)
    for r, b in enumerate(B):
        z = np.zeros(n)
        for j in range(n):
            z[j] = (b[j] - z[:j] @ LU[:j, j]) / LU[j, j]
        y = np.zeros(n)
        for j in range(n - 1, -1, -1):
            y[j] = z[j] - y[j + 1:] @ LU[j + 1:, j]
        X[r, perm] = y
    return X


def compose(p, dp, f=False):
    """the parameters of M(p) M(dp)^-1, or None when M(dp) is singular; f: the factors of M(dp) (lu's return) where the caller has them"""
    if f is False:
        f = lu(M_of(dp))
    if f is None:
        return None
    M = np.zeros((10, 10))
    M[1:4] = solve_rows(f, M_of(p)[1:4])
    return p_of(M)


def step_norm(dp, r):
    e = np.asarray(dp, np.float64).reshape(3, 10)
    with np.errstate(invalid="ignore", over="ignore"):
        s = np.sum(e[:, 0] ** 2) + r ** 2 * np.sum(e[:, 1:4] ** 2) + r ** 4 * (0.25 * np.sum(e[:, 4:7] ** 2) + np.sum(e[:, 7:] ** 2))
        return float(np.sqrt(s))


def in_domain(shape, p, q, r, cubic):
    """the conservative closed-form rule: the 8 corners of the affine part, widened by B_a per axis"""
    nz, ny, nx = shape
    e = np.asarray(p, np.float64).reshape(3, 10)
    c = np.array([[sx, sy, sz] for sz in (-r, r) for sy in (-r, r) for sx in (-r, r)], np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        pos = icgn_ref.warp(first_order_of(p), np.asarray(q, np.float64), c)
        B = r * r * (0.5 * np.abs(e[:, 4:7]).sum(1) + np.abs(e[:, 7:]).sum(1))
        lo_f, hi_f = np.floor(pos.min(0) - B), np.floor(pos.max(0) + B)
    if not (np.all(np.isfinite(lo_f)) and np.all(np.isfinite(hi_f))):
        return False
    lo, hi = (1, 2) if cubic else (0, 1)
    return bool(np.all(lo_f - lo >= 0) and np.all(hi_f + hi <= np.array([nx, ny, nz]) - 1))


def refine(R, T, q, init=None, subset_radius=16, max_iterations=20, tolerance=1e-3, interpolation=0, f32=False, coefficients_given=False):
    """one POI: dict(p, zncc, last_step, iterations, status) as sift3d_icgn2_result, steps (the norm of every computed step) and perms
    (the row permutation of the LU of M(dp) for every step that reached it; None: singular).  interpolation 2: T is prefiltered
    (bspline_ref) unless coefficients_given"""
    if interpolation == 2:
        C = bspline_ref.coefficients(T, coefficients_given)
        with bspline_ref._bspline_weights():
            return _refine(R, C, q, init, subset_radius, max_iterations, tolerance, True, f32)
    return _refine(R, T, q, init, subset_radius, max_iterations, tolerance, interpolation == 0, f32)


def _refine(R, T, q, init, r, max_iterations, tolerance, cubic, f32):
    q = np.asarray(q, np.int64)
    p = np.zeros(30) if init is None else np.array(init, np.float64)
    steps, perms = [], []

    def res(p, zncc, last, it, status):
        return dict(p=np.array(p, np.float64), zncc=float(zncc), last_step=float(last), iterations=int(it), status=int(status),
                    steps=tuple(steps), perms=tuple(perms))

    if not np.all(np.isfinite(p)):
        return res(p, 0, 0, 0, 5)
    nz, ny, nx = R.shape
    if np.any(q - r - 1 < 0) or np.any(q + r + 1 > np.array([nx, ny, nz]) - 1):
        return res(p, 0, 0, 0, 2)
    d = icgn_ref.offsets(r)
    di = d.astype(np.int64)
    x, y, z = q[0] + di[:, 0], q[1] + di[:, 1], q[2] + di[:, 2]
    Rf = np.asarray(R, np.float32)
    half = np.float32(0.5)
    g = [(half * (Rf[z, y, x + 1] - Rf[z, y, x - 1])).astype(np.float64), (half * (Rf[z, y + 1, x] - Rf[z, y - 1, x])).astype(np.float64),
         (half * (Rf[z + 1, y, x] - Rf[z - 1, y, x])).astype(np.float64)]
    Rs = Rf[z, y, x].astype(np.float64)
    Rm = Rs.mean()
    Rp = Rs - Rm
    dR = np.sqrt(np.sum(Rp * Rp))
    v = xip(d)
    SD = np.concatenate([gc[:, None] * v for gc in g], 1)
    if not dR > 0:
        return res(p, 0, 0, 0, 4)
    with np.errstate(invalid="ignore", over="ignore"):
        H = SD.T @ SD
    if not icgn_ref.positive_definite(H):
        return res(p, 0, 0, 0, 4)
    if not in_domain(T.shape, p, q, r, cubic):
        return res(p, 0, 0, 0, 3)
    N = float(len(d))
    it, last, done, status = 0, 0.0, False, None
    while True:
        Tp = icgn_ref.interp(T, warp(p, q, d), cubic, f32) - Rm
        sT = Tp.sum()
        sTT = np.sum(Tp * Tp)
        tm = sT / N
        dt2 = sTT - sT * tm
        flat = not dt2 > 1e-10 * sTT
        dT = 0.0 if flat else np.sqrt(dt2)
        zncc = 0.0 if flat else np.sum(Rp * (Tp - tm)) / (dR * dT)
        if done:
            return res(p, zncc, last, it, status)
        if flat:
            return res(p, 0.0, last, it, 4)
        b = SD.T @ (Rp - (dR / dT) * (Tp - tm))
        dp = -np.linalg.solve(H, b)
        last = step_norm(dp, r)
        steps.append(last)
        if not np.all(np.isfinite(dp)):
            return res(p, zncc, last, it, 6)
        f = lu(M_of(dp))
        perms.append(None if f is None else tuple(int(i) for i in f[1]))
        pn = compose(p, dp, f)
        if pn is None:
            return res(p, zncc, last, it, 6)
        if not in_domain(T.shape, pn, q, r, cubic):
            return res(p, zncc, last, it, 3)
        p = pn
        it += 1
        if last < tolerance:
            status, done = 0, True
        elif it >= max_iterations:
            status, done = 1, True


def icgn2(R, T, points, init=None, interpolation=0, coefficients_given=False, **opts):
    """every POI of points ((m, 3) x, y, z): arrays like capi.icgn2's"""
    pts = np.asarray(points, np.int64).reshape(-1, 3)
    cubic = interpolation != 1
    f32 = opts.pop("f32", False)
    r, mi, tol = opts.pop("subset_radius", 16), opts.pop("max_iterations", 20), opts.pop("tolerance", 1e-3)
    if opts:
        raise TypeError(f"unknown options {sorted(opts)}")

    def rows(V):
        return [_refine(R, V, q, None if init is None else init[i], r, mi, tol, cubic, f32) for i, q in enumerate(pts)]

    if interpolation == 2:
        C = bspline_ref.coefficients(T, coefficients_given)
        with bspline_ref._bspline_weights():
            out = rows(C)
    else:
        out = rows(T)
    p = np.array([w["p"] for w in out]).reshape(-1, 30)
    e = p.reshape(-1, 3, 10)
    return {"p": p, "displacement": e[:, :, 0].copy(), "gradient": e[:, :, 1:4].copy(), "second": e[:, :, 4:].copy(),
            **{k: np.array([w[k] for w in out]) for k in ("zncc", "last_step", "iterations", "status")}, "steps": [w["steps"] for w in out],
            "perms": [w["perms"] for w in out]}


def init_from_icgn(p12, status):
    """sift3d_icgn2_init_from_icgn: status 0 or 1 -> the 12 parameters and zero second derivatives; any other status -> a NaN row"""
    out = from_first_order(np.asarray(p12, np.float64).reshape(-1, 12))
    out[~np.isin(np.asarray(status), (0, 1))] = np.nan
    return out


# ---- the quadratic scene ---------------------------------------------------------------------------------------------------------

T_VEC = (0.37, -0.52, 0.21)
G_MAT = ((0.01, -0.004, 0.002), (0.003, -0.008, 0.005), (-0.002, 0.006, 0.004))
# second derivatives of u, v, w: xx yy zz xy xz yz
Q_SEC = ((0.004, -0.002, 0.003, 0.001, 0.0, 0.0005), (-0.003, 0.002, -0.001, 0.0, 0.001, 0.0), (0.001, 0.004, -0.002, 0.002, 0.0, -0.001))
POIS = np.array([[x, y, z] for x in (24, 40) for y in (25, 39) for z in (24, 38)], np.int32)


def blobs_at(Y, centres, sg, am, reach=0.0):
    """the sum of the blobs at the positions Y (nz, ny, nx, 3), each within `reach` voxels (Chebyshev) of its grid point; a blob is cut
    off outside the box of 5 sigma about its centre, as icgn_ref.render cuts it"""
    nz, ny, nx = Y.shape[:3]
    out = np.zeros((nz, ny, nx), np.float64)
    for c, s, a in zip(centres, sg, am):
        rr = 5.0 * s
        lo = np.maximum(np.floor(c - rr - reach).astype(int), 0)
        hi = np.minimum(np.ceil(c + rr + reach).astype(int), [nx - 1, ny - 1, nz - 1])
        if np.any(lo > hi):
            continue
        sl = (slice(lo[2], hi[2] + 1), slice(lo[1], hi[1] + 1), slice(lo[0], hi[0] + 1))
        e = Y[sl] - c
        inside = np.abs(e).max(-1) <= rr
        out[sl] += np.where(inside, a * np.exp(-0.5 * np.sum(e * e, -1) / (s * s)), 0.0)
    return out


def quadratic_scene(shape=(64, 64, 64), t=T_VEC, G=G_MAT, Q=Q_SEC, seed=1234, per=512, rounds=30):
    """R = blobs on the grid, T[x] = blobs(phi^-1(x)) with phi(y) = y + t + G (y - mid) + 1/2 Q (y - mid)(y - mid); returns R, T and a
    function giving the true 30 parameters at points (phi expanded about each point: exact)"""
    nz, ny, nx = shape
    b = max(8, nz * ny * nx // per)
    rng = np.random.Generator(np.random.PCG64(seed))
    c = np.stack([rng.uniform(0, nx, b), rng.uniform(0, ny, b), rng.uniform(0, nz, b)], 1)
    sg, am = rng.uniform(1.5, 4.5, b), rng.uniform(0.3, 1.3, b)
    t, G = np.asarray(t, np.float64), np.asarray(G, np.float64)
    Qm = np.zeros((3, 3, 3))
    for a, (xx, yy, zz, xy, xz, yz) in enumerate(Q):
        Qm[a] = [[xx, xy, xz], [xy, yy, yz], [xz, yz, zz]]
    mid = (np.array([nx, ny, nz], np.float64) - 1) / 2

    def disp(y):
        e = y - mid
        return t + e @ G.T + 0.5 * np.stack([np.sum((e @ Qm[a]) * e, -1) for a in range(3)], -1)

    zz_, yy_, xx_ = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    X = np.stack([xx_, yy_, zz_], -1).astype(np.float64)
    Y = X.copy()
    for _ in range(rounds):
        Y = X - disp(Y)
    R = blobs_at(X, c, sg, am).astype(np.float32)
    T = blobs_at(Y, c, sg, am, reach=float(np.abs(Y - X).max())).astype(np.float32)

    def truth(points):
        q = np.asarray(points, np.float64).reshape(-1, 3)
        out = np.zeros((len(q), 30))
        e = q - mid
        u = disp(q)
        g = G + np.einsum("ajk,nk->naj", Qm, e)
        for a in range(3):
            out[:, 10 * a] = u[:, a]
            out[:, 10 * a + 1:10 * a + 4] = g[:, a]
            out[:, 10 * a + 4:10 * a + 10] = Q[a]
        return out

    return R, T, truth
