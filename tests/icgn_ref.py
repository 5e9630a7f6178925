"""NumPy fp64 restatement of the IC-GN contract of include/sift3d_hip.h (sift3d_icgn, sift3d_icgn_init_from_fits), vectorised over
each subset: test infrastructure only.  The GPU follows the same steps with per-voxel fp32 interpolation and fixed-order sums, so
the two agree to a tolerance, not bit for bit.  Also the blob renderer the tests use: isotropic blobs whose centres move rigidly (or
scale together with the widths) render the deformed volume exactly."""
import numpy as np


def keys_weights(t):
    """Catmull-Rom weights (a = -0.5) of the taps -1, 0, 1, 2 for the fraction t: (..., 4)"""
    t2 = t * t
    t3 = t2 * t
    return np.stack([(-t3 + 2 * t2 - t) / 2, (3 * t3 - 5 * t2 + 2) / 2, (-3 * t3 + 4 * t2 + t) / 2, (t3 - t2) / 2], -1)


def interp(T, pos, cubic=True, f32=False):
    """T (nz, ny, nx) at positions (n, 3) (x, y, z) whose taps lie inside T: the taps are weighted and summed along x, then y, then z,
    each sum in tap order.  f32: the header's "per-voxel interpolation in fp32" -- the fraction, the weights, every product and every
    sum rounded to float32 (same weights, same order, not fused); the result is returned as float64"""
    fl = np.floor(pos)
    dt = np.float32 if f32 else np.float64
    t = (pos - fl).astype(dt)
    i = fl.astype(np.int64)
    if cubic:
        off, w = (-1, 0, 1, 2), keys_weights(t)
    else:
        off, w = (0, 1), np.stack([1 - t, t], -1)
    nz, ny, nx = T.shape
    flat = np.ascontiguousarray(T).reshape(-1)
    base = (i[:, 2] * ny + i[:, 1]) * nx + i[:, 0]
    out = None
    for kz, oz in enumerate(off):
        vz = None
        for ky, oy in enumerate(off):
            row = base + (oz * ny + oy) * nx
            vy = None
            for kx, ox in enumerate(off):
                term = flat[row + ox].astype(dt) * w[:, 0, kx]
                vy = term if vy is None else vy + term
            term = vy * w[:, 1, ky]
            vz = term if vz is None else vz + term
        term = vz * w[:, 2, kz]
        out = term if out is None else out + term
    return out.astype(np.float64)


def offsets(r):
    """the subset offsets d (N, 3) = (dx, dy, dz), x fastest"""
    d = np.arange(-r, r + 1)
    dz, dy, dx = np.meshgrid(d, d, d, indexing="ij")
    return np.stack([dx.ravel(), dy.ravel(), dz.ravel()], 1).astype(np.float64)


def sentinels(r):
    """linear subset indices (x fastest) worth a spike: both corners, the last voxel of a thread's first round and the first of its
    second, the first voxels that the kernels' walk (SubsetWalk) reaches through a carry into y and into z, two seeded random ones (six at least)"""
    D = 2 * r + 1
    N = D ** 3
    sz = 256 // (D * D)
    sy = (256 - sz * D * D) // D
    sx = 256 - sz * D * D - sy * D
    out = {"first": 0, "last": N - 1}
    if N > 255:
        out["i255"] = 255
    if N > 256:
        out["i256"] = 256
        for i in range(256, N):
            j = i - 256
            cx = j % D + sx >= D
            if cx and "ycarry" not in out:
                out["ycarry"] = i
            if (j // D) % D + sy + cx >= D and "zcarry" not in out:
                out["zcarry"] = i
            if "ycarry" in out and "zcarry" in out:
                break
    rng = np.random.default_rng(2000 + r)
    k = 0
    while len(out) < 6 or k < 2:
        i = int(rng.integers(1, N - 1))
        if i not in out.values():
            out[f"rand{k}"] = i
            k += 1
    return out


def F_of(p):
    return np.array([[1 + p[1], p[2], p[3]], [p[5], 1 + p[6], p[7]], [p[9], p[10], 1 + p[11]]])


def M_of(p):
    M = np.eye(4)
    M[:3, :3] = F_of(p)
    M[:3, 3] = p[[0, 4, 8]]
    return M


def p_of(M):
    G = M[:3, :3] - np.eye(3)
    return np.array([M[0, 3], *G[0], M[1, 3], *G[1], M[2, 3], *G[2]])


def warp(p, q, d):
    return (q + d @ F_of(p).T) + p[[0, 4, 8]]


def in_domain(shape, p, q, r, cubic):
    nz, ny, nx = shape
    c = np.array([[sx, sy, sz] for sz in (-r, r) for sy in (-r, r) for sx in (-r, r)], np.float64)
    with np.errstate(invalid="ignore"):
        f = np.floor(warp(p, q, c))
    if not np.all(np.isfinite(f)):
        return False
    n = np.array([nx, ny, nz])
    lo, hi = (1, 2) if cubic else (0, 1)
    return bool(np.all(f - lo >= 0) and np.all(f + hi <= n - 1))


def positive_definite(H):
    """the contract's test of H: a column Cholesky (the order of k_icgn_prepare) that stops at the first pivot that is <= 0 or NaN.
    np.linalg.cholesky does not state it: it returns a NaN factor for a NaN entry and accepts an infinite pivot's NaN remainder."""
    A = np.array(H, np.float64)
    n = len(A)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for k in range(n):
            d = A[k, k]
            if not d > 0:
                return False
            A[k, k] = np.sqrt(d)
            A[k + 1:, k] = A[k + 1:, k] / A[k, k]
            for j in range(k + 1, n):
                A[j:, j] = A[j:, j] - A[j:, k] * A[j, k]
    return True


def refine(R, T, q, init=None, subset_radius=16, max_iterations=20, tolerance=1e-3, interpolation=0, f32=False):
    """one POI: dict(p, zncc, last_step, iterations, status) as sift3d_icgn_result, and steps (||dp||_r of every computed step).
    f32: interp's float32 form"""
    r, cubic = subset_radius, interpolation == 0
    q = np.asarray(q, np.int64)
    p = np.zeros(12) if init is None else np.array(init, np.float64)

    steps = []  # ||dp||_r of every computed step, in order

    def res(p, zncc, last, it, status):
        return dict(p=np.array(p, np.float64), zncc=float(zncc), last_step=float(last), iterations=int(it), status=int(status),
                    steps=tuple(steps))

    if not np.all(np.isfinite(p)):
        return res(p, 0, 0, 0, 5)
    nz, ny, nx = R.shape
    if np.any(q - r - 1 < 0) or np.any(q + r + 1 > np.array([nx, ny, nz]) - 1):
        return res(p, 0, 0, 0, 2)
    d = offsets(r)
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
    v = np.concatenate([np.ones((len(d), 1)), d], 1)
    SD = np.concatenate([gc[:, None] * v for gc in g], 1)
    if not dR > 0:
        return res(p, 0, 0, 0, 4)
    with np.errstate(invalid="ignore", over="ignore"):
        H = SD.T @ SD
    if not positive_definite(H):
        return res(p, 0, 0, 0, 4)
    if not in_domain(T.shape, p, q, r, cubic):
        return res(p, 0, 0, 0, 3)
    N = float(len(d))
    it, last, done, status = 0, 0.0, False, None
    while True:
        Tp = interp(T, warp(p, q, d), cubic, f32) - Rm  # ZNSSD does not change when T is shifted
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
        gd = dp.reshape(3, 4)[:, 1:]
        with np.errstate(invalid="ignore", over="ignore"):
            last = float(np.sqrt(dp[0] ** 2 + dp[4] ** 2 + dp[8] ** 2 + r * r * np.sum(gd * gd)))
        steps.append(last)
        if not np.all(np.isfinite(dp)):
            return res(p, zncc, last, it, 6)
        det = np.linalg.det(F_of(dp))
        if det == 0 or not np.isfinite(det):
            return res(p, zncc, last, it, 6)
        pn = p_of(M_of(p) @ np.linalg.inv(M_of(dp)))
        if not in_domain(T.shape, pn, q, r, cubic):
            return res(p, zncc, last, it, 3)
        p = pn
        it += 1
        if last < tolerance:
            status, done = 0, True
        elif it >= max_iterations:
            status, done = 1, True


def icgn(R, T, points, init=None, **opts):
    """every POI of points ((m, 3) x, y, z): arrays like capi.icgn's"""
    pts = np.asarray(points, np.int64).reshape(-1, 3)
    rows = [refine(R, T, q, None if init is None else init[i], **opts) for i, q in enumerate(pts)]
    p = np.array([w["p"] for w in rows]).reshape(-1, 12)
    return {"p": p, "displacement": p[:, [0, 4, 8]], "gradient": p.reshape(-1, 3, 4)[:, :, 1:],
            **{k: np.array([w[k] for w in rows]) for k in ("zncc", "last_step", "iterations", "status")}, "steps": [w["steps"] for w in rows]}


def init_from_fits(A, status, points):
    """sift3d_icgn_init_from_fits: (u, v, w) = L q + b - q and F = L, in the C order of operations; status != 0 -> NaN row"""
    A = np.asarray(A, np.float64).reshape(-1, 3, 4)
    out = np.full((len(A), 12), np.nan)
    for i, (a, s, q) in enumerate(zip(A, status, np.asarray(points, np.float64).reshape(-1, 3))):
        if s != 0:
            continue
        for k in range(3):
            out[i, 4 * k] = (((a[k, 0] * q[0] + a[k, 1] * q[1]) + a[k, 2] * q[2]) + a[k, 3]) - q[k]
            out[i, 4 * k + 1:4 * k + 4] = a[k, :3] - np.eye(3)[k]
    return out


# ---- synthetic scenes ------------------------------------------------------------------------------------------------------------

def render(shape, centres, sg, am):
    """synth.blobs' rendering with explicit blob centres (x, y, z) and widths"""
    nz, ny, nx = shape
    vol = np.zeros(shape, np.float64)
    for (x0, y0, z0), s, a in zip(centres, sg, am):
        rr = 5.0 * s
        xl, xh = max(0, int(np.floor(x0 - rr))), min(nx - 1, int(np.ceil(x0 + rr)))
        yl, yh = max(0, int(np.floor(y0 - rr))), min(ny - 1, int(np.ceil(y0 + rr)))
        zl, zh = max(0, int(np.floor(z0 - rr))), min(nz - 1, int(np.ceil(z0 + rr)))
        if xl > xh or yl > yh or zl > zh:
            continue
        gx = np.exp(-0.5 * ((np.arange(xl, xh + 1) - x0) / s) ** 2)
        gy = np.exp(-0.5 * ((np.arange(yl, yh + 1) - y0) / s) ** 2)
        gz = np.exp(-0.5 * ((np.arange(zl, zh + 1) - z0) / s) ** 2)
        vol[zl:zh + 1, yl:yh + 1, xl:xh + 1] += a * gz[:, None, None] * gy[None, :, None] * gx[None, None, :]
    return vol.astype(np.float32)


def rot(deg_x, deg_y, deg_z):
    ax, ay, az = np.radians([deg_x, deg_y, deg_z])
    Rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
    Ry = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]])
    Rz = np.array([[np.cos(az), -np.sin(az), 0], [np.sin(az), np.cos(az), 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def scene(shape, Lmat=np.eye(3), tvec=(0.0, 0.0, 0.0), seed=1234, per=512, blob_params=None):
    """R and T = R under x -> L (x - mid) + mid + t (blob centres moved, widths scaled by det(L)^(1/3): exact for a rotation or an
    isotropic scaling), about one blob per `per` voxels; returns R, T and a function giving the true 12 parameters at points"""
    nz, ny, nx = shape
    b = max(8, nz * ny * nx // per)
    rng = np.random.Generator(np.random.PCG64(seed))
    c = np.stack([rng.uniform(0, nx, b), rng.uniform(0, ny, b), rng.uniform(0, nz, b)], 1)
    sg, am = rng.uniform(1.5, 4.5, b), rng.uniform(0.3, 1.3, b)
    Lmat = np.asarray(Lmat, np.float64)
    t = np.asarray(tvec, np.float64)
    mid = (np.array([nx, ny, nz], np.float64) - 1) / 2
    c2 = (c - mid) @ Lmat.T + mid + t
    s2 = sg * abs(np.linalg.det(Lmat)) ** (1 / 3)
    R, T = render(shape, c, sg, am), render(shape, c2, s2, am)

    def truth(points):
        q = np.asarray(points, np.float64).reshape(-1, 3)
        u = (q - mid) @ Lmat.T + mid + t - q
        out = np.zeros((len(q), 12))
        for k in range(3):
            out[:, 4 * k] = u[:, k]
            out[:, 4 * k + 1:4 * k + 4] = Lmat[k] - np.eye(3)[k]
        return out

    return R, T, truth
