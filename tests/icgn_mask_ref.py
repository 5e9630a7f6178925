"""NumPy fp64 restatement of the masked IC-GN contract of include/sift3d_hip.h (sift3d_icgn_masked, sift3d_mask_from_level): test
infrastructure only.  It is icgn_ref.refine with every sum taken over the active voxels of the subset (selected, not multiplied by
zero: R and T are not read elsewhere), the active count n in N's place and status 7.  interp, warp, positive_definite, the domain test
and the scenes are icgn_ref's; interpolation 2 uses bspline_ref's coefficients and weights."""
import numpy as np

import bspline_ref
import icgn_ref as ref


def active_of(mask):
    """the active voxels of a mask (nz, ny, nx), any non-zero byte in: a voxel that, with its six face neighbours, lies in the volume
    and is in the mask.  Boolean (nz, ny, nx); the volume's boundary voxels are never active."""
    m = np.asarray(mask) != 0
    a = np.zeros(m.shape, bool)
    if min(m.shape) < 3:
        return a
    c = m[1:-1, 1:-1, 1:-1]
    a[1:-1, 1:-1, 1:-1] = (c & m[1:-1, 1:-1, :-2] & m[1:-1, 1:-1, 2:] & m[1:-1, :-2, 1:-1] & m[1:-1, 2:, 1:-1] & m[:-2, 1:-1, 1:-1] &
                           m[2:, 1:-1, 1:-1])
    return a


def needed_of(mask):
    """the voxels of R a masked call may read: the active ones and their face neighbours.  Boolean (nz, ny, nx)."""
    a = active_of(mask)
    n = a.copy()
    n[:, :, 1:] |= a[:, :, :-1]
    n[:, :, :-1] |= a[:, :, 1:]
    n[:, 1:, :] |= a[:, :-1, :]
    n[:, :-1, :] |= a[:, 1:, :]
    n[1:, :, :] |= a[:-1, :, :]
    n[:-1, :, :] |= a[1:, :, :]
    return n


def mask_from_level(vol, level):
    """sift3d_mask_from_level: 1 where float64(vol) >= level, else 0 (a NaN voxel is 0)"""
    with np.errstate(invalid="ignore"):
        return (np.asarray(vol, np.float32).astype(np.float64) >= float(level)).astype(np.uint8)


def refine(R, T, mask, q, init=None, min_fraction=0.0, subset_radius=16, max_iterations=20, tolerance=1e-3, interpolation=0, f32=False,
           active=None):
    """one POI: icgn_ref.refine's dict and `active`, the subset's active count (0 with status 5 or 2).  T: the volume, or for
    interpolation 2 the coefficients (masked_icgn prefilters).  active: active_of(mask) where the caller has it."""
    r, cubic = subset_radius, interpolation != 1
    q = np.asarray(q, np.int64)
    p = np.zeros(12) if init is None else np.array(init, np.float64)
    steps = []

    def res(p, zncc, last, it, status, n):
        return dict(p=np.array(p, np.float64), zncc=float(zncc), last_step=float(last), iterations=int(it), status=int(status),
                    steps=tuple(steps), active=int(n))

    if not np.all(np.isfinite(p)):
        return res(p, 0, 0, 0, 5, 0)
    nz, ny, nx = R.shape
    if np.any(q - r - 1 < 0) or np.any(q + r + 1 > np.array([nx, ny, nz]) - 1):
        return res(p, 0, 0, 0, 2, 0)
    act = active_of(mask) if active is None else active
    d_all = ref.offsets(r)
    N_all = len(d_all)
    di = d_all.astype(np.int64)
    on = act[q[2] + di[:, 2], q[1] + di[:, 1], q[0] + di[:, 0]]
    n = int(on.sum())
    # float32(min_fraction) widened, as the C entry takes it
    if n == 0 or float(n) < float(np.float32(min_fraction)) * float(N_all):
        return res(p, 0, 0, 0, 7, n)
    d, di = d_all[on], di[on]  # the active voxels, in the walk's (x fastest) order
    x, y, z = q[0] + di[:, 0], q[1] + di[:, 1], q[2] + di[:, 2]
    Rf = np.asarray(R, np.float32)
    half = np.float32(0.5)
    with np.errstate(invalid="ignore", over="ignore"):
        g = [(half * (Rf[z, y, x + 1] - Rf[z, y, x - 1])).astype(np.float64), (half * (Rf[z, y + 1, x] - Rf[z, y - 1, x])).astype(np.float64),
             (half * (Rf[z + 1, y, x] - Rf[z - 1, y, x])).astype(np.float64)]
        Rs = Rf[z, y, x].astype(np.float64)
        Rm = Rs.sum() / float(n)
        Rp = Rs - Rm
        dR = np.sqrt(np.sum(Rp * Rp))
    v = np.concatenate([np.ones((len(d), 1)), d], 1)
    SD = np.concatenate([gc[:, None] * v for gc in g], 1)
    if not dR > 0:
        return res(p, 0, 0, 0, 4, n)
    with np.errstate(invalid="ignore", over="ignore"):
        H = SD.T @ SD
    if not ref.positive_definite(H):
        return res(p, 0, 0, 0, 4, n)
    if not ref.in_domain(T.shape, p, q, r, cubic):  # the 8 corners of the full box
        return res(p, 0, 0, 0, 3, n)
    Nn = float(n)
    it, last, done, status = 0, 0.0, False, None
    while True:
        Tp = ref.interp(T, ref.warp(p, q, d), cubic, f32) - Rm
        sT = Tp.sum()
        sTT = np.sum(Tp * Tp)
        tm = sT / Nn
        dt2 = sTT - sT * tm
        flat = not dt2 > 1e-10 * sTT
        dT = 0.0 if flat else np.sqrt(dt2)
        zncc = 0.0 if flat else np.sum(Rp * (Tp - tm)) / (dR * dT)
        if done:
            return res(p, zncc, last, it, status, n)
        if flat:
            return res(p, 0.0, last, it, 4, n)
        b = SD.T @ (Rp - (dR / dT) * (Tp - tm))
        dp = -np.linalg.solve(H, b)
        gd = dp.reshape(3, 4)[:, 1:]
        with np.errstate(invalid="ignore", over="ignore"):
            last = float(np.sqrt(dp[0] ** 2 + dp[4] ** 2 + dp[8] ** 2 + r * r * np.sum(gd * gd)))
        steps.append(last)
        if not np.all(np.isfinite(dp)):
            return res(p, zncc, last, it, 6, n)
        det = np.linalg.det(ref.F_of(dp))
        if det == 0 or not np.isfinite(det):
            return res(p, zncc, last, it, 6, n)
        pn = ref.p_of(ref.M_of(p) @ np.linalg.inv(ref.M_of(dp)))
        if not ref.in_domain(T.shape, pn, q, r, cubic):
            return res(p, zncc, last, it, 3, n)
        p = pn
        it += 1
        if last < tolerance:
            status, done = 0, True
        elif it >= max_iterations:
            status, done = 1, True


def icgn_masked(R, T, mask, points, init=None, min_fraction=0.0, tar_is_coefficients=False, **opts):
    """every POI of points ((m, 3) x, y, z): arrays like capi.icgn_masked's"""
    pts = np.asarray(points, np.int64).reshape(-1, 3)
    act = active_of(mask)
    bspline = opts.get("interpolation", 0) == 2
    Tq = bspline_ref.coefficients(T, tar_is_coefficients) if bspline else T

    def rows():
        return [refine(R, Tq, mask, q, None if init is None else init[i], min_fraction, active=act, **opts) for i, q in enumerate(pts)]

    if bspline:
        with bspline_ref._bspline_weights():
            rows = rows()
    else:
        rows = rows()
    p = np.array([w["p"] for w in rows]).reshape(-1, 12)
    return {"p": p, "displacement": p[:, [0, 4, 8]], "gradient": p.reshape(-1, 3, 4)[:, :, 1:],
            **{k: np.array([w[k] for w in rows]) for k in ("zncc", "last_step", "iterations", "status", "active")},
            "steps": [w["steps"] for w in rows]}


# ---- the two-body scene of the issue: two bodies sliding along the plane x = X_CUT ---------------------------------------------

SHAPE, X_CUT, RADIUS = (48, 48, 48), 24, 6
T_A, T_B = (0.0, 0.3, -0.2), (0.0, -0.6, 0.5)
TWO_BODY_POIS = np.array([(23 - k, 20, 22) for k in range(5)] + [(23 - k, 27, 25) for k in range(5)], np.int32)


def two_body_scene():
    """R, T (body A = scene seed 21 moved by T_A in x < X_CUT, body B = seed 22 moved by T_B in x >= X_CUT, in R and T alike), the
    mask of body A and the true parameters of A's POIs"""
    Ra, Ta, truth = ref.scene(SHAPE, np.eye(3), T_A, seed=21)
    Rb, Tb, _ = ref.scene(SHAPE, np.eye(3), T_B, seed=22)
    R, T = Ra.copy(), Ta.copy()
    R[:, :, X_CUT:] = Rb[:, :, X_CUT:]
    T[:, :, X_CUT:] = Tb[:, :, X_CUT:]
    mask = np.zeros(SHAPE, np.uint8)
    mask[:, :, :X_CUT] = 1
    return R, T, mask, truth
