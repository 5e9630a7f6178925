"""CPU restatement of the RANSAC rigid / similarity fit contract (include/sift3d_hip.h, "RANSAC rigid and similarity fits").

Test infrastructure only: nothing under 3dsift_amd/ imports it.  As in ransac_ref.py (whose sampler, scoring, threshold and neighbour
lists are the contract's and are imported), numpy float64 element-wise operations are single IEEE operations, so the arrays below
evaluate the contract's expressions term by term, in the order written, with the bits the GPU produces.  The refit sums run in
numpy's order, which the contract leaves free: its results are compared to a tolerance."""
import numpy as np

from ransac_ref import draws, fmix32, neighbours, resid2, seed_state, tau2_of

MODELS = {"rigid": 0, "similarity": 1}
PLANES = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))
SWEEPS = 8


def draws3(seed, p, H, c):
    """(H, 3) candidate positions: draws 0..2 of the affine sampler (its draw 3 is not made, so c = 3 terminates)"""
    if c >= 4:
        return draws(seed, p, H, c)[:, :3]
    sp = fmix32((seed_state(seed) + int(p)) & 0xFFFFFFFF)[0]
    h = np.arange(H, dtype=np.uint64)
    idx = np.zeros((H, 3), np.int64)
    for j in range(3):
        u = fmix32(((sp + (4 * h + j)) & 0xFFFFFFFF).astype(np.uint32)).astype(np.uint64)
        i = ((u * np.uint64(c)) >> np.uint64(32)).astype(np.int64)
        while True:
            dup = np.zeros(H, bool)
            for q in range(j):
                dup |= idx[:, q] == i
            if not dup.any():
                break
            i = np.where(dup, np.where(i + 1 == c, 0, i + 1), i)
        idx[:, j] = i
    return idx


def dot(u, v):
    return (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]


def cross(u, v):
    return np.stack([u[..., 1] * v[..., 2] - u[..., 2] * v[..., 1], u[..., 2] * v[..., 0] - u[..., 0] * v[..., 2],
                     u[..., 0] * v[..., 1] - u[..., 1] * v[..., 0]], -1)


def _frame(Q):
    """Q (..., 3, 3) samples -> x, y, z (..., 3), c.c, (a.a + b.b) + (b - a).(b - a)"""
    a, b = Q[..., 1, :] - Q[..., 0, :], Q[..., 2, :] - Q[..., 0, :]
    c = cross(a, b)
    aa, cc = dot(a, a), dot(c, c)
    x, z = a / np.sqrt(aa)[..., None], c / np.sqrt(cc)[..., None]
    d = b - a
    return x, cross(z, x), z, cc, (aa + dot(b, b)) + dot(d, d)


def _with_offset(L, p0, t0):
    """(..., 12) rows [L | t0 - L p0]"""
    A = np.empty(L.shape[:-2] + (12,))
    for i in range(3):
        A[..., 4 * i:4 * i + 3] = L[..., i, :]
        A[..., 4 * i + 3] = t0[..., i] - ((L[..., i, 0] * p0[..., 0] + L[..., i, 1] * p0[..., 1]) + L[..., i, 2] * p0[..., 2])
    return A


def triad(P, T, min_det, model=0):
    """P, T: (..., 3, 3) float64 samples -> (A (..., 12), ok (...))"""
    md2 = float(min_det) * float(min_det)
    with np.errstate(all="ignore"):
        x, y, z, cc, ln = _frame(P)
        xt, yt, zt, cct, lnt = _frame(T)
        ok = (cc >= md2) & (cct > 0.0)
        L = np.empty(P.shape[:-2] + (3, 3))
        for i in range(3):
            for j in range(3):
                L[..., i, j] = (xt[..., i] * x[..., j] + yt[..., i] * y[..., j]) + zt[..., i] * z[..., j]
        if model == 1:
            L = np.sqrt(lnt / ln)[..., None, None] * L
        A = _with_offset(L, P[..., 0, :], T[..., 0, :])
    return A, ok


def jacobi4(N, sweeps=SWEEPS):
    """cyclic Jacobi on the symmetric 4x4 N, element by element: (diagonal (4,), V (4, 4))"""
    a = np.array(N, np.float64)
    v = np.eye(4)
    with np.errstate(all="ignore"):
        for _ in range(sweeps):
            for p, q in PLANES:
                apq = a[p, q]
                if apq == 0.0:
                    continue
                theta = (a[q, q] - a[p, p]) / (2.0 * apq)
                t = (1.0 if theta >= 0.0 else -1.0) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
                c = 1.0 / np.sqrt(t * t + 1.0)
                s = t * c
                a[p, p] -= t * apq
                a[q, q] += t * apq
                a[p, q] = a[q, p] = 0.0
                for r in range(4):
                    if r != p and r != q:
                        arp, arq = a[r, p], a[r, q]
                        a[r, p] = a[p, r] = c * arp - s * arq
                        a[r, q] = a[q, r] = s * arp + c * arq
                    vrp, vrq = v[r, p], v[r, q]
                    v[r, p] = c * vrp - s * vrq
                    v[r, q] = s * vrp + c * vrq
    return np.diag(a).copy(), v


def horn_matrix(S):
    """N of the contract from S_ab = sum d_a e_b"""
    (Sxx, Sxy, Sxz), (Syx, Syy, Syz), (Szx, Szy, Szz) = S
    N = np.zeros((4, 4))
    N[0, 0], N[1, 1], N[2, 2], N[3, 3] = (Sxx + Syy) + Szz, (Sxx - Syy) - Szz, (-Sxx + Syy) - Szz, (-Sxx - Syy) + Szz
    N[0, 1], N[0, 2], N[0, 3] = Syz - Szy, Szx - Sxz, Sxy - Syx
    N[1, 2], N[1, 3], N[2, 3] = Sxy + Syx, Szx + Sxz, Syz + Szy
    return N + np.triu(N, 1).T


def rotation_of(q):
    w, x, y, z = q
    ww, xx, yy, zz = w * w, x * x, y * y, z * z
    return np.array([[((ww + xx) - yy) - zz, 2.0 * (x * y - w * z), 2.0 * (x * z + w * y)],
                     [2.0 * (x * y + w * z), ((ww - xx) + yy) - zz, 2.0 * (y * z - w * x)],
                     [2.0 * (x * z - w * y), 2.0 * (y * z + w * x), ((ww - xx) - yy) + zz]])


def e2_of(Cov):
    return ((Cov[0, 0] * Cov[1, 1] - Cov[0, 1] * Cov[0, 1]) + (Cov[0, 0] * Cov[2, 2] - Cov[0, 2] * Cov[0, 2])) + \
        (Cov[1, 1] * Cov[2, 2] - Cov[1, 2] * Cov[1, 2])


def horn(r, t, min_det, model=0):
    """one refit round on the pairs r -> t ((n, 3) float64, n >= 3): (A (12,) or None when singular, e2)"""
    rb, tb = r.mean(0), t.mean(0)
    d, e = r - rb, t - tb
    Cov, S, E = d.T @ d, d.T @ e, float((e * e).sum())
    with np.errstate(all="ignore"):
        e2 = e2_of(Cov)
        if not e2 >= float(min_det) * float(min_det):
            return None, e2
        lam, V = jacobi4(horn_matrix(S))
        best = 0
        for i in range(1, 4):
            if lam[i] > lam[best]:
                best = i
        q = V[:, best]
        q = q / np.sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3])
        L = rotation_of(q)
        if model == 1:
            L = np.sqrt(E / ((Cov[0, 0] + Cov[1, 1]) + Cov[2, 2])) * L
        return _with_offset(L, rb, tb), e2


def hypotheses(pairs, p=0, iterations=4096, inlier_thresh=3.0, seed=1, min_det=1.0, model=0, chunk=1 << 22):
    """every hypothesis of one problem (c >= 3 candidates): draws (H, 3), transforms (H, 12), counts (H,), -1 where degenerate"""
    pairs = np.asarray(pairs, np.float32).reshape(-1, 6)
    c = len(pairs)
    r = pairs[:, :3].astype(np.float64)
    t = pairs[:, 3:].astype(np.float64)
    idx = draws3(seed, p, iterations, c)
    A, ok = triad(r[idx], t[idx], float(np.float32(min_det)), model)
    tau2 = tau2_of(inlier_thresh)
    counts = np.zeros(iterations, np.int64)
    step = max(1, chunk // c)
    with np.errstate(invalid="ignore", over="ignore"):
        for h0 in range(0, iterations, step):
            counts[h0:h0 + step] = (resid2(A[h0:h0 + step], r, t) <= tau2).sum(1)
    counts[~ok] = -1
    return idx, A, counts


def fit(pairs, p=0, iterations=4096, inlier_thresh=3.0, seed=1, refine=1, min_det=1.0, model=0, chunk=1 << 22):
    """the fit of one problem whose candidates are the rows of pairs (c, 6) float32, in order: the dict of ransac_ref.fit"""
    model = MODELS.get(model, model)
    pairs = np.asarray(pairs, np.float32).reshape(-1, 6)
    c = len(pairs)
    out = dict(status=1, candidates=c, best_hypothesis=-1, best_count=0, inliers=0, hyp=np.zeros(12), A=np.zeros(12), mask=np.zeros(c, bool),
               rms=0.0)
    if c < 3:
        return out
    md = float(np.float32(min_det))
    tau2 = tau2_of(inlier_thresh)
    r = pairs[:, :3].astype(np.float64)
    t = pairs[:, 3:].astype(np.float64)
    idx, A, counts = hypotheses(pairs, p, iterations, inlier_thresh, seed, min_det, model, chunk)
    if counts.max() < 0:
        out["status"] = 2
        return out
    bh = int(np.argmax(counts))  # first maximum: the smallest h
    hyp = A[bh].copy()
    out.update(status=0, best_hypothesis=bh, best_count=int(counts[bh]), hyp=hyp)
    cur = hyp.copy()
    for rnd in range(refine + 1):
        with np.errstate(invalid="ignore", over="ignore"):
            d2 = resid2(cur, r, t)
        mask = d2 <= tau2
        cnt = int(mask.sum())
        if rnd == refine or cnt < 3:
            break
        new, e2 = horn(r[mask], t[mask], md, model)
        if new is None:
            out["status"] = 3
            break
        cur = new
    out.update(A=cur, mask=mask, inliers=cnt, rms=float(np.sqrt(d2[mask].sum() / cnt)) if cnt else 0.0)
    return out


def fit_local(pairs, points, k=16, radius=0.0, which=None, iterations=256, **opts):
    """per-point fits (dicts with 'neighbours' padded by -1 to k) of the points listed in `which` (default: all)"""
    pairs = np.asarray(pairs, np.float32).reshape(-1, 6)
    points = np.asarray(points, np.float32).reshape(-1, 3)
    res = []
    for p in (range(len(points)) if which is None else which):
        nb = neighbours(pairs, points[p], k, radius)
        f = fit(pairs[nb], p=int(p), iterations=iterations, **opts)
        f["neighbours"] = np.concatenate([nb, -np.ones(k - len(nb), np.int64)])
        res.append(f)
    return res


def kabsch(r, t, model=0):
    """independent check: SVD Kabsch / Umeyama with the determinant correction -> (s R (3, 3), b (3,))"""
    rb, tb = r.mean(0), t.mean(0)
    d, e = r - rb, t - tb
    U, sv, Vt = np.linalg.svd(e.T @ d)
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt))])
    R = U @ D @ Vt
    s = np.sqrt((e * e).sum() / (d * d).sum()) if model == 1 else 1.0
    return s * R, tb - s * R @ rb


def rotation(axis, deg):
    """Rodrigues rotation about axis by deg degrees"""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    th = np.radians(deg)
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def synth_pairs(n, rng, R=None, s=1.0, b=None, noise=0.3, outliers=0.4, extent=256.0, planar=False):
    """n correspondences of t = s R r + b with Gaussian noise and a share of uniform outliers; planar: rz constant"""
    if R is None:
        R = rotation([0.3, -0.5, 0.8], 7.0)
    if b is None:
        b = np.array([7.5, -3.25, 11.0])
    r = rng.uniform(0, extent, (n, 3))
    if planar:
        r[:, 2] = 40.0
    r = r.astype(np.float32).astype(np.float64)
    t = s * r @ R.T + b + rng.normal(0, noise, (n, 3))
    bad = rng.random(n) < outliers
    t[bad] = rng.uniform(0, extent, (int(bad.sum()), 3))
    return np.concatenate([r, t], 1).astype(np.float32), R, b, ~bad
