"""CPU restatement of the RANSAC affine fit contract (include/sift3d_hip.h, "RANSAC affine fits of matched keypoints").

Test infrastructure only: nothing under 3dsift_amd/ imports it.  numpy float64 element-wise operations are single IEEE operations
(no contraction), so the arrays below evaluate the contract's expressions term by term, in the order written, with the bits the
GPU produces; the neighbour distances are float32 arrays for the same reason.  The refit sums run in numpy's order, which the
contract leaves free: its results are compared to a tolerance."""
import numpy as np

U32 = np.uint32


def fmix32(x):
    x = np.array(x, dtype=np.uint32, copy=True, ndmin=1)
    x ^= x >> U32(16)
    x *= U32(0x85EBCA6B)
    x ^= x >> U32(13)
    x *= U32(0xC2B2AE35)
    x ^= x >> U32(16)
    return x


def seed_state(seed):
    return int(fmix32((int(seed) & 0xFFFFFFFF) ^ 0x9E3779B9)[0])


def draws(seed, p, H, c):
    """(H, 4) candidate positions of hypotheses 0..H-1 of problem p over c candidates"""
    s = seed_state(seed)
    sp = fmix32((s + int(p)) & 0xFFFFFFFF)[0]
    h = np.arange(H, dtype=np.uint64)
    idx = np.zeros((H, 4), np.int64)
    for j in range(4):
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


def _inv3(M, min_det, with_det=False):
    """cofactor inverse of (..., 3, 3); returns (inv, ok), with_det: (inv, ok, det)"""
    C = np.empty_like(M)
    for r in range(3):
        r1, r2 = [x for x in range(3) if x != r]
        for c in range(3):
            c1, c2 = [x for x in range(3) if x != c]
            with np.errstate(invalid="ignore", over="ignore"):
                v = M[..., r1, c1] * M[..., r2, c2] - M[..., r1, c2] * M[..., r2, c1]
            C[..., r, c] = -v if (r + c) & 1 else v
    with np.errstate(invalid="ignore", over="ignore"):
        det = (M[..., 0, 0] * C[..., 0, 0] + M[..., 0, 1] * C[..., 0, 1]) + M[..., 0, 2] * C[..., 0, 2]
        ok = np.abs(det) >= min_det
    inv = np.empty_like(M)
    with np.errstate(divide="ignore", invalid="ignore"):
        for i in range(3):
            for j in range(3):
                inv[..., i, j] = C[..., j, i] / det
    return (inv, ok, det) if with_det else (inv, ok)


def _affine(N, inv, p0, t0):
    """(..., 12) rows [L | b] with L = N inv, b = t0 - L p0, in the contract's order"""
    A = np.empty(N.shape[:-2] + (12,))
    for i in range(3):
        for j in range(3):
            A[..., 4 * i + j] = (N[..., i, 0] * inv[..., 0, j] + N[..., i, 1] * inv[..., 1, j]) + N[..., i, 2] * inv[..., 2, j]
        A[..., 4 * i + 3] = t0[..., i] - ((A[..., 4 * i] * p0[..., 0] + A[..., 4 * i + 1] * p0[..., 1]) + A[..., 4 * i + 2] * p0[..., 2])
    return A


def minimal_solve(P, T, min_det):
    """P, T: (H, 4, 3) float64 -> (A (H, 12), ok (H,))"""
    M = np.empty(P.shape[:-2] + (3, 3))
    N = np.empty_like(M)
    with np.errstate(invalid="ignore"):
        for k in range(1, 4):
            M[..., :, k - 1] = P[..., k, :] - P[..., 0, :]
            N[..., :, k - 1] = T[..., k, :] - T[..., 0, :]
    inv, ok = _inv3(M, float(min_det))
    with np.errstate(invalid="ignore", over="ignore"):
        A = _affine(N, inv, P[..., 0, :], T[..., 0, :])
    return A, ok


def resid2(A, r, t):
    """A (..., 12) against candidates r, t (n, 3) float64 -> d2 (..., n)"""
    A = A[..., None, :]
    e = []
    for i in range(3):
        e.append((((A[..., 4 * i] * r[:, 0] + A[..., 4 * i + 1] * r[:, 1]) + A[..., 4 * i + 2] * r[:, 2]) + A[..., 4 * i + 3]) - t[:, i])
    return (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]


def tau2_of(tau):
    return float(np.float32(tau)) * float(np.float32(tau))


def hypotheses(pairs, p=0, iterations=4096, inlier_thresh=3.0, seed=1, min_det=1.0, chunk=1 << 22):
    """every hypothesis of one problem (c >= 4 candidates): draws (H, 4), transforms (H, 12), counts (H,), -1 where degenerate"""
    pairs = np.asarray(pairs, np.float32).reshape(-1, 6)
    c = len(pairs)
    r = pairs[:, :3].astype(np.float64)
    t = pairs[:, 3:].astype(np.float64)
    idx = draws(seed, p, iterations, c)
    A, ok = minimal_solve(r[idx], t[idx], float(np.float32(min_det)))
    tau2 = tau2_of(inlier_thresh)
    counts = np.zeros(iterations, np.int64)
    step = max(1, chunk // c)
    with np.errstate(invalid="ignore", over="ignore"):
        for h0 in range(0, iterations, step):
            counts[h0:h0 + step] = (resid2(A[h0:h0 + step], r, t) <= tau2).sum(1)
    counts[~ok] = -1
    return idx, A, counts


def fit(pairs, p=0, iterations=4096, inlier_thresh=3.0, seed=1, refine=1, min_det=1.0, chunk=1 << 22, trace=None):
    """the fit of one problem whose candidates are the rows of pairs (c, 6) float32, in order; trace (a list) receives one
    dict(round, d2, det) per scoring of the refit: the candidates' d2 under the round's transform and the det Cov that followed
    (None where no covariance was formed)"""
    pairs = np.asarray(pairs, np.float32).reshape(-1, 6)
    c = len(pairs)
    out = dict(status=1, candidates=c, best_hypothesis=-1, best_count=0, inliers=0, hyp=np.zeros(12), A=np.zeros(12), mask=np.zeros(c, bool),
               rms=0.0)
    if c < 4:
        return out
    md = float(np.float32(min_det))
    tau2 = tau2_of(inlier_thresh)
    r = pairs[:, :3].astype(np.float64)
    t = pairs[:, 3:].astype(np.float64)
    idx, A, counts = hypotheses(pairs, p, iterations, inlier_thresh, seed, min_det, chunk)
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
        if trace is not None:
            trace.append(dict(round=rnd, d2=d2, det=None))
        if rnd == refine or cnt < 4:
            break
        rb, tb = r[mask].mean(0), t[mask].mean(0)
        dr, dt = r[mask] - rb, t[mask] - tb
        Cov, S = dr.T @ dr, dt.T @ dr
        inv, ok1, det = _inv3(Cov, md, with_det=True)
        if trace is not None:
            trace[-1]["det"] = float(det)
        if not ok1:
            out["status"] = 3
            break
        cur = _affine(S, inv, rb, tb)
    out.update(A=cur, mask=mask, inliers=cnt, rms=float(np.sqrt(d2[mask].sum() / cnt)) if cnt else 0.0)
    return out


def distances(pairs, q):
    """fp32 d2_i of the contract (NaN and +inf included)"""
    pairs = np.asarray(pairs, np.float32).reshape(-1, 6)
    q = np.asarray(q, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        dx = pairs[:, 0] - q[0]
        dy = pairs[:, 1] - q[1]
        dz = pairs[:, 2] - q[2]
        return (dx * dx + dy * dy) + dz * dz


def radius2(radius):
    return np.float32(radius) * np.float32(radius)


def neighbours(pairs, q, k, radius=0.0):
    """candidate list of query q: the k smallest (d2, i), float32 d2, among the pairs within radius (radius <= 0: all)"""
    pairs = np.asarray(pairs, np.float32).reshape(-1, 6)
    q = np.asarray(q, np.float32)
    d2 = distances(pairs, q)
    keep = ~np.isnan(d2)
    if radius > 0:
        keep &= d2 <= radius2(radius)
    i = np.nonzero(keep)[0]
    order = np.lexsort((i, d2[i]))
    return i[order[:k]]


def fit_local(pairs, points, k=32, radius=0.0, which=None, iterations=256, **opts):
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


def synth_pairs(n, rng, L=None, b=None, noise=0.3, outliers=0.4, extent=256.0):
    """n correspondences of a known affine t = L r + b with Gaussian noise and a share of uniform outliers"""
    if L is None:
        th = 0.2
        R = np.array([[np.cos(th), -np.sin(th), 0], [np.sin(th), np.cos(th), 0], [0, 0, 1]])
        L = R @ np.diag([1.05, 0.97, 1.02])
    if b is None:
        b = np.array([7.5, -3.25, 11.0])
    r = rng.uniform(0, extent, (n, 3))
    t = r @ L.T + b + rng.normal(0, noise, (n, 3))
    bad = rng.random(n) < outliers
    t[bad] = rng.uniform(0, extent, (int(bad.sum()), 3))
    return np.concatenate([r, t], 1).astype(np.float32), L, b, ~bad
