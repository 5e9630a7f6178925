"""NumPy restatement of the displacement validation's contract (sift3d_validate_displacements and its host-only helpers,
include/sift3d_hip.h): test infrastructure only.  Windows are brute force; every arithmetic step is the single fp64 operation the
contract names, in its association, so the GPU's records must equal these as numbers, with no tolerance."""
import numpy as np

COORD_MAX = 2 ** 24
RESULT_DTYPE = np.dtype([("median", "<f8", (3,)), ("mad", "<f8", (3,)), ("score", "<f8"), ("neighbours", "<i4"), ("status", "<i4"),
                         ("flagged", "<i4"), ("pass", "<i4")])
DEFAULTS = dict(radius=16, min_neighbours=6, passes=2, threshold=2.0, eps=0.1)


def contributes(points, disp, grad=None, valid=None):
    """the contract's rule, per POI; also which POIs have every coordinate in range"""
    q = np.asarray(points, np.int64).reshape(-1, 3)
    in_range = (np.abs(q) <= COORD_MAX).all(1)
    on = in_range & np.isfinite(np.asarray(disp, np.float64).reshape(-1, 3)).all(1)
    if valid is not None:
        on &= np.asarray(valid).reshape(-1) != 0
    if grad is not None:
        on &= np.isfinite(np.asarray(grad, np.float64).reshape(-1, 9)).all(1)
    return on, in_range


def median(v):
    """the exact order statistic of a 1-d array, n >= 1: the middle value, or 0.5 * (lo + hi) of the two middle values"""
    n = len(v)
    if n & 1:
        return np.partition(v, n // 2)[n // 2]
    p = np.partition(v, [n // 2 - 1, n // 2])
    return 0.5 * (p[n // 2 - 1] + p[n // 2])


class _Field:
    def __init__(self, points, disp, grad, valid, radius):
        self.q = np.asarray(points, np.int64).reshape(-1, 3)
        self.u = np.asarray(disp, np.float64).reshape(-1, 3)
        self.G = None if grad is None else np.asarray(grad, np.float64).reshape(-1, 3, 3)
        self.on, self.in_range = contributes(points, disp, grad, valid)
        self.radius = radius
        self.cand = np.flatnonzero(self.on)

    def stats(self, i, flagged):
        """(n, median[3], mad[3]) of POI i over its neighbours that are not flagged"""
        c = self.cand
        near = (np.abs(self.q[c] - self.q[i]) <= self.radius).all(1) & (c != i) & ~flagged[c]
        j = c[near]
        n = len(j)
        if n == 0:
            return 0, np.zeros(3), np.zeros(3)
        e = self.u[j]
        if self.G is not None:
            d = (self.q[i] - self.q[j]).astype(np.float64)
            g = self.G[j]
            e = e + ((g[:, :, 0] * d[:, None, 0] + g[:, :, 1] * d[:, None, 1]) + g[:, :, 2] * d[:, None, 2])
        med = np.array([median(e[:, k]) for k in range(3)])
        mad = np.array([median(np.abs(e[:, k] - med[k])) for k in range(3)])
        return n, med, mad

    def score(self, i, med, mad, eps):
        return np.max(np.abs(self.u[i] - med) / (mad + eps))


def validate(points, disp, grad=None, valid=None, trace=None, **opts):
    """the records (RESULT_DTYPE) of the contract.  trace (a list): receives (pass, POI, score) of every score a pass computes"""
    o = dict(DEFAULTS)
    assert set(opts) <= set(o), opts
    o.update(opts)
    f = _Field(points, disp, grad, valid, o["radius"])
    m = len(f.q)
    flagged = np.zeros(m, bool)
    pass_of = np.zeros(m, np.int32)
    out = np.zeros(m, RESULT_DTYPE)
    with np.errstate(all="ignore"):
        for p in range(1, o["passes"] + 1):
            new = flagged.copy()
            for i in np.flatnonzero(f.on & ~flagged):
                n, med, mad = f.stats(i, flagged)
                if n < o["min_neighbours"]:
                    continue
                s = f.score(i, med, mad, o["eps"])
                if trace is not None:
                    trace.append((p, int(i), float(s)))
                if s > o["threshold"]:
                    new[i] = True
                    pass_of[i] = p
            if (new == flagged).all():
                break   # the later passes would repeat this one
            flagged = new
        for i in range(m):
            r = out[i]
            if not f.in_range[i]:
                r["status"] = 2
                continue
            r["flagged"], r["pass"] = flagged[i], pass_of[i]
            n, med, mad = f.stats(i, flagged)
            r["neighbours"] = n
            if n < o["min_neighbours"]:
                r["status"] = 1
                continue
            r["median"], r["mad"] = med, mad
            if f.on[i]:
                r["status"], r["score"] = 0, f.score(i, med, mad, o["eps"])
            else:
                r["status"] = 3
    return out


def input_from_icgn(p, zncc, status, zncc_min=0.0, accept_unconverged=False):
    """sift3d_validate_input_from_icgn / _icgn2 by the width of p (12 or 30): disp (m, 3), grad (m, 9), valid (m,) uint8"""
    p = np.asarray(p, np.float64)
    w = p.shape[1] // 3
    disp = p[:, [0, w, 2 * w]].copy()
    grad = p[:, [1, 2, 3, w + 1, w + 2, w + 3, 2 * w + 1, 2 * w + 2, 2 * w + 3]].copy()
    status = np.asarray(status)
    done = (status == 0) | ((status == 1) & bool(accept_unconverged))
    with np.errstate(invalid="ignore"):
        valid = done & (np.asarray(zncc, np.float64) >= zncc_min) & np.isfinite(disp).all(1)
    return disp, grad, valid.astype(np.uint8)


def keep(rec, valid=None):
    """sift3d_validate_keep"""
    k = (rec["status"] == 0) & (rec["flagged"] == 0)
    if valid is not None:
        k &= np.asarray(valid) != 0
    return k.astype(np.uint8)


def init_from_validation(rec, init12):
    """sift3d_icgn_init_from_validation: (the rows, how many were written)"""
    out = np.array(init12, np.float64).reshape(-1, 12)
    rows = ((rec["flagged"] != 0) & (rec["status"] == 0)) | (rec["status"] == 3)
    out[rows] = 0.0
    out[rows, 0], out[rows, 4], out[rows, 8] = rec["median"][rows, 0], rec["median"][rows, 1], rec["median"][rows, 2]
    return out, int(rows.sum())


def same(a, b):
    """the fields of two record arrays that differ as numbers (-0 = +0; NaN never expected): empty when they agree"""
    bad = []
    for k in RESULT_DTYPE.names:
        if not np.array_equal(np.asarray(a[k]), np.asarray(b[k])):
            rows = np.flatnonzero((np.asarray(a[k]) != np.asarray(b[k])).reshape(len(a), -1).any(1))
            bad.append((k, rows[:8].tolist(), np.asarray(a[k])[rows[:3]].tolist(), np.asarray(b[k])[rows[:3]].tolist()))
    return bad
