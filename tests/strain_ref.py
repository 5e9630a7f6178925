"""NumPy fp64 restatement of the strain contract (sift3d_strain, include/sift3d_hip.h): the neighbours by the integer window test, the
plane fit once from the normal equations as the header writes them (solve="normal") and once from numpy.linalg.lstsq on [1, d]
(solve="lstsq"), the eigenvalues from numpy.linalg.eigvalsh.  Also the inputs of the GPU parity test and parity_error(): e, the
largest absolute difference between the two solves over every field of every status-0 POI of those inputs; and the Cholesky pivots
of a window in exact rational arithmetic (exact_pivot_ratios), which the edge cases (tests/strain_cases.py) are placed by."""
import functools

import numpy as np

COORD_MAX = 2 ** 24
PIVOT_REL = 1e-9
FLOATS = ("disp", "G", "E", "principal", "equivalent", "rms")
PARITY_RADII = (1, 3, 7, 20, 64)
PARITY_MIN_NEIGHBOURS = 6   # under the default: the windows of radius 3 hold 4 POIs on average, radius 7 some 40
MEASURES = (0, 1)


def contributes(points, disp, valid=None):
    q = np.asarray(points, np.int64).reshape(-1, 3)
    u = np.asarray(disp, np.float64).reshape(-1, 3)
    ok = np.isfinite(u).all(1) & (np.abs(q) <= COORD_MAX).all(1)
    if valid is not None:
        ok &= np.asarray(valid).reshape(-1) != 0
    return ok


def strain_of(G, measure=0):
    """E (xx yy zz xy yz zx), its eigenvalues (descending) and the equivalent strain of a 3 x 3 gradient"""
    G = np.asarray(G, np.float64)
    E = 0.5 * (G + G.T + (G.T @ G if measure == 0 else 0.0))
    dev = E - np.trace(E) / 3.0 * np.eye(3)
    return (np.array([E[0, 0], E[1, 1], E[2, 2], E[0, 1], E[1, 2], E[2, 0]]), np.linalg.eigvalsh(E)[::-1].copy(),
            float(np.sqrt(2.0 / 3.0 * (dev * dev).sum())))


def fit(d, u, solve="normal"):
    """the plane through the neighbours' displacements u (n, 3) at the offsets d (n, 3), u[0] the lowest index's: status (0 or 4),
    disp (3,), G (3, 3), rms"""
    n = len(d)
    d = np.asarray(d, np.float64)
    a = u - u[0]
    S1, S2 = d.sum(0), d.T @ d
    C = S2 - np.outer(S1, S1) / n
    floor = PIVOT_REL * max(C[0, 0], C[1, 1], C[2, 2])
    with np.errstate(invalid="ignore", divide="ignore"):
        l00 = np.sqrt(C[0, 0]); l10 = C[0, 1] / l00; l20 = C[0, 2] / l00
        p1 = C[1, 1] - l10 * l10
        l11 = np.sqrt(p1); l21 = (C[1, 2] - l20 * l10) / l11
        p2 = (C[2, 2] - l20 * l20) - l21 * l21
    if not (C[0, 0] > floor and p1 > floor and p2 > floor):
        return 4, np.zeros(3), np.zeros((3, 3)), 0.0
    if solve == "normal":
        l22 = np.sqrt(p2)
        U, P = a.sum(0), a.T @ d
        B = P - np.outer(U, S1) / n
        G = np.zeros((3, 3))
        for c in range(3):
            y0 = B[c, 0] / l00; y1 = (B[c, 1] - l10 * y0) / l11; y2 = ((B[c, 2] - l20 * y0) - l21 * y1) / l22
            G[c, 2] = y2 / l22
            G[c, 1] = (y1 - l21 * G[c, 2]) / l11
            G[c, 0] = ((y0 - l10 * G[c, 1]) - l20 * G[c, 2]) / l00
        disp = (u[0] + U / n) - (G @ S1) / n
    else:
        coef = np.linalg.lstsq(np.concatenate([np.ones((n, 1)), d], 1), u, rcond=None)[0]
        disp, G = coef[0].copy(), coef[1:].T.copy()
    res = (u - disp) - d @ G.T
    return 0, disp, G, float(np.sqrt((res * res).sum() / (3 * n)))


def strain(points, disp, valid=None, radius=16, min_neighbours=10, measure=0, solve="normal"):
    """every POI: arrays like capi.strain's (without the seconds)"""
    q = np.asarray(points, np.int64).reshape(-1, 3)
    u = np.asarray(disp, np.float64).reshape(-1, 3)
    m = len(q)
    on = np.flatnonzero(contributes(q, u, valid))
    qn, un = q[on], u[on]
    out = {"disp": np.zeros((m, 3)), "G": np.zeros((m, 3, 3)), "E": np.zeros((m, 6)), "principal": np.zeros((m, 3)), "equivalent": np.zeros(m),
           "rms": np.zeros(m), "neighbours": np.zeros(m, np.int32), "status": np.zeros(m, np.int32)}
    for i in range(m):
        if (np.abs(q[i]) > COORD_MAX).any():
            out["status"][i] = 2
            continue
        nb = np.flatnonzero((np.abs(qn - q[i]) <= radius).all(1))   # ascending index: on is sorted
        out["neighbours"][i] = len(nb)
        if len(nb) < min_neighbours:
            out["status"][i] = 1
            continue
        st, d0, G, rms = fit(qn[nb] - q[i], un[nb], solve)
        out["status"][i] = st
        if st:
            continue
        out["disp"][i], out["G"][i], out["rms"][i] = d0, G, rms
        out["E"][i], out["principal"][i], out["equivalent"][i] = strain_of(G, measure)
    return out


def bar(e, umax):
    """the bar of every fp64 field of a case whose largest |u| is umax"""
    return max(4.0 * e, 1e-12) * max(1.0, umax)


def largest_u(disp, valid=None):
    u = np.asarray(disp, np.float64)
    u = u[np.isfinite(u)]
    return float(np.abs(u).max()) if u.size else 0.0


@functools.lru_cache(maxsize=None)
def parity_inputs():
    """about 1500 distinct integer POIs in a 60 x 50 x 40 box, a smooth field plus noise with |u| up to 10, 10 % invalid"""
    rng = np.random.default_rng(2024)
    flat = rng.choice(60 * 50 * 40, 1500, replace=False)
    q = np.stack([flat % 60, flat // 60 % 50, flat // 3000], 1).astype(np.int32)
    x, y, z = (q[:, k].astype(np.float64) for k in range(3))
    u = np.stack([6.0 * np.sin(x / 17.0) + 0.04 * y - 1.5, 5.0 * np.cos(y / 13.0 + z / 29.0) + 0.03 * x, 0.002 * x * z - 0.05 * y + 2.0], 1)
    u += rng.normal(0.0, 0.3, u.shape)
    u = np.clip(u, -10.0, 10.0)
    valid = (rng.random(len(q)) >= 0.1).astype(np.uint8)
    return q, u, valid


@functools.lru_cache(maxsize=None)
def parity_reference(radius, measure, solve="normal"):
    q, u, valid = parity_inputs()
    return strain(q, u, valid, radius=radius, min_neighbours=PARITY_MIN_NEIGHBOURS, measure=measure, solve=solve)


@functools.lru_cache(maxsize=None)
def parity_error():
    e = 0.0
    for r in PARITY_RADII:
        for ms in MEASURES:
            a, b = parity_reference(r, ms), parity_reference(r, ms, "lstsq")
            ok = a["status"] == 0
            for k in FLOATS:
                if ok.any():
                    e = max(e, float(np.abs(a[k][ok] - b[k][ok]).max()))
    return e


def exact_pivot_ratios(d):
    """the three Cholesky pivots of C = S2 - S1 S1^T / n (c00, c11 - l10^2, c22 - l20^2 - l21^2: the LDL^T pivots, which are the
    squares of L's diagonal) over C's largest diagonal entry, as fractions.Fraction from the integer offsets d (n, 3).  A pivot behind
    a zero one is 0 / 0 in the contract's arithmetic and None here; C = 0 gives (0, None, None)."""
    from fractions import Fraction

    d = [[int(v) for v in row] for row in np.asarray(d).reshape(-1, 3)]
    n = len(d)
    s1 = [sum(row[a] for row in d) for a in range(3)]
    c = [[Fraction(sum(row[a] * row[b] for row in d)) - Fraction(s1[a] * s1[b], n) for b in range(3)] for a in range(3)]
    top = max(c[0][0], c[1][1], c[2][2])
    if top == 0 or c[0][0] == 0:
        return Fraction(0), None, None
    p1 = c[1][1] - c[0][1] ** 2 / c[0][0]
    if p1 == 0:
        return c[0][0] / top, Fraction(0), None
    m12 = c[1][2] - c[0][2] * c[0][1] / c[0][0]
    p2 = c[2][2] - c[0][2] ** 2 / c[0][0] - m12 ** 2 / p1
    return c[0][0] / top, p1 / top, p2 / top


def smallest_pivot_ratio(d):
    """rho: the smallest defined entry of exact_pivot_ratios(d), as a float"""
    return float(min(p for p in exact_pivot_ratios(d) if p is not None))
