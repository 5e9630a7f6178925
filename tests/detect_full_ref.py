"""CPU restatement of the opt-in detection rules of sift3d_set_detect_options (include/sift3d_hip.h), for the tests of
tests/test_gpu_detect_full.py: the 8- and 80-neighbour extremum tests on DoG levels (NumPy), and the sub-voxel quadratic fit with its
rejection tests in plain Python floats (IEEE fp64, no fused multiply-add) -- the arithmetic of quad_fit / fit_accepts / k_refine in
3dsift_amd/csrc/kernels_detect_full.hip, operation for operation, so that decisions and values agree bit for bit."""
import numpy as np

# 26 in-level offsets (dz, dy, dx), then the 27 of the levels below and above
_OFFS27 = [(dz, dy, dx) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]
_OFFS26 = [o for o in _OFFS27 if o != (0, 0, 0)]
_OFFS8 = [(0, 0, 1), (0, 0, -1), (0, 1, 0), (0, -1, 0), (1, 0, 0), (-1, 0, 0)]


def _shift(a, dz, dy, dx):
    nz, ny, nx = a.shape
    return a[1 + dz:nz - 1 + dz, 1 + dy:ny - 1 + dy, 1 + dx:nx - 1 + dx]


def level_absmax(cur):
    """max|level| by the reference's comparison `fabs(v) > max ? fabs(v) : max` (Src/cUtil.cc:548): a NaN never wins, an all-NaN level gives 0"""
    return np.float32(np.fmax.reduce(np.abs(np.asarray(cur, np.float32)).ravel(), initial=np.float32(0.0)))


def level_threshold(cur, peak_thresh):
    """peak_thresh * max|level|: the fp32 product the detection kernels form"""
    return np.float32(peak_thresh) * level_absmax(cur)


def extrema_mask(prev, cur, nxt, peak_thresh, neighbours):
    """bool [nz-2, ny-2, nx-2] of the interior voxels of `cur` that are extrema under the 8- or 80-neighbour rule"""
    c = cur[1:-1, 1:-1, 1:-1]
    cand = np.abs(c) > level_threshold(cur, peak_thresh)
    mx = cand.copy()
    mn = cand.copy()
    if neighbours == 80:
        nbs = [(cur, o) for o in _OFFS26] + [(prev, o) for o in _OFFS27] + [(nxt, o) for o in _OFFS27]
    else:
        nbs = [(cur, o) for o in _OFFS8] + [(prev, (0, 0, 0)), (nxt, (0, 0, 0))]
    for lvl, (dz, dy, dx) in nbs:
        w = _shift(lvl, dz, dy, dx)
        mx &= c > w
        mn &= c < w
    return mx | mn


def extrema_table(dogs, peak_thresh, neighbours):
    """dogs[o][i]: DoG level i of octave o ([z, y, x] float32).  Rows (octave, level, x, y, z) in emit order (octave, level, z, y, x)."""
    rows = []
    for o, D in enumerate(dogs):
        for lv in range(1, len(D) - 1):
            if min(D[lv].shape) < 3:
                continue
            z, y, x = np.nonzero(extrema_mask(D[lv - 1], D[lv], D[lv + 1], peak_thresh, neighbours))
            for k in range(len(z)):
                rows.append((o, lv, int(x[k]) + 1, int(y[k]) + 1, int(z[k]) + 1))
    return np.array(rows, np.int64).reshape(-1, 5)


def quad_fit(prev, cur, nxt, x, y, z):
    """(ok, d[4], contrast, Hs) exactly as quad_fit of kernels_detect_full.hip (axis order x, y, z, s)"""
    offs = [(0, 0, 1), (0, 1, 0), (1, 0, 0)]  # (dz, dy, dx) of the axes x, y, z

    def at(lvl, *os):
        dz = sum(o[0] for o in os)
        dy = sum(o[1] for o in os)
        dx = sum(o[2] for o in os)
        return float(lvl[z + dz, y + dy, x + dx])

    def neg(o):
        return (-o[0], -o[1], -o[2])

    D0 = float(cur[z, y, x])
    g = [0.0] * 4
    H = [[0.0] * 4 for _ in range(4)]
    for a in range(3):
        dp, dm = at(cur, offs[a]), at(cur, neg(offs[a]))
        g[a] = 0.5 * (dp - dm)
        H[a][a] = (dp + dm) - 2.0 * D0
    dp, dm = float(nxt[z, y, x]), float(prev[z, y, x])
    g[3] = 0.5 * (dp - dm)
    H[3][3] = (dp + dm) - 2.0 * D0
    for a in range(3):
        for b in range(a + 1, 3):
            app = at(cur, offs[a], offs[b])
            apm = at(cur, offs[a], neg(offs[b]))
            amp = at(cur, neg(offs[a]), offs[b])
            amm = at(cur, neg(offs[a]), neg(offs[b]))
            H[a][b] = H[b][a] = 0.25 * (((app - apm) - amp) + amm)
    for a in range(3):
        app, apm = at(nxt, offs[a]), at(prev, offs[a])
        amp, amm = at(nxt, neg(offs[a])), at(prev, neg(offs[a]))
        H[a][3] = H[3][a] = 0.25 * (((app - apm) - amp) + amm)
    A = [H[r][:] + [-g[r]] for r in range(4)]
    for k in range(4):
        p = k
        for r in range(k + 1, 4):
            if abs(A[r][k]) > abs(A[p][k]):
                p = r
        if p != k:
            A[k], A[p] = A[p], A[k]
        if A[k][k] == 0.0:
            return False, None, None, None
        for r in range(k + 1, 4):
            f = A[r][k] / A[k][k]
            for cc in range(k, 5):
                A[r][cc] = A[r][cc] - f * A[k][cc]
    d = [0.0] * 4
    for k in range(3, -1, -1):
        s = A[k][4]
        for cc in range(k + 1, 4):
            s = s - A[k][cc] * d[cc]
        d[k] = s / A[k][k]
    contrast = D0 + 0.5 * (((g[0] * d[0] + g[1] * d[1]) + g[2] * d[2]) + g[3] * d[3])
    return True, d, contrast, [row[:3] for row in H[:3]]


def fit_accepts(d, contrast, Hs, absmax, max_offset=0.5, contrast_thresh=0.0, edge_ratio=0.0):
    """fit_accepts of kernels_detect_full.hip; absmax = max|level| (fp32)"""
    mo, ct, er = np.float32(max_offset), np.float32(contrast_thresh), np.float32(edge_ratio)
    if mo > 0:
        if any(abs(v) > float(mo) for v in d):
            return False
    if ct > 0:
        thr = float(ct * np.float32(absmax))
        if abs(contrast) < thr:
            return False
    if er > 0:
        tr = (Hs[0][0] + Hs[1][1]) + Hs[2][2]
        det = (Hs[0][0] * (Hs[1][1] * Hs[2][2] - Hs[1][2] * Hs[2][1]) - Hs[0][1] * (Hs[1][0] * Hs[2][2] - Hs[1][2] * Hs[2][0])) + \
            Hs[0][2] * (Hs[1][0] * Hs[2][1] - Hs[1][1] * Hs[2][0])
        r = float(er)
        q = 2.0 * r + 1.0
        lim = ((q * q) * q) / (r * r)
        if not (tr * det > 0.0 and ((tr * tr) * tr) / det < lim):
            return False
    return True


def refined_table(dogs, rows, peak_thresh, neighbours, opts):
    """the rows of extrema_table(dogs, peak_thresh, neighbours) that the fit accepts (the extrema of a refining run)"""
    keep = []
    for r in rows:
        o, lv, x, y, z = (int(v) for v in r)
        D = dogs[o]
        ok, d, contrast, Hs = quad_fit(D[lv - 1], D[lv], D[lv + 1], x, y, z)
        if ok and fit_accepts(d, contrast, Hs, level_absmax(D[lv]), **opts):
            keep.append(r)
    return np.array(keep, np.int64).reshape(-1, 5)


def refined_record(dogs, kp, num_kp_levels):
    """(rx, ry, rz, scale, dx, dy, dz, ds, contrast) as float32, k_refine's arithmetic, for one keypoint record"""
    o, lv, x, y, z = int(kp["octave"]), int(kp["level"]), int(kp["x"]), int(kp["y"]), int(kp["z"])
    D = dogs[o]
    ok, d, contrast, _ = quad_fit(D[lv - 1], D[lv], D[lv + 1], x, y, z)
    assert ok
    f = float(1 << o)
    vals = [(float(x) + d[0]) * f, (float(y) + d[1]) * f, (float(z) + d[2]) * f,
            float(kp["scale"]) * 2.0 ** (d[3] / float(num_kp_levels)), d[0], d[1], d[2], d[3], contrast]
    return np.array(vals, np.float64).astype(np.float32)
