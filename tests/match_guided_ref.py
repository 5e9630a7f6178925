"""The restatement of sift3d_match_guided (include/sift3d_hip.h) that the tests compare the GPU with.  Plain NumPy + the CPU oracle.

  in_range(xyz)                         the positions a gate can hold: three finite coordinates within +-2^24
  gate(tar_xyz, pred_xyz, radius)       the (n, m) relation "target j is in the gate of row i", in float32 as the contract writes it
  match_guided(orc, a, ax, b, bx, pred, radius, thresh, mode)

The forward and the reverse rows come from the CPU oracle's own matcher -- orc.match in mode 1 on the gated columns, the indices
mapped back -- so no sum is re-derived here; the bookkeeping (ratio filter, count / mask, bijection, pairs: reference
Src/cMatcher.cc:81-144) is restated in Python.
"""
import numpy as np

F32 = np.float32
FLT_MIN = float(np.finfo(np.float32).tiny)
EMPTY_D = F32(2 - 2 * FLT_MIN)   # the distance an empty place holds (2.0f)
COORD_MAX = F32(2.0 ** 24)
# orc.match filters by (double)(gd / sd) >= thresh * thresh, an IEEE comparison (the oracle is built without fast-math): with a NaN
# threshold it is false for every row, so the indices come back as the scan left them.
NO_FILTER = float("nan")


def in_range(xyz):
    xyz = np.asarray(xyz, F32).reshape(-1, 3)
    with np.errstate(invalid="ignore"):
        return (np.abs(xyz) <= COORD_MAX).all(1)   # False for NaN and +-inf


def gate(tar_xyz, pred_xyz, radius):
    tar = np.asarray(tar_xyz, F32).reshape(-1, 3)
    pred = np.asarray(pred_xyz, F32).reshape(-1, 3)
    r = F32(radius)
    g = np.outer(in_range(pred), in_range(tar))
    with np.errstate(invalid="ignore", over="ignore"):
        for c in range(3):
            d = tar[None, :, c] - pred[:, None, c]   # float32: one rounded subtraction
            assert d.dtype == F32
            g &= np.abs(d) <= r
    return g


def _rows(orc, a, b, rows, cols_of):
    """best / second best of the listed rows of a over the columns cols_of(row) of b (ascending): calMatches by the oracle"""
    n = len(a)
    gi = np.full(n, -1, np.int32); si = np.full(n, -1, np.int32)
    gd = np.full(n, EMPTY_D, F32); sd = np.full(n, EMPTY_D, F32)
    z1 = np.zeros((1, 3), F32)
    for i in rows:
        cols = cols_of(i)
        if not len(cols):
            continue
        w = orc.match(a[i:i + 1], z1, b[cols], np.zeros((len(cols), 3), F32), NO_FILTER, 1)
        g, s = int(w["gIdx"][0]), int(w["sIdx"][0])
        gi[i] = cols[g] if g >= 0 else -1
        si[i] = cols[s] if s >= 0 else -1
        gd[i], sd[i] = w["gDist"][0], w["sDist"][0]
    return gi, si, gd, sd


def ratio_filter(gi, gd, sd, thresh):
    """filter, Src/cMatcher.cc:81-97: a float division, compared as a double; a rejected index is negated (0 stays 0)"""
    with np.errstate(all="ignore"):
        ratio = gd / sd
    assert ratio.dtype == F32
    ratio = ratio.astype(np.float64)
    flip = (gi >= 0) & (ratio >= thresh * thresh)
    return np.where(flip, -gi, gi).astype(np.int32)


def match_guided(orc, a, ax, b, bx, pred, radius, thresh=0.85, mode=3, forward=None):
    """forward: the (gi, si, gd, sd) of an earlier call on the same inputs (it does not depend on thresh and mode)"""
    a = np.ascontiguousarray(a, F32); b = np.ascontiguousarray(b, F32)
    ax = np.asarray(ax, F32).reshape(-1, 3); bx = np.asarray(bx, F32).reshape(-1, 3)
    n, m = len(a), len(b)
    G = gate(bx, pred, radius)
    if forward is None:
        forward = _rows(orc, a, b, range(n), lambda i: np.flatnonzero(G[i]))
    gi, si, gd, sd = (v.copy() for v in forward)
    raw = (gi.copy(), si.copy(), gd.copy(), sd.copy())
    gi = ratio_filter(gi, gd, sd, thresh)
    if mode != 1:
        cnt = np.bincount(gi[gi >= 0], minlength=m)                     # countMatched :114-120
        mask = cnt > (0 if mode == 2 else 1)                            # toMask :122-131
        gi2, _, gd2, sd2 = _rows(orc, b, a, np.flatnonzero(mask), lambda j: np.flatnonzero(G[:, j]))
        gd2[~mask] = 0; sd2[~mask] = 0                                  # masked-out targets are never scanned
        gi2 = ratio_filter(gi2, gd2, sd2, thresh)
        for i in range(n):                                              # bijectFilter :133-144
            j = gi[i]
            if j < 0 or not mask[j]:
                continue
            if gi2[j] != i:
                gi[i] *= -1
    keep = np.flatnonzero(gi >= 0)                                      # toCvec :99-112
    pairs = np.concatenate([ax[keep], bx[gi[keep]]], 1).astype(F32) if len(keep) else np.zeros((0, 6), F32)
    return dict(gIdx=gi, sIdx=si, gDist=gd, sDist=sd, candidates=G.sum(1).astype(np.int32), pairs=pairs, forward=raw)
