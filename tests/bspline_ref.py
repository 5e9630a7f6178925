"""NumPy restatement of the cubic B-spline contract of include/sift3d_hip.h (sift3d_bspline_prefilter, sift3d_icgn_bspline): test
infrastructure only.  The prefilter is the header's truncated, differenced FIR with a mirror boundary, in fp64 or with every product
and sum rounded to float32; the IC-GN mode is icgn_ref's algorithm run on the coefficients with the B-spline weights in place of
the Keys weights (icgn_ref is reused, not copied)."""
import numpy as np

import icgn_ref

K = 16
Z1 = np.sqrt(3.0) - 2.0


def taps():
    """h_1 .. h_K in fp64: z1^k / (1 + 2 sum z1^j)"""
    pw = Z1 ** np.arange(1, K + 1)
    return pw / (1.0 + 2.0 * pw.sum())


def mirror(i, n):
    """the whole-sample symmetric index map of period 2n - 2 (n = 1: 0)"""
    i = np.asarray(i, np.int64)
    if n == 1:
        return np.zeros_like(i)
    p = 2 * n - 2
    j = np.mod(i, p)
    return np.where(j < n, j, p - j)


def prefilter_axis(s, axis, h, ks=None):
    """one axis pass of the header's formula on s, in s's type (h in the same type): the sum over k runs over ks, K down to 1 unless
    a test hands in a deliberately wrong order or set of taps, and is added to s last"""
    n = s.shape[axis]
    i = np.arange(n)
    acc = np.zeros_like(s)
    for k in (range(K, 0, -1) if ks is None else ks):
        lo, hi = np.take(s, mirror(i - k, n), axis), np.take(s, mirror(i + k, n), axis)
        acc = acc + h[k - 1] * ((lo - s) + (hi - s))
    return s + acc


def prefilter(T, f32=False, ks=None, passes=None):
    """the coefficients of T (nz, ny, nx): x, then y, then z.  fp64 by default; f32: the intermediate volumes, every product and
    every sum are float32 (the sum over k runs from K down to 1 and is added to s last, as in the header).  ks: prefilter_axis's;
    passes: a list that receives the volume after each axis pass"""
    dt = np.float32 if f32 else np.float64
    h = taps().astype(dt)
    c = np.asarray(T, dt)
    with np.errstate(invalid="ignore", over="ignore"):
        for axis in (2, 1, 0):
            c = prefilter_axis(c, axis, h, ks)
            assert c.dtype == dt
            if passes is not None:
                passes.append(c)
    return c


def weights(t):
    """cubic B-spline weights of the taps -1, 0, 1, 2 for the fraction t: (..., 4), in t's type"""
    t2 = t * t
    t3 = t2 * t
    u = 1 - t
    return np.stack([(u * u) * u / 6, (3 * t3 - 6 * t2 + 4) / 6, (-3 * t3 + 3 * t2 + 3 * t + 1) / 6, t3 / 6], -1)


class _bspline_weights:
    """icgn_ref interpolates with the B-spline weights while this is entered"""

    def __enter__(self):
        self.keep = icgn_ref.keys_weights
        icgn_ref.keys_weights = weights

    def __exit__(self, *exc):
        icgn_ref.keys_weights = self.keep


def coefficients(T, coefficients=False):
    """what the GPU interpolates: the float32 prefilter's output as stored (T itself when it already holds coefficients)"""
    return np.asarray(T, np.float32) if coefficients else prefilter(T, f32=True)


def refine(R, T, q, init=None, coefficients_given=False, **opts):
    """icgn_ref.refine with the B-spline interpolation of T (interpolation must stay 0)"""
    if opts.get("interpolation", 0) != 0:
        raise ValueError("interpolation must be 0")
    C = coefficients(T, coefficients_given)
    with _bspline_weights():
        return icgn_ref.refine(R, C, q, init, **opts)


def icgn(R, T, points, init=None, coefficients_given=False, **opts):
    """every POI of points ((m, 3) x, y, z): arrays like capi.icgn_bspline's"""
    if opts.get("interpolation", 0) != 0:
        raise ValueError("interpolation must be 0")
    C = coefficients(T, coefficients_given)
    with _bspline_weights():
        return icgn_ref.icgn(R, C, points, init, **opts)
