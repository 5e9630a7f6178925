"""GPU tests of what the one-shot entry points share (3dsift_amd/csrc/call_state.h), the same for all six: sift3d_match,
sift3d_fit_affine, sift3d_fit_affine_local, sift3d_icgn, sift3d_zncc_search and sift3d_strain.  The grow-only blocks are outgrown and
reused, the families interleave, host arrays and device tensors give the same bits with every optional table present and absent, the
device seconds are positive for a call that launched and exactly 0 for one that did not, and a bad device index is refused with its
text.  What the calls compute is the business of each family's own module; here every result is compared with another result of the
same call, bit for bit (floats by their bytes, so a NaN equals itself).

Sizes of the grow-and-reuse calls (a block grows to want + want / 4 + 4096 bytes, so after a call with 7 rows a family's pinned block
holds at most 1.25 x the figure below + 4096 bytes, and the call with 5000 rows needs more than that; the device scratch holds the same
results and more):
  fit_affine        256 + al256(n) mask bytes:     512 -> capacity 4736;   n = 5000 needs 5376
  fit_affine_local  al256(224 m) + 4 m k, k = 4:   1904 -> capacity 6476;  m = 5000 needs 1 200 000
  icgn              128 m:                         896 -> capacity 5216;   m = 5000 needs 640 000
  zncc_search       48 m:                          336 -> capacity 4516;   m = 5000 needs 240 000
  match             al256(16 max(n, m)) + 256:     512 -> capacity 4736;   700 x 900 needs 14 848
  strain            keeps no block: its temporaries live for one call
The two fits share one state, and a module that ran earlier in the same process may have left larger blocks behind: the first test
outgrows them for certain only where it runs first, as it does when this module runs alone."""
import importlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

capi = importlib.import_module("3dsift_amd.capi")
C = capi.C
RNG = np.random.default_rng(20261018)
REF = RNG.random((20, 20, 20), dtype=np.float32)
TAR = (np.roll(REF, 1, axis=2) + 0.01 * RNG.random((20, 20, 20), dtype=np.float32)).astype(np.float32)
DESC_A = RNG.random((700, 768), dtype=np.float32)
DESC_B = RNG.random((900, 768), dtype=np.float32)
XYZ_A = (RNG.random((700, 3)) * 64).astype(np.float32)
XYZ_B = (RNG.random((900, 3)) * 64).astype(np.float32)


def pois(m):
    """m points of the 20^3 volumes, far enough inside for subset_radius 2 and a search radius of 1"""
    return np.random.default_rng(m).integers(6, 14, (m, 3)).astype(np.int32)


def pairs(n):
    """n matched pairs of an affine map, a fifth of them outliers"""
    g = np.random.default_rng(100 + n)
    r = g.random((n, 3)) * 60
    t = r @ np.array([[1.02, 0.01, 0.0], [-0.01, 0.99, 0.02], [0.0, 0.01, 1.01]]).T + np.array([1.5, -2.0, 0.5])
    t[::5] += g.random((len(t[::5]), 3)) * 20
    return np.concatenate([r, t], 1).astype(np.float32)


def cloud(m):
    """m POIs with a displacement each"""
    g = np.random.default_rng(200 + m)
    q = g.integers(0, 40, (m, 3)).astype(np.int32)
    return q, q @ np.full((3, 3), 0.01) + g.random((m, 3)) * 1e-3


def dev(a):
    import torch

    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def match(n, m, on_device=False):
    M = capi.muBruteMatcher()
    if on_device:
        t = [dev(a) for a in (DESC_A[:n], XYZ_A[:n], DESC_B[:m], XYZ_B[:m])]
        r = dict(M.enhancedMatch(*(v.data_ptr() for v in t), 0.95, on_device=True, n=n, m=m))
    else:
        r = dict(M.enhancedMatch(DESC_A[:n], XYZ_A[:n], DESC_B[:m], XYZ_B[:m], 0.95))
    r["seconds"] = M.totalTime
    return r


# family -> the call at size m (the matcher: m x (m + 2) for 7, 64 x 80 and 700 x 900 otherwise), on host arrays or device tensors
def _size(m):
    return (7, 9) if m == 7 else (64, 80) if m == 64 else (700, 900)


CALLS = {
    "match": lambda m, f: match(*_size(m), on_device=f is dev),
    "fit_affine": lambda m, f: capi.fit_affine(f(pairs(m))),
    "fit_affine_local": lambda m, f: capi.fit_affine_local(f(pairs(m)), f(pois(m).astype(np.float32) * 4), k=4),
    "icgn": lambda m, f: capi.icgn(f(REF), f(TAR), f(pois(m)), subset_radius=2),
    "zncc_search": lambda m, f: capi.zncc_search(f(REF), f(TAR), f(pois(m)), subset_radius=2, search_radius=1),
    "strain": lambda m, f: capi.strain(*(f(a) for a in cloud(m)), radius=8, min_neighbours=4),
}


def host(a):
    return a


def same(a, b):
    """every field but the seconds, bit for bit"""
    assert a.keys() == b.keys()
    for k in a:
        if k != "seconds":
            x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
            assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), k


@pytest.mark.parametrize("family", list(CALLS))
def test_grow_and_reuse(family):
    first = CALLS[family](7, host)
    large = CALLS[family](5000, host)
    again = CALLS[family](7, host)
    same(again, first)
    assert all(np.isfinite(r["seconds"]) and r["seconds"] > 0 for r in (first, large, again))


def test_interleaved_families():
    first = {k: call(7 if k != "match" else 64, host) for k, call in CALLS.items()}
    for _ in range(2):
        for k, call in CALLS.items():
            same(call(7 if k != "match" else 64, host), first[k])


@pytest.mark.parametrize("family", list(CALLS))
def test_host_and_device_inputs_agree(family):
    m = 64 if family == "match" else 7
    h, d = CALLS[family](m, host), CALLS[family](m, dev)
    same(d, h)
    assert np.isfinite(d["seconds"]) and d["seconds"] > 0 and np.isfinite(h["seconds"]) and h["seconds"] > 0


@pytest.mark.parametrize("f", [host, dev], ids=["host", "device"])
def test_optional_tables_present_and_absent(f):
    q = pois(7)
    init = np.zeros((7, 12))
    init[:, 0] = 1.0
    guess = np.tile(np.array([1, 0, 0], np.int32), (7, 1))
    # IC-GN: no init is a zero init; the search: no guess is a zero guess; strain: no valid is all valid
    same(capi.icgn(f(REF), f(TAR), f(q), init=None, subset_radius=2), capi.icgn(f(REF), f(TAR), f(q), init=f(np.zeros((7, 12))), subset_radius=2))
    a, b = capi.icgn(f(REF), f(TAR), f(q), init=f(init), subset_radius=2), capi.icgn(REF, TAR, q, init=init, subset_radius=2)
    same(a, b)
    kw = dict(subset_radius=2, search_radius=1)
    same(capi.zncc_search(f(REF), f(TAR), f(q), guess=None, **kw), capi.zncc_search(f(REF), f(TAR), f(q), guess=f(np.zeros((7, 3), np.int32)), **kw))
    same(capi.zncc_search(f(REF), f(TAR), f(q), guess=f(guess), **kw), capi.zncc_search(REF, TAR, q, guess=guess, **kw))
    p, u = cloud(7)
    valid = np.array([1, 1, 0, 1, 1, 1, 1], np.uint8)
    same(capi.strain(f(p), f(u), None, radius=8, min_neighbours=4), capi.strain(f(p), f(u), f(np.ones(7, np.uint8)), radius=8, min_neighbours=4))
    same(capi.strain(f(p), f(u), f(valid), radius=8, min_neighbours=4), capi.strain(p, u, valid, radius=8, min_neighbours=4))
    # the fits: without the mask / the neighbour table (the binding always asks for them) the fit records are the same bytes
    L, o, sec = capi.lib(), capi._ransac_options({}), C.c_double(0)
    pr, pt = f(pairs(7)), f(pois(7).astype(np.float32) * 4)
    pp, n, keep_p, on_dev = capi._rows(pr, 6, "pairs")
    qp, m, keep_q, _ = capi._rows(pt, 3, "points")
    want, out = capi.fit_affine(pr), np.zeros(1, capi.FIT_DTYPE)
    capi._check(L.sift3d_fit_affine(pp, n, C.byref(o), on_dev, 0, out.ctypes.data_as(C.c_void_p), None, C.byref(sec)))
    assert sec.value > 0
    for k in capi.FIT_FIELDS:
        assert out[k].tobytes() == np.asarray(want[k], out[k].dtype).tobytes(), k
    want, out = capi.fit_affine_local(pr, pt, k=4), np.zeros(7, capi.FIT_DTYPE)
    capi._check(L.sift3d_fit_affine_local(pp, n, qp, m, 4, 0.0, C.byref(o), on_dev, 0, out.ctypes.data_as(C.c_void_p), None, C.byref(sec)))
    assert sec.value > 0
    for k in capi.FIT_FIELDS:
        assert out[k].tobytes() == np.ascontiguousarray(want[k]).tobytes(), k


def test_no_launch_gives_zero_seconds():
    none3, none6 = np.zeros((0, 3), np.int32), np.zeros((0, 6), np.float32)
    r = capi.fit_affine(pairs(3))
    assert r["seconds"] == 0 and r["status"] == 1 and r["candidates"] == 3
    assert capi.fit_affine_local(pairs(7), none3.astype(np.float32), k=4)["seconds"] == 0
    assert capi.fit_affine(none6)["seconds"] == 0
    assert capi.icgn(REF, TAR, none3, subset_radius=2)["seconds"] == 0
    assert capi.zncc_search(REF, TAR, none3, subset_radius=2, search_radius=1)["seconds"] == 0
    assert capi.strain(none3, np.zeros((0, 3)))["seconds"] == 0


def test_bad_device_index():
    nd = capi.device_count()
    q, (p, u) = pois(7), cloud(7)
    calls = {
        "match": lambda: capi.muBruteMatcher(device=nd).enhancedMatch(DESC_A[:7], XYZ_A[:7], DESC_B[:9], XYZ_B[:9]),
        "fit_affine": lambda: capi.fit_affine(pairs(7), device=nd),
        "fit_affine_local": lambda: capi.fit_affine_local(pairs(7), q.astype(np.float32), k=4, device=nd),
        "icgn": lambda: capi.icgn(REF, TAR, q, device=nd, subset_radius=2),
        "zncc_search": lambda: capi.zncc_search(REF, TAR, q, device=nd, subset_radius=2, search_radius=1),
        "strain": lambda: capi.strain(p, u, device=nd),
    }
    assert calls.keys() == CALLS.keys()
    for call in calls.values():
        with pytest.raises(capi.Sift3dError, match="bad device index"):
            call()
    assert capi.lib().sift3d_match_warmup(nd) != 0 and b"bad device index" in capi.lib().sift3d_last_error()
