"""GPU tests of the ZNCC integer search (sift3d_zncc_search) against its NumPy restatement (tests/zncc_search_ref.py): parity on
subsets of 5^3 to 33^3 voxels with the truth inside and at the edge of the search range, POIs and search windows on the borders of R
and T, flat subsets and targets, reproducibility and independence of the POIs, and the chain search -> init -> IC-GN.

The zncc bar: e = the largest |zncc(float32 restatement) - zncc(fp64 restatement)| over every scored candidate of the parity inputs,
computed on the CPU (zncc_search_ref.parity_error; tests/test_search_cpu.py prints it), and the bar is max(4 e, 1e-6).  Measured:
e = 2.50e-07, bar = 1.0e-06.  The parity inputs' best score beats every other by at least 0.05 (tests/test_search_cpu.py checks it),
which is why d is compared exactly and no POI is excluded."""
import importlib

import numpy as np
import pytest

import icgn_ref
import zncc_search_ref as ref

pytestmark = pytest.mark.gpu

capi = importlib.import_module("3dsift_amd.capi")
INT_MAX, INT_MIN = 2 ** 31 - 1, -2 ** 31
FIELDS = ("d", "status", "zncc", "zncc_second", "candidates")


@pytest.fixture(scope="module")
def bar():
    b = ref.parity_bar()
    print(f"e = {ref.parity_error():.3e}, zncc bar = {b:.3e}")
    return b


def same_bytes(a, b):
    return all(np.ascontiguousarray(a[k]).tobytes() == np.ascontiguousarray(b[k]).tobytes() for k in FIELDS)


def agree(got, want, bar):
    assert np.array_equal(got["status"], want["status"]), (got["status"], want["status"])
    assert np.array_equal(got["d"], want["d"]), (got["d"], want["d"])
    assert np.array_equal(got["candidates"], want["candidates"]), (got["candidates"], want["candidates"])
    dz = np.abs(got["zncc"] - want["zncc"]).max()
    d2 = np.abs(got["zncc_second"] - want["zncc_second"]).max()
    print(f"max |zncc - ref| = {dz:.3e}, max |zncc_second - ref| = {d2:.3e}, bar = {bar:.3e}")
    assert dz <= bar and d2 <= bar, (dz, d2, bar)


CASES = [(r, s, edge) for (r, s) in ref.PARITY for edge in ref.EDGES]


@pytest.mark.parametrize("r,s,edge", CASES, ids=[f"r{r}-s{s}-{('zero', 'plus', 'minus')[e]}" for r, s, e in CASES])
def test_parity_with_restatement(bar, r, s, edge):
    R, T, q, g, d = ref.parity_case(r, s, edge)
    want = ref.parity_reference(r, s, edge)
    got = capi.zncc_search(R, T, q, guess=g if edge else None, subset_radius=r, search_radius=s)
    assert (got["status"] == 0).all() and (got["d"] == d).all()
    agree(got, want, bar)
    assert got["seconds"] > 0


@pytest.fixture(scope="module")
def border_scene():
    # narrow dense blobs moved by whole voxels: T(x + D) = R(x) up to the blobs cut at the faces
    return ref.scene((40, 44, 48), (1.0, -1.0, 2.0), seed=31) + (np.array([1, -1, 2]),)


def margin(tab):
    v = np.sort(tab[np.isfinite(tab)])[::-1]
    return v[0] - v[1] if len(v) > 1 else 1.0


def test_borders(bar, border_scene):
    R, T, D = border_scene
    r, s = 5, 3
    nz, ny, nx = R.shape
    c = np.array([nx // 2, ny // 2, nz // 2])
    n = np.array([nx, ny, nz])
    q, g = [], []
    for ax in range(3):
        for v in (r, r - 1, n[ax] - 1 - r, n[ax] - r):  # the subset touches R's face (status 0) / leaves R by one voxel (status 2)
            p = c.copy()
            p[ax] = v
            q.append(p)
            g.append([0, 0, 0])
    # the truth is the last admissible candidate: the subset at q + D touches T's face
    for ax, v in ((0, nx - 1 - r - D[0]), (1, r - D[1]), (2, nz - 1 - r - D[2])):
        p = c.copy()
        p[ax] = v
        q.append(p)
        g.append([0, 0, 0])
    # guesses that leave no admissible candidate
    far = [[s + 2, 0, 0], [0, -(s + 2), 0], [100, 0, 0], [0, 0, -100], [INT_MAX, 0, 0], [0, INT_MIN, 0], [0, 0, INT_MAX], [2 ** 24 + 1, 0, 0],
           [INT_MIN, INT_MAX, INT_MIN]]
    q += [np.array([nx - 1 - r, c[1], c[2]]), np.array([c[0], r, c[2]])] + [c.copy() for _ in far[2:]]
    g += far
    # corners: the window hangs over two and three faces of T at once, by different amounts
    q += [np.array([r, r + 1, c[2]]), np.array([nx - 1 - r, ny - 2 - r, r + 2])]
    g += [[0, 0, 0], [0, 0, 0]]
    q, g = np.array(q, np.int32), np.array(g, np.int64).astype(np.int32)
    want = ref.search(R, T, q, g, subset_radius=r, search_radius=s, tables=True)
    assert list(want["status"][:12]) == [0, 2, 0, 2] * 3 and (want["status"][12:15] == 0).all() and (want["status"][15:24] == 3).all()
    assert (want["status"][24:] == 0).all() and [int(v) for v in want["candidates"][24:]] == [4 * 5 * 7, 4 * 5 * 6]
    assert (want["d"][12:15] == D).all() and len(set(want["candidates"][want["status"] == 0])) > 3
    got = capi.zncc_search(R, T, q, guess=g, subset_radius=r, search_radius=s)
    assert np.array_equal(got["status"], want["status"]), (got["status"], want["status"])
    assert np.array_equal(got["candidates"], want["candidates"]), (got["candidates"], want["candidates"])
    for i in np.flatnonzero(want["status"] == 0):
        tab = want["tables"][i]
        ex, ey, ez = got["d"][i] - g[i] + s
        assert np.nanmax(tab) - tab[ez, ey, ex] <= bar and abs(got["zncc"][i] - tab[ez, ey, ex]) <= bar, i
        if margin(tab) >= 0.05:  # the restatement's choice is not a matter of rounding: the same d, the same runner-up
            assert np.array_equal(got["d"][i], want["d"][i]) and abs(got["zncc_second"][i] - want["zncc_second"][i]) <= bar, i
    assert all(margin(want["tables"][i]) >= 0.05 for i in (12, 13, 14))
    fail = got["status"] != 0
    assert np.array_equal(got["d"][fail], g[fail]) and not got["zncc"][fail].any() and (got["zncc_second"][fail] == -2.0).all()
    assert not got["candidates"][fail].any()


def test_flat(border_scene):
    R, T, D = border_scene
    r, s = 4, 2
    q = np.array([[20, 22, 20]], np.int32)
    for const in (0.0, 1.0, -5.5, 3e7):
        flat = capi.zncc_search(np.full_like(R, const), T, q, subset_radius=r, search_radius=s)
        assert (flat["status"][0], flat["candidates"][0], flat["zncc"][0], list(flat["d"][0])) == (4, 0, 0.0, [0, 0, 0])
        for g in ([0, 0, 0], [3, -2, 1]):
            Tc = T.copy()
            w = r + s
            Tc[20 + g[2] - w:20 + g[2] + w + 1, 22 + g[1] - w:22 + g[1] + w + 1, 20 + g[0] - w:20 + g[0] + w + 1] = const  # the search region
            got = capi.zncc_search(R, Tc, q, guess=[g], subset_radius=r, search_radius=s)
            assert (got["status"][0], got["candidates"][0], got["zncc"][0], list(got["d"][0])) == (3, 0, 0.0, g), const
    # one voxel off the constant, in the region's corner: the one candidate that sees it is scored
    Tc = T.copy()
    Tc[20 - w:20 + w + 1, 22 - w:22 + w + 1, 20 - w:20 + w + 1] = 1.0
    Tc[20 - w, 22 - w, 20 - w] = 2.0
    got = capi.zncc_search(R, Tc, q, subset_radius=r, search_radius=s)
    assert (got["status"][0], got["candidates"][0]) == (0, 1)


def test_reproducible_and_independent(bar):
    import torch

    r, s = 5, 7
    R, T, q, g, d = ref.parity_case(r, s, 1)
    a = capi.zncc_search(R, T, q, guess=g, subset_radius=r, search_radius=s)
    b = capi.zncc_search(R, T, q, guess=g, subset_radius=r, search_radius=s)
    assert same_bytes(a, b)
    perm = np.random.default_rng(4).permutation(len(q))
    p = capi.zncc_search(R, T, q[perm], guess=g[perm], subset_radius=r, search_radius=s)
    assert same_bytes(p, {k: a[k][perm] for k in FIELDS})
    one = capi.zncc_search(R, T, q[5:6], guess=g[5:6], subset_radius=r, search_radius=s)
    assert same_bytes(one, {k: a[k][5:6] for k in FIELDS})
    dev = capi.zncc_search(torch.from_numpy(R).cuda(), torch.from_numpy(T).cuda(), torch.from_numpy(q).cuda(), guess=torch.from_numpy(g).cuda(),
                           subset_radius=r, search_radius=s)
    assert same_bytes(a, dev)
    empty = capi.zncc_search(R, T, np.zeros((0, 3), np.int32))
    assert empty["d"].shape == (0, 3) and empty["status"].shape == (0,)
    # a target of period 6 <= s along x: several candidates carry the best score up to rounding
    blk = ref.scene((40, 40, 6), (0.0, 0.0, 0.0), seed=41)[0]
    P = np.tile(blk, (1, 1, 8))
    qp = np.array([[24, 20, 20], [23, 17, 22]], np.int32)
    got = capi.zncc_search(P, P, qp, subset_radius=r, search_radius=s)
    again = capi.zncc_search(P, P, qp, subset_radius=r, search_radius=s)
    assert same_bytes(got, again) and (got["status"] == 0).all()
    want = ref.search(P, P, qp, subset_radius=r, search_radius=s, tables=True)
    for i, tab in enumerate(want["tables"]):
        ex, ey, ez = got["d"][i] + s
        assert np.nanmax(tab) - tab[ez, ey, ex] <= bar and abs(got["zncc"][i] - tab[ez, ey, ex]) <= bar
        assert got["d"][i][0] % 6 == 0 and got["d"][i][1] == 0 and got["d"][i][2] == 0
    assert np.array_equal(got["candidates"], want["candidates"])


def test_end_to_end():
    move = np.array([6.37, -5.52, 4.21])
    R, T, truth = icgn_ref.scene((72, 72, 72), tvec=move, seed=5)
    gr = np.arange(24, 49, 8)
    q = np.stack(np.meshgrid(gr, gr, gr, indexing="ij"), -1).reshape(-1, 3).astype(np.int32)[::2]  # 32 POIs
    tr = truth(q)
    rng = np.random.default_rng(8)
    init = tr + np.where(np.arange(12) % 4 == 0, rng.uniform(-0.3, 0.3, tr.shape), rng.uniform(-0.005, 0.005, tr.shape))
    init[::2] = np.nan  # half of the POIs have no fit
    res = capi.zncc_search(R, T, q[::2], subset_radius=8, search_radius=8)
    assert (res["status"] == 0).all() and np.abs(res["d"] - move).max() < 1.0, res["d"]
    full = {"d": np.zeros((len(q), 3), np.int32), "status": np.full(len(q), 3, np.int32)}
    full["d"][::2], full["status"][::2] = res["d"], res["status"]
    start = capi.icgn_init_from_search(full, init, only_missing=True)
    assert np.array_equal(start[1::2].view(np.uint64), init[1::2].view(np.uint64)) and np.isfinite(start).all()
    got = capi.icgn(R, T, q, init=start, subset_radius=8)
    assert (got["status"] == 0).all(), got["status"]
    err = np.abs(got["displacement"] - move).max()
    print(f"max displacement error {err:.4f}")
    assert err <= 0.02, err
