"""GPU tests of the strain fields (sift3d_strain) against their NumPy restatement (tests/strain_ref.py): parity on scattered POIs from
windows of 3^3 voxels to one that holds every POI, a known affine field and a constant one, the window's edge across cell borders,
every status, a crowded cell and grids the cell cap must coarsen, device pointers, repeatability, and the chain IC-GN -> strain.

The bar of every fp64 field: max(4 e, 1e-12) x max(1, the largest |u| of the case), e = the largest absolute difference between the
restatement's two solves (normal equations as the header writes them / numpy.linalg.lstsq) over every field of every status-0 POI of
the parity inputs, computed on the CPU (strain_ref.parity_error; tests/test_strain_cpu.py prints it).  Measured: e = 4.35e-14, so the
bar is 1e-12 x max(1, max |u|): 7.2e-12 on the parity inputs.  status and neighbours are compared exactly and no POI is excluded."""
import importlib

import numpy as np
import pytest

import icgn_ref
import strain_ref as ref

pytestmark = pytest.mark.gpu

capi = importlib.import_module("3dsift_amd.capi")
FIELDS = ref.FLOATS + ("neighbours", "status")
G0 = np.array([[0.010, -0.004, 0.002], [0.003, -0.020, 0.001], [-0.002, 0.005, 0.015]])
B0 = np.array([1.25, -2.5, 0.75])


@pytest.fixture(scope="module")
def e():
    v = ref.parity_error()
    print(f"e = {v:.3e}")
    return v


def same_bytes(a, b):
    return all(np.ascontiguousarray(a[k]).tobytes() == np.ascontiguousarray(b[k]).tobytes() for k in FIELDS)


def agree(got, want, bar):
    assert np.array_equal(got["status"], want["status"]), (got["status"], want["status"])
    assert np.array_equal(got["neighbours"], want["neighbours"]), (got["neighbours"], want["neighbours"])
    worst = {k: float(np.abs(got[k] - want[k]).max()) if len(want[k]) else 0.0 for k in ref.FLOATS}
    print("max |got - ref|: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()) + f"; bar {bar:.2e}")
    assert all(np.isfinite(got[k]).all() for k in ref.FLOATS)
    assert max(worst.values()) <= bar, (worst, bar)
    failed = got["status"] != 0
    assert not any(got[k][failed].any() for k in ref.FLOATS)


def check(e, q, u, valid=None, **opts):
    """the call against the restatement on the same input, within the case's bar"""
    got = capi.strain(q, u, valid, **opts)
    want = ref.strain(q, u, valid, **opts)
    agree(got, want, ref.bar(e, ref.largest_u(u)))
    return got


CASES = [(r, ms) for r in ref.PARITY_RADII for ms in ref.MEASURES]


@pytest.mark.parametrize("radius,measure", CASES, ids=[f"r{r}-{('green', 'small')[ms]}" for r, ms in CASES])
def test_parity_with_restatement(e, radius, measure):
    q, u, valid = ref.parity_inputs()
    got = capi.strain(q, u, valid, radius=radius, min_neighbours=ref.PARITY_MIN_NEIGHBOURS, measure=measure)
    agree(got, ref.parity_reference(radius, measure), ref.bar(e, ref.largest_u(u)))
    assert got["seconds"] > 0


def affine_grid():
    g = [np.arange(n) * 3 for n in (9, 8, 7)]
    q = np.stack(np.meshgrid(*g, indexing="ij"), -1).reshape(-1, 3).astype(np.int32)
    return q, q @ G0.T + B0


def test_affine_and_constant_field(e):
    q, u = affine_grid()
    bar = ref.bar(e, ref.largest_u(u))
    for measure in ref.MEASURES:
        got = check(e, q, u, radius=6, measure=measure)
        E, pr, eq = ref.strain_of(G0, measure)
        assert (got["status"] == 0).all() and got["neighbours"].min() == 27 and got["neighbours"].max() == 125
        assert np.abs(got["G"] - G0).max() <= bar and np.abs(got["E"] - E).max() <= bar and np.abs(got["disp"] - u).max() <= bar
        assert np.abs(got["principal"] - pr).max() <= bar and np.abs(got["equivalent"] - eq).max() <= bar and got["rms"].max() <= bar
    const = capi.strain(q, np.tile(B0, (len(q), 1)), radius=6)
    assert (const["status"] == 0).all()
    assert not const["G"].any() and not const["E"].any() and not const["rms"].any() and not const["principal"].any()
    assert not const["equivalent"].any() and (const["disp"] == B0).all()


def test_window_edge_across_cell_borders(e):
    """stars: a centre, and on each axis and side one POI at distance r (counted) and one at r + 1 (not counted).  The cells have side
    r from the box's lowest corner, and the stars sit at every offset 0 .. r - 1 from it on each axis, so the two POIs of a side fall
    into the same cell, into neighbouring cells and across the last cell the window touches.  POIs at the eight corners of the box."""
    r = 5
    q = []
    for k in range(r):
        c = np.array([20 + 40 * k + k, 20 + (2 * k) % r, 20 + (3 * k) % r])
        q.append(c)
        for ax in range(3):
            for sg in (-1, 1):
                for dist in (r, r + 1):
                    p = c.copy()
                    p[ax] += sg * dist
                    q.append(p)
    q = np.array(q)
    lo, hi = q.min(0) - 3, q.max(0) + 3
    corners = np.array([[(lo, hi)[b][a] for a, b in enumerate(bits)] for bits in np.ndindex(2, 2, 2)])
    q = np.concatenate([q, corners]).astype(np.int32)
    rng = np.random.default_rng(3)
    u = q @ G0.T + rng.normal(0, 0.01, (len(q), 3))
    got = check(e, q, u, radius=r, min_neighbours=4)
    centres = np.arange(r) * 13
    assert (got["neighbours"][centres] == 7).all() and (got["status"][centres] == 0).all()
    assert (got["neighbours"][-8:] == 1).all() and (got["status"][-8:] == 1).all()
    # the same stars around a centre that does not contribute: its window is the same, it is not counted
    valid = np.ones(len(q), np.uint8)
    valid[centres] = 0
    got = check(e, q, u, valid, radius=r, min_neighbours=4)
    assert (got["neighbours"][centres] == 6).all() and (got["status"][centres] == 0).all()


def test_statuses(e):
    q, u = affine_grid()
    u = u + np.random.default_rng(9).normal(0, 0.01, u.shape)
    # n = min_neighbours - 1 and n = min_neighbours: the corner of the grid sees 27 POIs at radius 6
    for mn, st in ((27, 0), (28, 1)):
        got = check(e, q, u, radius=6, min_neighbours=mn)
        assert (got["status"][0], got["neighbours"][0]) == (st, 27)
    # coplanar and collinear neighbours
    plane = q[:, 2] == 6
    got = check(e, q[plane], u[plane], radius=6, min_neighbours=4)
    assert (got["status"] == 4).all() and got["neighbours"].min() == 9
    line = plane & (q[:, 1] == 3)
    got = check(e, q[line], u[line], radius=30, min_neighbours=4)
    assert (got["status"] == 4).all() and (got["neighbours"] == 9).all()
    # an invalid centre is fitted from its neighbours; a NaN or infinite displacement is ignored whatever its byte says
    mid = int(np.flatnonzero((q == (12, 12, 9)).all(1))[0])
    valid = np.ones(len(q), np.uint8)
    valid[mid] = 0
    holes = u.copy()
    holes[mid + 1, 1] = np.nan
    holes[mid - 1, 2] = -np.inf
    got = check(e, q, holes, valid, radius=6)
    assert (got["status"][mid], got["neighbours"][mid]) == (0, 122) and (got["status"][[mid - 1, mid + 1]] == 0).all()
    # a coordinate past 2^24: status 2, and never a neighbour
    far = np.concatenate([q, [[2 ** 24 + 1, 12, 9], [12, -2 ** 24 - 1, 9], [12, 12, 2 ** 31 - 1], [-2 ** 31, 12, 9]]]).astype(np.int32)
    ufar = np.concatenate([u, np.ones((4, 3))])
    got = check(e, far, ufar, radius=4096)
    assert (got["status"][-4:] == 2).all() and not got["neighbours"][-4:].any() and (got["neighbours"][:-4] == len(q)).all()
    # nobody contributes; m = 0; m = 1
    got = check(e, q, u, np.zeros(len(q), np.uint8), radius=6)
    assert (got["status"] == 1).all() and not got["neighbours"].any()
    got = check(e, far[-4:], ufar[-4:], radius=6)
    assert (got["status"] == 2).all()
    got = capi.strain(np.zeros((0, 3), np.int32), np.zeros((0, 3)))
    assert got["status"].shape == (0,) and got["G"].shape == (0, 3, 3) and got["E"].shape == (0, 6)
    got = check(e, q[:1], u[:1], radius=6)
    assert (got["status"][0], got["neighbours"][0]) == (1, 1)


def test_crowded_and_sparse(e):
    rng = np.random.default_rng(12)
    # 300 POIs in one cell, duplicates among them: the lanes wrap several times
    q = rng.integers(0, 8, (300, 3)).astype(np.int32)
    assert len(np.unique(q, axis=0)) < 300
    u = q @ G0.T + rng.normal(0, 0.05, (300, 3))
    valid = (rng.random(300) >= 0.1).astype(np.uint8)
    got = check(e, q, u, valid, radius=16)
    assert (got["neighbours"] == valid.sum()).all() and (got["status"] == 0).all()
    check(e, q, u, valid, radius=2, min_neighbours=4)
    # two clusters 3000 voxels apart at radius 1: 3001^3 cells of side 1 are over the cap, the cells grow
    blk = np.stack(np.meshgrid(*[np.arange(3)] * 3, indexing="ij"), -1).reshape(-1, 3)
    q = np.concatenate([blk, blk + 3000]).astype(np.int32)
    u = q @ G0.T + rng.normal(0, 0.05, (len(q), 3))
    got = check(e, q, u, radius=1, min_neighbours=4)
    assert got["neighbours"].max() == 27 and got["neighbours"].min() == 8 and (got["status"] == 0).all()
    # the same at the ends of the coordinate range: the box spans 2^25 + 1 voxels on every axis
    q = np.concatenate([blk - 2 ** 24, blk + 2 ** 24 - 2]).astype(np.int32)
    u = (q / 2.0 ** 24) @ G0.T + rng.normal(0, 0.05, (len(q), 3))
    got = check(e, q, u, radius=1, min_neighbours=4)
    assert got["neighbours"].max() == 27 and (got["status"] == 0).all()


def test_device_pointers_and_repeatability():
    import torch

    q, u, valid = ref.parity_inputs()
    for radius in (3, 20):
        a = capi.strain(q, u, valid, radius=radius, min_neighbours=ref.PARITY_MIN_NEIGHBOURS)
        b = capi.strain(q, u, valid, radius=radius, min_neighbours=ref.PARITY_MIN_NEIGHBOURS)
        assert same_bytes(a, b)
        dev = capi.strain(torch.from_numpy(q).cuda(), torch.from_numpy(u).cuda(), torch.from_numpy(valid).cuda(), radius=radius,
                          min_neighbours=ref.PARITY_MIN_NEIGHBOURS)
        assert same_bytes(a, dev)
    every = capi.strain(torch.from_numpy(q).cuda(), torch.from_numpy(u).cuda(), radius=7)
    assert same_bytes(every, capi.strain(q, u, np.ones(len(q), np.uint8), radius=7))
    with pytest.raises(ValueError):
        capi.strain(torch.from_numpy(q).cuda(), u)


def test_chain_icgn_to_strain(e):
    """a 96^3 scene dilated by 1.02 about its centre: IC-GN on a 4 x 4 x 4 grid, its results through strain_input_from_icgn into strain.
    The strain of the call equals the restatement's on the same IC-GN output; the error against the true E = (1.02^2 - 1) / 2 I is
    printed (DESIGN.md section 4.9 records it), not asserted."""
    R, T, truth = icgn_ref.scene((96, 96, 96), Lmat=1.02 * np.eye(3), seed=7)
    g = np.arange(30, 67, 12)
    q = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(np.int32)
    res = capi.icgn(R, T, q, subset_radius=12)
    disp, valid = capi.strain_input_from_icgn(res, zncc_min=0.5)
    assert valid.sum() >= 48, (res["status"], res["zncc"])
    assert np.array_equal(disp, res["displacement"])
    got = check(e, q, disp, valid, radius=36)
    assert (got["status"] == 0).all() and (got["neighbours"] == valid.sum()).all()
    true_e = 0.5 * (1.02 ** 2 - 1)
    err = np.abs(got["E"] - np.array([true_e] * 3 + [0.0] * 3)).max()
    print(f"true E = {true_e:.6f} I; max |E - true| = {err:.3e}; max rms {got['rms'].max():.3e}; IC-GN status counts "
          f"{np.bincount(res['status'], minlength=7).tolist()}; max |u - true| = {np.abs(disp[valid != 0] - truth(q)[valid != 0][:, [0, 4, 8]]).max():.3e}")
