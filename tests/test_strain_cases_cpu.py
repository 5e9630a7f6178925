"""CPU tests of the strain fields' edge cases (tests/strain_cases.py): every claim a case makes about itself is checked here, against the
restatement (tests/strain_ref.py) and exact rational arithmetic, before the case reaches a GPU (tests/test_gpu_strain_edges.py).  The
windows at the pivot floor keep 5 % off it and get the status their exact pivot ratio rho asks for; the tilted ones print their measured
error and bar; the restatement has the invariances the GPU test asks of the kernel; the restated cell grid keeps the caps, equals
poi_choose_grid (a host program against poi_grid.h) and every planted block spans the cell borders it is planted across."""
import os
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import strain_cases as cases
import strain_ref as ref
import validate_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ref.FLOATS + ("neighbours", "status")


def two_solves(c):
    """the restatement's answer and the largest difference between its two solves over the status-0 POIs"""
    a, b = cases.reference(c), cases.reference(c, solve="lstsq")
    ok = a["status"] == 0
    assert np.array_equal(a["status"], b["status"]) and np.array_equal(a["neighbours"], b["neighbours"])
    return a, max(float(np.abs(a[k][ok] - b[k][ok]).max()) if ok.any() else 0.0 for k in ref.FLOATS)


def well_conditioned(c):
    """the premise of the ordinary bar: the two solves agree within a quarter of it"""
    a, diff = two_solves(c)
    assert diff <= 0.25 * ref.bar(0.0, cases.umax(c)), diff
    return a


# ---- the pivot floor -------------------------------------------------------------------------------------------------------------------
def test_exact_pivot_ratios():
    # an orthogonal cross: C = diag(2 a^2, 2 b^2, 2 c^2), the pivots are the diagonal
    d = [(3, 0, 0), (-3, 0, 0), (0, 2, 0), (0, -2, 0), (0, 0, 1), (0, 0, -1)]
    assert ref.exact_pivot_ratios(d) == (Fraction(1), Fraction(4, 9), Fraction(1, 9))
    # a sheared lattice: the product of the pivots is det C, whatever the shear; the floats agree with the fractions
    rng = np.random.default_rng(1)
    d = rng.integers(-9, 10, (30, 3))
    C = np.cov(d.T, bias=True) * len(d)
    p = ref.exact_pivot_ratios(d)
    top = C.diagonal().max()
    assert abs(float(p[0] * p[1] * p[2]) * top ** 3 / np.linalg.det(C) - 1) < 1e-12
    L = np.linalg.cholesky(C)
    assert np.allclose([float(v) for v in p], L.diagonal() ** 2 / top, rtol=1e-12, atol=0)
    assert ref.smallest_pivot_ratio(d) == float(min(p))
    # translation does not change C
    assert ref.exact_pivot_ratios(d + np.array([100, -7, 3])) == p
    assert ref.exact_pivot_ratios([(1, 2, 3)] * 5) == (0, None, None)
    assert ref.exact_pivot_ratios([(0, 1, 0), (0, 2, 5), (0, 3, 1)])[0] == 0
    assert ref.exact_pivot_ratios([(t, 2 * t, -t) for t in range(5)])[:2] == (Fraction(1, 4), 0)


@pytest.mark.parametrize("name", list(cases.THIN) + list(cases.TILTED))
def test_windows_at_the_pivot_floor(name):
    c = cases.pivot_case(name)
    rho, lo, hi, status = c["rho"], *cases.stated(name)
    ratios = ref.exact_pivot_ratios(c["offsets"])
    assert rho == float(min(ratios)) and ratios[c["deciding"]] == min(ratios)   # each of c00, p1, p2 decides in turn
    assert not 0.95e-9 <= rho <= 1.05e-9
    assert lo * 1e-9 <= rho <= hi * 1e-9 and c["status"] == status
    got = cases.reference(c)
    assert (got["status"][0], got["neighbours"][0]) == (status, c["n"])
    for solve in ("normal", "lstsq"):
        st = ref.fit(c["offsets"], c["disp"][1:], solve)[0]
        assert st == (0 if rho > 1e-9 else 4)
    # every other POI's window holds a subset of these sites under the same rule: no status but 0 and 4, nothing else in reach
    assert set(np.unique(got["status"])) <= {0, 4} and got["neighbours"].max() == c["n"]
    line = f"{name}: n = {c['n']}, rho = {rho:.4e}, status {status}, {int((got['status'] == 0).sum())} POIs fitted"
    if name in cases.TILTED:
        line += f", e_case = {cases.e_case(name):.3e}, bar = {cases.tilted_bar(name):.3e} (max |u| = {cases.umax(c):.1f})"
        assert cases.tilted_bar(name) == ref.bar(2.0 * cases.e_case(name), cases.umax(c))
    elif status == 0:
        # the thin windows are well conditioned in what they fit: two solves and 20 neighbour orders agree far inside the ordinary bar
        a, diff = two_solves(c)
        rng = np.random.default_rng(20)
        for _ in range(20):
            p = np.concatenate([[0], 1 + rng.permutation(c["n"])])
            b = ref.strain(c["points"][p], c["disp"][p], c["valid"][p], **c["opts"])
            diff = max(diff, max(float(np.abs(b[k][0] - a[k][0]).max()) for k in ref.FLOATS))
        line += f", two solves and 20 orders differ by {diff:.2e}, bar = {ref.bar(0.0, cases.umax(c)):.3e}"
        assert diff <= 0.25 * ref.bar(0.0, cases.umax(c))
    print(line)


@pytest.mark.parametrize("name", list(cases.DEGENERATE))
def test_exactly_degenerate_windows(name):
    c = cases.DEGENERATE[name]()
    ratios = ref.exact_pivot_ratios(c["offsets"])
    assert min(p for p in ratios if p is not None) == 0
    assert (ratios[0] == 0) == (name in ("plane-x", "coincident"))   # c00 = 0: l10 = 0 / 0
    for solve in ("normal", "lstsq"):
        got = cases.reference(c, solve=solve)
        assert (got["status"] == 4).all() and (got["neighbours"] == len(c["points"])).all()
        assert not any(got[k].any() for k in ref.FLOATS)


# ---- sums on u - u0 --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", cases.SHIFT_RADII)
def test_restatement_under_a_constant_shift(radius):
    q, u, valid = cases.dyadic_parity_inputs()
    assert np.array_equal(u * cases.SHIFT, np.round(u * cases.SHIFT)) and np.array_equal((u + cases.SHIFT) - cases.SHIFT, u)
    e = ref.parity_error()
    for measure in ref.MEASURES:
        opts = dict(radius=radius, min_neighbours=ref.PARITY_MIN_NEIGHBOURS, measure=measure)
        a, b = ref.strain(q, u, valid, **opts), ref.strain(q, u + cases.SHIFT, valid, **opts)
        assert (a["status"] == 0).sum() > 1000
        assert not cases.shift_disagreement(a, b, e)
    # a restatement that summed raw u would be caught: the check itself is not vacuous
    raw = {k: v.copy() for k, v in b.items()}
    raw["G"][0, 0, 0] += 1e-10
    assert cases.shift_disagreement(a, raw, e) == ["G"]


# ---- the cell grid ---------------------------------------------------------------------------------------------------------------------
def test_grid_restatement():
    assert cases.choose_grid((59, 49, 39), 7) == (7, (9, 8, 6))
    assert cases.choose_grid((10, 10, 10), 5) == (5, (3, 3, 3)) and cases.choose_grid((9, 11, 10), 5) == (5, (2, 3, 3))
    for box, extent in cases.BOXES.items():
        for r in (1, 3, 5, 4096):
            side, (nx, ny, nz) = cases.choose_grid(extent, r)
            assert side >= r and nx * ny <= cases.MAX_CELLS and nx * ny * nz <= cases.MAX_CELLS
            assert all(n == e // side + 1 for n, e in zip((nx, ny, nz), extent))
            print(f"{box} r{r}: side {side}, grid {nx} x {ny} x {nz} = {nx * ny * nz} cells")
    # the growth: 1 2 3 4 5 7 9 12 15 19 ... by (side + 3) / 4
    assert cases.choose_grid((3000, 3000, 3000), 1)[0] == 12 and cases.choose_grid((cases.BIG, 39, 39), 1)[0] == 19
    # the sheet: nx * ny decides; the third axis is one cell
    assert cases.choose_grid((cases.BIG, cases.BIG, 39), 1) == (8279, (4053, 4053, 1))


GRID_PROGRAM = r"""
#include <stdio.h>
#include <stdlib.h>
#include "poi_grid.h"
int main(int argc, char **argv) {
	for (int i = 1; i + 6 < argc; i += 7) {
		int v[7];
		for (int k = 0; k < 7; k++) v[k] = atoi(argv[i + k]);
		const int box[6] = {v[0], v[1], v[2], -(v[0] + v[3]), -(v[1] + v[4]), -(v[2] + v[5])};
		const s3d::PoiGrid g = s3d::poi_choose_grid(box, v[6]);
		printf("%d %d %d %d %d %d %d\n", g.x0, g.y0, g.z0, g.side, g.nx, g.ny, g.nz);
	}
	return 0;
}
"""


def test_grid_restatement_equals_strain_choose_grid(tmp_path):
    """poi_grid.h needs the HIP headers (no runtime: nothing of it is called or linked), so the program is built where they are"""
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    cxx = shutil.which("g++")
    if not cxx or not os.path.exists(os.path.join(rocm, "include", "hip", "hip_runtime.h")):
        pytest.skip("no host compiler or no HIP headers")
    src = tmp_path / "grid.cpp"
    src.write_text(GRID_PROGRAM)
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-w", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(rocm, "include"),
                        "-I", os.path.join(ROOT, "3dsift_amd", "csrc"), "-o", str(tmp_path / "grid"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    asked = []
    for c in ([cases.coarsened(b, r) for b, r in cases.COARSE_CASES] + [cases.extents(*k) for k in cases.EXTENT_CASES] +
              [cases.stars(r) for r in cases.STAR_RADII] + [cases.outside(r) for r in cases.OUTSIDE_RADII] +
              [cases.translated(n, r) for n in cases.translations() for r in cases.INVARIANCE_RADII]):
        lo, extent = cases.box_of(c)
        asked.append((lo, extent, c["opts"]["radius"]))
    args = [str(int(v)) for lo, extent, r in asked for v in (*lo, *extent, r)]
    out = subprocess.run([str(tmp_path / "grid")] + args, capture_output=True, text=True, check=True, timeout=60).stdout.split("\n")
    for (lo, extent, r), line in zip(asked, out):
        side, n = cases.choose_grid(extent, r)
        assert [int(v) for v in line.split()] == [*lo, side, *n], (lo, extent, r, line)


@pytest.mark.parametrize("r,axis,delta", cases.EXTENT_CASES)
def test_extent_cases(r, axis, delta):
    c = cases.extents(r, axis, delta)
    lo, extent = cases.box_of(c)
    assert np.array_equal(extent, c["extent"]) and extent[axis] == 5 * r + delta and (np.delete(extent, axis) == 3 * r).all()
    side, n = cases.choose_grid(extent, r)
    assert side == r and n[axis] == (5 * r + delta) // r + 1 and len(c["points"]) <= 400
    q = c["points"][c["planted"]] - lo
    assert c["valid"][c["planted"]].all() and (q[:4, axis] == 0).all() and (q[4:8, axis] == extent[axis]).all()
    assert {tuple(v) for v in q[8:]} == {tuple(v) for v in cases.corners_of(np.zeros(3, np.int64), extent)}
    got = well_conditioned(c)
    assert np.median(got["neighbours"]) >= 6 and (got["status"] == 0).mean() > 0.6


@pytest.mark.parametrize("r", cases.STAR_RADII + (5,))
def test_star_cases(r):
    for contribute, n in ((True, 7), (False, 6)):
        c = cases.stars(r, contribute)
        lo, extent = cases.box_of(c)
        assert cases.choose_grid(extent, r)[0] == r and len(c["centres"]) == len(cases.star_offsets(r))
        # the stars sit at the stated offsets from the cell borders
        off = (c["points"][c["centres"]] - lo) % r
        k = np.array(cases.star_offsets(r))
        assert np.array_equal(off, np.stack([k % r, (2 * k) % r, (3 * k) % r], 1))
        got = well_conditioned(c)
        assert (got["neighbours"][c["centres"]] == n).all() and (got["status"][c["centres"]] == 0).all()
        assert (got["neighbours"][c["corners"]] == 1).all() and (got["status"][c["corners"]] == 1).all()
    assert set(cases.star_offsets(5)) == set(range(5))


@pytest.mark.parametrize("box,r", cases.COARSE_CASES)
def test_coarsened_cases(box, r):
    c = cases.coarsened(box, r)
    lo, extent = cases.box_of(c)
    assert np.array_equal(lo, c["lo"]) and np.array_equal(extent, c["extent"])   # no block leaves the box
    side, n = cases.choose_grid(extent, r)
    assert (side, n) == c["grid"] and side > r and n[0] * n[1] <= cases.MAX_CELLS and n[0] * n[1] * n[2] <= cases.MAX_CELLS
    print(f"{box} r{r}: side {side}, grid {n[0]} x {n[1]} x {n[2]} = {n[0] * n[1] * n[2]} cells, {len(c['block_centres'])} blocks, "
          f"{len(c['points'])} POIs")
    seen = np.zeros(3, bool)
    for k, (ctr, span) in enumerate(zip(c["block_centres"], c["block_spans"])):
        blk = c["points"][27 * k:27 * k + 27].astype(np.int64)
        assert np.array_equal(blk, ctr + cases.BLOCK)
        cells = (blk - lo) // side
        spans = cells.max(0) - cells.min(0)
        assert np.array_equal(spans, span), (ctr, spans, span)   # the block spans two cells on exactly the axes it claims
        assert ((ctr - lo)[span == 1] % side == 0).all()           # voxels lo + c side - 1 and lo + c side
        seen |= span == 1
    assert np.array_equal(seen, np.array(n) > 1)                   # every axis that has a border is straddled
    assert (c["block_spans"].sum(1) == (np.array(n) > 1).sum()).any()   # and a cell corner
    got = well_conditioned(c)
    assert (got["status"][:-2] == 0).all() and got["neighbours"][:-2].min() >= 8 and (got["status"][-2:] == 1).all()


@pytest.mark.parametrize("r", cases.OUTSIDE_RADII)
def test_outside_cases(r):
    c = cases.outside(r)
    rows = c["outsiders"]
    on = ref.contributes(c["points"], c["disp"], c["valid"])
    assert not on[rows].any() and on[:125].all() and on.sum() == 125
    lo, extent = cases.box_of(c)
    assert (extent == 12).all()
    rel = c["points"][rows].astype(np.int64) - lo
    assert ((rel < 0) | (rel > 12)).any(1).all()   # every one of them is outside the box
    side = cases.choose_grid(extent, r)[0]
    far_low = rel[(rel < -1000).any(1)]
    assert len(far_low) == 3 and (far_low.min(1) % side != 0).all()   # the far offsets on the low side are no multiples of the side
    near_low = rel[((rel < 0) & (rel > -1000)).any(1)].min(1)
    assert (near_low % side != 0).any() and set(-near_low) == {1, r - 1, r, r + 1}
    got = well_conditioned(c)
    # distance 1 beyond a face: two planes in reach, a fit; r - 1 and r: one plane, degenerate; r + 1 and far away: nothing
    reach = np.maximum(np.maximum(-rel, rel - 12), 0).max(1)
    kinds = np.array(c["kinds"])
    assert (got["status"][rows][reach == 1] == 0).all()
    assert (got["status"][rows][(kinds == "face") & ((reach == r - 1) | (reach == r))] == 4).all()
    assert (got["neighbours"][rows][(reach == r) & (kinds == "face")] == (5 if r == 7 else 3) ** 2).all()
    assert (got["status"][rows][reach > r] == 1).all() and not got["neighbours"][rows][reach > r].any()
    assert (got["status"][:125] == 0).all()


# ---- invariances -----------------------------------------------------------------------------------------------------------------------
def test_restatement_under_translation():
    t = cases.translations()
    q, u, valid = ref.parity_inputs()
    on = ref.contributes(q, u, valid)
    assert np.array_equal(q[on].min(0) + t["low-corner"], [-2 ** 24] * 3) and np.array_equal(q[on].max(0) + t["high-corner"], [2 ** 24] * 3)
    lo = q[on].min(0)
    assert ((cases.OUTSIDERS - lo < 0) | (cases.OUTSIDERS > q[on].max(0))).any(1).all() and (cases.OUTSIDERS[0] - lo)[0] % 7 != 0
    for r in cases.INVARIANCE_RADII:
        base = cases.reference(cases.translated("none", r))
        assert base["neighbours"][-2:].min() > 0   # the outsiders' windows reach the box
        for name in t:
            c = cases.translated(name, r)
            assert len(c["out_of_range"]) == (1 if name.endswith("corner") else 0)
            assert not cases.translation_disagreement(base, cases.reference(c), c["out_of_range"])
            if r == 7 and name == "low-corner":   # the median test's restatement does not see the translation either
                v0 = validate_ref.validate(q, u, None, valid, radius=r, min_neighbours=3)
                v1 = validate_ref.validate(c["points"][:-2], u, None, valid, radius=r, min_neighbours=3)
                assert not validate_ref.same(v0, v1)


@pytest.mark.parametrize("radius", cases.INVARIANCE_RADII)
def test_restatement_under_permutation_and_axis_maps(radius):
    q, u, valid = ref.parity_inputs()
    bar = ref.bar(ref.parity_error(), ref.largest_u(u))
    base = ref.parity_reference(radius, 0)
    p = np.random.default_rng(radius).permutation(len(q))
    got = ref.strain(q[p], u[p], valid[p], radius=radius, min_neighbours=ref.PARITY_MIN_NEIGHBOURS)
    assert np.array_equal(got["status"], base["status"][p]) and np.array_equal(got["neighbours"], base["neighbours"][p])
    worst = max(float(np.abs(got[k] - base[k][p]).max()) for k in ref.FLOATS)
    print(f"r{radius}: the restatement moves by {worst:.2e} under a permutation of the POIs (bar {bar:.2e})")
    assert worst <= 0.25 * bar
    shapes = set()
    for perm, signs in cases.AXIS_MAPS:
        Q = cases.axis_matrix(perm, signs)
        assert abs(round(np.linalg.det(Q))) == 1 and np.array_equal(np.abs(Q).sum(0), [1, 1, 1])
        want = cases.mapped_result(base, Q)
        got = ref.strain(q @ Q.T, u @ Q.T, valid, radius=radius, min_neighbours=ref.PARITY_MIN_NEIGHBOURS)
        shapes.add(tuple(np.abs(Q) @ np.array([60, 50, 40])))
        assert np.array_equal(got["status"], want["status"]) and np.array_equal(got["neighbours"], want["neighbours"])
        worst = max(float(np.abs(got[k] - want[k]).max()) for k in ref.FLOATS)
        print(f"r{radius}: axes {perm} signs {signs}: the restatement moves by {worst:.2e} (bar {bar:.2e})")
        assert worst <= 0.25 * bar
    assert len(shapes) == 6 and (np.array([s for _, s in cases.AXIS_MAPS]) < 0).any(0).all()


def test_mapped_result_on_a_known_gradient():
    """G' = Q G Q^T and E' = Q E Q^T, checked on one gradient through strain_of"""
    G = cases.G0
    for perm, signs in cases.AXIS_MAPS:
        Q = cases.axis_matrix(perm, signs).astype(np.float64)
        E, pr, eq = ref.strain_of(G, 0)
        res = {"G": G[None], "E": E[None], "disp": cases.B0[None], "principal": pr[None], "equivalent": np.array([eq]), "rms": np.zeros(1),
               "neighbours": np.zeros(1, np.int32), "status": np.zeros(1, np.int32)}
        m = cases.mapped_result(res, Q.astype(np.int64))
        E2, pr2, eq2 = ref.strain_of(Q @ G @ Q.T, 0)
        assert np.allclose(m["G"][0], Q @ G @ Q.T, atol=1e-18) and np.allclose(m["E"][0], E2, atol=1e-17)
        assert np.allclose(pr, pr2, atol=1e-16) and abs(eq - eq2) < 1e-16 and np.allclose(m["disp"][0], Q @ cases.B0)
    assert np.array_equal(cases.six_of(cases.sym_of(np.arange(6.0)[None])), np.arange(6.0)[None])


# ---- known fields ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cases.known_fields()))
def test_known_fields(name):
    c = cases.known(name)
    G, b = c["G"], c["b"]
    bits = {"rotation": 30, "graded": 40}.get(name, 10)
    assert np.array_equal(G * 2.0 ** bits, np.round(G * 2.0 ** bits))
    q = c["points"].astype(np.float64)
    exact = np.array([[sum(Fraction(G[a, k]) * int(p[k]) for k in range(3)) + Fraction(b[a]) for a in range(3)] for p in c["points"][::57]])
    assert (np.array([[Fraction(v) for v in row] for row in c["disp"][::57]]) == exact).all()   # u = G q + b without rounding
    bar = ref.bar(ref.parity_error(), cases.umax(c))
    for measure in ref.MEASURES:
        got = cases.reference(c, measure=measure)
        E, pr, eq = ref.strain_of(G, measure)
        assert (got["status"] == 0).all() and got["neighbours"].min() == 27 and got["neighbours"].max() == 125
        worst = max(np.abs(got["G"] - G).max(), np.abs(got["disp"] - (q @ G.T + b)).max(), np.abs(got["E"] - E).max(),
                    np.abs(got["principal"] - pr).max(), np.abs(got["equivalent"] - eq).max(), got["rms"].max())
        print(f"{name} measure {measure}: the restatement is within {worst:.2e} of the closed form (bar {bar:.2e})")
        assert worst <= 0.25 * bar
    if name == "rotation":   # a rigid rotation: no Green strain beyond the rounding of R, the infinitesimal one is sym(R) - I
        R = G + np.eye(3)
        assert np.abs(R @ R.T - np.eye(3)).max() < 4e-9 and np.abs(ref.strain_of(G, 0)[0]).max() < 4e-9
        assert np.allclose(ref.strain_of(G, 1)[0][:3], (0.5 * (R + R.T) - np.eye(3)).diagonal())
    if name == "large":
        assert 3.5 < np.linalg.norm(G) < 4.5
    if name == "graded":
        assert np.allclose(ref.strain_of(G, 1)[1], [1e-1, 1e-6, 1e-11], rtol=0.2, atol=0)
