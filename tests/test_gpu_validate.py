"""GPU tests of the displacement validation (sift3d_validate_displacements) against its NumPy restatement (tests/validate_ref.py) on
the cases of tests/validate_cases.py.  Every field of every record must equal the restatement's as a number (==, so -0 = +0), the
integers exactly: nothing in the contract is a reduction, so there is no tolerance.  The cases: planted outliers in a curved field
with and without gradients and noise, the passes on a shifted block, neighbour counts at the minimum, odd and even, one and two POIs,
windows on both sides of the kernel's staging capacity with ties, both zeros, subnormals and a POI of 1e300, the contribution rules
(valid bytes, non-finite values, coordinates at and past 2^24, negative ones, duplicates, clusters 2^25 apart), the invariances
(permutation, device inputs, repeatability, a linear field with its gradients) and the chain IC-GN -> validate -> re-seed -> IC-GN ->
keep -> strain."""
import importlib

import numpy as np
import pytest

import icgn_ref
import strain_ref
import validate_cases as cases
import validate_ref as ref

pytestmark = pytest.mark.gpu

capi = importlib.import_module("3dsift_amd.capi")


def run(c, **more):
    got = capi.validate(c["points"], c["disp"], c["grad"], c["valid"], **dict(c["opts"], **more))
    assert got["seconds"] > 0 or len(c["points"]) == 0
    return got["records"]


def agree(got, want):
    assert len(got) == len(want)
    bad = ref.same(got, want)
    assert not bad, bad
    assert all(np.isfinite(got[k]).all() for k in ("median", "mad", "score"))


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_equals_restatement(name):
    c = cases.get(name)
    want = cases.reference(name)[0]
    got = run(c)
    agree(got, want)
    if "planted" in c:
        assert np.array_equal(np.flatnonzero(got["flagged"]), c["planted"])


def test_passes_on_the_shifted_block():
    one, two = run(cases.get("block-p1")), run(cases.get("block-p2"))
    centre = cases.get("block-p2")["centre"]
    assert one["flagged"].sum() == 20 and two["flagged"].sum() == 26 and (two["pass"] == 2).sum() == 6
    assert (two["flagged"][centre], two["status"][centre], two["neighbours"][centre]) == (0, 1, 0)
    for p in (3, 4):
        assert not ref.same(run(cases.get(f"block-p{p}")), two)


CAP_CASES = ("cap-minus-1", "cap", "cap-plus-1", "cap-plus-2", "cap-times-3")


@pytest.mark.parametrize("name", CAP_CASES)
def test_around_the_staging_capacity(name):
    cap = capi.validate_stage_capacity()
    c = cases.get(name, cap)
    want = cases.reference(name, cap)[0]
    got = run(c)
    agree(got, want)
    n = got["neighbours"][c["centre"]]
    print(f"{name}: capacity {cap}, the centre POI has {n} neighbours in the report, the largest window {got['neighbours'].max()}")
    if name != "cap-times-3":   # the first pass sees one neighbour more than the report: the huge POI, which that pass flags
        assert n + 1 == cap + {"cap-minus-1": -1, "cap": 0, "cap-plus-1": 1, "cap-plus-2": 2}[name]
    assert np.flatnonzero(got["flagged"]).tolist() == [c["big"]]


def test_empty_and_defaults():
    empty = capi.validate(np.zeros((0, 3), np.int32), np.zeros((0, 3)))
    assert empty["records"].shape == (0,) and empty["median"].shape == (0, 3)
    c = cases.get("planted-k0.002-n0.02-grad")
    want = ref.validate(c["points"], c["disp"], c["grad"])   # every option at its default: radius 16
    got = capi.validate(c["points"], c["disp"], c["grad"])
    agree(got["records"], want)
    centre = int(np.flatnonzero((c["points"] == 16).all(1))[0])   # sees every other POI, less the flagged ones
    assert got["neighbours"][centre] == 728 - (36 - got["flagged"][centre]) == got["neighbours"].max()


def test_permutation_permutes_the_records():
    for name in ("rules", "planted-k0.002-n0.02-grad", "n-odd-flags"):
        c = cases.get(name)
        base = run(c)
        perm = np.random.default_rng(9).permutation(len(base))
        moved = {k: (None if c[k] is None else c[k][perm]) for k in ("points", "disp", "grad", "valid")}
        moved["opts"] = c["opts"]
        assert not ref.same(run(moved), base[perm]), name


def test_device_inputs_and_repeatability():
    import torch

    cap = capi.validate_stage_capacity()
    for c in (cases.get("rules"), cases.get("planted-k0.0002-n0.02-plain"), cases.get("cap-plus-1", cap)):
        a, b = run(c), run(c)
        assert a.tobytes() == b.tobytes()
        dev = {k: (None if c[k] is None else torch.from_numpy(c[k]).cuda()) for k in ("points", "disp", "grad", "valid")}
        d = capi.validate(dev["points"], dev["disp"], dev["grad"], dev["valid"], **c["opts"])["records"]
        assert a.tobytes() == d.tobytes()


def test_linear_field_with_its_gradients():
    got = run(cases.get("linear-grad"))
    assert (got["status"] == 0).all() and got["score"].max() < 1e-9 and not got["flagged"].any()
    assert (got["neighbours"] == 7).sum() == 8   # the domain's corners are among them


STRAIN_E = 4.36e-14   # strain_ref.parity_error(), printed by tests/test_strain_cpu.py; the bar's floor max(4 e, 1e-12) holds either way


def test_chain_validate_reseed_keep_strain():
    """IC-GN -> validate -> icgn_init_from_validation -> IC-GN on the re-seeded rows -> validate_keep -> strain on the 64^3 scene of the
    IC-GN tests (rotation and translation, 4 x 4 x 4 POIs at a step of 10, subset radius 12).  Five POIs start 6 to 9 voxels off the
    truth.  Whether such a start converges on another peak depends on the blob texture around the POI; a row that did not (IC-GN gave
    up, or found its way back) gets a wrong vector planted directly into its record -- status 0, a respectable ZNCC, 3 voxels off --
    and the test prints how many rows needed that (on an MI355X all five: none of these starts ended as a converged wrong vector
    by itself).  The re-seeded rows must then land within the IC-GN test's own displacement bar
    (0.02 voxel) of the truth, and strain with the keep bytes must match the strain restatement on the same inputs within the strain
    test's bar."""
    R, T, truth = icgn_ref.scene((64, 64, 64), icgn_ref.rot(2.0, -1.0, 3.0), (0.4, -0.3, 0.25), seed=7)
    g = np.arange(17, 48, 10)
    q = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(np.int32)
    tr = truth(q)
    rng = np.random.default_rng(21)
    init = tr + np.where(np.arange(12) % 4 == 0, rng.uniform(-0.25, 0.25, tr.shape), rng.uniform(-0.005, 0.005, tr.shape))
    wrong = np.array([5, 22, 38, 42, 63])
    init[wrong[:, None], [0, 4, 8]] += rng.choice([-1.0, 1.0], (5, 3)) * rng.uniform(6.0, 9.0, (5, 3))
    opts = dict(subset_radius=12)
    first = capi.icgn(R, T, q, init=init, **opts)
    good = np.setdiff1d(np.arange(len(q)), wrong)
    assert (first["status"][good] == 0).all() and np.abs(first["p"] - tr)[good][:, [0, 4, 8]].max() <= 0.02
    off = np.abs(first["p"] - tr)[:, [0, 4, 8]].max(1)
    own = (first["status"][wrong] == 0) & (off[wrong] > 1.0) & (first["zncc"][wrong] >= 0.5)
    print(f"wrong starts that converged elsewhere on their own: {int(own.sum())} of 5; planted: {int((~own).sum())}")
    res = {k: first[k].copy() for k in ("p", "zncc", "status")}
    for i in wrong[~own]:
        res["p"][i] = tr[i]
        res["p"][i, [0, 4, 8]] += (3.0, -3.0, 3.0)
        res["zncc"][i], res["status"][i] = 0.95, 0
    disp, grad, valid = capi.validate_input_from_icgn(res, zncc_min=0.5)
    assert valid.all()
    val = capi.validate(q, disp, grad, valid, radius=10)
    assert np.array_equal(np.flatnonzero(val["flagged"]), wrong) and (val["status"] == 0).all()
    agree(val["records"], ref.validate(q, disp, grad, valid, radius=10))
    seeds, count = capi.icgn_init_from_validation(val)
    assert count == 5 and np.isfinite(seeds[wrong]).all() and np.isnan(seeds[good]).all()
    assert np.abs(seeds[wrong][:, [0, 4, 8]] - tr[wrong][:, [0, 4, 8]]).max() < 0.5
    second = capi.icgn(R, T, q[wrong], init=seeds[wrong], **opts)
    err = np.abs(second["p"] - tr[wrong])[:, [0, 4, 8]].max()
    print(f"re-seeded POIs: statuses {second['status']}, largest displacement error {err:.4f} voxel")
    assert (second["status"] == 0).all() and err <= 0.02
    keep = capi.validate_keep(val, valid)
    assert keep.sum() == len(q) - 5 and not keep[wrong].any()
    res["p"][wrong] = second["p"]
    disp2, _, _ = capi.validate_input_from_icgn(res)
    got = capi.strain(q, disp2, keep, radius=20)
    want = strain_ref.strain(q, disp2, keep, radius=20)
    assert np.array_equal(got["status"], want["status"]) and np.array_equal(got["neighbours"], want["neighbours"]) and (got["status"] == 0).all()
    bar = strain_ref.bar(STRAIN_E, strain_ref.largest_u(disp2))
    worst = max(float(np.abs(got[k] - want[k]).max()) for k in strain_ref.FLOATS)
    print(f"strain with the keep bytes: max |got - ref| {worst:.2e}, bar {bar:.2e}")
    assert worst <= bar
