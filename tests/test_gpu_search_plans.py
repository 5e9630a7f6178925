"""GPU tests of the ZNCC integer search (sift3d_zncc_search) beyond the parity cases of tests/test_gpu_search.py, against the NumPy
restatement (tests/zncc_search_ref.py, which also holds the inputs; tests/test_search_cpu.py proves their margins without a device):
every launch plan (ec, zs) -- all 240 pairs (r, s), three POIs each: an interior one, one whose window is clipped at T's low z and
high x faces, one clipped at the high z and low y faces; one call of 2 * 512 + 37 POIs, in which a workgroup walks three POIs of
different kinds; the exact invariances of the contract on integer-quantised volumes; and the voxel classes of real CT data, the
outlier at q + g among them.

The zncc bars follow the rule of tests/test_gpu_search.py: e = the largest |zncc(float32 restatement) - zncc(fp64 restatement)| over
the scored candidates of the inputs, bar = max(4 e, 1e-6) against the fp64 restatement.  status, d and candidates are compared
exactly: the best score of every input beats every other by at least 0.05, in fp64 and in float32.

Measured on the CPU (tests/test_search_cpu.py prints them), e / bar:
  plans and long call 4.28e-07 / 1.71e-06     invariance pair   1.31e-07 / 1.00e-06
  plain, negated      4.78e-07 / 1.91e-06     negdom            1.15e-06 / 4.59e-06
  quantised1000       1.26e-06 / 5.04e-06     quantised30000    7.25e-07 / 2.90e-06
  offset32768         1.1e-16  / 1.00e-06     nan/inf_corner    4.78e-07 / 1.91e-06
  nan_tc              9.00e-07 / 3.60e-06     outlier0          1.89e-07 / 1.00e-06
  outlier65535        1.63e-06 / 6.52e-06     outlier0_amp20    1.98e-07 / 1.00e-06
  outlier65535_amp20  1.45e-07 / 1.00e-06     nan/inf_subset, huge: nothing scored, bar 1.00e-06
Before the sums were centred on a voxel near the subset's mean (kernels_search.hip, "Tc"), the restatement's float32 mode gave
e = 6.3e-03 for the outlier class at amplitude 200 and scores up to 8.9 at amplitude 20.
The largest |zncc - ref| and |zncc_second - ref| of a device run have not been recorded yet: every test prints them (pytest -s).
"""
import importlib

import numpy as np
import pytest

import zncc_search_ref as ref

pytestmark = pytest.mark.gpu

capi = importlib.import_module("3dsift_amd.capi")
FIELDS = ("d", "status", "zncc", "zncc_second", "candidates")


def same_bytes(a, b):
    return all(np.ascontiguousarray(a[k]).tobytes() == np.ascontiguousarray(b[k]).tobytes() for k in FIELDS)


def agree(got, want, bar, what):
    assert np.array_equal(got["status"], want["status"]), (got["status"], want["status"])
    assert np.array_equal(got["d"], want["d"]), (got["d"], want["d"])
    assert np.array_equal(got["candidates"], want["candidates"]), (got["candidates"], want["candidates"])
    dz = np.abs(got["zncc"] - want["zncc"]).max()
    d2 = np.abs(got["zncc_second"] - want["zncc_second"]).max()
    print(f"{what}: max |zncc - ref| = {dz:.3e}, max |zncc_second - ref| = {d2:.3e}, bar = {bar:.3e}")
    assert dz <= bar and d2 <= bar, (dz, d2, bar)


@pytest.fixture(scope="module")
def plan_bar():
    b = ref.plan_bar()
    print(f"plans and long call: e = {ref.plan_error():.3e}, zncc bar = {b:.3e}")
    return b


@pytest.mark.parametrize("r,s", ref.PAIRS, ids=[f"r{r}-s{s}" for r, s in ref.PAIRS])
def test_every_plan(plan_bar, r, s):
    R, T, q = ref.plan_case(r, s)
    got = capi.zncc_search(R, T, q, subset_radius=r, search_radius=s)
    assert (got["status"] == 0).all() and (got["d"] == ref.PLAN_D).all(), (got["status"], got["d"])
    agree(got, ref.plan_reference(r, s), plan_bar, f"plan r{r} s{s} (ec, zs) = {ref.search_plan(r, s)}")


def test_long_call(plan_bar):
    R, T, q, g, kinds = ref.long_case()
    r, s = ref.LONG_R, ref.LONG_S
    assert len(q) == 2 * ref.MAX_GROUPS + 37
    got = capi.zncc_search(R, T, q, guess=g, subset_radius=r, search_radius=s)
    agree(got, ref.long_reference(), plan_bar, "long call")
    fail = got["status"] != 0
    assert np.array_equal(got["d"][fail], g[fail]) and not got["zncc"][fail].any() and (got["zncc_second"][fail] == -2.0).all()
    parts = [capi.zncc_search(R, T, q[i:i + 400], guess=g[i:i + 400], subset_radius=r, search_radius=s) for i in range(0, len(q), 400)]
    assert same_bytes(got, {k: np.concatenate([p[k] for p in parts]) for k in FIELDS})
    perm = np.random.default_rng(9).permutation(len(q))
    p = capi.zncc_search(R, T, q[perm], guess=g[perm], subset_radius=r, search_radius=s)
    assert same_bytes(p, {k: got[k][perm] for k in FIELDS})


def test_exact_invariances():
    R, T, q = ref.invariance_case()
    r, s = ref.INV_R, ref.INV_S
    bar = ref.invariance_bar()
    call = lambda R_, T_: capi.zncc_search(R_, T_, q, subset_radius=r, search_radius=s)  # noqa: E731
    f = lambda k: np.float32(2.0 ** k)  # noqa: E731
    base = call(R, T)
    assert (base["status"] == 0).all() and (base["d"] == ref.INV_D).all()
    agree(base, ref.invariance_reference(), bar, "invariance pair")
    for k in (7, -7):
        assert same_bytes(call(R * f(k), T), base), ("R scaled", k)
        assert same_bytes(call(R, T * f(k)), base), ("T scaled", k)
    for k in (40, -40):
        assert same_bytes(call(R * f(k), T * f(k)), base), ("both scaled", k)
    for add in ref.INV_T_OFFSETS:
        Ta = T + np.float32(add)
        assert Ta.max() < 2 ** 24 and np.array_equal(Ta.astype(np.float64), T.astype(np.float64) + add)
        assert same_bytes(call(R, Ta), base), ("T offset", add)
    off = call(R + np.float32(ref.INV_R_OFFSET), T)
    agree(off, ref.invariance_reference(True), bar, "R offset")
    assert all(np.array_equal(off[k], base[k]) for k in ("d", "status", "candidates"))
    assert np.abs(off["zncc"] - base["zncc"]).max() <= bar and np.abs(off["zncc_second"] - base["zncc_second"]).max() <= bar


@pytest.mark.parametrize("name", ref.CLASSES)
def test_voxel_class(name):
    R, T, q = ref.class_case(name)
    e, bar = ref.class_error(name)[0], ref.class_bar(name)
    print(f"class {name}: e = {e:.3e}, zncc bar = {bar:.3e}")
    got = capi.zncc_search(R, T, q, subset_radius=ref.CLASS_R, search_radius=ref.CLASS_S)
    if name == "huge":  # the float32 products overflow: every fp32 sum is non-finite and no candidate is scored
        want = ref.class_reference(name, True)
        assert (want["status"] == 3).all()
    else:
        want = ref.class_reference(name)
    if name.endswith("amp20"):
        assert np.abs(got["zncc"]).max() <= 1.0 + bar and np.abs(got["zncc_second"]).max() <= 1.0 + bar, (got["zncc"], got["zncc_second"])
    agree(got, want, bar, f"class {name}")
    if name in ("nan_subset", "inf_subset"):
        assert (got["status"] == 4).all()
    elif name != "huge":
        assert (got["status"] == 0).all() and (got["d"] == ref.CLASS_D).all()
