"""GPU tests of the masked IC-GN (sift3d_icgn_masked, sift3d_mask_from_level; cases: tests/icgn_mask_cases.py, restatement:
tests/icgn_mask_ref.py): with a mask whose bytes are all non-zero every field has the bits of icgn / icgn_bspline; half-space masks
through the subset along each axis and from each side agree with the restatement; R's values at voxels the contract does not read
-- finite, NaN, Inf -- leave every bit as it is, and a NaN under a single masked-out voxel at each sentinel of the walk is not read;
status 7 is met from both sides of its bound and status 4 for fewer than 12 active voxels; on two bodies sliding along a plane the
masked call recovers the displacement where the plain one is wrong by tenths of a voxel; two calls, host and device inputs return the
same bytes; mask_from_level is (float64(R) >= level); a volume larger than one launch of the mask kernels covers is walked to its end;
the C++ shell returns the bits of the Python binding."""
import importlib
import os
import shutil
import subprocess

import numpy as np
import pytest

import icgn_mask_cases as cases
import icgn_mask_ref as mref
import icgn_ref as ref

pytestmark = pytest.mark.gpu

capi = importlib.import_module("3dsift_amd.capi")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("p", "zncc", "last_step", "iterations", "status")


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype == np.float64:
        return a.shape == b.shape and np.array_equal(a.view(np.uint64), np.asarray(b, np.float64).view(np.uint64))
    return np.array_equal(a, b)


def assert_same_records(a, b, fields=FIELDS):
    for k in fields:
        assert same_bits(a[k], b[k]), (k, a[k], b[k])


def assert_within_bars(got, want, bars=cases.BARS):
    """status, iterations and active equal; p and zncc within the bars; the figures are printed before they are judged"""
    assert np.array_equal(got["status"], want["status"]), (got["status"], want["status"])
    assert np.array_equal(got["iterations"], want["iterations"]), (got["iterations"], want["iterations"])
    assert np.array_equal(got["active"], want["active"]), (got["active"], want["active"])
    dd = np.abs(got["p"][:, [0, 4, 8]] - want["p"][:, [0, 4, 8]]).max()
    dg = np.abs(got["p"][:, cases.GRAD] - want["p"][:, cases.GRAD]).max()
    dz = np.abs(got["zncc"] - want["zncc"]).max()
    print(f"displacement {dd:.3e} gradient {dg:.3e} zncc {dz:.3e}")
    assert dd <= bars[0] and dg <= bars[1] and dz <= bars[2], (dd, dg, dz)


# ---- 1. all-ones identity -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("r", [2, 3, 6, 16])
def test_all_ones_mask_is_the_unmasked_call(r):
    R, T, _, truth = cases.volumes()
    q = cases.pois(r)
    assert len(q) == 12 and (q[0, 0], q[2, 1], q[4, 2]) == (r + 1, r + 1, r + 1)
    rng = np.random.default_rng(r)
    init = cases.perturbed(truth(q), rng)
    ones = rng.choice(np.array([1, 2, 255], np.uint8), R.shape)
    for interp in (0, 1, 2):
        got = capi.icgn_masked(R, T, ones, q, init=init, subset_radius=r, interpolation=interp)
        want = capi.icgn_bspline(R, T, q, init=init, subset_radius=r) if interp == 2 else capi.icgn(R, T, q, init=init, subset_radius=r,
                                                                                                    interpolation=interp)
        assert_same_records(got, want)
        assert (got["active"] == (2 * r + 1) ** 3).all(), got["active"]
        assert np.isin(got["status"], (0, 1)).mean() >= 0.75, got["status"]
        assert same_bits(got["displacement"], got["p"][:, [0, 4, 8]]) and same_bits(got["gradient"], got["p"].reshape(-1, 3, 4)[:, :, 1:])
    # zero init (NULL) and the coefficients brought by the caller
    assert_same_records(capi.icgn_masked(R, T, ones, q, subset_radius=r), capi.icgn(R, T, q, subset_radius=r))
    Cg = capi.bspline_prefilter(T)
    assert_same_records(capi.icgn_masked(R, Cg, ones, q, init=init, tar_is_coefficients=True, subset_radius=r, interpolation=2),
                        capi.icgn_bspline(R, Cg, q, init=init, coefficients=True, subset_radius=r))


# ---- 2. half-spaces -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("r,axis,side", cases.HALF_SPACES, ids=cases.HALF_IDS)
def test_half_space_agrees_with_restatement(r, axis, side):
    R, T, Cf, _ = cases.volumes()
    mask, q, init, n = cases.half_space(r, axis, side)
    for max_it, interp in cases.RUNS:
        opts = cases.run_options(r, max_it, interp)
        Tq = Cf if interp == 2 else T
        got = capi.icgn_masked(R, Tq, mask, q, init=init, tar_is_coefficients=interp == 2, **opts)
        want = mref.icgn_masked(R, Tq, mask, q, init=init, tar_is_coefficients=True, **opts)
        assert (got["active"] == n).all() and (got["status"] == 1).all(), (got["active"], got["status"])
        assert_within_bars(got, want)
        assert got["seconds"] > 0


# ---- 3. dead-region invariance ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which,r", [("half", 6), ("random", 6), ("random", 10)])
def test_dead_region_does_not_reach_the_result(which, r):
    R, T, _, truth = cases.volumes()
    rng = np.random.default_rng(40 + r)
    q = cases.pois(r)
    init = cases.perturbed(truth(q), rng)
    mask = cases.axis_mask(1, ">", 14) if which == "half" else (rng.random(R.shape) < 0.5).astype(np.uint8)
    dead = ~mref.needed_of(mask)
    assert 0.1 < dead.mean() < 0.99  # (a random 50 % mask: one voxel in 128 is active, about one in 20 is read)
    base = {k: capi.icgn_masked(R, T, mask, q, init=init, subset_radius=r, interpolation=k) for k in (0, 1, 2)}
    assert np.array_equal(base[0]["active"], mref.icgn_masked(R, T, mask, q, init=init, subset_radius=r, max_iterations=1)["active"])
    assert len(set(base[0]["active"])) > 1 and base[0]["active"].max() >= 12
    for fill in (rng.uniform(-50, 50, int(dead.sum())).astype(np.float32), np.float32(np.nan), np.float32(np.inf), np.float32(-np.inf)):
        R2 = R.copy()
        R2[dead] = fill
        for k in (0, 1, 2):
            got = capi.icgn_masked(R2, T, mask, q, init=init, subset_radius=r, interpolation=k)
            assert_same_records(got, base[k], FIELDS + ("active",))


@pytest.mark.parametrize("r", cases.SENTINEL_R)
def test_nan_under_one_masked_out_voxel(r):
    _, T, _, truth = cases.volumes()
    init = cases.perturbed(truth(cases.SENTINEL_Q), np.random.default_rng(4))
    opts = cases.run_options(r, 5, 0)
    for name, i in ref.sentinels(r).items():
        R, mask = cases.sentinel_case(r, i)
        got = capi.icgn_masked(R, T, mask, cases.SENTINEL_Q, init=init, **opts)
        assert np.isfinite(got["p"]).all() and np.isfinite(got["zncc"]).all() and np.isfinite(got["last_step"]).all(), name
        assert_within_bars(got, mref.icgn_masked(R, T, mask, cases.SENTINEL_Q, init=init, **opts))
        # the same mask over a finite R: the NaN was not read
        clean = capi.icgn_masked(cases.volumes()[0], T, mask, cases.SENTINEL_Q, init=init, **opts)
        assert_same_records(got, clean, FIELDS + ("active",))


# ---- 4. status 7 from both sides, status 4 --------------------------------------------------------------------------------------

def test_status_7_and_4():
    R, T, _, truth = cases.volumes()
    s = cases.status_masks()
    q, r = cases.STATUS_Q, cases.STATUS_R
    init = cases.perturbed(truth(q), np.random.default_rng(3))
    run = lambda mask, mf, **kw: capi.icgn_masked(R, T, mask, q, init=init, min_fraction=mf, subset_radius=r, **kw)  # noqa: E731
    a = run(s["full"], s["min_fraction"])
    assert a["active"][0] == s["n"] and a["status"][0] in (0, 1) and a["zncc"][0] > 0.9
    b = run(s["less"], s["min_fraction"])
    assert (b["active"][0], b["status"][0], b["iterations"][0], b["zncc"][0], b["last_step"][0]) == (s["n"] - 1, 7, 0, 0.0, 0.0)
    assert same_bits(b["p"], init)
    assert run(s["less"], 0.0)["status"][0] in (0, 1)
    assert run(s["full"], 1.0)["status"][0] == 7 and run(np.ones_like(s["full"]), 1.0)["status"][0] in (0, 1)
    for name, n in (("eleven", 11), ("one", 1)):
        c = run(s[name], 0.0)
        assert (c["active"][0], c["status"][0], c["iterations"][0], c["zncc"][0]) == (n, 4, 0, 0.0) and same_bits(c["p"], init), name
    for interp in (0, 1, 2):
        e = run(s["empty"], 0.0, interpolation=interp)
        assert (e["active"][0], e["status"][0], e["iterations"][0], e["zncc"][0]) == (0, 7, 0, 0.0) and same_bits(e["p"], init)
    # the order of the checks: 5 and 2 come before 7 and count nothing; 7 comes before 3
    qs = np.array([q[0], [r, 18, 22], q[0]], np.int32)
    ini = np.zeros((3, 12))
    ini[0, 3] = np.inf
    ini[2, 0] = 60.0
    o = capi.icgn_masked(R, T, s["empty"], qs, init=ini, subset_radius=r)
    assert list(o["status"]) == [5, 2, 7] and list(o["active"]) == [0, 0, 0] and same_bits(o["p"], ini)
    o = capi.icgn_masked(R, T, s["full"], qs, init=ini, subset_radius=r)
    assert list(o["status"]) == [5, 2, 3] and list(o["active"]) == [0, 0, s["n"]] and same_bits(o["p"], ini)


# ---- 5. two bodies sliding along a plane ----------------------------------------------------------------------------------------

def test_two_bodies_recovered_where_the_plain_call_fails():
    R, T, mask, truth = mref.two_body_scene()
    q = mref.TWO_BODY_POIS
    tr = truth(q)[:, [0, 4, 8]]
    masked = capi.icgn_masked(R, T, mask, q, subset_radius=mref.RADIUS)
    plain = capi.icgn(R, T, q, subset_radius=mref.RADIUS)
    em = np.abs(masked["displacement"] - tr).max(1)
    ep = np.abs(plain["displacement"] - tr).max(1)
    print("masked", em, masked["status"], masked["iterations"], "plain", ep, plain["zncc"])
    assert np.isin(masked["status"], (0, 1)).all(), masked["status"]
    assert em.max() <= 0.02, em
    assert ep.min() >= 0.1, ep
    k = np.tile(np.arange(5), 2)
    assert np.array_equal(masked["active"], 13 * 13 * (7 + k - 1)) and masked["active"][0] == 1014


# ---- 6. determinism, input paths, mask_from_level -------------------------------------------------------------------------------

def test_reproducible_host_and_device_inputs_and_independent_pois():
    import torch

    R, T, _, truth = cases.volumes()
    rng = np.random.default_rng(6)
    r = 5
    q = cases.pois(r, 20, seed=3)
    init = cases.perturbed(truth(q), rng)
    mask = ((rng.random(R.shape) < 0.97) & (cases.axis_mask(2, "<", 30) != 0)).astype(np.uint8) * 200
    Rd, Td = torch.tensor(R).cuda(), torch.tensor(T).cuda()  # (copies: the shared volumes are read-only)
    for interp in (0, 2):
        a = capi.icgn_masked(R, T, mask, q, init=init, subset_radius=r, interpolation=interp, min_fraction=0.3)
        b = capi.icgn_masked(R, T, mask, q, init=init, subset_radius=r, interpolation=interp, min_fraction=0.3)
        d = capi.icgn_masked(Rd, Td, torch.from_numpy(mask).cuda(), torch.from_numpy(q).cuda(), init=torch.from_numpy(init).cuda(),
                             subset_radius=r, interpolation=interp, min_fraction=0.3)
        assert_same_records(a, b, FIELDS + ("active",))
        assert_same_records(a, d, FIELDS + ("active",))
        assert {0, 7} <= set(a["status"]), a["status"]
        # a POI's record does not depend on the others: reversed order, and one at a time
        rev = capi.icgn_masked(R, T, mask, q[::-1].copy(), init=init[::-1].copy(), subset_radius=r, interpolation=interp, min_fraction=0.3)
        assert_same_records({k: v[::-1] for k, v in rev.items() if k != "seconds"}, a, FIELDS + ("active",))
        one = capi.icgn_masked(R, T, mask, q[7:8], init=init[7:8], subset_radius=r, interpolation=interp, min_fraction=0.3)
        assert_same_records(one, {k: v[7:8] for k, v in a.items() if k != "seconds"}, FIELDS + ("active",))
    with pytest.raises(ValueError):
        capi.icgn_masked(Rd, Td, mask, q, subset_radius=r)
    empty = capi.icgn_masked(R, T, mask, np.zeros((0, 3), np.int32))
    assert empty["p"].shape == (0, 12) and empty["status"].shape == (0,) and empty["active"].shape == (0,)
    assert empty["active"].dtype == np.int32


def test_mask_from_level():
    import torch

    R = cases.volumes()[0].copy()
    R[3, 4, 5], R[10, 11, 12], R[0, 0, 0], R[-1, -1, -1] = np.nan, np.inf, -np.inf, np.nan
    level = float(np.median(cases.volumes()[0]))
    for lv in (level, float(R[7, 7, 7]), np.inf, -np.inf):
        want = mref.mask_from_level(R, lv)
        with np.errstate(invalid="ignore"):
            assert np.array_equal(want != 0, R.astype(np.float64) >= lv)
        got, sec = capi.mask_from_level(R, lv, with_seconds=True)
        assert got.dtype == np.uint8 and got.shape == R.shape and np.array_equal(got, want) and sec > 0
        dev = capi.mask_from_level(torch.from_numpy(R).cuda(), lv)
        assert dev.dtype == torch.uint8 and dev.is_cuda and np.array_equal(dev.cpu().numpy(), want)
    assert 0.2 < capi.mask_from_level(R, level).mean() < 0.8
    odd = R[:5, :7, :3].copy()  # 105 voxels: not a multiple of the workgroup
    assert np.array_equal(capi.mask_from_level(odd, level), mref.mask_from_level(odd, level))
    # the chain: the mask of a level feeds the masked call
    Rv, T, _, truth = cases.volumes()
    q = cases.pois(6)
    m = capi.mask_from_level(Rv, -np.inf)
    a = capi.icgn_masked(Rv, T, m, q, subset_radius=6)
    assert_same_records(a, capi.icgn(Rv, T, q, subset_radius=6))


def test_volume_beyond_one_grid():
    """the two mask kernels launch at most 2^16 workgroups of 256 threads and walk a larger volume in a grid-stride loop: a volume of
    more than 2^24 voxels, the mask of a level compared everywhere, and POIs whose subsets lie beyond voxel 2^24"""
    rng = np.random.default_rng(8)
    nz, ny, nx, r = 280, 256, 256, 3
    R = rng.random((nz, ny, nx), dtype=np.float32)
    assert R.size > 1 << 24
    level = mref.mask_from_level(R, 0.5)
    assert np.array_equal(capi.mask_from_level(R, 0.5), level) and 0.4 < level.mean() < 0.6
    q = np.array([[100, 120, 268], [200, 31, 272], [17, 248, 273]], np.int32)  # (every tap of the cubic kernel inside: q + r + 2 <= n - 1)
    assert ((q[:, 2].astype(np.int64) - r - 1) * ny * nx > 1 << 24).all()
    ones = np.ones(R.shape, np.uint8)
    a = capi.icgn_masked(R, R, ones, q, subset_radius=r)
    assert_same_records(a, capi.icgn(R, R, q, subset_radius=r))
    assert (a["active"] == 343).all() and (a["status"] == 0).all()
    half = ones.copy()
    half[:, :, 102:] = 0  # POI 0: offsets dx <= 1 in the mask, dx <= 0 active; POI 1: nothing; POI 2: everything
    b = capi.icgn_masked(R, R, half, q, subset_radius=r)
    assert list(b["active"]) == [4 * 49, 0, 343] and list(b["status"]) == [0, 7, 0], (b["active"], b["status"])
    act = mref.active_of(level)
    want = [int(act[z - r:z + r + 1, y - r:y + r + 1, x - r:x + r + 1].sum()) for x, y, z in q]
    c = capi.icgn_masked(R, R, level, q, subset_radius=r)
    assert list(c["active"]) == want and max(want) > 0, (c["active"], want)


# ---- the C++ shell ----------------------------------------------------------------------------------------------------------------

CXX_MASKED = r"""
#include <cstdio>
#include <vector>
#include "cRegistration.h"
template <class V> static bool rd(FILE *f, V &v, size_t n) { v.resize(n); return std::fread(v.data(), sizeof(v[0]), n, f) == n; }
int main(int argc, char **argv) {
	FILE *f = std::fopen(argv[1], "rb");
	int h[7];
	float frac, level;
	std::vector<float> R, T;
	std::vector<unsigned char> mask;
	std::vector<int> Q;
	if (!f || std::fread(h, sizeof(int), 7, f) != 7 || std::fread(&frac, 4, 1, f) != 1 || std::fread(&level, 4, 1, f) != 1) return 2;
	const size_t nr = (size_t)h[0] * h[1] * h[2], nt = (size_t)h[3] * h[4] * h[5];
	const int m = h[6];
	if (!rd(f, R, nr) || !rd(f, T, nt) || !rd(f, mask, nr) || !rd(f, Q, 3 * (size_t)m)) return 3;
	std::fclose(f);
	std::vector<CPUSIFT::Cvec> pts;
	for (int i = 0; i < m; i++) pts.push_back(CPUSIFT::Cvec((float)Q[3 * i], (float)Q[3 * i + 1], (float)Q[3 * i + 2]));
	std::vector<unsigned char> lm(nr);
	if (!CPUSIFT::MaskFromLevel(R.data(), h[0], h[1], h[2], level, lm.data())) return 4;
	size_t in = 0;
	for (unsigned char b : lm) in += b;
	std::printf("%zu\n", in);
	CPUSIFT::IcgnOptions o;
	o.subset_radius = 6;
	for (int interp = 0; interp < 3; interp++) {
		o.interpolation = interp;
		std::vector<int> active;
		std::vector<CPUSIFT::IcgnResult> res = CPUSIFT::RefineDisplacementsMasked(R.data(), h[0], h[1], h[2], T.data(), h[3], h[4], h[5], mask.data(),
		                                                                          pts, nullptr, o, frac, &active);
		for (int i = 0; i < m; i++) {
			std::printf("%d %d %d %.17g %.17g", res[i].status, res[i].iterations, active[i], res[i].zncc, res[i].last_step);
			for (int k = 0; k < 12; k++) std::printf(" %.17g", res[i].p[k]);
			std::printf("\n");
		}
	}
	return 0;
}
"""


def test_cpp_shell_has_the_bits_of_the_binding(tmp_path):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no host compiler")
    d = os.path.join(ROOT, "3dsift_amd")
    src, exe = tmp_path / "masked.cpp", tmp_path / "masked"
    src.write_text(CXX_MASKED)
    subprocess.check_call([cxx, "-std=c++14", "-O2", "-o", str(exe), str(src), "-I", os.path.join(d, "host", "Include"), "-L" + d, "-lsift3d",
                           "-lsift3d_hip", "-Wl,-rpath," + d])
    R, T, mask, _ = mref.two_body_scene()
    q = np.concatenate([mref.TWO_BODY_POIS, [[27, 20, 22], [20, 20, 22]]]).astype(np.int32)  # one POI across the plane: too few voxels
    frac, level = np.float32(0.3), np.float32(np.median(R))
    blob = tmp_path / "in.bin"
    with open(blob, "wb") as fh:
        fh.write(np.int32([R.shape[2], R.shape[1], R.shape[0], T.shape[2], T.shape[1], T.shape[0], len(q)]).tobytes())
        fh.write(frac.tobytes() + level.tobytes())
        for a in (R, T, mask, q):
            fh.write(np.ascontiguousarray(a).tobytes())
    out = subprocess.run([str(exe), str(blob)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stderr)
    lines = out.stdout.strip().splitlines()
    assert int(lines[0]) == int(capi.mask_from_level(R, float(level)).sum())
    rows = np.array([[float(x) for x in line.split()] for line in lines[1:]]).reshape(3, len(q), 17)
    for interp in (0, 1, 2):
        py = capi.icgn_masked(R, T, mask, q, min_fraction=float(frac), subset_radius=6, interpolation=interp)
        got = rows[interp]
        assert np.array_equal(got[:, 0].astype(int), py["status"]) and np.array_equal(got[:, 1].astype(int), py["iterations"])
        assert np.array_equal(got[:, 2].astype(int), py["active"])
        assert same_bits(got[:, 3], py["zncc"]) and same_bits(got[:, 4], py["last_step"]) and same_bits(got[:, 5:], py["p"])
        assert 7 in py["status"] and np.isin(py["status"][:10], (0, 1)).all(), py["status"]
