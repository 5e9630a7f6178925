"""CPU tests of guided matching's boundary (sift3d_match_guided / sift3d_predict_positions, include/sift3d_hip.h): the inputs of
tests/test_gpu_match_guided.py (tests/match_guided_cases.py) do what they claim on the restatement (tests/match_guided_ref.py), the
restatement with a gate that holds everything is the CPU oracle's matcher, sift3d_predict_positions needs no GPU and computes what
NumPy fp64 computes, bad arguments are refused before any device call, and the C++ shell's cRegistration.h links."""
import ctypes as C
import importlib
import os
import shutil
import subprocess

import numpy as np
import pytest

import match_cases as mc
import match_guided_cases as cs
import match_guided_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["sift3d_match_guided", "sift3d_predict_positions"]
ERR_ARG, NO_DEVICE = 1, 2
F32 = np.float32


@pytest.fixture(scope="module")
def capi():
    m = importlib.import_module("3dsift_amd.capi")
    if not os.path.exists(m.LIB_PATH):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "3dsift_amd", "csrc"), "-j8"])
    return m


def test_exports(capi):
    L = capi.lib()
    for n in NEW:
        assert hasattr(L, n), n
        assert n in capi.SYMBOLS


PROBE = r"""
#include "sift3d_hip.h"
int probe(const float *a, const float *ax, int n, const float *b, const float *bx, int m, const sift3d_affine_fit *fit, float *pred) {
	int gi[4], si[4], cand[4], np;
	float gd[4], sd[4], pairs[24];
	double s;
	return sift3d_predict_positions(fit, 1, ax, n, pred) +
	       sift3d_match_guided(a, ax, n, b, bx, m, pred, 6.0f, 0.85, 3, 0, 0, gi, si, gd, sd, cand, pairs, &np, &s);
}
"""


@pytest.mark.parametrize("lang", ["c", "c++"])
def test_header_compiles(tmp_path, lang):
    cc = shutil.which("gcc" if lang == "c" else "g++")
    if not cc:
        pytest.skip("no host compiler")
    src = tmp_path / ("probe.c" if lang == "c" else "probe.cpp")
    src.write_text(PROBE)
    std = "-std=c11" if lang == "c" else "-std=c++14"
    r = subprocess.run([cc, std, "-Wall", "-Werror", "-c", str(src), "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "probe.o")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


# ---- the cases on the restatement ---------------------------------------------------------------------------------------------------

def test_case_list():
    assert len(cs.NAMES) == len(set(cs.NAMES))
    for r in cs.RADII:
        assert f"edges_r{r:g}" in cs.CASES and f"scene_r{r:g}" in cs.CASES
    for name in cs.NAMES:
        c = cs.CASES[name]()
        n, m = len(c["a"]), len(c["b"])
        assert n <= 700 and m <= 700, name
        assert c["ax"].shape == c["pred"].shape == (n, 3) and c["bx"].shape == (m, 3) and c["a"].shape[1:] == c["b"].shape[1:] == (768,)
        assert all(c[k].dtype == F32 for k in ("a", "ax", "b", "bx", "pred"))
        assert 0 < c["radius"] <= 2.0 ** 20
    assert len(cs.CASES["empty_m0"]()["b"]) == 0 and len(cs.CASES["empty_n0"]()["a"]) == 0


@pytest.mark.parametrize("name", cs.NAMES)
def test_case_claims(orc, name):
    """gate sizes, gate membership and the best / second column are what the case was built for"""
    c = cs.CASES[name]()
    G = ref.gate(c["bx"], c["pred"], c["radius"])
    w = cs.restated(orc, name, 1)
    assert np.array_equal(w["candidates"], G.sum(1))
    for row, k in c.get("sizes", {}).items():
        assert G[row].sum() == k, (row, G[row].sum(), k)
    for row, col in c.get("in_gate", []):
        assert G[row, col], (row, col)
    for row, col in c.get("not_in_gate", []):
        assert not G[row, col], (row, col)
    gi, si = cs._want[(name, "forward", c["radius"])][:2]
    for row, (g, s) in c.get("best", {}).items():
        assert gi[row] == g, (row, gi[row], g)
        assert s is None or si[row] == s, (row, si[row], s)
    if "target" in c and len(c["b"]):   # a row whose planted target is in its gate finds it
        t = c["target"]
        hit = G[np.arange(len(t)), t]
        assert hit.any() and np.array_equal(gi[hit], t[hit])


def test_gate_sizes_sit_on_the_chunk_edges():
    c = cs.CASES["gate_sizes"]()
    sizes = ref.gate(c["bx"], c["pred"], c["radius"]).sum(1)
    assert tuple(sizes[:8]) == (0, 1, 2, 63, 64, 65, 128, 129)
    assert len(set(sizes[8:])) > 3   # partial views of the clusters
    d = cs.CASES["dense"]()
    sizes = ref.gate(d["bx"], d["pred"], d["radius"]).sum(1)
    assert sizes[0] == cs.DENSE == 400 and (sizes[1:] > 129).any()


def test_window_width_case():
    """the rounding case is in the fp32 gate although its floors differ by 17: a window of half width ceil(radius) misses it, the
    index must walk ceil(radius) + 1"""
    c = cs.CASES["edges_r16"]()
    G = ref.gate(c["bx"], c["pred"], 16.0)
    signs = []
    for row in c["rounding"]:
        p, t = c["pred"][row], c["bx"][2 * row + 1]
        axis = int(np.argmax(np.abs(t - p)))
        assert G[row, 2 * row + 1]
        assert abs(float(t[axis]) - float(p[axis])) > 16.0            # outside in exact arithmetic
        assert F32(t[axis] - p[axis]) in (F32(16), F32(-16))          # rounds onto the edge
        assert abs(int(np.floor(t[axis])) - int(np.floor(p[axis]))) == 17
        signs.append((axis, float(np.sign(t[axis] - p[axis]))))
    assert sorted(signs) == [(a, s) for a in range(3) for s in (-1.0, 1.0)]   # three axes, both signs
    kinds = {(row, col) for row, col in c["not_in_gate"]}
    assert len(kinds) == 6 and len(c["in_gate"]) == 18 + 12


@pytest.mark.parametrize("radius", cs.RADII)
def test_edge_targets(radius):
    c = cs.CASES[f"edges_r{radius:g}"]()
    r = F32(radius)
    for row, col in c["not_in_gate"]:
        d = np.abs(c["bx"][col] - c["pred"][row])
        assert d.max() == np.nextafter(r, F32(np.inf)) or (d.max() > r and d.max() - r < 1e-3 * radius)
    exact = [(row, col) for row, col in c["in_gate"] if col % 2 and row not in c["rounding"]]
    assert len(exact) == 6 and all(np.abs(c["bx"][col] - c["pred"][row]).max() == r for row, col in exact)
    assert all(np.abs(c["bx"][col].astype(np.float64) - c["pred"][row]).max() == radius for row, col in exact)   # exactly, not by rounding


def test_index_seams():
    s = cs.side(16.0)
    c = cs.CASES["all_cells"]()
    G = ref.gate(c["bx"], c["pred"], 16.0)
    cell = (np.floor(c["bx"]).astype(int) - np.floor(c["bx"]).astype(int).min(0)) // s
    assert cell.max(0).tolist() == [2, 2, 2]
    for row in c["cells27"]:
        assert len({tuple(v) for v in cell[G[row]]}) == 27, row
    c = cs.CASES["one_cell"]()
    f = np.floor(c["bx"]).astype(int)
    assert ((f.max(0) - f.min(0)) < s).all()
    c = cs.CASES["outside_box"]()
    lo, hi = c["bx"].min(0), c["bx"].max(0)
    out = ((c["pred"] < lo) | (c["pred"] > hi)).any(1)
    assert out.all() and len(out) == 19
    sizes = ref.gate(c["bx"], c["pred"], 16.0).sum(1)
    assert (sizes == 0).sum() == 13 and (sizes > 0).sum() == 6
    c = cs.CASES["negative"]()
    assert (c["bx"] < 0).any() and (c["bx"] > 0).any() and (np.floor(c["bx"]) != np.trunc(c["bx"])).any()


def test_order_case(orc):
    c = cs.CASES["order"]()
    G = ref.gate(c["bx"], c["pred"], 16.0)
    key = c["walk_key"]
    for i in range(20):
        lo, hi = c["best"][i]
        assert lo < hi and G[i, lo] and G[i, hi] and np.array_equal(c["b"][lo], c["b"][hi])
        walk = sorted(np.flatnonzero(G[i]), key=key)
        assert walk.index(hi) < walk.index(lo)   # the walk meets the higher column first
    for i in range(20, 40):
        walk = sorted(np.flatnonzero(G[i]), key=key)
        assert c["best"][i][0] == (walk[0] if i < 30 else walk[-1]) and len(walk) > 64


def test_bad_positions_case():
    c = cs.CASES["bad_positions"]()
    G = ref.gate(c["bx"], c["pred"], 16.0)
    assert not G[:, c["dead_targets"]].any()
    assert np.isnan(c["pred"][0]).all() and np.isnan(c["pred"][1]).sum() == 1 and np.isinf(c["pred"][2]).sum() == 1
    assert c["bx"][6, 0] == F32(2.0 ** 24 + 2) and c["pred"][4, 0] == c["bx"][6, 0]   # difference 0, yet in no gate
    assert G[3, 5] and G[3, 9] and G[3].sum() == 2 and G[5, 7]


def test_purpose_case(orc):
    """every row is rejected by the plain matcher's ratio test and accepted, with the near copy, by the restatement at radius 8"""
    c = cs.CASES["purpose"]()
    plain = orc.match(c["a"], c["ax"], c["b"], c["bx"], cs.THRESH, 1)
    assert (plain["gIdx"] < 0).all() and len(plain["pairs"]) == 0
    assert np.array_equal(plain["gDist"], plain["sDist"])   # the two copies score alike: ratio 1
    w = cs.restated(orc, "purpose", 1)
    assert np.array_equal(w["gIdx"], c["want"]) and (w["candidates"] == 1).all()
    assert (w["sIdx"] == -1).all() and (w["sDist"] == F32(2.0)).all() and len(w["pairs"]) == cs.PURPOSE_ROWS
    assert (c["want"] > cs.PURPOSE_ROWS).sum() == cs.PURPOSE_ROWS // 2   # the near copy is the higher column for every other row


@pytest.mark.parametrize("name", ["random_big", "purpose", "scene_r4096", "hostile_nonfinite_pinf_tar5", "hostile_zero_tar_rows"])
@pytest.mark.parametrize("mode", cs.MODES)
def test_gate_of_everything_is_the_plain_matcher(orc, name, mode):
    c = cs.CASES[name]()
    assert ref.gate(c["bx"], c["pred"], cs.ALL_GATE).all()
    got = cs.restated(orc, name, mode, cs.ALL_GATE)
    want = orc.match(c["a"], c["ax"], c["b"], c["bx"], cs.THRESH, mode)
    for k in want:
        assert mc.same(got[k], want[k]), k
    assert (got["candidates"] == len(c["b"])).all()


def test_modes_differ_somewhere(orc):
    """the reverse pass decides something in the scenes: modes 2 and 3 are not mode 1"""
    for name in ("scene_r16", "scene_r2.5"):
        w = [cs.restated(orc, name, mode) for mode in cs.MODES]
        assert len(w[0]["pairs"]) > len(w[2]["pairs"]) > 0, name
        assert not np.array_equal(w[1]["gIdx"], w[2]["gIdx"]) or not np.array_equal(w[0]["gIdx"], w[1]["gIdx"]), name


# ---- sift3d_predict_positions -------------------------------------------------------------------------------------------------------

def _numpy_predict(A, xyz):
    r = np.asarray(xyz, F32).astype(np.float64)
    A = np.broadcast_to(np.asarray(A, np.float64).reshape(-1, 3, 4), (len(r), 3, 4))
    return (((A[:, :, 0] * r[:, None, 0] + A[:, :, 1] * r[:, None, 1]) + A[:, :, 2] * r[:, None, 2]) + A[:, :, 3]).astype(F32)


def test_predict_positions_global(capi):
    rng = np.random.default_rng(5)
    xyz = rng.uniform(-300, 300, (257, 3)).astype(F32)
    A = np.concatenate([np.eye(3) + 0.05 * rng.normal(size=(3, 3)), rng.uniform(-20, 20, (3, 1))], 1)
    got = capi.predict_positions(dict(A=A, status=0), xyz)
    assert got.dtype == F32 and mc.same(got, _numpy_predict(A, xyz))
    np.testing.assert_allclose(got, xyz.astype(np.float64) @ A[:, :3].T + A[:, 3], rtol=0, atol=1e-4)
    assert np.isnan(capi.predict_positions(dict(A=A, status=2), xyz)).all()
    assert capi.predict_positions(dict(A=A, status=0), np.zeros((0, 3), F32)).shape == (0, 3)


def test_predict_positions_per_row(capi):
    rng = np.random.default_rng(6)
    n = 100
    xyz = rng.uniform(0, 500, (n, 3)).astype(F32)
    A = np.concatenate([np.eye(3) + 0.02 * rng.normal(size=(n, 3, 3)), rng.uniform(-5, 5, (n, 3, 1))], 2)
    status = np.zeros(n, np.int32)
    status[[0, 17, 99]] = (1, 2, 3)
    got = capi.predict_positions(dict(A=A, status=status), xyz)
    want = _numpy_predict(A, xyz)
    want[status != 0] = np.nan
    assert np.array_equal(np.isnan(got), np.isnan(want)) and mc.same(got[status == 0], want[status == 0])
    assert np.isnan(got[[0, 17, 99]]).all()


def test_predict_positions_bad_arguments(capi):
    L = capi.lib()
    f = np.zeros(4, capi.FIT_DTYPE)
    x = np.zeros((4, 3), F32)
    o = np.zeros((4, 3), F32)
    Fp, X, O = (v.ctypes.data_as(C.c_void_p) for v in (f, x, o))
    assert L.sift3d_predict_positions(Fp, 1, X, 4, O) == 0 and L.sift3d_predict_positions(Fp, 4, X, 4, O) == 0
    for args in [(Fp, 1, X, -1, O), (Fp, 2, X, 4, O), (Fp, 0, X, 4, O), (None, 1, X, 4, O), (Fp, 1, None, 4, O), (Fp, 1, X, 4, None)]:
        assert L.sift3d_predict_positions(*args) == ERR_ARG, args


# ---- sift3d_match_guided: refused before any device is touched ----------------------------------------------------------------------

def test_bad_arguments_refused(capi):
    L = capi.lib()
    a = np.zeros((4, 768), F32); b = np.zeros((5, 768), F32)
    x = np.zeros((4, 3), F32); y = np.zeros((5, 3), F32); p = np.zeros((4, 3), F32)
    A, X, B, Y, P = (v.ctypes.data_as(C.c_void_p) for v in (a, x, b, y, p))
    out = (None,) * 8

    def call(A=A, X=X, n=4, B=B, Y=Y, m=5, P=P, radius=6.0, mode=3, device=0):
        return L.sift3d_match_guided(A, X, n, B, Y, m, P, radius, 0.85, mode, 0, device, *out)

    for radius in (0.0, -1.0, float("nan"), float("inf"), 2.0 ** 20 + 1, np.nextafter(F32(2.0 ** 20), F32(np.inf))):
        assert call(radius=float(radius)) == ERR_ARG, radius
        assert b"sift3d_match_guided: bad argument" in L.sift3d_last_error()
    for mode in (0, 4, -1):
        assert call(mode=mode) == ERR_ARG, mode
    assert call(n=-1) == ERR_ARG and call(m=-1) == ERR_ARG
    for k in ("A", "X", "B", "Y", "P"):
        assert call(**{k: None}) == ERR_ARG, k
    # the checks come before the device: without a GPU the same call with good arguments gets as far as the device pick
    assert call() == (0 if capi.device_count() > 0 else NO_DEVICE)


def test_python_wrapper_checks(capi):
    c = cs.CASES["purpose"]()
    with pytest.raises(ValueError):
        capi.match_guided(c["a"], c["ax"], c["b"], c["bx"], c["pred"][:-1], 8.0)
    with pytest.raises(ValueError):
        capi.match_guided(c["a"], c["ax"], c["b"], c["bx"], c["pred"], 8.0, mode="both")
    with pytest.raises(capi.Sift3dError):
        capi.match_guided(c["a"], c["ax"], c["b"], c["bx"], c["pred"], 0.0)


# ---- the C++ shell ------------------------------------------------------------------------------------------------------------------

SHELL = r"""
#include <cstdio>
#include <vector>
#include "cRegistration.h"
int main() {
	std::vector<CPUSIFT::Cvec> ref, tar;
	for (int i = 0; i < 16; i++) { ref.push_back(CPUSIFT::Cvec(i, 2 * i % 7, i * i % 5)); tar.push_back(ref.back()); }
	std::vector<CPUSIFT::Keypoint> ref_kp(3), tar_kp(4);
	CPUSIFT::AffineFit f = CPUSIFT::EstimateAffine(ref, tar);
	std::vector<CPUSIFT::Cvec> pred = CPUSIFT::PredictPositions(f, ref_kp);
	std::vector<CPUSIFT::AffineFit> lf(3);
	std::vector<CPUSIFT::Cvec> pred2 = CPUSIFT::PredictPositions(lf, ref_kp);
	std::vector<CPUSIFT::Cvec> refMatch, tarMatch;
	CPUSIFT::GuidedMatchResult g = CPUSIFT::GuidedMatch(refMatch, tarMatch, ref_kp, tar_kp, pred, 6.0f);
	CPUSIFT::GuidedMatchResult h = CPUSIFT::GuidedMatch(refMatch, tarMatch, ref_kp, tar_kp, pred2, 6.0f, 0.8, CPUSIFT::Inject);
	std::printf("%d %zu %zu %zu %zu %zu %g %d\n", (int)g.ok, g.glodenIdx.size(), g.silverIdx.size(), g.candidates.size(),
	            g.glodenDistSquare.size(), g.silverDistSquare.size(), g.seconds, (int)h.ok);
	return 0;
}
"""


def test_shell_registration_links(tmp_path):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no host compiler")
    d = os.path.join(ROOT, "3dsift_amd")
    subprocess.check_call(["make", "-C", os.path.join(d, "host")], stdout=subprocess.DEVNULL)
    src = tmp_path / "reg.cpp"
    src.write_text(SHELL)
    r = subprocess.run([cxx, "-std=c++14", "-Wall", "-Werror", "-o", str(tmp_path / "reg"), str(src), "-I", os.path.join(d, "host", "Include"),
                        "-L" + d, "-lsift3d", "-lsift3d_hip", "-Wl,-rpath," + d], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
