"""GPU tests of guided matching (sift3d_match_guided, include/sift3d_hip.h): every case of tests/match_guided_cases.py in every mode
equals the restatement (tests/match_guided_ref.py: the CPU oracle's matcher on the gated columns) in every output without a
tolerance; a gate that holds everything returns sift3d_match's bytes; host arrays, device tensors and a second call give the same
bytes; and the chain match -> fit -> predict -> guided match end to end on a synthetic volume pair.  tests/test_match_guided_cpu.py
proves what the cases claim."""
import importlib

import numpy as np
import pytest

import match_guided_cases as cs
import match_guided_ref as ref

pytestmark = pytest.mark.gpu

capi = importlib.import_module("3dsift_amd.capi")
MODE_NAMES = {1: "inject", 2: "biject", 3: "enhanced"}


def guided(c, mode, radius=None, **kw):
    return capi.match_guided(c["a"], c["ax"], c["b"], c["bx"], c["pred"], c["radius"] if radius is None else radius, cs.THRESH, mode, **kw)


def assert_same(got, want, what):
    for k in cs.FIELDS:
        assert cs.same(got[k], want[k]), (what, k)


@pytest.mark.parametrize("name", cs.NAMES)
def test_case_equals_restatement(orc, name):
    c = cs.CASES[name]()
    for mode in cs.MODES:
        got = guided(c, mode)
        assert_same(got, cs.restated(orc, name, mode), (name, mode))
        assert got["seconds"] >= 0


@pytest.mark.parametrize("name", ["random_big", "purpose"])
def test_gate_of_everything_is_sift3d_match(name):
    c = cs.CASES[name]()
    m = capi.muBruteMatcher()
    for mode in cs.MODES:
        want = m._match(c["a"], c["ax"], c["b"], c["bx"], cs.THRESH, mode)
        got = guided(c, mode, radius=cs.ALL_GATE)
        for k in ("gIdx", "sIdx", "gDist", "sDist", "pairs"):
            assert cs.same(got[k], want[k]), (name, mode, k)
        assert (got["candidates"] == len(c["b"])).all()


def test_purpose():
    """sift3d_match rejects every row of the doubled targets; the guided call at radius 8 accepts them all with the near copy"""
    c = cs.CASES["purpose"]()
    plain = capi.muBruteMatcher().injectMatch(c["a"], c["ax"], c["b"], c["bx"], cs.THRESH)
    assert len(plain["pairs"]) == 0 and (plain["gIdx"] < 0).all()
    for mode in cs.MODES:
        got = guided(c, mode)
        assert np.array_equal(got["gIdx"], c["want"]) and len(got["pairs"]) == cs.PURPOSE_ROWS
        assert np.array_equal(got["pairs"][:, 3:], c["bx"][c["want"]]) and np.array_equal(got["pairs"][:, :3], c["ax"])


@pytest.mark.parametrize("name", ["scene_r16", "dense", "bad_positions", "random_big"])
def test_device_tensors_and_second_call(name):
    import torch

    c = cs.CASES[name]()
    dev = [torch.from_numpy(c[k]).cuda() for k in ("a", "ax", "b", "bx", "pred")]
    for mode in cs.MODES:
        host = guided(c, mode)
        again = guided(c, mode)
        on_dev = capi.match_guided(*dev, c["radius"], cs.THRESH, MODE_NAMES[mode])
        assert_same(again, host, (name, mode, "second call"))
        assert_same(on_dev, host, (name, mode, "device tensors"))


# ---- end to end: extraction, enhancedMatch, the fit, the prediction, the guided match ---------------------------------------------

def _rot(deg_x, deg_y, deg_z):
    ax, ay, az = np.radians([deg_x, deg_y, deg_z])
    Rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
    Ry = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]])
    Rz = np.array([[np.cos(az), -np.sin(az), 0], [np.sin(az), np.cos(az), 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def _render(shape, centres, sg, am):
    """synth.blobs' rendering with explicit blob centres (x, y, z)"""
    nz, ny, nx = shape
    vol = np.zeros(shape, np.float64)
    for (x0, y0, z0), s, a in zip(centres, sg, am):
        rr = 5.0 * s
        lo = [max(0, int(np.floor(v - rr))) for v in (x0, y0, z0)]
        hi = [min(n - 1, int(np.ceil(v + rr))) for v, n in ((x0, nx), (y0, ny), (z0, nz))]
        if any(l > h for l, h in zip(lo, hi)):
            continue
        g = [np.exp(-0.5 * ((np.arange(l, h + 1) - v) / s) ** 2) for l, h, v in zip(lo, hi, (x0, y0, z0))]
        vol[lo[2]:hi[2] + 1, lo[1]:hi[1] + 1, lo[0]:hi[0] + 1] += a * g[2][:, None, None] * g[1][None, :, None] * g[0][None, None, :]
    return vol.astype(np.float32)


def test_end_to_end(synth, capsys):
    size, radius = 96, 6.0
    shape = (size, size, size)
    cx, cy, cz, sg, am = synth.blob_params(shape, seed=1234)
    centres = np.stack([cx, cy, cz], 1)
    mid = np.full(3, (size - 1) / 2.0)
    Lm = 1.01 * _rot(3.0, -2.0, 5.0)
    shift = np.array([2.0, -1.5, 1.0])
    truth = lambda r: (r - mid) @ Lm.T + mid + shift
    desc, xyz = [], []
    for v in (_render(shape, centres, sg, am), _render(shape, truth(centres), sg, am)):
        g = capi.CSIFT3D(v).KpSiftAlgorithm()
        kp, d = g.GetKeypoints()
        desc.append(d)
        xyz.append(np.stack([kp["rx"], kp["ry"], kp["rz"]], 1).astype(np.float32))
        g.close()
    n, m = len(desc[0]), len(desc[1])
    assert n > 50 and m > 50
    matcher = capi.muBruteMatcher()
    first = matcher.enhancedMatch(desc[0], xyz[0], desc[1], xyz[1], cs.THRESH)
    fit = capi.fit_affine(first["pairs"])
    assert fit["status"] == 0
    pred = capi.predict_positions(fit, xyz[0])
    assert np.abs(pred - truth(xyz[0].astype(np.float64))).max() < radius / 2   # the fit is good enough to guide by: half the gate
    G = ref.gate(xyz[1], pred, radius)
    lines = []
    for mode in (1, 3):
        plain = matcher._match(desc[0], xyz[0], desc[1], xyz[1], cs.THRESH, mode)
        plain = {k: v.copy() for k, v in plain.items()}
        got = capi.match_guided(desc[0], xyz[0], desc[1], xyz[1], pred, radius, cs.THRESH, mode)
        assert np.array_equal(got["candidates"], G.sum(1))
        ok = np.flatnonzero(got["gIdx"] >= 0)
        # every guided pair lies within its gate (index 0 may be a rejected 0: the reference's sign flip leaves it)
        assert G[ok, got["gIdx"][ok]][got["gIdx"][ok] > 0].all()
        assert np.array_equal(got["pairs"][:, :3], xyz[0][ok]) and np.array_equal(got["pairs"][:, 3:], xyz[1][got["gIdx"][ok]])
        assert (np.abs(got["pairs"][:, 3:] - pred[ok])[got["gIdx"][ok] > 0] <= np.float32(radius)).all()
        if mode == 1:
            # a pair sift3d_match accepts whose target is in the row's gate is accepted by the guided call whenever sDist > 0
            acc = np.flatnonzero((plain["gIdx"] > 0) & (plain["sDist"] > 0))
            acc = acc[G[acc, plain["gIdx"][acc]]]
            assert len(acc) > 10
            assert np.array_equal(got["gIdx"][acc], plain["gIdx"][acc])
        for who, r in (("sift3d_match", plain), ("sift3d_match_guided", got)):
            p = r["pairs"]
            err = np.abs(p[:, 3:] - truth(p[:, :3].astype(np.float64))).max(1) if len(p) else np.zeros(0)
            lines.append(f"end to end {size}^3 (n = {n}, m = {m}, radius {radius:g}), mode {mode}, {who}: {len(p)} pairs, "
                         f"{int((err <= 1.5).sum())} within 1.5 voxels of the true map ({100.0 * (err <= 1.5).mean() if len(p) else 0:.1f} %)")
    with capsys.disabled():
        print()
        for line in lines:
            print(line)
