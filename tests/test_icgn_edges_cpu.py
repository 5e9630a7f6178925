"""CPU tests of the IC-GN restatement (tests/icgn_ref.py) where it has to state the contract of include/sift3d_hip.h by itself: status 4
is "a Cholesky pivot <= 0 or NaN" (np.linalg.cholesky returns a NaN factor for a NaN entry and accepts an infinite pivot), the
float32 form of the per-voxel interpolation, and the invariances the GPU tests assert bit for bit."""
import numpy as np
import pytest

import icgn_ref as ref

Q, RAD = (20, 20, 20), 5


@pytest.fixture(scope="module")
def scene():
    return ref.scene((40, 40, 40), tvec=(0.3, -0.2, 0.1), seed=41)


def test_numpy_cholesky_is_not_the_contract():
    """what the restatement relied on: np.linalg.cholesky raises for none of the NaN and infinite matrices below; the contract refuses the NaN ones"""
    for i, j in ((3, 3), (7, 2)):
        H = np.eye(12)
        H[i, j] = H[j, i] = np.nan
        assert not ref.positive_definite(H)
    H = np.eye(12)
    H[5, 5] = np.inf
    assert ref.positive_definite(H)  # every pivot is > 0: the contract names no test for infinity
    H[5, 6] = H[6, 5] = 1.0          # inf's column scales to 0: still positive pivots
    assert ref.positive_definite(H)
    H = np.eye(12)
    H[4, 4] = 0.0
    assert not ref.positive_definite(H)
    H[4, 4] = -1e-300
    assert not ref.positive_definite(H)
    A = np.random.default_rng(0).normal(size=(40, 12))
    assert ref.positive_definite(A.T @ A)
    assert not ref.positive_definite(np.zeros((12, 12)))


@pytest.mark.parametrize("at", [(20, 20, 20 + RAD + 1), (20 - RAD - 1, 21, 20), (20, 20 + RAD + 1, 19)], ids=["x-margin", "z-margin", "y-margin"])
def test_nan_in_the_margin_only_is_status_4(scene, at):
    """dR is finite (the subset holds no NaN), the gradient of one face voxel is NaN, so H is: the GPU returns 4"""
    R, T, _ = scene
    Rb = R.copy()
    Rb[at] = np.nan
    d = ref.offsets(RAD).astype(int) + np.array(Q)
    assert np.isfinite(Rb[d[:, 2], d[:, 1], d[:, 0]]).all()
    w = ref.refine(Rb, T, Q, init=[0.2] + [0.0] * 11, subset_radius=RAD)
    assert (w["status"], w["iterations"], w["zncc"], w["last_step"]) == (4, 0, 0.0, 0.0) and w["p"][0] == 0.2


def test_nan_on_and_off_the_diagonal_of_H(scene, monkeypatch):
    R, T, _ = scene
    for i, j in ((0, 0), (6, 6), (9, 2), (1, 11)):
        real = ref.positive_definite

        def poisoned(H, i=i, j=j, real=real):
            H = np.array(H)
            H[i, j] = H[j, i] = np.nan
            return real(H)

        monkeypatch.setattr(ref, "positive_definite", poisoned)
        assert ref.refine(R, T, Q, subset_radius=RAD)["status"] == 4, (i, j)
        monkeypatch.setattr(ref, "positive_definite", real)


def test_well_conditioned_case_keeps_its_bits(scene, monkeypatch):
    """the explicit pivots decide like np.linalg.cholesky on a healthy subset and touch nothing else: same bits either way"""
    R, T, _ = scene

    def numpy_rule(H):
        try:
            np.linalg.cholesky(H)
        except np.linalg.LinAlgError:
            return False
        return True

    new = [ref.refine(R, T, Q, subset_radius=RAD, interpolation=i) for i in (0, 1)]
    monkeypatch.setattr(ref, "positive_definite", numpy_rule)
    old = [ref.refine(R, T, Q, subset_radius=RAD, interpolation=i) for i in (0, 1)]
    for a, b in zip(new, old):
        assert a["status"] == 0 and b["status"] == 0 and a["iterations"] == b["iterations"]
        for k in ("p", "zncc", "last_step"):
            assert np.array_equal(np.float64(a[k]).view(np.uint64), np.float64(b[k]).view(np.uint64)), k
        assert len(a["steps"]) == a["iterations"] and a["steps"][-1] == a["last_step"]


@pytest.mark.parametrize("cubic", [True, False])
def test_float32_interpolation(cubic):
    """the float32 form rounds every product and sum to float32: exact on a constant (linear) and on integer positions, within a few
    float32 ulps of the fp64 form elsewhere, and not equal to it"""
    rng = np.random.default_rng(3)
    T = rng.uniform(0.5, 1.5, (20, 22, 24)).astype(np.float32)
    pos = np.stack([rng.uniform(1, 21.9, 4000), rng.uniform(1, 19.9, 4000), rng.uniform(1, 17.9, 4000)], 1)
    a, b = ref.interp(T, pos, cubic), ref.interp(T, pos, cubic, f32=True)
    assert np.array_equal(b, b.astype(np.float32).astype(np.float64))
    gap = np.abs(a - b).max()
    assert 0 < gap <= 16 * 2.0 ** -24 * 1.5 * (3.4 if cubic else 1.0), gap  # sum |w| <= 1.5^3 (Catmull-Rom), 1 (linear)
    ipos = np.floor(pos)
    assert np.array_equal(ref.interp(T, ipos, cubic, f32=True), T[ipos[:, 2].astype(int), ipos[:, 1].astype(int), ipos[:, 0].astype(int)])
    # tap order and axes: a volume that varies along one axis only interpolates along that axis only
    for axis in range(3):
        ramp = np.moveaxis(np.broadcast_to(np.arange(30, dtype=np.float32) ** 2, (30, 30, 30)), 2, 2 - axis)
        want = pos[:, axis] ** 2 if cubic else None
        got = ref.interp(ramp, pos, cubic)
        if cubic:
            assert np.abs(got - want).max() <= 1e-9  # Catmull-Rom reproduces quadratics
        else:
            fl = np.floor(pos[:, axis])
            assert np.abs(got - (fl ** 2 + (pos[:, axis] - fl) * (2 * fl + 1))).max() <= 1e-9


INTERP_GOLDEN = {  # the restatement's interp before its gather was rewritten as a tap loop, on the volume and positions below
    True: ["0x1.07062d57fd300p-2", "0x1.8787880000000p-1", "0x1.e1a289adfbbccp-2", "0x1.08bbf013ef237p-1", "0x1.dbad2e8c37000p-2"],
    False: ["0x1.0d2d2d6400000p-2", "0x1.8787880000000p-1", "0x1.e1dcb5983abe1p-2", "0x1.08bbeffffffffp-1", "0x1.ed2d2e6000000p-2"],
}


@pytest.mark.parametrize("cubic", [True, False])
def test_interp_keeps_its_bits(cubic):
    """elementwise products and sums in a fixed order: the fp64 form returns the bits it returned before the rewrite"""
    z, y, x = np.meshgrid(np.arange(9), np.arange(10), np.arange(11), indexing="ij")
    T = (((x * 7 + y * 13 + z * 29 + x * y * z) % 17) / np.float32(17)).astype(np.float32)
    pos = np.array([[1.25, 2.5, 3.75], [4.0, 5.0, 6.0], [7.999, 1.001, 2.3333333333333335], [3.1, 6.9, 1.0], [5.5, 3.0, 4.875]])
    assert [float(v).hex() for v in ref.interp(T, pos, cubic)] == INTERP_GOLDEN[cubic]


SCALINGS = {"both_2^-10": (2.0 ** -10, 2.0 ** -10), "both_2^13": (2.0 ** 13, 2.0 ** 13), "T_2^7": (1.0, 2.0 ** 7), "negated": (-1.0, -1.0)}


@pytest.mark.parametrize("name", list(SCALINGS))
def test_restatement_invariant_to_rounding(scene, name):
    """every threshold of the contract is relative: scaling both volumes, or T alone, by a power of two, or negating both, changes
    the fp64 restatement by rounding only"""
    R, T, _ = scene
    a, b = SCALINGS[name]
    q = [(20, 20, 20), (17, 22, 19), (23, 18, 21)]
    init = np.zeros((3, 12))
    init[:, [0, 4, 8]] = (0.1, 0.1, -0.1)
    base = ref.icgn(R, T, q, init=init, subset_radius=8)
    got = ref.icgn(np.float32(a) * R, np.float32(b) * T, q, init=init, subset_radius=8)
    assert (base["status"] == 0).all()
    assert np.array_equal(got["status"], base["status"]) and np.array_equal(got["iterations"], base["iterations"])
    assert np.abs(got["p"] - base["p"]).max() <= 1e-9 and np.abs(got["zncc"] - base["zncc"]).max() <= 1e-9
