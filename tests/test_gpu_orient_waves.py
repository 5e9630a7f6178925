"""-m gpu: what k_orient (kernels_orient.hip) carries from window to window and from plane to plane in scalar registers.

MANY WINDOWS PER WAVE.  sift3d_orient_keypoint orients one keypoint, and the small parity volumes have fewer extrema than the 32 768 waves
of the product's grid: there a wave never meets a second window.  hook("ori_grid", n) launches both k_orient instantiations with n
workgroups of four waves; with n = 1 and n = 3 the extrema of a 56 x 48 x 40 volume are dealt to 4 and 12 waves, each of which orients
many windows of different levels one after the other -- bounds, trip counts, the table of running starts and the wave's weight copy of
the previous window must not leak into the next.  The three runs (n = 1, 3, default) agree byte for byte on every record and the codes
equal the oracle's.  Twice: the default sigma and sigma_default = 2.0 (other window sizes).

PLANE SIZES AT THE PASS BOUNDARY.  The entries of a plane are fetched and processed in passes of 64 for ceil(cnt / 64) passes.  A lattice
disc has 4 k + 1 points, never a multiple of 64: the boundary that exists is "full passes plus one point" (129 = 2 * 64 + 1, 193 = 3 * 64
+ 1).  Planted keypoints whose sphere has the largest squared offset nin = 40, 61, 131 (421 points: the default's largest), 164 (517
points > 512: the list is declined), at the centre and two voxels from the x, y and z faces of the 52 x 44 x 48 level, against the
oracle's orient_one with the bars of tests/test_gpu_orient_edges.py.  A whole window of nin = 164 is 29 voxels wide, more than the LDS
tile: at those four positions it takes the global path (asserted), so the box scan over the LDS tiles it is here for is reached at two
more positions, two voxels from an x AND a y face.  The same two positions carry nin = 160: 505 points, the largest plane the list
takes, so that the planes of the list windows need every number of passes from 1 to 8 (asserted).  The list windows also fetch only
the tile pieces their sphere can read: accepted keypoints bit-identical to the oracle at the centre and clipped at three faces."""
import importlib

import numpy as np
import pytest

import kp_cases as K
from hipcheck import bits, nan_equal_bits

pytestmark = pytest.mark.gpu

VOLUME = dict(shape=(56, 48, 40), seed=7, noise=0.01)   # the volume of test_gpu_parity.py::test_orientation_codes_vs_oracle


@pytest.fixture(scope="module")
def capi():
    m = importlib.import_module("3dsift_amd.capi")
    assert m.device_count() >= 1, "GPU tests need a visible MI355X (no CPU fallback exists)"
    return m


@pytest.mark.parametrize("params", [dict(), dict(sigma_default=2.0)], ids=["default", "sigma2.0"])
def test_many_windows_per_wave(capi, orc, synth, params):
    vol = synth.blobs(VOLUME["shape"], seed=VOLUME["seed"], noise=VOLUME["noise"])
    runs = {}
    for n in (1, 3, 0):
        with capi.hook("ori_grid", n):
            g = capi.CreateCSIFT3D(vol, **params).run_stages(4)
            runs[n] = (g.extrema(), g.orientation_codes())
    ext, codes = runs[0]
    accepted = int((codes == 1).sum())
    print("%d extrema, %d accepted; 4 and 12 waves" % (len(ext), accepted))
    assert len(ext) > 12, "every wave of the 3-workgroup run must meet a second window"
    assert accepted > 4, "the reference-order pass orients the accepted extrema: its 4 waves of the 1-workgroup run must loop too"
    for n in (1, 3):
        assert runs[n][0].tobytes() == ext.tobytes(), "records differ between %d workgroups and the default grid" % n
        assert runs[n][1].tobytes() == codes.tobytes(), "codes differ between %d workgroups and the default grid" % n
    o = orc.extractor(vol, **params).run(3)
    e = o.extrema()
    assert len(codes) == len(e)
    want = []
    for k in e:
        lvl = o.gss(int(k["octave"]), int(k["level"]))
        unit = o.level_info(0, int(k["octave"]) * 6 + int(k["level"]))[1][0]
        want.append(orc.orient_one(k, lvl, unit, np.float32(1.5) * k["scale"])[0])
    assert np.array_equal(codes, np.array(want, np.int32))


# ---- plane sizes ---------------------------------------------------------------------------------------------------------------------
# nin -> (points of the central plane, path of the four face positions c / x2 / y2 / z2, path two voxels from an x AND a y face or None)
# (nin = 160: 505 points, the largest plane the list takes -- all eight passes; whole, that window is 29 wide as well)
PLANES = {40: (129, "lds_list", None), 61: (193, "lds_list", None), 131: (421, "lds_list", None), 160: (505, "global", "lds_list"),
          164: (517, "global", "lds_box")}


def sigma_for(nin):
    """a sigma whose radius 3 sigma (fp32) has nin as the largest squared offset inside the sphere at unit 1"""
    sigma = float(K.f32(np.sqrt(nin + 0.4) / 3.0))
    assert K.lut_len_nin(K.ori_radius(sigma), 1.0)[1] == nin
    return sigma


def plane_counts(nin):
    """lattice points of the sphere n <= nin in every plane dz = -R .. R"""
    r = int(np.floor(np.sqrt(nin)))
    d = np.arange(-r, r + 1)
    n2 = d[:, None] ** 2 + d[None, :] ** 2
    return [int((n2 + dz * dz <= nin).sum()) for dz in d]


def plane_cases(orc):
    L = K.levels(orc)["L0"]
    nz, ny, nx = L.shape
    assert (nx, ny, nz) == (52, 44, 48)
    out = []
    for nin, (central, path, corner_path) in PLANES.items():
        sigma = sigma_for(nin)
        pos = [(tag, x, y, z, path) for tag, x, y, z in K.size_positions(L.shape)]
        if corner_path:
            pos += [("x2y2", 2, 2, nz // 2, corner_path), ("x2y2far", nx - 3, ny - 3, nz // 2, corner_path)]
        for tag, x, y, z, p in pos:
            out.append((K.Case("oplane_n%d_%s" % (nin, tag), L, 1.0, K.rec_at(x, y, z, 2.0), (sigma, 0.9, 0.4)), p))
    return out


def test_plane_cases_are_what_they_claim(orc):
    for nin, (central, _, _) in PLANES.items():
        counts = plane_counts(nin)
        assert max(counts) == counts[len(counts) // 2] == central == K.central_plane(nin), (nin, counts)
        assert all(c % 4 == 1 for c in counts), "a lattice disc has 4 k + 1 points"
        assert (central <= 512) == (nin != 164)
    assert 129 == 2 * 64 + 1 and 193 == 3 * 64 + 1   # full passes plus one point
    # the planes of the list windows need every number of passes from 1 to 8
    assert {-(-c // 64) for nin in (40, 61, 131, 160) for c in plane_counts(nin)} == set(range(1, 9))
    for c, path in plane_cases(orc):
        got = K.orient_path(c.level.shape, c.unit, c.rec, c.args[0])
        assert got[0] == path, (c.name, got)
    paths = [p for _, p in plane_cases(orc)]
    assert paths.count("lds_list") == 14 and paths.count("lds_box") == 2 and paths.count("global") == 8


def test_plane_sizes_at_the_pass_boundary(capi, orc):
    bad, worst = [], 0.0
    for c, _ in plane_cases(orc):
        sigma, mer, ct = c.args
        rec = np.array([c.rec], dtype=capi.KP_DTYPE)
        got, rec = capi.orient_keypoint(c.level, c.unit, rec, sigma, mer, ct), rec[0]
        want, ko = K.oracle_orient(orc, c)
        st = rec["str_tensor"]
        if got != want:
            bad.append((c.name, "code %d, oracle %d" % (got, want)))
        elif not (bits(st[3]) == bits(st[1]) and bits(st[6]) == bits(st[2]) and bits(st[7]) == bits(st[5])):
            bad.append((c.name, "str_tensor is not symmetric"))
        elif want == 1:
            for f in ("str_tensor", "win", "eigvalue", "Rotation"):
                if nan_equal_bits(rec[f], ko[f]):
                    bad.append((c.name, "%s differs from the oracle's in %d elements" % (f, nan_equal_bits(rec[f], ko[f]))))
        else:
            q = K.sum_ratio(rec, *K.orient_sums(c.level, c.unit, c.rec, sigma))
            assert q is not None, c.name   # L0 is finite
            worst = max(worst, q)
            if not q <= K.FP64_BAR:
                bad.append((c.name, "window sums off the fp64 sums by %.3g of sum |term| (bar %.3g)" % (q, K.FP64_BAR)))
    print("%d cases, %d wrong; rejected keypoints: window sums within %.3g of the fp64 sums (bar %.3g)" % (len(plane_cases(orc)), len(bad), worst, K.FP64_BAR))
    assert not bad, bad
