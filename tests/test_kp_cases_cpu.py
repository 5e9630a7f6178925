"""CPU: the planted-keypoint cases of tests/kp_cases.py do what they claim, asserted on the oracle alone (tests/test_gpu_orient_edges.py and
tests/test_gpu_describe_edges.py then hold the HIP path to the oracle on every one of them).  Prints the coverage counts and the measured
fp64 ratio of the oracle's sequential sums (run with -s to see them)."""
import collections

import numpy as np
import pytest

import kp_cases as K
import oracle_lib as ol
from hipcheck import bits, descriptor_errors, nan_equal_bits


def _all_orient_cases(orc):
    ratio, corner = K.orient_straddles(orc)
    out = []
    for u in K.UNITS:
        out += K.orient_border(orc, u) + K.orient_sizes(orc, u)
    out += K.orient_tiles(orc) + K.orient_codes(orc) + K.orient_amplitude(orc) + ratio + corner
    for weak, strong, _, _ in K.orient_gg_straddles(orc):
        out += [weak, strong]
    out += [c for _, c, _ in K.orient_plants(orc)]
    return out


def test_every_code_occurs_and_clipped_windows_are_accepted(orc):
    codes = collections.Counter(K.oracle_orient(orc, c)[0] for c in K.orient_codes(orc))
    print("codes of the code family:", dict(codes))
    assert all(codes[k] > 0 for k in (-1, -2, -3, 1)), codes
    by_name = {c.name: K.oracle_orient(orc, c)[0] for c in K.orient_codes(orc)}
    assert by_name["code_constant"] == -1
    assert all(by_name["code_blob%d" % i] == -2 for i in range(3))
    ramps = [v for n, v in by_name.items() if n.startswith("code_ramp")]
    assert ramps.count(-2) >= 6 and -1 not in ramps, ramps   # the ratio test runs on rounding noise: some ramps pass it and end at the corner test
    n_clipped = 0
    for c in K.orient_border(orc, 1.0):
        if c.name.startswith("oborder_L0") and "_face" in c.name and K.clipped(c.level.shape, 1.0, c.rec, K.ori_radius(c.args[0])):
            n_clipped += K.oracle_orient(orc, c)[0] == 1
    print("accepted keypoints with a clipped window in the face sweep of L0:", n_clipped)
    assert n_clipped >= 8
    for u in K.UNITS:
        cc = collections.Counter(K.oracle_orient(orc, c)[0] for c in K.orient_border(orc, u) + K.orient_sizes(orc, u))
        print("unit %g border + size families:" % u, dict(cc))
        assert len(cc) >= 2


def test_level_rows_are_not_multiples_of_four(orc):
    nz, ny, nx = K.levels(orc)["L1"].shape
    assert nx % 4 and ny % 4 and (nx * ny) % 4


def test_straddle_triples_flip_at_the_planted_threshold(orc):
    ratio, corner = K.orient_straddles(orc)
    assert len(ratio) >= 60 and len(corner) >= 60
    rc = [K.oracle_orient(orc, c)[0] for c in ratio]
    cc = [K.oracle_orient(orc, c)[0] for c in corner]
    assert rc == [-2, 1, 1] * (len(ratio) // 3), rc
    assert cc == [1, 1, -3] * (len(corner) // 3), cc
    n_border = sum(K.clipped(c.level.shape, 1.0, c.rec, 9.0) for c in ratio[::3])
    gg = K.orient_gg_straddles(orc)
    assert len(gg) >= 5
    for weak, strong, lo, hi in gg:
        assert np.nextafter(np.float32(lo), np.float32(2)) == np.float32(hi)
        assert K.oracle_orient(orc, weak)[0] == -1 and K.oracle_orient(orc, strong)[0] != -1
    print("straddles: %d ratio triples (%d with a clipped window), %d corner triples, %d |mean gradient|^2 pairs at factors %s"
          % (len(ratio) // 3, n_border, len(corner) // 3, len(gg), ["%.8g" % lo for _, _, lo, _ in gg]))


def test_path_table_of_the_orientation_windows(orc):
    seen = collections.Counter()
    for c in K.orient_sizes(orc, 1.0):
        _, R, side, pos, _ = c.name.split("_")
        path, tw, th, n_len, cp = K.orient_path(c.level.shape, 1.0, c.rec, c.args[0])
        want = K.SIZE_PATHS[(int(R[1:]), side)]["c x2 y2 z2".split().index(pos)]
        assert K._LETTER[path] == want, (c.name, path, tw, th, n_len, cp)
        seen[path] += 1
    tiles = {n: (s, t, p) for n, s, t, p in K.TILE_PATHS}
    for c in K.orient_tiles(orc):
        sigma, (tw, th), want = tiles[c.name.rsplit("_", 2)[0]]
        path, gtw, gth, n_len, cp = K.orient_path(c.level.shape, 1.0, c.rec, c.args[0])
        assert (gtw, gth, path) == (tw, th, want), (c.name, gtw, gth, n_len, cp, path)
        # restated from the condition itself, not from orient_path
        lds = gtw <= 28 and gth <= 27 and n_len <= 256
        assert (path == "global") == (not lds) and (path == "lds_list") == (lds and cp <= 512)
        seen[path] += 1
    assert K.orient_path(K.levels(orc)["L0"].shape, 1.0, K.orient_tiles(orc)[-1].rec, 5.4)[3] > 256
    for u in K.UNITS[1:]:
        for c in K.orient_border(orc, u) + K.orient_sizes(orc, u):
            seen[K.orient_path(c.level.shape, u, c.rec, c.args[0])[0]] += 1
    print("path classes:", dict(seen))
    assert seen["lds_list"] > 0 and seen["lds_box"] >= 8 and seen["global"] > 0 and seen["empty"] == 0


def test_fp64_bar_of_the_sequential_sums(orc):
    """|sum - fp64 sum| / sum |term| of the oracle's fp32 sequential window sums, over every orientation case: the number the GPU test's
    bar on rejected keypoints is 4x of (kp_cases.ORACLE_SEQ_RATIO)"""
    worst, name, n, poisoned = 0.0, None, 0, 0
    for c in _all_orient_cases(orc):
        _, k = K.oracle_orient(orc, c)
        q = K.sum_ratio(k, *K.orient_sums(c.level, c.unit, c.rec, c.args[0]))
        n += 1
        if q is None:
            poisoned += 1
        elif q > worst:
            worst, name = q, c.name
    print("fp64 ratio of the oracle's sequential sums: %.4g at %s (%d cases, %d poisoned); bar of the GPU test: %.4g" % (worst, name, n, poisoned, K.FP64_BAR))
    assert 0.99 * K.ORACLE_SEQ_RATIO <= worst <= K.ORACLE_SEQ_RATIO, worst   # the constant IS the measurement
    assert poisoned >= 20


def test_value_plants(orc):
    """(a) and (d) leave the oracle's result bit-identical to the unplanted level, (b) and (c) change it -- both stages"""
    kinds = collections.Counter()
    for kind, c, base in K.orient_plants(orc):
        r1, k1 = K.oracle_orient(orc, c)
        r0, k0 = K.oracle_orient(orc, base)
        same = r1 == r0 and k1.tobytes() == k0.tobytes()
        assert same == (kind in "ad"), c.name
        kinds["orient " + kind] += 1
    for kind, c, base in K.describe_plants(orc):
        k1, d1 = K.oracle_describe(orc, c)
        k0, d0 = K.oracle_describe(orc, base)
        same = d1.tobytes() == d0.tobytes()
        assert same == (kind == "a"), c.name
        kinds["describe " + kind] += 1
    print("value plants:", dict(kinds))
    assert len(kinds) == 7


def test_amplitude_sweep_samples_the_absolute_tests(orc):
    """the reference is not amplitude invariant (|g|^2 >= eps and fabs(det) < eps are absolute): the oracle's rows at e and e + 1 differ by
    more than the descriptor bars for at least 5 exponents, else the sweep samples nothing"""
    cases = K.describe_amplitude(orc)
    rows = {c.name: K.oracle_describe(orc, c)[1] for c in cases}
    moved = set()
    for c in cases:
        head, e = c.name.rsplit("_e", 1)
        nxt = rows.get("%s_e%d" % (head, int(e) + 1))
        if nxt is not None:
            _, worst_kp, worst_abs = descriptor_errors(rows[c.name][None], nxt[None])
            if worst_kp > 2e-5 or worst_abs > 1e-4:
                moved.add(int(e))
    print("amplitude: the oracle's row moves by more than the bars between e and e + 1 at e =", sorted(moved))
    assert len(moved) >= 5
    zero = [c.name for c in cases if not rows[c.name].any()]
    print("amplitude: all-zero rows:", len(zero))


def test_descriptor_families_cover_their_forms(orc):
    assert len(K.rotations()) == 35 and len(K.mesh_directions(orc)) == 62
    for n, m in K.rotations():
        assert np.allclose(m.astype(np.float64) @ m.astype(np.float64).T, np.eye(3), atol=1e-6) and np.linalg.det(m.astype(np.float64)) > 0, n
    lens = [K.lut_len_nin(K.desc_radius(s), 1.0) for s in K.DESC_SCALES]
    assert lens[2][0] <= 1536 < lens[3][0]                       # either side of kMaxDescLut
    assert 4.18879 * lens[4][1] ** 1.5 > 2 ** 18                 # the `share` branch of unit_fails
    assert int(np.ceil(float(K.desc_radius(3.9)))) == 56 and int(np.ceil(float(K.desc_radius(1.0)))) == 15
    sizes = K.describe_sizes(orc)
    flat = [c for c in sizes if "flat" in c.name]
    assert len(flat) == 2 and all(not K.oracle_describe(orc, c)[1].any() for c in flat)
    assert all(K.oracle_describe(orc, c)[1].any() for c in sizes if "flat" not in c.name)
    # the icosahedron family: the rotated gradients of every window hit more than one face
    for c in K.describe_icosahedron(orc)[::7]:
        assert np.count_nonzero(K.oracle_describe(orc, c)[1].reshape(64, 12).sum(axis=0)) >= 3, c.name
    guess = K.describe_first_guess(orc)
    assert len(guess) == 3 * 18


def _subsample(orc):
    ratio, corner = K.orient_straddles(orc)
    o = K.orient_border(orc, 1.0)[::9] + K.orient_border(orc, 4.0)[::23] + K.orient_sizes(orc, 1.0)[::11] + K.orient_tiles(orc)[::3] + \
        K.orient_codes(orc)[:16] + K.orient_amplitude(orc)[::9] + ratio[:9] + corner[:9] + [c for _, c, _ in K.orient_plants(orc)][::6]
    d = K.describe_border(orc, 1.0)[::17] + K.describe_border(orc, 2.0)[::29] + K.describe_rotations(orc)[::6] + K.describe_icosahedron(orc)[::9] + \
        K.describe_amplitude(orc)[::9] + [c for _, c, _ in K.describe_plants(orc)][::3] + [c for c in K.describe_sizes(orc) if c.level.shape[0] < 100]
    return o, d


@pytest.mark.skipif(not ol.available("ref"), reason="oracle/_ref/libref3dsift.so is built only where the reference tree exists")
def test_cases_agree_with_the_reference(orc):
    """the real reference's orient_one / describe_one on a fixed subsample: codes equal, records and descriptors bit for bit (the fields
    tests/test_oracle_vs_ref.py compares; a NaN by position, hipcheck.nan_equal_bits)"""
    ref = ol.load("ref")
    o, d = _subsample(orc)
    # a structure tensor that is not finite is left out HERE only (the GPU tests hold the HIP path to the oracle on these cases too): Eigen's
    # EigenSolver returns early with NumericalIssue on such a matrix and the reference goes on to read eigenvalues that were never written
    o = [c for c in o if np.isfinite(K.oracle_orient(orc, c)[1]["str_tensor"]).all()]
    assert len(o) >= 40 and len(d) >= 40
    for c in o:
        sigma, mer, ct = c.args
        r0, k0 = orc.orient_one(c.rec, c.level, c.unit, sigma, mer, ct)
        r1, k1 = ref.orient_one(c.rec, c.level, c.unit, sigma, mer, ct)
        assert r0 == r1, (c.name, r0, r1)
        fields = ("str_tensor", "win") + (("eigvalue", "Rotation") if r0 == 1 else ())
        for f in fields:
            assert nan_equal_bits(k0[f], k1[f]) == 0, (c.name, f)
    for c in d:
        k0, d0 = orc.describe_one(c.rec, c.level, c.unit)
        k1, d1 = ref.describe_one(c.rec, c.level, c.unit)
        assert np.array_equal(bits(k0["Rotation"]), bits(k1["Rotation"])), c.name
        assert nan_equal_bits(d0, d1) == 0, (c.name, nan_equal_bits(d0, d1))
    print("reference agreement: %d orientation and %d descriptor cases" % (len(o), len(d)))
