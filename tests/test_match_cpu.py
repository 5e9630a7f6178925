"""CPU tests: the inputs of tests/match_cases.py do what they claim, on the CPU oracle (and, where oracle/_ref/libref3dsift.so was
built, on the reference's own matcher).  tests/test_gpu_match_edges.py runs the same cases through the HIP matcher and relies on what
is shown here: which column is best and second, which dealing regime a size reaches, that the guard has no reason to fire on the
planted cases and every reason on the tie cases.  Prints (pytest -s) the smallest gap / E ratios and the regime per size."""
import numpy as np
import pytest

import match_cases as mc
import oracle_lib as ol

THREADS = 16   # set explicitly: the oracle's default is the machine's CPU count


@pytest.fixture(scope="module", autouse=True)
def threads(orc):
    orc.set_threads(THREADS)
    yield
    orc.set_threads(0)


def want(orc, name, mode=1):
    return mc.oracle_match(orc, name, mode)


PLANTED = [k for k, v in mc.CASES.items() if v.quiet]


# ---- dealing ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m", list(mc.SIZES))
def test_dealing_regime_of_every_size(n, m):
    for v2 in (True, False):
        d = mc.dealing(n, m, v2)
        owned = np.zeros((d["rb"], d["nunits"]), int)
        for p in d["pieces"]:
            assert 0 <= p["slot"] < d["slots"], p
            assert p["slot"] < d["used"][p["rbi"]], ("the merge does not read a written slot", p)
            assert not (p["from_half"] and p["to_half"] and p["u_hi"] - p["u_lo"] == 1)
            owned[p["rbi"], p["u_lo"]:p["u_hi"]] += 1
        assert (owned == 1).all()
        print(f"({n}, {m}) v2={int(v2)}: rb {d['rb']} units {d['nunits']} nwg {d['nwg']} slots {d['slots']} used {sorted(set(d['used']))} "
              f"shares {d['share_sizes']} crosses {d['crosses']} -- {mc.SIZES[(n, m)]}")
    d, pieces = mc.dealing(n, m, True), mc.dealing(n, m, True)["pieces"]
    if (n, m) == (421, 421):
        assert d["nwg"] == 32 and d["share_sizes"] == [1] and set(d["used"]) == {8}
        assert [p["from_half"] for p in pieces] == [bool(w & 1) for w in range(32)] and all(p["to_half"] != p["from_half"] for p in pieces)
    if (n, m) == (40, 1500):
        assert d["slots"] == mc.MAX_SPLITS
    if (n, m) == (300, 1100):
        assert d["nwg"] == 15 * d["rb"] and d["share_sizes"] == [1, 2] and not d["crosses"]
        assert not any(p["from_half"] and p["to_half"] for p in pieces)   # every 2-unit share starts on a tile border: (300, 1300)
    if (n, m) == (300, 1300):
        assert d["nwg"] == 15 * d["rb"] and d["share_sizes"] == [1, 2] and not d["crosses"]
        assert any(p["from_half"] and p["to_half"] for p in pieces)
    if (n, m) == (6600, 1100):
        assert d["nwg"] == 768 < 15 * d["rb"] and d["crosses"]
        assert not mc.dealing(n, m, False)["crosses"]   # the whole-tile forms need (6700, 1200)
    if (n, m) == (6700, 1200):
        d1 = mc.dealing(n, m, False)
        assert d["crosses"] and d1["crosses"] and d1["nwg"] == 512 < 15 * d1["rb"]
    if max(n, m) <= 129:
        assert not d["crosses"] and d["share_sizes"] == [1]


def test_awkward_sizes_of_the_parity_module_never_cross_a_row_block():
    """what tests/test_gpu_parity.py::test_matcher_awkward_sizes reaches: its shares end on every row-block border"""
    for n, m in ((1500, 40), (2100, 2300)):
        assert not mc.dealing(n, m, True)["crosses"] and not mc.dealing(n, m, False)["crosses"]


# ---- planted cases --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", PLANTED)
def test_planted_columns_and_margins(orc, name):
    c = mc.CASES[name]()
    a, b = c["a"], c["b"]
    n, m = len(a), len(b)
    w = want(orc, name)
    first, second = mc.planted_columns(c)
    both = (first >= 0) & (second >= 0) & (first != second)
    if n <= m and m > 1:
        assert both.all()
    # the planted columns win wherever they exist, and the ratio filter keeps them
    assert np.array_equal(w["gIdx"][both], first[both]) and np.array_equal(w["sIdx"][both], second[both])
    only_second = (first < 0) & (second >= 0)
    assert np.array_equal(np.abs(w["gIdx"][only_second]), second[only_second])
    # the restatement over the planted columns alone gives the oracle's bits
    r = mc.restate(a[both], b, list(zip(first[both], second[both])))
    for k in r:
        assert mc.same(r[k], w[k][both]), k
    # gaps: second - third > 100 E on every row that has both planted columns
    g = mc.margins(a, b)
    with np.errstate(invalid="ignore"):
        ratio = ((g["second"] - g["third"]) / g["E"])[both]
    if both.any() and m > 2:
        print(f"{name}: min (second - third) / E = {ratio.min():.1f} over {int(both.sum())} rows")
        assert ratio.min() > 100
    # and on EVERY row of every pass the guard provably stays quiet (match_cases.quiet_margin: > 2 is the proof; E itself is
    # twice the first-order bound 768 * 2^-24 |a| |b| of an fp32 chain)
    q = [mc.quiet_margin(a, b)]
    for mode in (2, 3):
        rows = mc.masked_targets(w["gIdx"], m, mode)
        if len(rows):
            q.append(mc.quiet_margin(b, a, rows))
    print(f"{name}: min guard margin (max(second, FLT_MIN) - sixth) / E = {min(q):.2f}")
    assert min(q) > 2


@pytest.mark.parametrize("signed", (True, False))
@pytest.mark.parametrize("n,m", mc.GAP_SIZES)
def test_planted_gaps(n, m, signed):
    c = mc.planted(n, m, mc._shift(max(n, m)), 11, signed)
    g = mc.margins(c["a"], c["b"])
    lo1, lo2 = (0.36, 0.21) if signed else (0.146, 0.078)
    print(f"({n}, {m}) signed={signed}: best - second >= {(g['best'] - g['second']).min():.3f}, second - third >= {(g['second'] - g['third']).min():.3f}")
    # (the table's figures, at the precision it gives them)
    assert round((g["best"] - g["second"]).min(), 3) >= lo1 and round((g["second"] - g["third"]).min(), 3) >= lo2
    assert ((g["second"] - g["third"]) / g["E"]).min() > 100


def test_placement_sweep_covers_every_position(orc):
    names = [k for k, v in mc.CASES.items() if v.kind == "place"]
    rows, best, second = set(), set(), set()
    for name in names:
        c, w = mc.CASES[name](), want(orc, name)
        n, m = len(c["a"]), len(c["b"])
        assert (w["gIdx"] >= 0).all()
        rows |= set(np.arange(n) % 128)
        best |= set(w["gIdx"] % 128)
        second |= set(w["sIdx"] % 128)
        assert m - 1 in set(w["gIdx"]) | set(w["sIdx"])   # the last column is somebody's best or second
    every = set(range(128))
    assert rows == every and best == every and second == every
    for r in mc.RESIDUES:
        c = mc.CASES[f"place_r{r}"]()
        assert (len(c["a"]), len(c["b"]) % 128) == (130, r % 128)
        w = want(orc, f"place_sq_r{r}")
        assert w["gIdx"][-1] == len(w["gIdx"]) - 1 and (len(w["gIdx"]) - 1) in set(w["sIdx"])   # column m - 1: a best and a second


# ---- value classes ------------------------------------------------------------------------------------------------------------------
def test_scaled_indices_equal_the_unscaled(orc):
    base = want(orc, "planted")
    for name in ("scaled_m8_m8", "scaled_8_8", "scaled_m8_8"):
        w = want(orc, name)
        assert np.array_equal(np.abs(w["gIdx"]), np.abs(base["gIdx"])) and np.array_equal(w["sIdx"], base["sIdx"]), name
    for k in base:   # (-8, 8): the same products, the same bits
        assert mc.same(want(orc, "scaled_m8_8")[k], base[k]), k


def test_zero_rows_and_negative_scores(orc):
    none = np.float32(2 - 2 * mc.FLT_MIN)
    assert none == np.float32(2)
    w = want(orc, "zero_ref_rows")
    z = list(mc.ZERO_REF_ROWS)
    assert (w["gIdx"][z] == -1).all() and (w["sIdx"][z] == -1).all() and (w["gDist"][z] == none).all() and (w["sDist"][z] == none).all()
    w = want(orc, "zero_tar_rows")
    assert not set(mc.ZERO_TAR_ROWS) & (set(np.abs(w["gIdx"])) | set(w["sIdx"]))
    w = want(orc, "negative_only")
    assert (w["gIdx"] == -1).all() and (w["sIdx"] == -1).all() and (w["gDist"] == none).all()
    assert len(mc.masked_targets(w["gIdx"], mc.VM, 2)) == 0   # a mode-2 call without a reverse pass
    c = mc.CASES["sparse"]()
    assert 0.88 < (c["a"] == 0).mean() < 0.92 and 0.78 < (c["b"] == 0).mean() < 0.84
    c = mc.CASES["signed"]()
    assert (c["a"] < 0).mean() > 0.4


def test_tie_classes(orc):
    c, w = mc.CASES["one_hot"](), want(orc, "one_hot")
    s = c["a"].astype(np.float64) @ c["b"].astype(np.float64).T
    assert set(np.unique(s)) == {0.0, 1.0}
    ties = (s == 1).sum(axis=1)
    print("one_hot: ties per row", int(ties.min()), "..", int(ties.max()))
    assert ties.min() > 2 * mc.TOPK
    for i in range(len(s)):   # the lowest two columns win
        j = np.flatnonzero(s[i] == 1)
        assert (w["gIdx"][i], w["sIdx"][i]) == (j[0], j[1])
    assert (w["gDist"] == 0).all() and (w["sDist"] == 0).all()
    rows = list(mc.DUP_ROWS)
    for k in (5, 6, 7, 8):
        c, w = mc.CASES[f"dup_{k}"](), want(orc, f"dup_{k}")
        b = c["b"]
        for i in rows:
            copies = np.flatnonzero((b == b[i]).all(axis=1))
            assert len(copies) == k and (w["gIdx"][i] in (copies[0], -copies[0])) and w["sIdx"][i] == copies[1]
            assert w["gDist"][i] == w["sDist"][i]
            v2_half, top4_half, tile = (copies % 32) // 16, (copies % 128) // 64, copies // 128
            assert len(set(v2_half)) == 2 and len(set(top4_half)) == 2 and len(set(tile)) >= 2, (k, i, copies)
    # graded: the exact gaps between a row's eight best straddle E
    c = mc.CASES["graded"]()
    g = c["a"][rows].astype(np.float64) @ c["b"].astype(np.float64).T
    top = -np.sort(-g, axis=1)[:, :8]
    gaps = np.abs(np.diff(top, axis=1)) / mc.E_REL
    print(f"graded: gaps among the eight best / E from {gaps.min():.2e} to {gaps.max():.2e}")
    assert gaps.min() < 0.01 and gaps.max() > 1 and ((gaps > 0.01) & (gaps < 1)).any()


@pytest.mark.parametrize("name", mc.NONFINITE)
def test_nonfinite_follows_the_reference_arithmetic(orc, name):
    c, w, base = mc.CASES[name](), want(orc, name), want(orc, "planted")
    v, where, idx = c["nonfinite"]
    a, b = c["a"], c["b"]
    assert np.isfinite(a).sum() + np.isfinite(b).sum() == a.size + b.size - 1
    assert not np.isnan(w["gDist"]).any() and not np.isnan(w["sDist"]).any()
    col = a[:, mc.NF_COMPONENT] if where == "tar" else b[:, mc.NF_COMPONENT]
    if where == "tar" and v == "pinf":
        hit = col > 0   # a[k] * inf = +inf: the column is the best of these rows; a[k] == 0 gives NaN: never chosen
        assert hit.any() and (~hit).any()
        assert (np.abs(w["gIdx"][hit]) == idx).all() and (w["gDist"][hit] == -np.inf).all()
        assert (np.abs(w["gIdx"][~hit]) != idx).all() and (w["sIdx"][~hit] != idx).all()
    elif where == "tar":   # NaN or -inf scores: the column is never chosen, nothing else changes unless it was chosen before
        assert (np.abs(w["gIdx"]) != idx).all() and (w["sIdx"] != idx).all()
        keep = (np.abs(base["gIdx"]) != idx) & (base["sIdx"] != idx)
        for k in ("gIdx", "sIdx", "gDist", "sDist"):
            assert mc.same(w[k][keep], base[k][keep]), k
    else:
        others = np.arange(len(a)) != idx
        for k in ("gIdx", "sIdx", "gDist", "sDist"):
            assert mc.same(w[k][others], base[k][others]), k
        if v == "pinf":   # +inf where b[k] > 0, NaN where it is 0: the lowest two +inf columns
            j = np.flatnonzero(col > 0)
            assert (abs(w["gIdx"][idx]), w["sIdx"][idx]) == (j[0], j[1]) and w["gDist"][idx] == -np.inf
        else:             # NaN or -inf everywhere
            assert (w["gIdx"][idx], w["sIdx"][idx]) == (-1, -1) and w["gDist"][idx] == np.float32(2)


# ---- reverse-pass subsets -------------------------------------------------------------------------------------------------------------
def test_reverse_pass_subsets(orc):
    for count in mc.REVERSE_COUNTS:
        for mode in (2, 3):
            name = f"reverse_m{mode}_{count}"
            c, w = mc.CASES[name](), want(orc, name)
            rows = mc.masked_targets(w["gIdx"], len(c["b"]), mode)
            assert len(rows) == count, (name, len(rows))
            assert len(c["b"]) - 1 in rows and (count == 1 or 0 in rows)
            if mode == 3:
                assert len(mc.masked_targets(w["gIdx"], len(c["b"]), 2)) > count
    w = want(orc, "planted")
    assert len(mc.masked_targets(w["gIdx"], mc.VM, 3)) == 0   # a mode-3 call without a reverse pass
    assert len(mc.masked_targets(w["gIdx"], mc.VM, 2)) == mc.VN


# ---- the reference itself ---------------------------------------------------------------------------------------------------------------
needs_ref = pytest.mark.skipif(not ol.available("ref"), reason="oracle/_ref/libref3dsift.so is built only where the reference tree exists")


@needs_ref
@pytest.mark.parametrize("name", mc.VALUE_CLASSES)
def test_value_classes_on_the_reference(orc, name):
    ref = ol.load("ref")
    c = mc.CASES[name]()
    for mode in (1, 2, 3):
        x = ref.match(c["a"], c["ax"], c["b"], c["bx"], mc.THRESH, mode)
        y = mc.oracle_match(orc, name, mode)
        for k in y:
            assert mc.same(x[k], y[k]), (mode, k)
