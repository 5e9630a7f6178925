"""Inputs and expectations of the matcher's edge tests (tests/test_match_cpu.py, tests/test_gpu_match_edges.py).  Plain NumPy, no GPU.

  planted(n, m, shift, seed, signed)  descriptor sets whose best and second-best column are known per row
  restate(a, b, cols)                 calMatches (Src/cMatcher.cc:17-23, 40-79) + filter (:81-97) over chosen columns
  dealing(n, m, v2)                   the share arithmetic of match_rows_device / the score kernels / k_merge_top4, restated
  margins(a, b)                       per row: exact best, second, third, sixth score and the guard's bound E
  SIZES, CASES                        every case by name; CASES[name]() builds it (cached)

A case is a dict: a, ax, b, bx (float32), kind ('size' | 'place' | 'value' | 'reverse'), and
  quiet   the fast path must answer by itself: the GPU test asserts exact_rows == 0 (the CPU module proves the margins first)
  fires   a lower bound of exact_rows in mode 1 (rows the guard MUST hand to k_exact_rows), or None
"""
import functools

import numpy as np

KD = 768
BM = BN = 128
TOPK = 6
MAX_SPLITS = 16
FLT_MIN = float(np.finfo(np.float32).tiny)
FLT_MAX = float(np.finfo(np.float32).max)
E_REL = 9.16e-5 * 1.0002   # k_rescore's bound, per unit |a_i| * max|b| (the 1.0002 covers its rounded-up norms)
THRESH = 0.85
F32 = np.float32


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def unit_rows(rng, n, signed, sparse=0.0):
    """n unit rows (float64): signed Gaussian, or clipped non-negative like the extractor's; `sparse` = share of exact zeros"""
    c = rng.normal(size=(n, KD)) if signed else np.clip(rng.normal(0.02, 0.03, size=(n, KD)), 0, None)
    if sparse:
        c = c * (rng.random((n, KD)) >= sparse)
    return c / np.linalg.norm(c, axis=1, keepdims=True)


def _xyz(rng, n):
    return rng.uniform(0, 100, (n, 3)).astype(F32)


def planted(n, m, shift, seed, signed, sparse=0.0):
    """A = c[:n], B[j] = normalize(c[j] + 0.5 c[(j + shift) % N]) cut to m, N = max(n, m): row i has best column i and second-best
    (i - shift) % N wherever those columns exist; every other score is far below."""
    N = max(n, m)
    rng = _rng(seed)
    c = unit_rows(rng, N, signed, sparse)
    b = c + 0.5 * c[(np.arange(N) + shift) % N]
    b /= np.linalg.norm(b, axis=1, keepdims=True)
    return dict(a=c[:n].astype(F32), ax=_xyz(rng, n), b=b[:m].astype(F32), bx=_xyz(rng, m), N=N, shift=shift, signed=signed)


def planted_columns(case):
    """per row: the planted (best, second) columns, -1 where the column is cut away"""
    n, m, N = len(case["a"]), len(case["b"]), case["N"]
    i = np.arange(n)
    first = np.where(i < m, i, -1)
    second = (i - case["shift"]) % N
    return first, np.where(second < m, second, -1)


def restate(a, b, cols, thresh=THRESH):
    """calMatches over the columns cols[i] of row i (any order), then the ratio filter: fp32 product, fp64 running sum in k order,
    strict '>' from FLT_MIN in ascending column order, d = float32(2 - 2 s)."""
    n = len(a)
    gi = np.full(n, -1, np.int32); si = np.full(n, -1, np.int32)
    gd = np.zeros(n, F32); sd = np.zeros(n, F32)
    with np.errstate(all="ignore"):
        for i in range(n):
            d1 = d2 = np.float64(FLT_MIN)
            i1 = i2 = -1
            for j in sorted(set(int(c) for c in cols[i] if c >= 0)):
                s = np.cumsum((a[i] * b[j]).astype(np.float64))[-1]   # sequential, like the reference's loop
                if s > d1:
                    d2, i2, d1, i1 = d1, i1, s, j
                elif s > d2:
                    d2, i2 = s, j
            gd[i], sd[i], gi[i], si[i] = F32(2 - 2 * d1), F32(2 - 2 * d2), i1, i2
        t2 = thresh * thresh
        for i in range(n):
            if gi[i] >= 0 and np.float64(gd[i] / sd[i]) >= t2:
                gi[i] *= -1
    return dict(gIdx=gi, sIdx=si, gDist=gd, sDist=sd)


def masked_targets(gIdx, m, mode):
    """countMatched + toMask (Src/cMatcher.cc:114-131) over a forward result: the targets the reverse pass of `mode` runs over"""
    cnt = np.bincount(gIdx[gIdx >= 0], minlength=m)
    return np.flatnonzero(cnt > (0 if mode == 2 else 1))


def margins(a, b, rows=None):
    """Exact (float64) scores of `rows` of a against every row of b: per row best, second, third and TOPK-th score (-inf where b has
    fewer rows) and the guard's bound E = E_REL |a_i| max|b|.  Only for finite inputs."""
    a64 = a.astype(np.float64) if rows is None else a[rows].astype(np.float64)
    b64 = b.astype(np.float64)
    s = a64 @ b64.T
    m = s.shape[1]
    k = min(m, TOPK)
    top = -np.sort(-np.partition(s, m - k, axis=1)[:, m - k:], axis=1) if m else np.zeros((len(a64), 0))
    top = np.concatenate([top, np.full((len(a64), TOPK - top.shape[1]), -np.inf)], axis=1)
    e = E_REL * np.linalg.norm(a64, axis=1) * (np.linalg.norm(b64, axis=1).max() if m else 0.0)
    return dict(best=top[:, 0], second=top[:, 1], third=top[:, 2], sixth=top[:, TOPK - 1], E=e)


def quiet_margin(a, b, rows=None):
    """min over rows of (max(second, FLT_MIN) - sixth) / E.  k_rescore sends a row to k_exact_rows unless s4 + E < d2, where d2 is
    the exact second-best score (at least FLT_MIN) and s4 the TOPK-th largest fp32 score.  Every fp32 score is within E of the exact
    one, so s4 <= sixth + E: a margin above 2 proves that the guard stays quiet.  inf where b has fewer than TOPK rows."""
    g = margins(a, b, rows)
    with np.errstate(all="ignore"):
        r = (np.maximum(g["second"], FLT_MIN) - g["sixth"]) / g["E"]
    return float(r.min()) if len(r) else np.inf


# ---------------------------------------------------------------------------------------------------------------------------------
# the dealing of (row block, unit) pairs to workgroups: match_rows_device, k_scores_topk2 / k_scores_top4, k_merge_top4
# ---------------------------------------------------------------------------------------------------------------------------------
def dealing(n, m, v2=True):
    rb, ntiles = -(-n // BM), -(-m // BN)
    nunits = 2 * ntiles if v2 else ntiles   # the second form deals half tiles
    total = rb * nunits
    nwg = max(1, min((3 if v2 else 2) * 256, total, (MAX_SPLITS - 1) * rb))
    slots = min(MAX_SPLITS, -(-nunits * nwg // total) + 1)
    pieces = []
    for w in range(nwg):
        L0, L1 = w * total // nwg, (w + 1) * total // nwg
        L = L0
        while L < L1:
            rbi = L // nunits
            u_lo = L - rbi * nunits
            u_hi = min(nunits, u_lo + (L1 - L))
            L += u_hi - u_lo
            wfirst = -(-((rbi * nunits + 1) * nwg) // total) - 1
            pieces.append(dict(wg=w, rbi=rbi, u_lo=u_lo, u_hi=u_hi, slot=w - wfirst, L0=L0, L1=L1,
                               from_half=bool(v2 and u_lo & 1), to_half=bool(v2 and u_hi & 1)))
    used = []
    for r in range(rb):   # k_merge_top4
        X, Y = r * nunits, (r + 1) * nunits
        wfirst, wlast = -(-((X + 1) * nwg) // total) - 1, -(-(Y * nwg) // total) - 1
        used.append(min(slots, wlast - wfirst + 1))
    per_wg = np.bincount([p["wg"] for p in pieces], minlength=nwg)
    return dict(rb=rb, ntiles=ntiles, nunits=nunits, total=total, nwg=nwg, slots=slots, pieces=pieces, used=used,
                crosses=bool((per_wg > 1).any()), share_sizes=sorted(set(p["L1"] - p["L0"] for p in pieces)))


# (n, m) -> the regime the size is there for (tests/test_match_cpu.py proves each with dealing()).  (6700, 1200) is the (6600, 1100)
# of the k_scores_top4 forms, which deal whole tiles to 512 workgroups: their shares cross a row block only once rb >= 35 and
# rb * ntiles > 512.
SIZES = {
    (6, 6): "around TOPK: exactly TOPK columns",
    (5, 7): "around TOPK: one column more",
    (7, 5): "around TOPK: a short list, s4 = -FLT_MAX",
    (1, 1): "single row, single column",
    (129, 33): "one row past a row block; one column past a 32-column block",
    (33, 129): "one row past a wave; one column past a tile",
    (421, 421): "32 workgroups of exactly one half tile, upper and lower halves alternating, 8 slots per row block",
    (40, 1500): "slots = 16, the cap",
    (300, 1100): "nwg = 15 rb; shares of 1 and 2 units, the 2-unit shares are whole tiles",
    (300, 1300): "nwg = 15 rb; shares of 1 and 2 units; a share from an upper half to a lower half",
    (6600, 1100): "nwg = 768 < 15 rb; a share crosses a row-block border (second form)",
    (6700, 1200): "nwg = 512 < 15 rb; a share crosses a row-block border in the k_scores_top4 forms too",
}
RESIDUES = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 0)
GAP_SIZES = ((421, 421), (300, 1100), (3840, 4096))   # where the planted gaps are checked for both kinds of rows

VN, VM, VSHIFT = 200, 333, 100
DUP_ROWS = (0, 5, 17, 31, 32, 47, 63, 64, 65, 100, 127, 128, 129, 150, 180, 199)   # rows whose best target gets copies
GRADED_SCALES = (2.0 ** -24, 2.0 ** -24, 2.0 ** -20, 2.0 ** -16, 2.0 ** -16, 2.0 ** -12, 2.0 ** -8)
NF_COMPONENT = 7
NF_VALUES = {"nan": np.nan, "pinf": np.inf, "ninf": -np.inf}
NF_PLACES = [("tar", 0), ("tar", 5), ("tar", 21), ("tar", 69), ("tar", VM - 1), ("ref", 0), ("ref", 127), ("ref", VN - 1)]
ZERO_REF_ROWS = (0, 63, 64, 199)
ZERO_TAR_ROWS = (0, 5, 21, 332)
REVERSE_COUNTS = (1, 127, 128, 129)


def _shift(N):
    return 1 if N < 8 else (5 * N) // 13


def _base(signed=False, sparse=0.0):
    return planted(VN, VM, VSHIFT, 900 + int(signed) + (2 if sparse else 0), signed, sparse)


def _copies(k=None, graded=False):
    """copies of the best target of every row in DUP_ROWS, written over the columns VN .. VM - 1 in a shuffled order: they land in
    the tiles 1 and 2 and in both lane halves of either form, the original stays in tile 0 or 1"""
    c = _base()
    rng = _rng(77)
    pool = list(VN + rng.permutation(VM - VN))
    per = len(GRADED_SCALES) if graded else k - 1
    assert per * len(DUP_ROWS) <= len(pool)
    place = lambda j: (j // 128, (j % 128) // 64, (j % 32) // 16)   # tile, lane half of k_scores_top4, lane half of k_scores_topk2
    seen = {r: set() for r in DUP_ROWS}
    b = c["b"].copy()
    for q in range(per):   # a row's first copies go to places it has no copy in yet
        for r in DUP_ROWS:
            j = next((j for j in pool if place(j) not in seen[r]), pool[0])
            pool.remove(j)
            seen[r].add(place(j))
            b[j] = (c["b"][r].astype(np.float64) * (1 + GRADED_SCALES[q] * rng.normal(size=KD))).astype(F32) if graded else c["b"][r]
    c["b"] = b
    return c


def _one_hot():
    rng = _rng(55)
    ks = np.sort(rng.choice(KD, 8, replace=False))
    eye = np.eye(KD, dtype=F32)
    a = eye[ks[np.arange(VN) % 8]]             # every k has reference rows
    b = eye[ks[rng.integers(0, 8, VM)]]
    return dict(a=a, ax=_xyz(rng, VN), b=b, bx=_xyz(rng, VM))


def _nonfinite(value, where, idx):
    c = _base()
    key = "b" if where == "tar" else "a"
    x = c[key].copy()
    x[idx, NF_COMPONENT] = NF_VALUES[value]
    c[key] = x
    return c


def _reverse(count, mode, seed):
    """A set whose reverse pass in `mode` runs over exactly `count` targets.  Targets are planted over m rows; the reference set
    holds one row for each target that is to be matched (mode 3: a second, weaker one for each target that is to be masked, and
    single rows for 60 more targets, which stay unmasked) and 40 unrelated rows, which the ratio filter rejects."""
    m, shift = 300, 7
    rng = _rng(seed)
    c = unit_rows(rng, m, True)
    b = c + 0.5 * c[(np.arange(m) + shift) % m]
    b /= np.linalg.norm(b, axis=1, keepdims=True)
    inner = 1 + rng.permutation(m - 2)
    chosen = np.array([m - 1] if count == 1 else [0, m - 1] + list(inner[:count - 2]))
    rows = [c[chosen]]
    if mode == 3:
        second = c[chosen] + 0.5 * unit_rows(rng, count, True)
        rows.append(second / np.linalg.norm(second, axis=1, keepdims=True))
        rows.append(c[inner[count:count + 60]])
    rows.append(unit_rows(rng, 40, True))
    a = np.concatenate(rows)
    a = a[rng.permutation(len(a))]
    return dict(a=a.astype(F32), ax=_xyz(rng, len(a)), b=b.astype(F32), bx=_xyz(rng, m), count=count, for_mode=mode)


def _scaled(ea, eb):
    c = _base()
    c["a"] = (c["a"] * F32(2.0 ** ea)).astype(F32)
    c["b"] = (c["b"] * F32(2.0 ** eb)).astype(F32)
    return c


def _edit(key, fn):
    c = _base()
    x = c[key].copy()
    fn(x)
    c[key] = x
    return c


def _zero(x, rows):
    x[list(rows)] = 0


def _negative_only():
    c = _base()
    c["a"], c["b"] = np.abs(c["a"]), -np.abs(c["b"])
    return c


def _build():
    cases = {}

    def add(name, kind, fn, quiet=False, fires=None, **extra):
        @functools.lru_cache(maxsize=None)
        def make():
            c = fn()
            c.update(name=name, kind=kind, quiet=quiet, fires=fires, **extra)
            return c
        make.kind, make.quiet, make.fires = kind, quiet, fires
        cases[name] = make

    for (n, m) in SIZES:
        add(f"size_{n}x{m}", "size", functools.partial(planted, n, m, _shift(max(n, m)), 100 + n + m, False), quiet=True)
    for r in RESIDUES:   # row n - 1 / column m - 1 in every residue class; shift 1: best and second are neighbours
        add(f"place_r{r}", "place", functools.partial(planted, 130, 256 + r, 1, 300 + r, True), quiet=True)
    for r in RESIDUES:   # square: column m - 1 is a best; shift 129: best and second in different tiles
        add(f"place_sq_r{r}", "place", functools.partial(planted, 256 + r, 256 + r, 129, 500 + r, False), quiet=True)

    add("planted", "value", _base, quiet=True)
    add("signed", "value", functools.partial(_base, True), quiet=True)
    add("sparse", "value", functools.partial(_base, True, 0.9), quiet=True)
    for ea, eb in ((-8, -8), (8, 8), (-8, 8)):
        add(f"scaled_{ea}_{eb}".replace("-", "m"), "value", functools.partial(_scaled, ea, eb), scale=(ea, eb))
    add("zero_ref_rows", "value", functools.partial(_edit, "a", lambda x: _zero(x, ZERO_REF_ROWS)))
    add("zero_tar_rows", "value", functools.partial(_edit, "b", lambda x: _zero(x, ZERO_TAR_ROWS)))
    add("negative_only", "value", _negative_only)
    add("one_hot", "value", _one_hot, fires=VN)
    for k in (5, 6, 7, 8):
        add(f"dup_{k}", "value", functools.partial(_copies, k), fires=len(DUP_ROWS) if k > TOPK else None)
    add("graded", "value", functools.partial(_copies, None, True))
    for v in NF_VALUES:
        for where, idx in NF_PLACES:
            add(f"nonfinite_{v}_{where}{idx}", "value", functools.partial(_nonfinite, v, where, idx), nonfinite=(v, where, idx))
    for count in REVERSE_COUNTS:
        for mode in (2, 3):
            add(f"reverse_m{mode}_{count}", "reverse", functools.partial(_reverse, count, mode, 700 + 10 * count + mode))
    return cases


CASES = _build()
NAMES = list(CASES)
VALUE_CLASSES = [k for k, v in CASES.items() if v.kind == "value"]
NONFINITE = [k for k in NAMES if k.startswith("nonfinite_")]


_want = {}


def oracle_match(orc, name, mode):
    """orc.match of a case, computed once per process and shared (never modified by the tests)"""
    key = (name, mode)
    if key not in _want:
        c = CASES[name]()
        _want[key] = orc.match(c["a"], c["ax"], c["b"], c["bx"], THRESH, mode)
        for v in _want[key].values():
            v.setflags(write=False)
    return _want[key]


def same(x, y):
    """exact equality of two matcher results' arrays: floats by bits"""
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    if x.shape != y.shape or x.dtype != y.dtype:
        return False
    if x.dtype == np.float32:
        return np.array_equal(x.view(np.uint32), y.view(np.uint32))
    return np.array_equal(x, y)
