"""-m gpu: sift3d_match on the cases of tests/match_cases.py -- the answer planted at every tile / lane-half / share position, every
dealing regime, hostile descriptor values, chosen reverse-pass subsets -- against the CPU oracle's matcher, every output key, bit for
bit, in modes 1, 2 and 3.  tests/test_match_cpu.py shows on the CPU what each case is (planted columns, margins, dealing regime).

Every case runs under two forms of the score kernel: the default (k_scores_topk2) and, with the hook match_nodma, the
register-staged k_scores_top4 that serves matrices of 4 GB and more.  There is no other form.

On the planted cases the candidate selection must give the answer by itself (exact_rows == 0: the CPU module proves that the guard
has no reason to fire); on the tie cases the guard must fire.  No comparison here has a tolerance."""
import contextlib
import importlib

import numpy as np
import pytest

import match_cases as mc

pytestmark = pytest.mark.gpu

FORMS = ("default", "nodma")
KEYS = ("gIdx", "sIdx", "gDist", "sDist", "pairs")


@pytest.fixture(scope="module")
def capi():
    m = importlib.import_module("3dsift_amd.capi")
    assert m.device_count() >= 1, "GPU tests need a visible MI355X (no CPU fallback exists)"
    return m


@pytest.fixture(scope="module", autouse=True)
def threads(orc):
    orc.set_threads(16)   # explicitly, not from the CPU count
    yield
    orc.set_threads(0)


def form_ctx(capi, form):
    return capi.hook("match_nodma", 1) if form == "nodma" else contextlib.nullcontext()


def check(got, want, what):
    assert set(KEYS) <= set(want)
    for k in want:
        if not mc.same(got[k], want[k]):
            g, w = got[k], want[k]
            bad = np.flatnonzero((g != w).reshape(len(g), -1).any(axis=1)) if g.shape == w.shape else (g.shape, w.shape)
            pytest.fail(f"{what} {k}: {len(bad)} rows differ, first {bad[:8]}")


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", mc.NAMES)
def test_parity_and_guard(capi, orc, name, form):
    c = mc.CASES[name]()
    mt = capi.muBruteMatcher()
    with form_ctx(capi, form):
        for mode in (1, 2, 3):
            want = mc.oracle_match(orc, name, mode)
            got = mt._match(c["a"], c["ax"], c["b"], c["bx"], mc.THRESH, mode)
            print(f"{name} {form} mode {mode}: exact_rows {mt.exact_rows}")
            check(got, want, (name, form, mode))
            if c["quiet"]:     # the fast path answers by itself, in the forward and in the reverse pass
                assert mt.exact_rows == 0, (name, form, mode, mt.exact_rows)
            if c["fires"]:     # more exact ties than the list holds: the guard must hand the row to k_exact_rows
                assert mt.exact_rows >= c["fires"], (name, form, mode, mt.exact_rows)


def _dev(arr):
    import torch
    return torch.from_numpy(np.ascontiguousarray(arr)).cuda()


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", ("size_300x1100", "nonfinite_nan_tar5"))
def test_device_resident_inputs_equal_the_host_path(capi, orc, name, form):
    c = mc.CASES[name]()
    mt = capi.muBruteMatcher()
    a, ax, b, bx = (_dev(c[k]) for k in ("a", "ax", "b", "bx"))
    with form_ctx(capi, form):
        for mode in (1, 2, 3):
            host = mt._match(c["a"], c["ax"], c["b"], c["bx"], mc.THRESH, mode)
            dev = mt._match(a.data_ptr(), ax.data_ptr(), b.data_ptr(), bx.data_ptr(), mc.THRESH, mode, on_device=True, n=len(c["a"]), m=len(c["b"]))
            for k in KEYS:
                assert host[k].tobytes() == dev[k].tobytes(), (name, form, mode, k)
            check(dev, mc.oracle_match(orc, name, mode), (name, form, mode, "device"))


@pytest.mark.parametrize("form", FORMS)
def test_repeatable_across_calls_of_other_sizes(capi, orc, form):
    """the same call twice, and again after a call with more rows and columns in between (the scratch grows and is reused, the
    partial lists are never initialised): byte-equal results"""
    c, other = mc.CASES["size_300x1100"](), mc.CASES["size_40x1500"]()
    mt = capi.muBruteMatcher()
    with form_ctx(capi, form):
        for mode in (1, 3):
            runs = [mt._match(c["a"], c["ax"], c["b"], c["bx"], mc.THRESH, mode) for _ in range(2)]
            mt._match(other["a"], other["ax"], other["b"], other["bx"], mc.THRESH, mode)
            runs.append(mt._match(c["a"], c["ax"], c["b"], c["bx"], mc.THRESH, mode))
            for r in runs[1:]:
                for k in KEYS:
                    assert r[k].tobytes() == runs[0][k].tobytes(), (form, mode, k)
            check(runs[0], mc.oracle_match(orc, "size_300x1100", mode), (form, mode))
