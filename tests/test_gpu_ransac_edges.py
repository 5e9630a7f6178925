"""GPU tests of the RANSAC affine fits at their edges (sift3d_fit_affine / sift3d_fit_affine_local): every k of the running top-k,
neighbour orders that shift the whole list or skip every chunk, equal distances, candidate counts around k under a radius, every
status and mixed workgroups, launch tails, the refit rounds per point, non-finite and extreme values, and the independence of a
point's record from the other waves of its workgroup.  The inputs and the assertions live in tests/ransac_cases.py; the reference is
tests/ransac_ref.py, the fp64 restatement of the header's contract.  tests/test_ransac_cpu.py runs the same assertions on the
restatement and checks what each input was built for (monotone distances, refit margins, the path each value class reaches)."""
import importlib

import numpy as np
import pytest

import ransac_cases as cs

pytestmark = pytest.mark.gpu

capi = importlib.import_module("3dsift_amd.capi")


class Gpu:
    """the binding; every call is counted, and one that raises (a bad return code: the library checks hipGetLastError and every
    HIP call of the fit) is recorded for test_no_call_raised"""
    calls = 0
    errors = []

    @classmethod
    def _run(cls, f, *a, **kw):
        cls.calls += 1
        try:
            return f(*a, **kw)
        except Exception as e:
            cls.errors.append(repr(e))
            raise

    @classmethod
    def fit(cls, pairs, **opts):
        return cls._run(capi.fit_affine, pairs, **opts)

    @classmethod
    def fit_local(cls, pairs, points, **kw):
        return cls._run(capi.fit_affine_local, pairs, points, **kw)

    @staticmethod
    def device(a):
        import torch

        return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


@pytest.mark.parametrize("k", cs.EVERY_K)
def test_every_k(k):
    cs.check_every_k(Gpu, k)


@pytest.mark.parametrize("order", cs.HOSTILE_ORDERS)
@pytest.mark.parametrize("n", cs.HOSTILE_N)
def test_hostile_order(n, order):
    cs.check_hostile(Gpu, n, order)


@pytest.mark.parametrize("n", cs.SPHERE_N)
def test_equal_distances(n):
    cs.check_sphere(Gpu, n)


@pytest.mark.parametrize("k", cs.HOSTILE_K)
def test_candidates_around_k_under_radius(k):
    cs.check_rim(Gpu, k)


def test_statuses_in_mixed_workgroups():
    cs.check_statuses(Gpu)


@pytest.mark.parametrize("n,H", cs.GLOBAL_TAILS)
def test_global_tails(n, H):
    cs.check_global_tail(Gpu, n, H)


@pytest.mark.parametrize("H", cs.LOCAL_TAIL_H)
def test_local_hypothesis_tails(H):
    cs.check_local_tail_h(Gpu, H)


@pytest.mark.parametrize("m", cs.LOCAL_TAIL_M)
def test_local_point_tails(m):
    cs.check_local_tail_m(Gpu, m)


@pytest.mark.parametrize("tau", cs.REFIT_TAU)
@pytest.mark.parametrize("k", cs.REFIT_K)
def test_local_refit_rounds(k, tau):
    cs.check_refit(Gpu, k, tau)


@pytest.mark.parametrize("name", cs.VALUE_CLASSES)
def test_values(name):
    cs.check_values(Gpu, name)


def test_independence_and_repeatability():
    cs.check_independence(Gpu)


def test_no_call_raised():
    """last in the module: none of its calls came back with an error code"""
    print(f"{Gpu.calls} calls; largest |A - ref| of the refit comparisons {cs.A_ERR[0]:.3e} (bar 1e-9)")
    assert Gpu.errors == []
