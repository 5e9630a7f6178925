"""The parameter-only geometry of the z-slab contexts (sift3d_slab_min_halo, _min_halo_partial, _min_halo_ghost, sift3d_slab_admits):
host arithmetic on the level schedule and the keypoint windows' reach, no device.  The table was recorded from the library before the
schedule and the reach rule were each written once; the functions must keep returning exactly these codes and values."""
import ctypes as C
import importlib

import pytest

capi = importlib.import_module("3dsift_amd.capi")

OK, ERR_ARG = 0, 1
UNSET = -7   # what the out-parameter holds before the call: an error must leave it alone
DIMS = [(128, 128, 128), (40, 40, 40), (39, 64, 64), (32, 32, 32), (64, 64, 16), (64, 64, 8)]

# (num_kp_levels, sigma_default): ((rc, min_halo), (rc, min_halo_partial), (rc, min_halo_ghost whole), (rc, min_halo_ghost partial),
#                                  rc of admits, admits per DIMS entry with first_octave 0 then 1)
TABLE = {
    (0, 1.0): ((1, -7), (1, -7), (1, -7), (1, -7), 1, "000000000000"),
    (0, 1.6): ((1, -7), (1, -7), (1, -7), (1, -7), 1, "000000000000"),
    (0, 2.4): ((1, -7), (1, -7), (1, -7), (1, -7), 1, "000000000000"),
    (1, 1.0): ((0, 25), (0, 18), (0, 37), (0, 37), 0, "000000000000"),
    (1, 1.6): ((0, 38), (0, 28), (0, 55), (0, 55), 0, "000000000000"),
    (1, 2.4): ((0, 56), (0, 41), (0, 80), (0, 80), 0, "000000000000"),
    (2, 1.0): ((0, 25), (0, 9), (0, 36), (0, 26), 0, "101000101000"),
    (2, 1.6): ((0, 38), (0, 13), (0, 53), (0, 37), 0, "111100110000"),
    (2, 2.4): ((0, 56), (0, 19), (0, 79), (0, 55), 0, "000000000000"),
    (3, 1.0): ((0, 25), (0, 9), (0, 38), (0, 25), 0, "101010101000"),
    (3, 1.6): ((0, 38), (0, 13), (0, 56), (0, 35), 0, "111100111100"),
    (3, 2.4): ((0, 56), (0, 19), (0, 83), (0, 51), 0, "000000000000"),
    (4, 1.0): ((0, 25), (0, 9), (0, 41), (0, 27), 0, "101010101000"),
    (4, 1.6): ((0, 38), (0, 13), (0, 60), (0, 36), 0, "111100111100"),
    (4, 2.4): ((0, 56), (0, 19), (0, 88), (0, 52), 0, "111100110000"),
    (5, 1.0): ((0, 25), (0, 9), (0, 44), (0, 29), 0, "101010101010"),
    (5, 1.6): ((0, 38), (0, 13), (0, 63), (0, 38), 0, "111100111100"),
    (5, 2.4): ((0, 56), (0, 19), (0, 91), (0, 54), 0, "111100111100"),
    (6, 1.0): ((1, -7), (1, -7), (1, -7), (1, -7), 1, "000000000000"),
    (6, 1.6): ((1, -7), (1, -7), (1, -7), (1, -7), 1, "000000000000"),
    (6, 2.4): ((1, -7), (1, -7), (1, -7), (1, -7), 1, "000000000000"),
}


def _lib():
    L = capi.lib()
    L.sift3d_slab_admits.argtypes = [C.POINTER(capi.Params), C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]
    L.sift3d_slab_min_halo_ghost.argtypes = [C.POINTER(capi.Params), C.c_int, C.POINTER(C.c_int)]
    return L


def _row(L, levels, sigma):
    p = capi._params(dict(num_kp_levels=levels, sigma_default=sigma))
    row = []
    for fn, extra in ((L.sift3d_slab_min_halo, ()), (L.sift3d_slab_min_halo_partial, ()), (L.sift3d_slab_min_halo_ghost, (0,)),
                      (L.sift3d_slab_min_halo_ghost, (1,))):
        h = C.c_int(UNSET)
        rc = fn(C.byref(p), *extra, C.byref(h))
        row.append((rc, h.value))
    rcs, bits = set(), ""
    for nx, ny, nz in DIMS:
        for first_octave in (0, 1):
            ok = C.c_int(UNSET)
            rcs.add(L.sift3d_slab_admits(C.byref(p), nx, ny, nz, first_octave, C.byref(ok)))
            assert ok.value in (0, 1)   # (cleared before the parameters are looked at)
            bits += str(ok.value)
    assert len(rcs) == 1
    return (*row, rcs.pop(), bits)


@pytest.mark.parametrize("levels,sigma", sorted(TABLE))
def test_parameter_only_geometry_is_what_it_was(levels, sigma):
    assert _row(_lib(), levels, sigma) == TABLE[(levels, sigma)]


def test_the_table_holds_the_known_values():
    """the table itself: the values the sharding was planned with, and the rules of the edges of the grid"""
    assert [TABLE[k][:4] for k in ((3, 1.6), (1, 1.6), (5, 2.4))] == [((OK, 38), (OK, 13), (OK, 56), (OK, 35)), ((OK, 38), (OK, 28), (OK, 55), (OK, 55)),
                                                                      ((OK, 56), (OK, 19), (OK, 91), (OK, 54))]
    for (levels, sigma), row in TABLE.items():
        if levels in (0, 6):
            assert row == ((ERR_ARG, UNSET),) * 4 + (ERR_ARG, "0" * 12)
        thin = DIMS.index((64, 64, 8)) * 2
        assert (row[5][thin] == "1") == ((levels, sigma) == (5, 1.0)) and row[5][thin + 1] == "0"


def test_null_parameters_are_the_defaults():
    L = _lib()
    for fn, extra, want in ((L.sift3d_slab_min_halo, (), 38), (L.sift3d_slab_min_halo_partial, (), 13), (L.sift3d_slab_min_halo_ghost, (0,), 56),
                            (L.sift3d_slab_min_halo_ghost, (1,), 35)):
        h = C.c_int(UNSET)
        assert fn(None, *extra, C.byref(h)) == OK and h.value == want
        assert fn(None, *extra, None) == ERR_ARG
    ok = C.c_int(UNSET)
    assert L.sift3d_slab_admits(None, 128, 128, 128, 1, C.byref(ok)) == OK and ok.value == 1
    assert L.sift3d_slab_admits(None, 128, 128, 0, 1, C.byref(ok)) == ERR_ARG
