"""Shared comparison helpers for the -m gpu parity tests (HIP path through the C-ABI vs the oracle)."""
import numpy as np


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def compare_pyramids(g, o):
    """g: capi.CSIFT3D after run_stages(>=1); o: oracle Extractor after run(>=2). Bit-exact, every level."""
    assert g.num_octaves == o.num_octaves
    for oc in range(g.num_octaves):
        for i in range(6):
            a, b = g.gss(oc, i), o.gss(oc, i)
            assert np.array_equal(bits(a), bits(b)), ("gss", oc, i, int((bits(a) != bits(b)).sum()))
            assert g.level_info(0, oc * 6 + i) == o.level_info(0, oc * 6 + i)
        for i in range(5):
            a, b = g.dog(oc, i), o.dog(oc, i)
            assert np.array_equal(bits(a), bits(b)), ("dog", oc, i, int((bits(a) != bits(b)).sum()))


def extrema_table(e):
    return np.stack([e["octave"], e["level"], e["x"].astype(np.int32), e["y"].astype(np.int32), e["z"].astype(np.int32)], 1)


def descriptor_errors(desc, odesc):
    """(global RMS, worst per-keypoint RMS, worst absolute element error) of two [n, 768] descriptor sets"""
    if len(desc) == 0:
        return 0.0, 0.0, 0.0
    d = desc.astype(np.float64) - odesc.astype(np.float64)
    per_kp = np.sqrt(np.mean(d * d, axis=1))
    return float(np.sqrt(np.mean(d * d))), float(per_kp.max()), float(np.abs(d).max())


def compare_keypoints(kp, desc, okp, odesc, rms_tol=2e-5, max_abs_tol=1e-4):
    """Same count, same (octave, level, x, y, z, scale, rx, ry, rz) in the same order; orientation
    frames bit-identical; descriptors within the tolerance of their fixed-point histograms.  BASELINE.json's bar is 1e-4 RMS; with
    bit-identical rotations the bars here are 2e-5 RMS PER KEYPOINT -- one bad keypoint cannot hide in the average -- and 1e-4 on
    every single element (0.3 % of the 0.0333 clamp); measured at 512^3: 5.5e-6 / 3.1e-5.  Returns the global descriptor RMS."""
    assert len(kp) == len(okp), (len(kp), len(okp))
    for f in ("x", "y", "z", "octave", "level", "scale", "rx", "ry", "rz"):
        assert np.array_equal(kp[f], okp[f]), f
    if len(kp) == 0:
        return 0.0
    # r03: the window sums of every accepted keypoint are added in the reference's order (k_orient<true>): structure tensor, mean
    # gradient, eigenvalues, eigenvectors and the rotation matrix are bit-identical
    for f in ("str_tensor", "win", "eigvalue", "Rotation"):
        assert np.array_equal(bits(kp[f]), bits(okp[f])), (f, int((bits(kp[f]) != bits(okp[f])).any(axis=1).sum()), len(kp))
    # the stored eigenvectors carry the solver's sign (Eigen in the reference, Jacobi here; the golden tests of the oracle skip the
    # field for the same reason): each of the three vectors equals the reference's or its negation, bit for bit
    ev, oev = kp["eigvector"].reshape(-1, 3, 3), okp["eigvector"].reshape(-1, 3, 3)
    same = (bits(ev) == bits(oev)).all(axis=2) | (bits(ev) == bits(-oev)).all(axis=2)
    assert same.all(), ("eigvector", int((~same).any(axis=1).sum()), len(kp))
    rms, worst_kp, worst_abs = descriptor_errors(desc, odesc)
    assert rms <= rms_tol, rms
    assert worst_kp <= rms_tol, ("worst per-keypoint RMS", worst_kp)
    assert worst_abs <= max_abs_tol, ("worst element", worst_abs)
    return rms


def nan_equal_bits(a, b):
    """NaN positions equal as a mask, the bits of every other value equal.  (A NaN's payload and sign are not part of the contract:
    x86 produces 0xFFC00000 for 0 / 0, the GPU need not.)  Returns the number of differing elements."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    assert a.shape == b.shape, (a.shape, b.shape)
    na, nb = np.isnan(a), np.isnan(b)
    return int((na != nb).sum()) + int(((bits(a) != bits(b)) & ~na & ~nb).sum())


def compare_pyramids_nan(g, o):
    """compare_pyramids for volumes with non-finite voxels: every level by nan_equal_bits"""
    assert g.num_octaves == o.num_octaves
    for oc in range(g.num_octaves):
        for i in range(6):
            bad = nan_equal_bits(g.gss(oc, i), o.gss(oc, i))
            assert bad == 0, ("gss", oc, i, bad)
            assert g.level_info(0, oc * 6 + i) == o.level_info(0, oc * 6 + i)
        for i in range(5):
            bad = nan_equal_bits(g.dog(oc, i), o.dog(oc, i))
            assert bad == 0, ("dog", oc, i, bad)


def compare_keypoints_nonfinite(kp, desc, okp, odesc, rms_tol=2e-5, max_abs_tol=1e-4):
    """compare_keypoints for volumes with non-finite voxels.  Same list in the same order; frame fields bit-identical where the
    oracle's are finite and NaN where they are NaN; descriptor rows under compare_keypoints' bars where the oracle's row is finite;
    where the oracle's row contains a NaN the row here must contain one too (not necessarily at the same elements): a finite row there
    would match where the reference's cannot.  (With the reference's truncation no such row is known to occur -- a NaN histogram ends as
    the constant row, tests/test_input_classes_cpu.py -- the rule is kept for a row that does.)  Returns (rows compared by value, rows that must hold a NaN)."""
    assert len(kp) == len(okp), (len(kp), len(okp))
    for f in ("x", "y", "z", "octave", "level", "scale"):
        assert np.array_equal(kp[f], okp[f]), f
    for f in ("rx", "ry", "rz", "str_tensor", "win", "eigvalue", "Rotation"):
        bad = nan_equal_bits(kp[f], okp[f])
        assert bad == 0, (f, bad)
    if len(kp) == 0:
        return 0, 0
    ev, oev = kp["eigvector"].reshape(-1, 3, 3), okp["eigvector"].reshape(-1, 3, 3)
    fin = np.isfinite(oev).all(axis=2)
    same = (bits(ev) == bits(oev)).all(axis=2) | (bits(ev) == bits(-oev)).all(axis=2)
    assert (same | ~fin).all(), ("eigvector", int((~same & fin).any(axis=1).sum()), len(kp))
    orow_nan = np.isnan(odesc).any(axis=1)
    assert np.isnan(desc[orow_nan]).any(axis=1).all(), ("finite descriptor row where the oracle's holds a NaN", np.nonzero(orow_nan)[0])
    assert np.isfinite(desc[~orow_nan]).all(), ("non-finite descriptor row where the oracle's is finite",
                                                np.nonzero(~np.isfinite(desc).all(axis=1) & ~orow_nan)[0])
    rms, worst_kp, worst_abs = descriptor_errors(desc[~orow_nan], odesc[~orow_nan])
    assert worst_kp <= rms_tol, ("worst per-keypoint RMS", worst_kp)
    assert worst_abs <= max_abs_tol, ("worst element", worst_abs)
    return int((~orow_nan).sum()), int(orow_nan.sum())
