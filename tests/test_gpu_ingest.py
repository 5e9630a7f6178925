"""-m gpu: the typed input (sift3d_create_typed, sift3d_volume_to_device; kernels_ingest.hip) against the float path of the same
library on the same voxels widened on the host.  Widening an 8 / 16-bit integer to fp32 is exact, the maximum is the same number and
the division is the same IEEE division, so every comparison here is of BYTES.  tests/test_ingest_cpu.py proves on the oracle that
the parity volumes of tests/ingest_cases.py hold the extremes they are named for and yield keypoints."""
import ctypes as C
import importlib
import math

import numpy as np
import pytest

import ingest_cases as cases
from hipcheck import bits, extrema_table, nan_equal_bits

pytestmark = pytest.mark.gpu

capi = importlib.import_module("3dsift_amd.capi")

BASE_N = (1, 2, 3, 7, 8, 9, 15, 16, 17, 31, 33, 255, 4095, 4096, 4097)


def sweep_elems(dtype):
    """elements one full sweep of k_ingest's launch covers: the whole capped grid of a grid-stride form, one workgroup of the
    one-piece-per-lane form"""
    block, elems, ingest_cap, _ = capi.ingest_launch(dtype)
    return block * elems * max(1, ingest_cap), block, elems


def to_host(t):
    import torch

    torch.cuda.synchronize()
    return t.cpu().numpy()


# ---- 1. conversion, every element position ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", cases.DTYPES)
def test_conversion_every_element_position(dtype):
    sweep, block, elems = sweep_elems(dtype)
    # 5 elements behind one full sweep (the second trip of a grid-stride loop / the tail behind a full workgroup), and the same behind a
    # second workgroup that 5 lanes fill
    extra = (sweep + 5, sweep + 5 * elems + 5)
    assert all(n > sweep for n in extra)
    for n in BASE_N + extra:
        v = cases.conversion_values(dtype, n, (elems, n // elems * elems, sweep)).reshape(1, 1, n)
        got = to_host(capi.to_device(v))
        assert got.dtype == np.float32 and got.shape == v.shape
        assert got.tobytes() == v.astype(np.float32).tobytes(), (n, int((bits(got) != bits(v.astype(np.float32))).sum()))


# ---- 2. alignment and bounds -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", cases.DTYPES)
def test_every_source_and_destination_alignment(dtype):
    """device-resident typed sources starting 0 .. 15 (8-bit) / 0 .. 7 (16-bit) elements into a 256-byte-aligned allocation x d_dst
    starting 0 .. 3 floats into its allocation, n = 4099: equal bytes, and 64 sentinel floats on either side of dst[0, n) untouched"""
    import torch

    n, guard = 4099, 64
    esize = np.dtype(dtype).itemsize
    per16 = 16 // esize
    v = cases.conversion_values(dtype, n, (per16, n - n % per16))
    want = v.astype(np.float32).tobytes()
    sentinel = np.float32(-12345.5)
    L = capi.lib()
    src = torch.zeros(256 + n * esize, dtype=torch.uint8, device="cuda")
    dst = torch.empty(guard + 4 + n + guard, dtype=torch.float32, device="cuda")
    assert src.data_ptr() % 256 == 0 and dst.data_ptr() % 16 == 0
    raw = torch.from_numpy(v.view(np.uint8).copy()).cuda()
    sec = C.c_double(0)
    for s_off in range(per16):
        src.zero_()
        src[s_off * esize:s_off * esize + n * esize] = raw
        for d_off in range(4):
            dst.fill_(float(sentinel))
            torch.cuda.synchronize()
            capi._check(L.sift3d_volume_to_device(C.c_void_p(src.data_ptr() + s_off * esize), cases.CODES[dtype], n, 1, 1, 1, 0,
                                                  C.c_void_p(dst.data_ptr() + 4 * (guard + d_off)), C.byref(sec)))
            got = to_host(dst)
            lo = guard + d_off
            assert got[lo:lo + n].tobytes() == want, (s_off, d_off)
            assert (got[:lo] == sentinel).all() and (got[lo + n:] == sentinel).all(), (s_off, d_off)


# ---- 3. staging seams at element widths other than 4 -----------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,shape,chunks", [("uint16", (195, 273, 315), 2), ("uint8", (195, 273, 315), 1),
                                                ("uint16", (195, 273, 401), 3), ("uint8", (195, 273, 401), 2)])
def test_staging_seams_at_integer_widths(dtype, shape, chunks):
    """195 x 273 x 315 is the shape csrc/staging.hip's comment names: 33 538 050 bytes as uint16, which is two 16 MiB pinned chunks
    (16 382 bytes short of filling both), and one partial chunk as uint8.  195 x 273 x 401 gives the three chunks (uint16) and two
    (uint8) this test was specified with.  In every case the last chunk is partial and not a multiple of the copy threads'
    page-aligned slices.  A float-sized byte count or stride in the typed path shows here."""
    nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
    assert math.ceil(nbytes / (16 << 20)) == chunks and nbytes % (16 << 20) and (nbytes % (16 << 20)) % 4096
    lo, hi = cases.EXTREMES[dtype]
    v = np.random.Generator(np.random.PCG64(11)).integers(lo, hi + 1, size=shape, dtype=np.int64).astype(dtype)
    v.flat[-1], v.flat[0] = hi, hi
    got = to_host(capi.to_device(v))
    want = v.astype(np.float32)
    assert got.tobytes() == want.tobytes(), int((bits(got) != bits(want)).sum())


def test_float_host_volume_goes_through_the_staging_pool():
    """SIFT3D_DT_F32: straight into d_dst, no kernel; two chunks"""
    v = np.random.Generator(np.random.PCG64(12)).standard_normal((65, 255, 257)).astype(np.float32)
    got = to_host(capi.to_device(v))
    assert got.tobytes() == v.tobytes()


# ---- 4. extractor parity ---------------------------------------------------------------------------------------------------------
_float_runs = {}


def run_record(g):
    g.KpSiftAlgorithm()
    kp, desc = g.GetKeypoints()
    return dict(input=g.input().tobytes(), num_octaves=g.num_octaves, extrema=extrema_table(g.extrema()).tobytes(),
                extrema_records=np.ascontiguousarray(g.extrema()).tobytes(), kp=kp.tobytes(), desc=desc.tobytes(), n=len(kp))


def float_run(dtype, key):
    if (dtype, key) not in _float_runs:
        _float_runs[(dtype, key)] = run_record(capi.CSIFT3D(cases.parity(dtype, key).astype(np.float32)))
    return _float_runs[(dtype, key)]


def assert_same_run(got, want, what):
    assert want["n"] >= cases.MIN_KEYPOINTS, want["n"]
    for k in ("num_octaves", "n", "input", "extrema", "extrema_records", "kp", "desc"):
        assert got[k] == want[k], (what, k)


@pytest.mark.parametrize("key", sorted(cases.SHAPES))
@pytest.mark.parametrize("dtype", cases.DTYPES)
def test_extractor_parity_host_volume(dtype, key):
    v = cases.parity(dtype, key)
    assert_same_run(run_record(capi.CSIFT3D(v, keep_dtype=True)), float_run(dtype, key), "keep_dtype")


@pytest.mark.parametrize("key", sorted(cases.SHAPES))
@pytest.mark.parametrize("dtype", cases.DTYPES)
def test_extractor_parity_device_volume(dtype, key):
    """device_ptr= with dtype=; uint16 voxels travel in an int16 tensor, which every torch has"""
    import torch

    v = cases.parity(dtype, key)
    t = torch.from_numpy(v.view(np.int16) if dtype == "uint16" else v).cuda()
    torch.cuda.synchronize()
    g = capi.CSIFT3D(None, device_ptr=t.data_ptr(), shape=v.shape, dtype=dtype)
    assert_same_run(run_record(g), float_run(dtype, key), "device_ptr")


def test_extractor_parity_float_through_create_typed():
    import torch

    dtype, key = "int16", "odd"
    f = cases.parity(dtype, key).astype(np.float32)
    assert_same_run(run_record(capi.CSIFT3D(f, keep_dtype=True)), float_run(dtype, key), "SIFT3D_DT_F32, host")
    t = torch.from_numpy(f).cuda()
    torch.cuda.synchronize()
    g = capi.CSIFT3D(None, device_ptr=t.data_ptr(), shape=f.shape, dtype="float32")
    assert_same_run(run_record(g), float_run(dtype, key), "SIFT3D_DT_F32, device")


@pytest.mark.parametrize("dtype,shape", [("int8", (129, 255, 257)), ("uint16", (65, 255, 257))])
def test_absmax_second_sweep(dtype, shape):
    """more elements than one sweep of k_absmax_t's capped grid, the maximum in the part only the second trip of its loop reads"""
    block, elems, _, absmax_cap = capi.ingest_launch(dtype)
    sweep = block * elems * absmax_cap
    n = int(np.prod(shape))
    assert sweep + 5 < n < 2 * sweep
    lo, hi = cases.EXTREMES[dtype]
    v = np.random.Generator(np.random.PCG64(13)).integers(lo // 2, hi // 2, size=n, dtype=np.int64)
    v[sweep + 5] = lo if lo < 0 else hi
    v = v.astype(dtype).reshape(shape)
    a, b = capi.CSIFT3D(v, keep_dtype=True), capi.CSIFT3D(v.astype(np.float32))
    want = (v.astype(np.float32) / np.float32(abs(float(v.reshape(-1)[sweep + 5])))).astype(np.float32)
    ia, ib = a.input(), b.input()
    assert ia.tobytes() == ib.tobytes() and ia.tobytes() == want.tobytes()


# ---- 5. degenerate values --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["zeros_u8", "const_i16"])
def test_degenerate_volumes(which):
    v = cases.degenerate(which)
    a, b = capi.CSIFT3D(v, keep_dtype=True), capi.CSIFT3D(v.astype(np.float32))
    ia, ib = a.input(), b.input()
    assert nan_equal_bits(ia, ib) == 0
    if which == "zeros_u8":
        assert np.isnan(ia).all()  # data_scale's 0 / 0
    else:
        assert (ia == np.float32(-1.0)).all()
    a.KpSiftAlgorithm(); b.KpSiftAlgorithm()
    assert len(a.extrema()) == 0 and len(b.extrema()) == 0


# ---- 6. upload once, correlate often ---------------------------------------------------------------------------------------------
def result_bytes(d):
    return {k: np.ascontiguousarray(v).tobytes() for k, v in d.items() if k != "seconds"}


def test_upload_once_correlate_often():
    ref, tar = cases.dvc_pair()
    g = np.arange(16, 33, 8)
    pts = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(np.int32)
    assert len(pts) == 27
    fr, ft = ref.astype(np.float32), tar.astype(np.float32)
    first = capi.icgn(fr, ft, pts, subset_radius=4)
    assert (np.asarray(first["status"]) <= 1).sum() >= 20, first["status"]  # the comparison is of real refinements, not of refusals
    want_i = result_bytes(first)
    want_s = result_bytes(capi.zncc_search(fr, ft, pts, subset_radius=4))
    dr, dt = capi.to_device(ref), capi.to_device(tar)
    assert to_host(dr).tobytes() == fr.tobytes() and to_host(dt).tobytes() == ft.tobytes()
    for again in range(2):
        assert result_bytes(capi.icgn(dr, dt, pts, subset_radius=4)) == want_i, again
        assert result_bytes(capi.zncc_search(dr, dt, pts, subset_radius=4)) == want_s, again


# ---- 7. *seconds and errors on a live GPU ----------------------------------------------------------------------------------------
def test_seconds_and_errors():
    import torch

    v = cases.parity("uint8", "fused")
    out, sec = capi.to_device(v, with_seconds=True)
    assert math.isfinite(sec) and sec >= 0 and out.dtype == torch.float32 and tuple(out.shape) == v.shape and out.is_cuda
    with pytest.raises(ValueError):
        capi.to_device(v[:, :, ::2])
    with pytest.raises(ValueError):
        capi.to_device(v.astype(np.float64))
    with pytest.raises(capi.Sift3dError):
        capi.to_device(v, dtype=9)
    with pytest.raises(capi.Sift3dError):
        capi.CSIFT3D(None, device_ptr=out.data_ptr(), shape=v.shape, dtype=9)
    # a device tensor of an integer dtype, and uint16 voxels held in an int16 tensor
    w = cases.parity("uint16", "odd")
    t = torch.from_numpy(w.view(np.int16)).cuda()
    assert to_host(capi.to_device(t, dtype="uint16")).tobytes() == w.astype(np.float32).tobytes()
    assert to_host(capi.to_device(t)).tobytes() == w.view(np.int16).astype(np.float32).tobytes()
