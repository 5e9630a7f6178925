"""CPU tests of the typed input (sift3d_create_typed, sift3d_volume_to_device, readNiiFileTyped): the ABI surface and its argument
checks on a machine without a GPU, the typed NIfTI reader against readNiiFile over the files of golden g9, and -- on the oracle alone
-- the preconditions of the parity cases of tests/ingest_cases.py that tests/test_gpu_ingest.py relies on."""
import ctypes as C
import gzip
import importlib
import os
import struct
import subprocess
import tempfile

import numpy as np
import pytest

import ingest_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "3dsift_amd")
capi = importlib.import_module("3dsift_amd.capi")

ERR_ARG, ERR_NO_DEVICE = 1, 2


@pytest.fixture(scope="module")
def L():
    subprocess.check_call(["make", "-C", os.path.join(PKG, "csrc"), "-j8"], stdout=subprocess.DEVNULL)
    return capi.lib()


def last_error(L):
    return L.sift3d_last_error().decode()


# ---- ABI surface ---------------------------------------------------------------------------------------------------------------
def test_symbols_and_dtype_bytes(L):
    for s in ("sift3d_dtype_bytes", "sift3d_create_typed", "sift3d_volume_to_device"):
        assert hasattr(L, s) and s in capi.SYMBOLS, s
    b = C.c_int(-1)
    for code, want in ((0, 4), (1, 1), (2, 1), (3, 2), (4, 2)):
        assert L.sift3d_dtype_bytes(code, C.byref(b)) == 0 and b.value == want, code
    for code in (-1, 5, 1 << 20):
        assert L.sift3d_dtype_bytes(code, C.byref(b)) == ERR_ARG and last_error(L), code
    assert L.sift3d_dtype_bytes(1, None) == ERR_ARG
    assert cases.CODES == capi.DTYPES


def test_launch_constants_are_exported(L):
    for dt in cases.DTYPES:
        block, elems, ingest_cap, absmax_cap = capi.ingest_launch(dt)
        assert block % 64 == 0 and block > 0 and elems * np.dtype(dt).itemsize == 16 and ingest_cap >= 0 and absmax_cap > 0


def test_argument_checks_come_before_the_device(L):
    """bad dtype, NULL pointers, zero dimensions: SIFT3D_ERR_ARG with a message; valid arguments where no GPU is visible:
    SIFT3D_ERR_NO_DEVICE (with a GPU the same calls would run: tests/test_gpu_ingest.py)"""
    v = np.zeros((4, 5, 6), np.uint16)
    vp = v.ctypes.data_as(C.c_void_p)
    h = C.c_void_p()
    dst = C.c_void_p(4096)  # never dereferenced: no device
    sec = C.c_double(0)

    def create(out=C.byref(h), vol=vp, dtype=3, dims=(6, 5, 4)):
        return L.sift3d_create_typed(out, vol, dtype, *dims, None, 0, 0)

    def upload(vol=vp, dtype=3, dims=(6, 5, 4), d=dst):
        return L.sift3d_volume_to_device(vol, dtype, *dims, 0, 0, d, C.byref(sec))

    bad_create = {"dtype 5": dict(dtype=5), "dtype -1": dict(dtype=-1), "NULL volume": dict(vol=None), "NULL out": dict(out=None),
                  "nx 0": dict(dims=(0, 5, 4)), "ny 0": dict(dims=(6, 0, 4)), "nz -1": dict(dims=(6, 5, -1)),
                  "2^31 voxels": dict(dims=(2048, 1024, 1024)), "NULL volume, float": dict(vol=None, dtype=0)}
    for why, kw in bad_create.items():
        assert create(**kw) == ERR_ARG and last_error(L), why
    bad_upload = {"dtype 5": dict(dtype=5), "dtype -1": dict(dtype=-1), "NULL volume": dict(vol=None), "NULL d_dst": dict(d=None),
                  "nx 0": dict(dims=(0, 5, 4)), "ny 0": dict(dims=(6, 0, 4)), "nz -1": dict(dims=(6, 5, -1))}
    for why, kw in bad_upload.items():
        assert upload(**kw) == ERR_ARG and last_error(L), why
    if capi.device_count() > 0:
        return
    for code in range(5):
        assert create(dtype=code) == ERR_NO_DEVICE and last_error(L), code
        assert not h.value
        assert upload(dtype=code) == ERR_NO_DEVICE and last_error(L), code


def test_python_binding_refuses_what_it_cannot_pass():
    """no GPU needed: the checks come before any call into the library"""
    v = np.zeros((4, 5, 6), np.uint16)
    for bad in (v[:, :, ::2], v.astype(np.float64), v.astype(np.int32), v[0]):
        with pytest.raises(ValueError):
            capi.to_device(bad)
    with pytest.raises(ValueError):
        capi.to_device(v, dtype="uint8")  # not vol's width
    with pytest.raises(ValueError):
        capi.to_device(v, dtype="float64")


# ---- readNiiFileTyped ----------------------------------------------------------------------------------------------------------
READER_PROGRAM = r"""
#include "Include/Util/readNii.h"
#include <cstdint>
#include <cstdio>
#include <cstring>

template <typename T> static int same(const void *typed, const float *wide, size_t n) {
    const T *t = static_cast<const T *>(typed);
    for (size_t i = 0; i < n; i++) { const float f = (float)t[i]; if (memcmp(&f, &wide[i], 4) != 0) return 0; }
    return 1;
}

// one line per file: <type code, -1 refused> <nx> <ny> <nz> <typed elements widened == readNiiFile's array> <readNiiFile refused>
int main(int argc, char **argv) {
    for (int a = 1; a < argc; a++) {
        int nx = -1, ny = -1, nz = -1, fx = -1, fy = -1, fz = -1;
        VoxelType type = VoxelType::I8;
        float *wide = readNiiFile(argv[a], fx, fy, fz);
        void *typed = readNiiFileTyped(argv[a], nx, ny, nz, type);
        int eq = 0;
        if (wide && typed && nx == fx && ny == fy && nz == fz) {
            const size_t n = (size_t)nx * ny * nz;
            switch (type) {
            case VoxelType::F32: eq = memcmp(typed, wide, n * 4) == 0; break;
            case VoxelType::U8: eq = same<uint8_t>(typed, wide, n); break;
            case VoxelType::I8: eq = same<int8_t>(typed, wide, n); break;
            case VoxelType::U16: eq = same<uint16_t>(typed, wide, n); break;
            case VoxelType::I16: eq = same<int16_t>(typed, wide, n); break;
            }
        }
        printf("%d %d %d %d %d %d\n", typed ? (int)type : -1, nx, ny, nz, eq, wide ? 0 : 1);
        switch (type) {  // delete[] of the matching element type
        case VoxelType::F32: delete[] static_cast<float *>(typed); break;
        case VoxelType::U8: delete[] static_cast<uint8_t *>(typed); break;
        case VoxelType::I8: delete[] static_cast<int8_t *>(typed); break;
        case VoxelType::U16: delete[] static_cast<uint16_t *>(typed); break;
        case VoxelType::I16: delete[] static_cast<int16_t *>(typed); break;
        }
        delete[] wide;
    }
    return 0;
}
"""
TYPE_OF_DATATYPE = {2: 1, 256: 2, 512: 3, 4: 4}  # NIfTI datatype -> VoxelType; every other: F32 (0)


def header_datatype(blob):
    """the datatype code a NIfTI-1 / NIfTI-2 / ANALYZE header declares, in either byte order"""
    for e in "<>":
        size = struct.unpack_from(e + "i", blob, 0)[0]
        if size in (348, 540):
            return struct.unpack_from(e + "h", blob, 12 if size == 540 else 70)[0]
    raise AssertionError("not a header")


def nifti1(vol, dtype, code, big_endian=False):
    nz, ny, nx = vol.shape
    e = ">" if big_endian else "<"
    h = bytearray(352)
    struct.pack_into(e + "i", h, 0, 348)
    struct.pack_into(e + "8h", h, 40, 3, nx, ny, nz, 1, 1, 1, 1)
    struct.pack_into(e + "h", h, 70, code)
    struct.pack_into(e + "h", h, 72, np.dtype(dtype).itemsize * 8)
    struct.pack_into(e + "f", h, 108, 352.0)
    h[344:348] = b"n+1\0"
    return bytes(h) + vol.astype(np.dtype(dtype).newbyteorder(e)).tobytes()


@pytest.fixture(scope="module")
def reader(L):
    subprocess.check_call(["make", "-C", os.path.join(PKG, "host")], stdout=subprocess.DEVNULL)
    with tempfile.TemporaryDirectory() as t:
        src, exe = os.path.join(t, "reader.cpp"), os.path.join(t, "reader")
        open(src, "w").write(READER_PROGRAM)
        subprocess.check_call(["g++", "-std=c++14", "-I" + os.path.join(PKG, "host"), "-o", exe, src, "-L" + PKG, "-lsift3d", "-lsift3d_hip",
                               "-Wl,-rpath," + PKG])

        def run(paths):
            r = subprocess.run([exe] + paths, capture_output=True, text=True, timeout=120)
            assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
            rows = [tuple(int(x) for x in line.split()) for line in r.stdout.splitlines()]
            assert len(rows) == len(paths)
            return rows

        yield run, t


def test_typed_reader_over_golden_g9(reader):
    """every file of g9, and the integer files g9 lacks (big-endian uint16, gzip-compressed 8 / 16-bit): the named type, the same
    extents, and elements that widen to readNiiFile's array exactly; every other datatype F32 with the same array"""
    run, t = reader
    g = np.load(os.path.join(ROOT, "tests", "golden", "g9_nifti.npz"))
    paths, want, shapes = [], [], []
    for name in map(str, g["names"]):
        if name + "_files" in g.files:
            blobs = {str(f): g[name + "_blob_" + str(f)].tobytes() for f in g[name + "_files"]}
            p = os.path.join(t, str(g[name + "_arg"]))
            hdr = next(b for f, b in blobs.items() if ".hdr" in f or ".nii" in f)
        else:
            p = os.path.join(t, name + (".nii.gz" if bool(g[name + "_gz"]) else ".nii"))
            blobs = {os.path.basename(p): g[name + "_file"].tobytes()}
            hdr = blobs[os.path.basename(p)]
        for f, b in blobs.items():
            open(os.path.join(t, f), "wb").write(b)
        hdr = gzip.decompress(hdr) if hdr[:2] == b"\x1f\x8b" else hdr
        paths.append(p); want.append(TYPE_OF_DATATYPE.get(header_datatype(hdr), 0)); shapes.append(g[name + "_data"].shape)
    rng = np.random.default_rng(3)
    for dt, code, be, gz in (("u2", 512, True, False), ("u2", 512, False, True), ("i2", 4, True, True), ("u1", 2, False, True),
                             ("i1", 256, True, False), ("i1", 256, False, True)):
        info = np.iinfo(np.dtype(dt))
        vol = rng.integers(info.min, info.max + 1, size=(5, 6, 7)).astype(dt)
        vol.flat[0], vol.flat[-1] = info.min, info.max
        blob = nifti1(vol, dt, code, big_endian=be)
        p = os.path.join(t, f"extra_{dt}_{int(be)}{int(gz)}.nii" + (".gz" if gz else ""))
        open(p, "wb").write(gzip.compress(blob) if gz else blob)
        paths.append(p); want.append(TYPE_OF_DATATYPE[code]); shapes.append(vol.shape)
    rows = run(paths)
    for p, w, s, (typ, nx, ny, nz, eq, float_refused) in zip(paths, want, shapes, rows):
        assert (typ, (nz, ny, nx), eq, float_refused) == (w, s, 1, 0), os.path.basename(p)
    seen = set(want)
    assert seen == {0, 1, 2, 3, 4}, seen
    # both byte orders, pairs and compressed files among the integer ones
    names = [os.path.basename(p) for p, w in zip(paths, want) if w]
    assert any("_be" in n for n in names) and any(".hdr" in n for n in names) and any(n.endswith(".gz") for n in names)


def test_typed_reader_refuses_what_read_nii_refuses(reader):
    run, t = reader
    vol = np.arange(5 * 6 * 7, dtype=np.int16).reshape(5, 6, 7)
    good = bytearray(nifti1(vol, "i2", 4))
    bad = {}
    b = bytearray(good); struct.pack_into("<h", b, 42, -7); bad["negative dim"] = b
    b = bytearray(good); struct.pack_into("<h", b, 72, 32); bad["bitpix != datatype size"] = b
    b = bytearray(good); struct.pack_into("<f", b, 108, float("nan")); bad["vox_offset NaN"] = b
    b = bytearray(good); struct.pack_into("<f", b, 108, 3.0e9); bad["vox_offset absurd"] = b
    b = bytearray(good); struct.pack_into("<h", b, 70, 1536); bad["unsupported datatype"] = b
    bad["truncated payload"] = good[:-10]
    b = bytearray(good); b[344:348] = b"ni1\0"; bad["header of a pair in a file that is not *.hdr"] = b
    b = bytearray(good); b[344:348] = b"xyz\0"; bad["unknown magic"] = b
    paths = []
    for i, blob in enumerate(bad.values()):
        paths.append(os.path.join(t, f"bad{i}.nii"))
        open(paths[-1], "wb").write(bytes(blob))
    paths.append(os.path.join(t, "missing.nii"))
    good_path = os.path.join(t, "good.nii")
    open(good_path, "wb").write(bytes(good))
    rows = run(paths + [good_path])
    for why, (typ, nx, ny, nz, eq, float_refused) in zip(list(bad) + ["missing file"], rows):
        assert typ == -1 and float_refused == 1 and (nx, ny, nz) == (0, 0, 0), why
    assert rows[-1] == (4, 7, 6, 5, 1, 0)


# ---- preconditions of the parity cases, on the oracle ---------------------------------------------------------------------------
def test_shapes_are_what_they_are_named_for():
    assert np.prod(cases.SHAPES["odd"]) % 2 == 1
    assert min(cases.SHAPES["fused"][1:]) >= 33 and min(cases.SHAPES["odd"][1:]) >= 33


@pytest.mark.parametrize("shape_key", sorted(cases.SHAPES))
@pytest.mark.parametrize("dtype", cases.DTYPES)
def test_parity_volumes_hold_their_extremes_and_yield_keypoints(orc, dtype, shape_key):
    v = cases.parity(dtype, shape_key)
    assert v.dtype == np.dtype(dtype) and v.shape == cases.SHAPES[shape_key] and v.tobytes() == cases.parity(dtype, shape_key).tobytes()
    lo, hi = cases.EXTREMES[dtype]
    a = np.abs(v.astype(np.int64))
    if lo < 0:
        # max|v| is attained by one voxel only, and that voxel is the type's most negative value: |v| does not exist in the type
        assert a.max() == -lo and int((a == a.max()).sum()) == 1 and int((v == lo).sum()) == 1
        assert (v > 0).any() and a[v != lo].max() == hi
    else:
        assert v.max() == hi and v.min() == 0
    assert len(np.unique(v)) > 100
    o = orc.extractor(v.astype(np.float32)).run(5)
    kp, _ = o.keypoints()
    print(dtype, shape_key, "oracle keypoints", len(kp), "extrema", len(o.extrema()))
    assert len(kp) >= cases.MIN_KEYPOINTS, len(kp)


def test_degenerate_and_conversion_cases():
    z, c = cases.degenerate("zeros_u8"), cases.degenerate("const_i16")
    assert z.dtype == np.uint8 and not z.any() and c.dtype == np.int16 and (c == -7).all()
    for dt in cases.DTYPES:
        lo, hi = cases.EXTREMES[dt]
        v = cases.conversion_values(dt, 4097, (16, 4080))
        assert v.dtype == np.dtype(dt) and {int(v[0]), int(v[-1])} <= {lo, hi}
        assert all(int(v[i]) in (lo, hi) for i in (15, 16, 4079, 4080)) and lo in v and hi in v
        assert len(np.unique(v)) > min(200, hi - lo) // 2
        assert cases.conversion_values(dt, 1, ())[0] in (lo, hi)


def test_dvc_pair_differs_by_its_shift():
    ref, tar = cases.dvc_pair()
    assert ref.dtype == tar.dtype == np.uint16 and ref.shape == tar.shape == (48, 48, 48)
    assert max(ref.max(), tar.max()) == 65535 and (ref != tar).mean() > 0.5
