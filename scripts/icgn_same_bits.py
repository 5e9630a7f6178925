#!/usr/bin/env python3
"""Same bits from two builds of the library on the IC-GN family (sift3d_icgn, sift3d_icgn_bspline, sift3d_icgn2): a fixed set of small
calls whose raw result records go to an .npz, one process per library (S3D_LIB selects it, as for the other A/B scripts), and a
comparison of two such files byte for byte.

    S3D_LIB=/path/to/parent/libsift3d_hip.so python scripts/icgn_same_bits.py --out a.npz
    python scripts/icgn_same_bits.py --out b.npz
    python scripts/icgn_same_bits.py --compare a.npz b.npz        (needs no GPU; cmp a.npz b.npz says the same: the files carry no time)

Scene: a 48^3 blob pair, the target moved by a sub-voxel shift and a 1-2 % affine about the centre; R and T have a block of constant voxels.
Calls: sift3d_icgn with Keys and with trilinear weights, sift3d_icgn_bspline with the prefilter inside the call and with given
coefficients, sift3d_icgn2 with the three interpolations started from the first-order Keys result; each at r = 2, 3, 7 and 16 (subset
walks with two, one and no carry per step, and the largest Cholesky load), with host and with device inputs, and with max_iterations 20
and 1.  POIs: a 4 x 4 x 4 lattice (at r = 16 the integer points 20, 22, 24, 26 per axis) started 0.1 voxel from the scene's map, and four more that end in
status 2 (subset over R's edge), 3 (init far outside T), 4 (inside the constant block) and 5 (NaN init); the run with max_iterations
1 gives status 1.  The script fails where a status 0 .. 5 is missing from a call pair."""
import argparse
import ctypes as C
import importlib
import io
import os
import sys
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N = 48
RADII = (2, 3, 7, 16)
SHIFT = (0.37, -0.52, 0.21)
LMAT = ((1.012, 0.008, -0.005), (-0.006, 0.985, 0.011), (0.009, -0.012, 1.018))
BLOCK_AT, BLOCK_VALUE = 30, 0.5  # the constant block of R: the cube of half width r + 1 about (30, 30, 30), a value whose sums are exact


def render(centres, sg, am):
    """synth.blobs' rendering with explicit centres (x, y, z)"""
    vol = np.zeros((N, N, N), np.float64)
    g = np.arange(N)
    for (x0, y0, z0), s, a in zip(centres, sg, am):
        w = [np.where(np.abs(g - c) <= 5.0 * s, np.exp(-0.5 * ((g - c) / s) ** 2), 0.0) for c in (x0, y0, z0)]
        vol += a * w[2][:, None, None] * w[1][None, :, None] * w[0][None, None, :]
    return vol.astype(np.float32)


def scene(synth, r):
    cx, cy, cz, sg, am = synth.blob_params((N, N, N), seed=1234, nblobs=N ** 3 // 256)
    c = np.stack([cx, cy, cz], 1)
    mid = (N - 1) / 2
    R, T = render(c, sg, am), render((c - mid) @ np.array(LMAT).T + mid + np.array(SHIFT), sg, am)
    lo, hi = BLOCK_AT - r - 1, BLOCK_AT + r + 2
    R[lo:hi, lo:hi, lo:hi] = BLOCK_VALUE
    T[lo:hi, lo:hi, lo:hi] = BLOCK_VALUE  # T too: a lattice subset that reaches into the block still has its minimum near the map
    return R, T


def pois(r):
    """the lattice, then the POIs of status 2, 3, 4, 5; the 12-parameter init rows"""
    g = 20 + 2 * np.arange(4) if r == 16 else np.rint(np.linspace(r + 4, N - 5 - r, 4)).astype(int)
    q = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)[:, ::-1]
    q = np.concatenate([q, [[r, 24, 24], [24, 24, 24], [BLOCK_AT] * 3, [24, 23, 24]]]).astype(np.int32)
    # the lattice starts 0.1 voxel from the scene's map (a subset that the constant block cuts into would not settle from zero)
    F = np.array(LMAT) - np.eye(3)
    u = (q - (N - 1) / 2) @ F.T + np.array(SHIFT) + np.array([0.1, -0.1, 0.05])
    init = np.concatenate([u[:, :, None], np.broadcast_to(F, (len(q), 3, 3))], 2).reshape(-1, 12)
    init[-4:] = 0.0
    init[-3, 0] = 40.0
    init[-1, 5] = np.nan
    return q, init


def call(capi, entry, dtype, width, R, T, q, init, coef, **opts):
    """one call through the C ABI; returns the raw records"""
    o = capi._icgn_options(opts)
    (rp, tp), (rdim, tdim), on_dev, keep = capi._volume_pair(R, T)
    qp, m, kq = capi._table(q, np.int32, 3, R)
    ip, mi, ki = capi._table(init, np.float64, width, R)
    out = np.zeros(m, dtype)
    sec = C.c_double(0)
    extra = () if coef is None else (int(coef),)
    capi._check(getattr(capi.lib(), entry)(rp, *rdim, tp, *tdim, qp, m, ip, C.byref(o), *extra, on_dev, int(0), capi._p(out), C.byref(sec)))
    return out


def run(out_path):
    capi = importlib.import_module("3dsift_amd.capi")
    synth = importlib.import_module("3dsift_amd.synth")
    if capi.device_count() < 1:
        raise SystemExit("no GPU: nothing to run")
    import torch

    rec, missing = {}, []
    for r in RADII:
        R, T = scene(synth, r)
        q, init = pois(r)
        for where in ("host", "device"):
            put = (lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()) if where == "device" else (lambda a: a)
            dR, dT, dq, dinit = put(R), put(T), put(q), put(init)
            dcoef = capi.bspline_prefilter(dT)
            for max_it in (20, 1):
                o = dict(subset_radius=r, max_iterations=max_it)
                first = {"icgn_keys": call(capi, "sift3d_icgn", capi.ICGN_DTYPE, 12, dR, dT, dq, dinit, None, interpolation=0, **o),
                         "icgn_linear": call(capi, "sift3d_icgn", capi.ICGN_DTYPE, 12, dR, dT, dq, dinit, None, interpolation=1, **o),
                         "bspline_prefilter": call(capi, "sift3d_icgn_bspline", capi.ICGN_DTYPE, 12, dR, dT, dq, dinit, 0, **o),
                         "bspline_coefficients": call(capi, "sift3d_icgn_bspline", capi.ICGN_DTYPE, 12, dR, dcoef, dq, dinit, 1, **o)}
                # the second order starts from the first-order Keys result; the POIs of status 2, 3, 4 keep a finite row (their init)
                keys = first["icgn_keys"]
                init2 = capi.icgn2_init_from_icgn({"p": keys["p"], "status": keys["status"]})
                init2[-4:-1] = capi.icgn2_init_from_icgn({"p": init[-4:-1], "status": [0, 0, 0]})
                dinit2 = put(init2)
                second = {f"icgn2_{name}": call(capi, "sift3d_icgn2", capi.ICGN2_DTYPE, 30, dR, dcoef if coef else dT, dq, dinit2, coef,
                                                interpolation=kind, **o)
                          for name, kind, coef in (("keys", 0, 0), ("linear", 1, 0), ("bspline_prefilter", 2, 0), ("bspline_coefficients", 2, 1))}
                for name, res in {**first, **second}.items():
                    rec[f"{name}_r{r}_{where}_it{max_it}"] = res
        for name in list(first) + list(second):
            seen = set()
            for where in ("host", "device"):
                for max_it in (20, 1):
                    seen |= set(rec[f"{name}_r{r}_{where}_it{max_it}"]["status"].tolist())
            counts = np.bincount(rec[f"{name}_r{r}_host_it20"]["status"] + 1, minlength=8)[1:].tolist()
            print(f"{name} r={r}: status counts at max_iterations 20 {counts}, statuses seen {sorted(seen)}", flush=True)
            if not set(range(6)) <= seen:
                missing.append((name, r, sorted(set(range(6)) - seen)))
    # an .npz without the time of day: two runs that compute the same bytes write the same file
    with zipfile.ZipFile(out_path, "w", zipfile.ZIP_STORED) as z:
        for k in sorted(rec):
            b = io.BytesIO()
            np.lib.format.write_array(b, np.frombuffer(rec[k].tobytes(), np.uint8))
            z.writestr(zipfile.ZipInfo(k + ".npy", (1980, 1, 1, 0, 0, 0)), b.getvalue())
    print(f"{len(rec)} calls, {sum(v.nbytes for v in rec.values())} bytes of records -> {out_path} ({os.path.basename(capi.LIB_PATH)} of "
          f"{os.path.dirname(capi.LIB_PATH)})", flush=True)
    if missing:
        raise SystemExit(f"statuses not covered: {missing}")


def compare(a_path, b_path):
    a, b = np.load(a_path), np.load(b_path)
    if sorted(a.files) != sorted(b.files):
        raise SystemExit("the two files hold different calls")
    bad = [k for k in sorted(a.files) if a[k].tobytes() != b[k].tobytes()]
    for k in bad:
        x, y = a[k], b[k]
        at = np.flatnonzero(x != y) if x.shape == y.shape else []
        print(f"{k}: {len(at)} bytes differ, the first at byte {at[0] if len(at) else '-'}")
    with open(a_path, "rb") as f, open(b_path, "rb") as g:
        same_file = f.read() == g.read()
    print(f"{len(a.files)} calls, {sum(a[k].nbytes for k in a.files)} bytes: {'every byte equal' if not bad else f'{len(bad)} calls differ'}; "
          f"the files are {'identical' if same_file else 'different'}")
    if bad or not same_file:
        raise SystemExit(1)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="run the calls with the library of S3D_LIB (default: the tree's) and write the records here")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"), help="compare two files of records byte for byte")
    a = ap.parse_args()
    if a.compare:
        compare(*a.compare)
    elif a.out:
        run(a.out)
    else:
        ap.error("--out or --compare")
