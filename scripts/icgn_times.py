"""Device times of the IC-GN displacement refinement (sift3d_icgn) with the default options (tricubic, tolerance 1e-3, at most 20
iterations): a 256^3 pair with a POI grid of step 8 and r = 16, and a 512^3 pair with a grid of step 16 at r = 10 and r = 16.  The
pair is synth.blobs_torch's dense blobs (one per 512 voxels) and the same blobs shifted by (0.37, -0.52, 0.21) voxel; the init is
zero.  Median over --steps calls after --warmup calls of the device seconds the call returns (HIP events; the volumes stay on the
device), the mean number of iterations, and the voxel evaluations of the iterate kernel: sum over the POIs of (passes) (2r+1)^3, one
pass per iteration plus the one that gives zncc.  Writes profiles/icgn_times.json (--out) and prints it.  Kernel times: run it under
rocprofv3 --kernel-trace --stats (scripts/README.md) and divide the evaluations by the k_icgn_iterate time.
--bspline adds the cubic B-spline leg: the device time of sift3d_bspline_prefilter on each volume size (median, its share of the HBM
roofline for the 6 volume transfers of its three passes, and of the 512_step16_r10 call), and in every case sift3d_icgn_bspline on
the prefiltered target (tar_is_coefficients = 1) timed in the same loop as the Keys call, the two alternating; the output then goes to
profiles/icgn_bspline_times.json.
--second-order adds the second-order leg: in every case sift3d_icgn2 (Keys) started from the first-order result
(sift3d_icgn2_init_from_icgn), timed in the same loop as the first-order call, the two alternating; its device time, mean iterations,
voxel evaluations per second and the ratio of that rate to the first-order call's in the same run go to profiles/icgn2_times.json.

    python scripts/icgn_times.py [--steps 20] [--warmup 3] [--bspline | --second-order] [--out profiles/icgn_times.json]
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHIFT = (0.37, -0.52, 0.21)
HBM_PEAK = 8.0e12  # bytes/s, the datasheet figure the roofline share is quoted against
CASES = [("256_step8_r16", 256, 8, 16), ("512_step16_r10", 512, 16, 10), ("512_step16_r16", 512, 16, 16)]


def grid(n, step, r):
    g = np.arange(r + 2, n - r - 2, step)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)[:, ::-1].astype(np.int32).copy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--bspline", action="store_true", help="add the B-spline prefilter and sift3d_icgn_bspline, alternating with the Keys calls")
    ap.add_argument("--second-order", action="store_true", help="add sift3d_icgn2 from the first-order result, alternating with the first-order calls")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.bspline and a.second_order:
        raise SystemExit("--bspline and --second-order are separate legs")
    a.out = a.out or os.path.join(ROOT, "profiles", "icgn_bspline_times.json" if a.bspline else "icgn2_times.json" if a.second_order else "icgn_times.json")
    capi = importlib.import_module("3dsift_amd.capi")
    synth = importlib.import_module("3dsift_amd.synth")
    if capi.device_count() < 1:
        raise SystemExit("no GPU: nothing to measure")
    import torch

    out = {"steps": a.steps, "warmup": a.warmup, "kernel_source_sha": capi.kernel_source_sha(), "defaults": capi.default_icgn_options(),
           "shift": SHIFT}
    vols = {}
    for name, n, step, r in CASES:
        if n not in vols:
            shape = (n, n, n)
            nb = n * n * n // 512
            vols = {n: (synth.blobs_torch(shape, "cuda", seed=1234, nblobs=nb).contiguous(),
                        synth.blobs_torch(shape, "cuda", seed=1234, shift=SHIFT, nblobs=nb).contiguous())}
            torch.cuda.synchronize()
            if a.bspline:
                coef = capi.bspline_prefilter(vols[n][1])  # what the B-spline calls below refine against
                for _ in range(a.warmup):
                    capi.bspline_prefilter(vols[n][1])
                pre = [capi.bspline_prefilter(vols[n][1], with_seconds=True)[1] for _ in range(a.steps)]
                med = float(np.median(pre))
                moved = 6 * 4 * n ** 3  # three passes, each reads and writes the volume once
                out[f"prefilter_{n}"] = {"volume": n, "device_ms": round(med * 1e3, 4), "device_ms_min": round(float(np.min(pre)) * 1e3, 4),
                                         "bytes_moved": moved, "bytes_per_s": float(f"{moved / med:.4g}"),
                                         "share_of_hbm_roofline": round(moved / HBM_PEAK / med, 4)}
                print(json.dumps({f"prefilter_{n}": out[f"prefilter_{n}"]}), flush=True)
        R, T = vols[n]
        q = grid(n, step, r)
        dq = torch.from_numpy(q).cuda()
        for _ in range(a.warmup):
            res = capi.icgn(R, T, dq, subset_radius=r)
        dev, wall, bdev, sdev = [], [], [], []
        if a.second_order:
            init2 = torch.from_numpy(capi.icgn2_init_from_icgn(res)).cuda()
            for _ in range(a.warmup):
                capi.icgn2(R, T, dq, init=init2, subset_radius=r)
        if a.bspline:
            for _ in range(a.warmup):
                capi.icgn_bspline(R, coef, dq, coefficients=True, subset_radius=r)
        for _ in range(a.steps):
            t0 = time.perf_counter()
            res = capi.icgn(R, T, dq, subset_radius=r)
            wall.append(time.perf_counter() - t0)
            dev.append(res["seconds"])
            if a.bspline:  # the same loop, the two alternating
                bres = capi.icgn_bspline(R, coef, dq, coefficients=True, subset_radius=r)
                bdev.append(bres["seconds"])
            if a.second_order:  # the same loop, the two alternating
                sres = capi.icgn2(R, T, dq, init=init2, subset_radius=r)
                sdev.append(sres["seconds"])
        st, it = res["status"], res["iterations"]
        passes = np.where((st <= 1) | (res["last_step"] > 0), it + 1, 0)
        evals = int(passes.sum()) * (2 * r + 1) ** 3
        ok = st == 0
        err = np.abs(res["displacement"][ok] - np.array(SHIFT)).max() if ok.any() else None
        med = float(np.median(dev))
        out[name] = {"volume": n, "grid_step": step, "subset_radius": r, "pois": len(q), "converged": int(ok.sum()),
                     "status_counts": np.bincount(st + 1, minlength=8)[1:].tolist(), "mean_iterations": round(float(it.mean()), 3),
                     "voxel_evaluations": evals, "device_ms": round(med * 1e3, 4), "device_ms_min": round(float(np.min(dev)) * 1e3, 4),
                     "wall_ms": round(float(np.median(wall)) * 1e3, 4), "evals_per_s_call": float(f"{evals / med:.4g}"),
                     "max_disp_error_converged": None if err is None else round(float(err), 6)}
        if a.bspline:
            bst, bit = bres["status"], bres["iterations"]
            bev = int(np.where((bst <= 1) | (bres["last_step"] > 0), bit + 1, 0).sum()) * (2 * r + 1) ** 3
            bok = bst == 0
            bmed = float(np.median(bdev))
            out[name]["bspline"] = {"converged": int(bok.sum()), "mean_iterations": round(float(bit.mean()), 3), "voxel_evaluations": bev,
                                    "device_ms": round(bmed * 1e3, 4), "device_ms_min": round(float(np.min(bdev)) * 1e3, 4),
                                    "evals_per_s_call": float(f"{bev / bmed:.4g}"),
                                    "max_disp_error_converged": round(float(np.abs(bres["displacement"][bok] - np.array(SHIFT)).max()), 6)
                                    if bok.any() else None,
                                    "prefilter_share_of_keys_call": round(out[f"prefilter_{n}"]["device_ms"] / out[name]["device_ms"], 4)}
        if a.second_order:
            sst, sit = sres["status"], sres["iterations"]
            sev = int(np.where((sst <= 1) | (sres["last_step"] > 0), sit + 1, 0).sum()) * (2 * r + 1) ** 3
            sok = sst == 0
            smed = float(np.median(sdev))
            out[name]["second_order"] = {"converged": int(sok.sum()), "status_counts": np.bincount(sst + 1, minlength=8)[1:].tolist(),
                                         "mean_iterations": round(float(sit.mean()), 3), "voxel_evaluations": sev,
                                         "device_ms": round(smed * 1e3, 4), "device_ms_min": round(float(np.min(sdev)) * 1e3, 4),
                                         "evals_per_s_call": float(f"{sev / smed:.4g}"),
                                         "rate_vs_first_order": round(sev / smed / (evals / med), 4),
                                         "max_disp_error_converged": round(float(np.abs(sres["displacement"][sok] - np.array(SHIFT)).max()), 6)
                                         if sok.any() else None}
        print(json.dumps({name: out[name]}), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
