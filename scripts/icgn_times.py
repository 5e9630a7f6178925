"""Device times of the IC-GN displacement refinement (sift3d_icgn) with the default options (tricubic, tolerance 1e-3, at most 20
iterations): a 256^3 pair with a POI grid of step 8 and r = 16, and a 512^3 pair with a grid of step 16 at r = 10 and r = 16.  The
pair is synth.blobs_torch's dense blobs (one per 512 voxels) and the same blobs shifted by (0.37, -0.52, 0.21) voxel; the init is
zero.  Median over --steps calls after --warmup calls of the device seconds the call returns (HIP events; the volumes stay on the
device), the mean number of iterations, and the voxel evaluations of the iterate kernel: sum over the POIs of (passes) (2r+1)^3, one
pass per iteration plus the one that gives zncc.  Writes profiles/icgn_times.json (--out) and prints it.  Kernel times: run it under
rocprofv3 --kernel-trace --stats (scripts/README.md) and divide the evaluations by the k_icgn_iterate time.

    python scripts/icgn_times.py [--steps 20] [--warmup 3] [--out profiles/icgn_times.json]
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
CASES = [("256_step8_r16", 256, 8, 16), ("512_step16_r10", 512, 16, 10), ("512_step16_r16", 512, 16, 16)]


def grid(n, step, r):
    g = np.arange(r + 2, n - r - 2, step)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)[:, ::-1].astype(np.int32).copy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "icgn_times.json"))
    a = ap.parse_args()
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
        R, T = vols[n]
        q = grid(n, step, r)
        dq = torch.from_numpy(q).cuda()
        for _ in range(a.warmup):
            res = capi.icgn(R, T, dq, subset_radius=r)
        dev, wall = [], []
        for _ in range(a.steps):
            t0 = time.perf_counter()
            res = capi.icgn(R, T, dq, subset_radius=r)
            wall.append(time.perf_counter() - t0)
            dev.append(res["seconds"])
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
        print(json.dumps({name: out[name]}), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
