"""Device times of the ZNCC integer search (sift3d_zncc_search): a 256^3 pair with a POI grid of step 16 at (r, s) = (8, 8) and
(16, 16).  The pair is synth.blobs_torch's dense blobs (one per 512 voxels) and the same blobs shifted by (3.37, -2.52, 1.21) voxels;
the guess is zero and every POI keeps its whole search window inside the target, so each scores (2s+1)^3 candidates.  Median over
--steps calls after --warmup calls of the device seconds the call returns (HIP events; the volumes stay on the device) and the
multiply-adds per second they imply: POIs x scored candidates x (2r+1)^3 (one multiply-add of sum R'T' per candidate and voxel; the
kernel forms sum T' and sum T'^2 beside it, which are not counted), with its fraction of the fp32 vector peak (157.3 TFLOP/s = 78.65e12
multiply-adds per second).  Writes profiles/search_times.json (--out) and prints it.

    python scripts/search_times.py [--steps 10] [--warmup 2] [--out profiles/search_times.json]
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
SHIFT = (3.37, -2.52, 1.21)
CASES = [("256_step16_r8_s8", 256, 16, 8, 8), ("256_step16_r16_s16", 256, 16, 16, 16)]
PEAK_FMA_PER_S = 157.3e12 / 2


def grid(n, step, reach):
    g = np.arange(reach + 4, n - reach - 4, step)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)[:, ::-1].astype(np.int32).copy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "search_times.json"))
    a = ap.parse_args()
    capi = importlib.import_module("3dsift_amd.capi")
    synth = importlib.import_module("3dsift_amd.synth")
    if capi.device_count() < 1:
        raise SystemExit("no GPU: nothing to measure")
    import torch

    out = {"steps": a.steps, "warmup": a.warmup, "kernel_source_sha": capi.kernel_source_sha(), "defaults": capi.default_search_options(),
           "shift": SHIFT, "peak_fma_per_s": PEAK_FMA_PER_S}
    n = 256
    shape = (n, n, n)
    nb = n * n * n // 512
    R = synth.blobs_torch(shape, "cuda", seed=1234, nblobs=nb).contiguous()
    T = synth.blobs_torch(shape, "cuda", seed=1234, shift=SHIFT, nblobs=nb).contiguous()
    torch.cuda.synchronize()
    for name, n, step, r, s in CASES:
        q = grid(n, step, r + s)
        dq = torch.from_numpy(q).cuda()
        for _ in range(a.warmup):
            res = capi.zncc_search(R, T, dq, subset_radius=r, search_radius=s)
        dev, wall = [], []
        for _ in range(a.steps):
            t0 = time.perf_counter()
            res = capi.zncc_search(R, T, dq, subset_radius=r, search_radius=s)
            wall.append(time.perf_counter() - t0)
            dev.append(res["seconds"])
        ok = res["status"] == 0
        fma = int(res["candidates"].astype(np.int64).sum()) * (2 * r + 1) ** 3
        med = float(np.median(dev))
        hit = int((np.abs(res["d"][ok] - np.array(SHIFT)).max(1) < 1.0).sum()) if ok.any() else 0
        out[name] = {"volume": n, "grid_step": step, "subset_radius": r, "search_radius": s, "pois": len(q), "found": int(ok.sum()),
                     "within_one_voxel": hit, "status_counts": np.bincount(res["status"], minlength=5).tolist(), "multiply_adds": fma,
                     "device_ms": round(med * 1e3, 4), "device_ms_min": round(float(np.min(dev)) * 1e3, 4),
                     "wall_ms": round(float(np.median(wall)) * 1e3, 4), "fma_per_s": float(f"{fma / med:.4g}"),
                     "fraction_of_fp32_peak": round(fma / med / PEAK_FMA_PER_S, 4)}
        print(json.dumps({name: out[name]}), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
