"""Device times of the subset screening (sift3d_subset_quality): a 256^3 volume of synth.blobs_torch's dense blobs (one per 512
voxels) with a POI grid of step 4 whose cubes of radius 32 plus margin lie inside it (48^3 = 110592 POIs), under the plans
(r_min, r_max) = (8, 8), (4, 16) and (4, 32), criterion 0.  The threshold of a plan is the restatement's (tests/subset_ref.py) median
c(rho) at the plan's middle radius (r_min + r_max) / 2 over a seeded sample of 256 POIs, so about half of the POIs stop by the
middle radius and the others walk on.  Beside each figure: one sift3d_icgn call with max_iterations = 1 on the same POIs at r_max
(the target is the same blobs shifted by (0.37, -0.52, 0.21) voxels), and the ratio of the two.  Median over --steps calls after
--warmup calls of the device seconds the calls return (HIP events; the volumes and the POIs stay on the device).  voxels: the voxels
the walks visited (the cube of each reported radius); seven loads each.  Writes profiles/subset_times.json (--out) and prints it.

    python scripts/subset_times.py [--steps 20] [--warmup 5] [--out profiles/subset_times.json]
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
SHIFT = (0.37, -0.52, 0.21)
PLANS = [(8, 8), (4, 16), (4, 32)]
N, STEP, REACH, SAMPLE = 256, 4, 33, 256


def grid(n, step, reach):
    g = np.arange(reach + 1, n - reach, step)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)[:, ::-1].astype(np.int32).copy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "subset_times.json"))
    a = ap.parse_args()
    capi = importlib.import_module("3dsift_amd.capi")
    synth = importlib.import_module("3dsift_amd.synth")
    if capi.device_count() < 1:
        raise SystemExit("no GPU: nothing to measure")
    import torch

    import subset_ref as ref

    shape = (N, N, N)
    nb = N * N * N // 512
    R = synth.blobs_torch(shape, "cuda", seed=1234, nblobs=nb).contiguous()
    T = synth.blobs_torch(shape, "cuda", seed=1234, shift=SHIFT, nblobs=nb).contiguous()
    torch.cuda.synchronize()
    Rh = R.cpu().numpy()
    q = grid(N, STEP, REACH)
    dq = torch.from_numpy(q).cuda()
    sample = q[np.random.default_rng(0).choice(len(q), SAMPLE, replace=False)]
    out = {"steps": a.steps, "warmup": a.warmup, "kernel_source_sha": capi.kernel_source_sha(), "volume": N, "grid_step": STEP, "pois": len(q),
           "threshold_sample": SAMPLE, "shift": SHIFT}

    def timed(call):
        for _ in range(a.warmup):
            res = call()
        dev = []
        for _ in range(a.steps):
            res = call()
            dev.append(res["seconds"])
        return res, float(np.median(dev)), float(np.min(dev))

    for r_min, r_max in PLANS:
        mid = (r_min + r_max) // 2
        t = float(np.median([ref.criteria(Rh, p, r_min, mid, 0)[1][-1] for p in sample]))
        res, med, lo = timed(lambda: capi.subset_quality(R, dq, r_min=r_min, r_max=r_max, threshold=t))
        vox = int(((2 * res["radius"].astype(np.int64) + 1) ** 3).sum())
        _, imed, ilo = timed(lambda: capi.icgn(R, T, dq, subset_radius=r_max, max_iterations=1))
        name = f"r{r_min}_{r_max}"
        out[name] = {"r_min": r_min, "r_max": r_max, "threshold": t, "status_counts": np.bincount(res["status"], minlength=4).tolist(),
                     "radius_counts": np.bincount(res["radius"], minlength=33).tolist(), "voxels": vox,
                     "device_ms": round(med * 1e3, 4), "device_ms_min": round(lo * 1e3, 4), "voxels_per_s": float(f"{vox / med:.4g}"),
                     "icgn_one_iteration_ms": round(imed * 1e3, 4), "icgn_one_iteration_ms_min": round(ilo * 1e3, 4),
                     "subset_over_icgn": round(med / imed, 4)}
        print(json.dumps({name: out[name]}), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
