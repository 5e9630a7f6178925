"""Device times of the displacement validation (sift3d_validate_displacements) beside sift3d_strain on the same input: a regular grid
of 47^3 = 103823 POIs at a step of 4 voxels with radius 16 (9^3 - 1 = 728 neighbours in the interior), scripts/strain_times.py's smooth
field plus noise, 0.5 % of the vectors off by 3 voxels, every POI valid.  Median over --steps calls after --warmup calls of the device
seconds each call returns (HIP events; the inputs stay on the device, the copy of the records to the host is inside).  Validation is
timed without and with the gradients, at its default options (2 passes and the report: three launches of the test kernel).  Writes
profiles/validate_times.json (--out) and prints it.

    python scripts/validate_times.py [--steps 20] [--warmup 5] [--out profiles/validate_times.json]
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
N, RADIUS = 47, 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "validate_times.json"))
    a = ap.parse_args()
    capi = importlib.import_module("3dsift_amd.capi")
    if capi.device_count() < 1:
        raise SystemExit("no GPU: nothing to measure")
    import torch
    from strain_times import field, grid

    q = grid(N)
    u = field(q)
    rng = np.random.default_rng(3)
    rows = rng.choice(len(q), len(q) // 200, replace=False)
    u[rows, rng.integers(0, 3, len(rows))] += rng.choice([-3.0, 3.0], len(rows))
    x, y, z = (q[:, k].astype(np.float64) for k in range(3))
    zero = np.zeros_like(x)
    g = np.stack([np.cos(x / 90.0) / 30.0, zero + 0.01, zero, zero, -np.sin(y / 70.0 + z / 110.0) / 35.0, -np.sin(y / 70.0 + z / 110.0) / 55.0,
                  1e-5 * z, zero - 0.02, 1e-5 * x], 1)   # the smooth field's gradient
    dq, du, dg = torch.from_numpy(q).cuda(), torch.from_numpy(u).cuda(), torch.from_numpy(g).cuda()
    torch.cuda.synchronize()
    calls = {"strain": lambda: capi.strain(dq, du, radius=RADIUS), "validate": lambda: capi.validate(dq, du, radius=RADIUS),
             "validate_with_gradients": lambda: capi.validate(dq, du, dg, radius=RADIUS)}
    out = {"steps": a.steps, "warmup": a.warmup, "kernel_source_sha": capi.kernel_source_sha(), "pois": len(q), "grid_step": 4, "radius": RADIUS,
           "planted": len(rows), "defaults": capi.default_validate_options(), "stage_capacity": capi.validate_stage_capacity()}
    for name, call in calls.items():
        for _ in range(a.warmup):
            res = call()
        dev = [call()["seconds"] for _ in range(a.steps)]
        out[name] = {"device_ms": round(float(np.median(dev)) * 1e3, 4), "device_ms_min": round(float(np.min(dev)) * 1e3, 4),
                     "device_ms_max": round(float(np.max(dev)) * 1e3, 4), "largest_window": int(res["neighbours"].max()),
                     "status_counts": np.bincount(res["status"], minlength=5).tolist()}
        if "flagged" in res:
            out[name]["flagged"] = int(res["flagged"].sum())
            out[name]["flagged_and_planted"] = int(res["flagged"][rows].sum())
        print(json.dumps({name: out[name]}), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
