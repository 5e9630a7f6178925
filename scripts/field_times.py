"""Device times of the field evaluation (sift3d_field_eval): 10^5 real-valued queries on 2 x 10^4 POIs (27^3 of a lattice of step 4,
each moved by up to a voxel) at radius 16 under both weightings, a dense lattice of 128^3 positions over the same POIs (step
104 / 127 voxels) at radius 16 under the biweight, and sift3d_strain on the same POIs at the same radius beside them.  The
displacement is a smooth field plus noise and every POI is valid.  Median over --steps calls after --warmup calls of the device
seconds the call returns (HIP events; the inputs stay on the device, the copy of the 128-byte records to the host is inside), and
what they imply: queries per second and member visits per second (counted members, counted once although the kernel walks a window
three times).  Writes profiles/field_times.json (--out) and prints it.

    python scripts/field_times.py [--steps 20] [--warmup 2] [--out profiles/field_times.json]
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
STEP, SIDE, RADIUS = 4, 27, 16


def pois(rng):
    g = (np.arange(SIDE) * STEP + 2).astype(np.int32)
    q = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    return (q + rng.integers(-1, 2, q.shape)).astype(np.int32)


def field(q, rng):
    x, y, z = (q[:, k].astype(np.float64) for k in range(3))
    u = np.stack([3.0 * np.sin(x / 90.0) + 0.01 * y, 2.0 * np.cos(y / 70.0 + z / 110.0), 1e-5 * x * z - 0.02 * y], 1)
    return u + rng.normal(0.0, 0.02, u.shape)


def timed(call, steps, warmup):
    for _ in range(warmup):
        res = call()
    dev, wall = [], []
    for _ in range(steps):
        t0 = time.perf_counter()
        res = call()
        wall.append(time.perf_counter() - t0)
        dev.append(res["seconds"])
    return res, dev, wall


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "field_times.json"))
    a = ap.parse_args()
    capi = importlib.import_module("3dsift_amd.capi")
    if capi.device_count() < 1:
        raise SystemExit("no GPU: nothing to measure")
    import torch

    rng = np.random.default_rng(1)
    q = pois(rng)
    u = field(q, rng)
    span = float(STEP * (SIDE - 1))
    scattered = 2.0 + rng.random((100000, 3)) * span
    g = 2.0 + np.arange(128) * (span / 127.0)
    lattice = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    dq, du = torch.from_numpy(q).cuda(), torch.from_numpy(u).cuda()
    out = {"steps": a.steps, "warmup": a.warmup, "kernel_source_sha": capi.kernel_source_sha(), "defaults": capi.default_field_options(),
           "pois": len(q), "grid_step": STEP, "radius": RADIUS}
    cases = [("scattered_1e5_uniform", scattered, 0), ("scattered_1e5_biweight", scattered, 1), ("lattice_128_cubed_biweight", lattice, 1)]
    for name, xs, weighting in cases:
        dx = torch.from_numpy(xs).cuda()
        torch.cuda.synchronize()
        res, dev, wall = timed(lambda: capi.field_eval(dq, du, None, dx, radius=RADIUS, weighting=weighting), a.steps, a.warmup)
        med = float(np.median(dev))
        visits = int(res["neighbours"].astype(np.int64).sum())
        out[name] = {"queries": len(xs), "weighting": weighting, "status_counts": np.bincount(res["status"], minlength=6).tolist(),
                     "member_visits": visits, "device_ms": round(med * 1e3, 4), "device_ms_min": round(float(np.min(dev)) * 1e3, 4),
                     "wall_ms": round(float(np.median(wall)) * 1e3, 4), "queries_per_s": float(f"{len(xs) / med:.4g}"),
                     "member_visits_per_s": float(f"{visits / med:.4g}")}
        print(json.dumps({name: out[name]}), flush=True)
        del dx, res
    res, dev, wall = timed(lambda: capi.strain(dq, du, radius=RADIUS), a.steps, a.warmup)
    med = float(np.median(dev))
    visits = int(res["neighbours"].astype(np.int64).sum())
    out["strain_same_pois"] = {"pois": len(q), "status_counts": np.bincount(res["status"], minlength=5).tolist(), "neighbour_visits": visits,
                               "device_ms": round(med * 1e3, 4), "device_ms_min": round(float(np.min(dev)) * 1e3, 4),
                               "wall_ms": round(float(np.median(wall)) * 1e3, 4), "pois_per_s": float(f"{len(q) / med:.4g}"),
                               "neighbour_visits_per_s": float(f"{visits / med:.4g}")}
    print(json.dumps({"strain_same_pois": out["strain_same_pois"]}), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
