"""Device times of the strain fields (sift3d_strain): regular grids of 64^3, 128^3 and 160^3 POIs at a step of 4 voxels, with windows
of 2 and of 5 grid steps (radius 8 and 20).  The displacement is a smooth field plus noise and every POI is valid.  Median over --steps
calls after --warmup calls of the device seconds the call returns (HIP events; the inputs stay on the device, the copy of the 192-byte
records to the host is inside), and what they imply: POIs per second, neighbour visits per second (accepted neighbours, counted once
although the kernel walks a window three times) and the cell grid's overhead -- the entries of the touched cells that a walk tests per
neighbour it accepts, computed here from the same grid the library builds (cells of side = radius from the lowest corner; none of
these grids reaches the cell cap).  Writes profiles/strain_times.json (--out) and prints it.

    python scripts/strain_times.py [--steps 20] [--warmup 2] [--out profiles/strain_times.json]
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
STEP = 4
CASES = [(n, k) for n in (64, 128, 160) for k in (2, 5)]


def grid(n):
    g = (np.arange(n) * STEP).astype(np.int32)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)[:, ::-1].copy()


def field(q, seed=1):
    x, y, z = (q[:, k].astype(np.float64) for k in range(3))
    u = np.stack([3.0 * np.sin(x / 90.0) + 0.01 * y, 2.0 * np.cos(y / 70.0 + z / 110.0), 1e-5 * x * z - 0.02 * y], 1)
    return u + np.random.default_rng(seed).normal(0.0, 0.02, u.shape)


def candidates_tested(q, radius):
    """entries of the cells each POI's window touches, summed over the POIs: the library's grid, restated with an integral image"""
    lo = q.min(0).astype(np.int64)
    c = (q - lo) // radius
    n = c.max(0) + 1
    cnt = np.zeros(tuple(n), np.int64)
    np.add.at(cnt, (c[:, 0], c[:, 1], c[:, 2]), 1)
    I = np.zeros(tuple(n + 1), np.int64)
    I[1:, 1:, 1:] = cnt.cumsum(0).cumsum(1).cumsum(2)
    a = np.clip((q - radius - lo) // radius, 0, n - 1)
    b = np.clip((q + radius - lo) // radius, 0, n - 1) + 1
    ax, ay, az = a.T
    bx, by, bz = b.T
    box = (I[bx, by, bz] - I[ax, by, bz] - I[bx, ay, bz] - I[bx, by, az] + I[ax, ay, bz] + I[ax, by, az] + I[bx, ay, az] - I[ax, ay, az])
    return int(box.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "strain_times.json"))
    a = ap.parse_args()
    capi = importlib.import_module("3dsift_amd.capi")
    if capi.device_count() < 1:
        raise SystemExit("no GPU: nothing to measure")
    import torch

    out = {"steps": a.steps, "warmup": a.warmup, "kernel_source_sha": capi.kernel_source_sha(), "defaults": capi.default_strain_options(),
           "grid_step": STEP}
    for n, k in CASES:
        radius = k * STEP
        q = grid(n)
        dq, du = torch.from_numpy(q).cuda(), torch.from_numpy(field(q)).cuda()
        torch.cuda.synchronize()
        for _ in range(a.warmup):
            res = capi.strain(dq, du, radius=radius)
        dev, wall = [], []
        for _ in range(a.steps):
            t0 = time.perf_counter()
            res = capi.strain(dq, du, radius=radius)
            wall.append(time.perf_counter() - t0)
            dev.append(res["seconds"])
        med = float(np.median(dev))
        visits = int(res["neighbours"].astype(np.int64).sum())
        tested = candidates_tested(q, radius)
        name = f"{n}_cubed_radius{radius}"
        out[name] = {"pois": len(q), "radius": radius, "window_grid_steps": k, "status_counts": np.bincount(res["status"], minlength=5).tolist(),
                     "neighbour_visits": visits, "candidates_tested": tested, "tested_per_accepted": round(tested / max(visits, 1), 4),
                     "device_ms": round(med * 1e3, 4), "device_ms_min": round(float(np.min(dev)) * 1e3, 4),
                     "wall_ms": round(float(np.median(wall)) * 1e3, 4), "pois_per_s": float(f"{len(q) / med:.4g}"),
                     "neighbour_visits_per_s": float(f"{visits / med:.4g}")}
        print(json.dumps({name: out[name]}), flush=True)
        del dq, du, res
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
