"""Device times of guided matching (sift3d_match_guided) beside the brute-force matcher (sift3d_match) on the same rows in the same
process: 11 292 x 11 292 descriptors whose positions are scattered uniformly in 512^3 (the keypoint count of a 512^3 extraction),
every reference row a noisy copy of a target drawn at random and expected within a voxel of it; radius 24 (about 10 targets per gate) and radius 96
(about 600: the dense gate).  Median over --steps calls after --warmup calls of the device seconds the call returns (HIP events around
the device work: the two indexes, the gated passes and the copies of the results; the inputs are device tensors).  Writes
profiles/match_guided_times.json (--out) and prints it.

    python scripts/match_guided_times.py [--steps 20] [--warmup 3] [--out profiles/match_guided_times.json]
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


def rows_of(n, seed=1):
    rng = np.random.default_rng(seed)
    b = np.clip(rng.normal(0.02, 0.03, (n, 768)), 0, None)
    b /= np.linalg.norm(b, axis=1, keepdims=True)
    t = rng.integers(0, n, n)   # a quarter of the targets are the partner of two rows or more: mode 3's reverse pass runs over them
    a = b[t] + 0.3 * np.clip(rng.normal(0.02, 0.03, (n, 768)), 0, None) / 0.92
    a /= np.linalg.norm(a, axis=1, keepdims=True)
    bx = rng.uniform(0, 512, (n, 3))
    pred = bx[t] + rng.normal(0, 0.5, (n, 3))
    ax = (pred - np.array([5.0, -3.0, 2.0])) / 1.02
    return [v.astype(np.float32) for v in (a, ax, b, bx, pred)]


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    dev, wall = [], []
    for _ in range(steps):
        t0 = time.perf_counter()
        r = fn()
        wall.append(time.perf_counter() - t0)
        dev.append(r["seconds"])
    return {"device_ms": round(float(np.median(dev)) * 1e3, 4), "device_ms_min": round(float(np.min(dev)) * 1e3, 4),
            "wall_ms": round(float(np.median(wall)) * 1e3, 4)}, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rows", type=int, default=11292)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "match_guided_times.json"))
    a = ap.parse_args()
    capi = importlib.import_module("3dsift_amd.capi")
    if capi.device_count() < 1:
        raise SystemExit("no GPU: nothing to measure")
    import torch

    n = a.rows
    dev = [torch.from_numpy(v).cuda() for v in rows_of(n)]
    ptr = [int(v.data_ptr()) for v in dev[:4]]
    matcher = capi.muBruteMatcher()
    out = {"steps": a.steps, "warmup": a.warmup, "rows": n, "box": 512, "kernel_source_sha": capi.kernel_source_sha()}
    for mode, name in ((1, "inject"), (3, "enhanced")):
        def plain():
            r = matcher._match(*ptr, 0.85, mode, on_device=True, n=n, m=n)
            return dict(r, seconds=matcher.totalTime)

        t, r = timed(plain, a.steps, a.warmup)
        out[f"sift3d_match_mode{mode}"] = dict(pairs=len(r["pairs"]), **t)
        for radius in (24.0, 96.0):
            t, r = timed(lambda: capi.match_guided(*dev, radius, 0.85, name), a.steps, a.warmup)
            out[f"match_guided_mode{mode}_r{radius:g}"] = dict(radius=radius, pairs=len(r["pairs"]),
                                                               mean_gate=round(float(r["candidates"].mean()), 2),
                                                               max_gate=int(r["candidates"].max()), **t)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
