"""Device times of the RANSAC affine fits (sift3d_fit_affine / sift3d_fit_affine_local) with the default options: the global fit on
11 292 pairs (the matched pairs of a 512^3 extraction; half of them outliers) and the local fits of 100 000 points with k = 32.
Median over --steps calls after --warmup calls of the device seconds the call returns (HIP events; the input upload excluded, the
copy of the results included), plus the host clock around the call.  Writes profiles/ransac_times.json (--out) and prints it.
Kernel times: run it under rocprofv3 --kernel-trace --stats (scripts/README.md).

    python scripts/ransac_times.py [--steps 20] [--warmup 3] [--out profiles/ransac_times.json]
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


def pairs_of(n, m, seed=1):
    rng = np.random.default_rng(seed)
    r = rng.uniform(0, 512, (n, 3))
    th = 0.15
    L = np.array([[np.cos(th), -np.sin(th), 0], [np.sin(th), np.cos(th), 0], [0, 0, 1]]) * 1.02
    t = r @ L.T + np.array([5.0, -3.0, 2.0]) + rng.normal(0, 0.5, r.shape)
    bad = rng.random(n) < 0.5
    t[bad] = rng.uniform(0, 512, (int(bad.sum()), 3))
    return np.concatenate([r, t], 1).astype(np.float32), rng.uniform(0, 512, (m, 3)).astype(np.float32)


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ransac_times.json"))
    a = ap.parse_args()
    capi = importlib.import_module("3dsift_amd.capi")
    if capi.device_count() < 1:
        raise SystemExit("no GPU: nothing to measure")
    n, m, k = 11292, 100000, 32
    pairs, pts = pairs_of(n, m)
    out = {"steps": a.steps, "warmup": a.warmup, "kernel_source_sha": capi.kernel_source_sha(), "defaults": capi.default_ransac_options()}
    t, r = timed(lambda: capi.fit_affine(pairs), a.steps, a.warmup)
    out["global"] = dict(pairs=n, hypotheses=4096, residuals=n * 4096, inliers=int(r["inliers"]), **t)
    t, r = timed(lambda: capi.fit_affine(pairs, iterations=65536), max(3, a.steps // 4), 1)
    out["global_h65536"] = dict(pairs=n, hypotheses=65536, residuals=n * 65536, **t)
    t, r = timed(lambda: capi.fit_affine_local(pairs, pts, k=k), a.steps, a.warmup)
    out["local"] = dict(pairs=n, points=m, k=k, hypotheses=256, residuals=m * 256 * k, ok=int((r["status"] == 0).sum()), **t)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
