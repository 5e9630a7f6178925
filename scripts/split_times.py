"""Device times of the distance transform (sift3d_mask_distance) and of the labels of touching bodies (sift3d_mask_split).
An n^3 mask (default 512^3) on the device, three masks: (i) the benchmark's synthetic blob volume thresholded at its median (the mask
of scripts/label_times.py), (ii) a packing of touching balls (a jittered lattice of pitch 40 with balls of radius 22), (iii) the
transform's worst case, every voxel in but one, with border = 0.  Beside each transform time: sift3d_mask_from_level on a volume of
the same size in the same session (a pure streaming pass: the floor of DESIGN 4.13's table), and with --scipy
scipy.ndimage.distance_transform_edt on the host, whose rounded square must equal the device result.  For (i) and (ii) the split: its
total time and round count at both connectivities, and the time of a growth round from the difference between max_rounds = 16 and 8
(two batches of eight rounds against one).  Median over --steps calls after --warmup calls of the device seconds a call returns (HIP
events); the worst case is called --worst-steps times after one call.  Writes profiles/split_times.json (--out) and prints it.

    python scripts/split_times.py [--n 512] [--steps 20] [--warmup 5] [--scipy] [--out profiles/split_times.json]
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
PITCH, RADIUS, JITTER, BALL_CORE_DIST2 = 40, 22, 3, 200


def median_seconds(call, steps, warmup):
    for _ in range(warmup):
        call()
    return float(np.median([call() for _ in range(steps)]))


def ball_packing(n, torch):
    """uint8 (n, n, n) on the device: balls of radius RADIUS on a lattice of pitch PITCH whose centres are moved by up to JITTER"""
    rng = np.random.default_rng(40)
    mask = torch.zeros((n, n, n), dtype=torch.uint8, device="cuda")
    r = RADIUS
    g = torch.arange(-r, r + 1, device="cuda")
    ball = ((g[:, None, None] ** 2 + g[None, :, None] ** 2 + g[None, None, :] ** 2) <= r * r).to(torch.uint8)
    count = 0
    for cz in range(PITCH // 2, n, PITCH):
        for cy in range(PITCH // 2, n, PITCH):
            for cx in range(PITCH // 2, n, PITCH):
                c = np.array([cz, cy, cx]) + rng.integers(-JITTER, JITTER + 1, 3)
                lo, hi = np.maximum(c - r, 0), np.minimum(c + r + 1, n)
                if (hi <= lo).any():
                    continue
                src = tuple(slice(int(l - (k - r)), int(h - (k - r))) for l, h, k in zip(lo, hi, c))
                dst = tuple(slice(int(l), int(h)) for l, h in zip(lo, hi))
                mask[dst] |= ball[src]
                count += 1
    return mask, count


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--worst-steps", type=int, default=3)
    ap.add_argument("--scipy", action="store_true", help="also time scipy.ndimage.distance_transform_edt on the host and compare")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "split_times.json"))
    a = ap.parse_args()
    capi = importlib.import_module("3dsift_amd.capi")
    synth = importlib.import_module("3dsift_amd.synth")
    if capi.device_count() < 1:
        raise SystemExit("no GPU: nothing to measure")
    import torch

    n, voxels = a.n, a.n ** 3
    out = {"n": n, "voxels": voxels, "steps": a.steps, "warmup": a.warmup, "worst_steps": a.worst_steps,
           "kernel_source_sha": capi.kernel_source_sha(), "copy_GBps": round(capi.copy_bandwidth(), 1)}
    vol = synth.blobs_torch((n, n, n), torch.device("cuda", 0))
    level = float(vol.flatten()[:: max(1, voxels // (1 << 24))].median())
    floor = median_seconds(lambda: capi.mask_from_level(vol, level, with_seconds=True)[1], a.steps, a.warmup)
    out["mask_from_level_ms"] = round(floor * 1e3, 4)
    blobs = capi.mask_from_level(vol, level)
    del vol
    packing, balls = ball_packing(n, torch)
    out["balls"] = {"count": balls, "pitch": PITCH, "radius": RADIUS, "jitter": JITTER}
    worst = torch.ones((n, n, n), dtype=torch.uint8, device="cuda")
    worst[n // 3, n // 2, n // 5] = 0
    cases = {"blobs_at_median": (blobs, 1, {"core_dist2": 16}, a.steps, a.warmup),
             "touching_balls": (packing, 1, {"core_dist2": BALL_CORE_DIST2}, a.steps, a.warmup),
             "all_in_but_one_border0": (worst, 0, None, a.worst_steps, 1)}
    for name, (mask, border, split, steps, warmup) in cases.items():
        t = median_seconds(lambda: capi.mask_distance(mask, border, with_seconds=True)[1], steps, warmup)
        dist = capi.mask_distance(mask, border)
        row = {"density": round(float(mask.float().mean()), 4), "border": border, "max_dist2": int(dist.max()),
               "distance_ms": round(t * 1e3, 4), "times_mask_from_level": round(t / floor, 2), "voxels_per_s": float(f"{voxels / t:.4g}")}
        if a.scipy:
            ndi = importlib.import_module("scipy.ndimage")
            host = mask.cpu().numpy()
            if border:
                host = np.pad(host, 1)
            t0 = time.perf_counter()
            edt = ndi.distance_transform_edt(host)
            row["scipy_host_s"] = round(time.perf_counter() - t0, 3)
            want = np.rint(edt * edt).astype(np.int32)
            if border:
                want = want[1:-1, 1:-1, 1:-1]
            row["scipy_equal"] = bool(np.array_equal(want, dist.cpu().numpy()))
            del host, edt, want
        del dist
        if split is not None:
            for connectivity in (6, 26):
                o = dict(split, connectivity=connectivity, border=border)
                lab, count, info = capi.mask_split(mask, **o)
                del lab
                total = median_seconds(lambda: capi.mask_split(mask, with_seconds=True, **o)[3], steps, warmup)
                plain = capi.mask_label(mask, connectivity)[1]
                r = {"options": o, "count": count, "info": info, "mask_label_count": plain, "split_ms": round(total * 1e3, 4),
                     "times_distance": round(total / t, 2)}
                r["mask_label_ms"] = round(median_seconds(lambda: capi.mask_label(mask, connectivity, with_seconds=True)[2], steps, warmup) * 1e3, 4)
                t8 = median_seconds(lambda: capi.mask_split(mask, with_seconds=True, max_rounds=8, **o)[3], steps, warmup)
                r["split_max_rounds_8_ms"] = round(t8 * 1e3, 4)
                if info["rounds"] >= 16:
                    t16 = median_seconds(lambda: capi.mask_split(mask, with_seconds=True, max_rounds=16, **o)[3], steps, warmup)
                    r["round_ms_from_16_minus_8"] = round((t16 - t8) / 8 * 1e3, 4)
                row[f"c{connectivity}"] = r
        out[name] = row
        print(json.dumps({name: row}), flush=True)
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:   # after every mask: the worst case comes last and takes the longest
            json.dump(out, f)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
