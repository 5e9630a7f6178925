"""Device times of the connected-component labels (sift3d_mask_label) and the cost of the label test in the window calls.
Labelling: an n^3 mask (default 512^3) on the device at both connectivities, on two masks: the benchmark's synthetic blob volume
thresholded at its median, and a random mask of density 0.3116 (the percolation threshold of 6-connectivity, the ramified case).
Beside each time: sift3d_mask_from_level on the same volume in the same session (a pure streaming pass over the same voxels: the
floor), the library's measured copy bandwidth and the fraction of it that the 5 bytes per voxel the labelling must move (1 read, 4
written) would reach in the measured time, and with --scipy scipy.ndimage.label on the host.  Window calls: sift3d_strain_labelled
with all labels equal against sift3d_strain on a grid of 47^3 = 103823 POIs at a step of 4, radius 8 and 20.  Median over --steps
calls after --warmup calls of the device seconds a call returns (HIP events).  Writes profiles/label_times.json (--out) and prints it.

    python scripts/label_times.py [--n 512] [--steps 20] [--warmup 5] [--scipy] [--out profiles/label_times.json]
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
DENSITY = 0.3116
STEP, SIDE = 4, 47


def median_seconds(call, steps, warmup):
    for _ in range(warmup):
        call()
    return float(np.median([call() for _ in range(steps)]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--scipy", action="store_true", help="also time scipy.ndimage.label on the host (seconds per mask at 512^3)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "label_times.json"))
    a = ap.parse_args()
    capi = importlib.import_module("3dsift_amd.capi")
    synth = importlib.import_module("3dsift_amd.synth")
    if capi.device_count() < 1:
        raise SystemExit("no GPU: nothing to measure")
    import torch

    n, voxels = a.n, a.n ** 3
    copy_gbs = capi.copy_bandwidth()
    out = {"n": n, "voxels": voxels, "steps": a.steps, "warmup": a.warmup, "kernel_source_sha": capi.kernel_source_sha(),
           "tile": capi.label_tile(), "copy_GBps": round(copy_gbs, 1)}
    vol = synth.blobs_torch((n, n, n), torch.device("cuda", 0))
    level = float(vol.flatten()[:: max(1, voxels // (1 << 24))].median())
    gen = torch.Generator(device="cuda")
    gen.manual_seed(3116)
    noise = torch.rand((n, n, n), device="cuda", generator=gen)
    masks = {"blobs_at_median": (vol, level), "random_0.3116": (noise, 1.0 - DENSITY)}
    for name, (src, lev) in masks.items():
        floor = median_seconds(lambda: capi.mask_from_level(src, lev, with_seconds=True)[1], a.steps, a.warmup)
        mask = capi.mask_from_level(src, lev)
        row = {"density": round(float(mask.float().mean()), 4), "mask_from_level_ms": round(floor * 1e3, 4)}
        host = mask.cpu().numpy() if a.scipy else None
        for connectivity in (6, 26):
            count = capi.mask_label(mask, connectivity)[1]
            t = median_seconds(lambda: capi.mask_label(mask, connectivity, with_seconds=True)[2], a.steps, a.warmup)
            row[f"c{connectivity}"] = {"count": count, "device_ms": round(t * 1e3, 4), "times_mask_from_level": round(t / floor, 2),
                                       "voxels_per_s": float(f"{voxels / t:.4g}"),
                                       "fraction_of_copy_at_5B_per_voxel": round(5.0 * voxels / t / (copy_gbs * 1e9), 4)}
            if host is not None:
                ndi = importlib.import_module("scipy.ndimage")
                t0 = time.perf_counter()
                lab, cnt = ndi.label(host, ndi.generate_binary_structure(3, 1 if connectivity == 6 else 3))
                row[f"c{connectivity}"]["scipy_host_s"] = round(time.perf_counter() - t0, 3)
                row[f"c{connectivity}"]["scipy_count_equal"] = bool(cnt == count)
                del lab
        out[name] = row
        print(json.dumps({name: row}), flush=True)
        del mask
    del vol, noise, masks
    torch.cuda.empty_cache()

    g = (np.arange(SIDE) * STEP).astype(np.int32)
    q = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)[:, ::-1].copy()
    x, y, z = (q[:, k].astype(np.float64) for k in range(3))
    u = np.stack([3.0 * np.sin(x / 90.0) + 0.01 * y, 2.0 * np.cos(y / 70.0 + z / 110.0), 1e-5 * x * z - 0.02 * y], 1)
    dq, du = torch.from_numpy(q).cuda(), torch.from_numpy(u).cuda()
    one = torch.ones(len(q), dtype=torch.int32, device="cuda")
    for radius in (8, 20):
        plain = median_seconds(lambda: capi.strain(dq, du, radius=radius)["seconds"], a.steps, a.warmup)
        own = median_seconds(lambda: capi.strain(dq, du, label=one, radius=radius)["seconds"], a.steps, a.warmup)
        out[f"strain_radius{radius}"] = {"pois": len(q), "plain_ms": round(plain * 1e3, 4), "labelled_all_equal_ms": round(own * 1e3, 4),
                                         "ratio": round(own / plain, 3)}
        print(json.dumps({f"strain_radius{radius}": out[f"strain_radius{radius}"]}), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
