"""Times of the two per-body calls against what one call per body costs -> profiles/bodies_times.json.

  fits      sift3d_fit_rigid_bodies on 10^5 pairs in 10^4 bodies and on the spheres scene of tests/body_cases.py, against a loop of
            sift3d_fit_rigid over host-gathered sub-lists (the same fits up to the problem index)
  labelled  sift3d_icgn_labelled on the spheres scene (12 labels, r = 6, the lattice POIs inside spheres, 5 fixed updates), against 12
            sift3d_icgn_masked calls with the mask labels == L, host inputs and device inputs

Wall-clock milliseconds of whole calls (what a user waits for), medians of alternating runs in one process; the calls' own device
seconds beside them.  Usage: python scripts/bodies_times.py [--repeats 5] [--out profiles/bodies_times.json]"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

capi = importlib.import_module("3dsift_amd.capi")
import body_cases as cases  # noqa: E402
import label_cases  # noqa: E402


def timed(f):
    t = time.perf_counter()
    out = f()
    return (time.perf_counter() - t) * 1e3, out


def alternate(named, repeats):
    """{name: median wall ms} and {name: median device ms} of the functions, run in turn `repeats` times after one warm-up each"""
    for f in named.values():
        f()
    wall, dev = {k: [] for k in named}, {k: [] for k in named}
    for _ in range(repeats):
        for k, f in named.items():
            ms, sec = timed(f)
            wall[k].append(ms)
            dev[k].append(sec * 1e3)
    return {k: float(np.median(v)) for k, v in wall.items()}, {k: float(np.median(v)) for k, v in dev.items()}


def fits_case(pairs, labels, count, repeats, **opts):
    rows = [np.flatnonzero(labels == L) for L in range(1, count + 1)]

    def bodies():
        return capi.fit_rigid_bodies(pairs, labels, count, **opts)["seconds"]

    def loop():
        sec = 0.0
        for r in rows:
            sec += capi.fit_rigid(np.ascontiguousarray(pairs[r]), iterations=256, **opts)["seconds"]
        return sec

    wall, dev = alternate({"fit_rigid_bodies": bodies, "fit_rigid_per_body": loop}, repeats)
    return {"pairs": int(len(pairs)), "bodies": int(count), "wall_ms": wall, "device_ms": dev}


def labelled_case(repeats):
    import torch

    vol, centres, q, u, body = label_cases.spheres()
    labels = np.ascontiguousarray(cases.sphere_labels())
    rng = np.random.default_rng(0)
    tar = np.ascontiguousarray(vol + rng.normal(0, 0.01, vol.shape).astype(np.float32))
    r = 6
    lo, hi = r + 1, np.array(vol.shape[::-1]) - 2 - r
    keep = (body > 0) & (q >= lo).all(1) & (q <= hi).all(1)
    q, body = np.ascontiguousarray(q[keep]), body[keep]
    opts = dict(subset_radius=r, max_iterations=5, tolerance=0.0)
    masks = {int(L): (labels == L).astype(np.uint8) for L in np.unique(body)}
    rows = {L: np.ascontiguousarray(q[body == L]) for L in masks}
    dv, dt, dl = torch.tensor(vol).cuda(), torch.tensor(tar).cuda(), torch.tensor(labels).cuda()
    dq = torch.from_numpy(q).cuda()
    dmasks = {L: torch.from_numpy(m).cuda() for L, m in masks.items()}
    drows = {L: torch.from_numpy(v).cuda() for L, v in rows.items()}

    named = {
        "icgn_labelled_host": lambda: capi.icgn_labelled(vol, tar, labels, q, **opts)["seconds"],
        "icgn_masked_per_body_host": lambda: sum(capi.icgn_masked(vol, tar, masks[L], rows[L], **opts)["seconds"] for L in masks),
        "icgn_labelled_device": lambda: capi.icgn_labelled(dv, dt, dl, dq, **opts)["seconds"],
        "icgn_masked_per_body_device": lambda: sum(capi.icgn_masked(dv, dt, dmasks[L], drows[L], **opts)["seconds"] for L in masks),
    }
    wall, dev = alternate(named, repeats)
    active = capi.icgn_labelled(vol, tar, labels, q, **opts)["active"]
    return {"pois": int(len(q)), "labels": len(masks), "subset_radius": r, "updates": 5, "active_voxels": int(active.sum()),
            "wall_ms": wall, "device_ms": dev}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bodies_times.json"))
    a = ap.parse_args()
    sizes = tuple(3 + (7 * i) % 15 for i in range(10000))   # 3 .. 17 pairs, 10 on average: 10^5 pairs but for a few
    pairs, labels, count = cases.bodies_of(sizes, 1, extra=(), noise=0.1, outliers=0.2)
    gp, gl, gc = cases.grains()
    out = {
        "fits_many_small_bodies": fits_case(pairs, labels, count, min(a.repeats, 3)),
        "fits_spheres": fits_case(np.array(gp), np.array(gl), gc, a.repeats, inlier_thresh=cases.TAU),
        "labelled_spheres": labelled_case(a.repeats),
    }
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
