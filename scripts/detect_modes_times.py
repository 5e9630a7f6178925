"""Stage times of the detection options (sift3d_set_detect_options): default (the reference's 8-neighbour rule), 80 neighbours, and
80 neighbours + sub-voxel refinement, at 512^3 and 256^3 on one GPU.  Per mode and size: median over --steps runs of
sift3d_stage_times after --warmup runs, plus the extrema / keypoint counts.  Prints one JSON line.

    python scripts/detect_modes_times.py [--steps 20] [--warmup 5] [--sizes 512,256]
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MODES = {"default": dict(), "n80": dict(neighbours=80), "n80_refine": dict(neighbours=80, refine=True)}
KEYS = ["d_TotalTime", "d_BuildGSS", "d_Detect", "d_AssignOrientation", "d_Extraction"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sizes", default="512,256")
    a = ap.parse_args()
    import torch

    capi = importlib.import_module("3dsift_amd.capi")
    synth = importlib.import_module("3dsift_amd.synth")
    dev = torch.device("cuda", 0)
    out = {"steps": a.steps, "warmup": a.warmup, "kernel_source_sha": capi.kernel_source_sha(), "sizes": {}}
    for n in (int(s) for s in a.sizes.split(",")):
        shape = (n, n, n)
        vol = synth.blobs_torch(shape, dev, seed=1234)
        torch.cuda.synchronize()
        res = {}
        for mode, opts in MODES.items():
            ex = capi.CSIFT3D(None, device=0, device_ptr=vol.data_ptr(), shape=shape)
            if opts:
                ex.set_detect_options(**opts)
            for _ in range(a.warmup):
                ex.KpSiftAlgorithm()
            t = {k: [] for k in KEYS}
            for _ in range(a.steps):
                ex.KpSiftAlgorithm()
                m = ex.m_timer
                for k in KEYS:
                    t[k].append(m[k] * 1e3)
            res[mode] = {k + "_ms": round(float(np.median(v)), 4) for k, v in t.items()}
            res[mode]["extrema"] = len(ex.extrema())
            res[mode]["keypoints"] = len(ex.GetKeypoints(with_desc=False)[0])
            ex.close()
        out["sizes"][f"{n}^3"] = res
        del vol
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
