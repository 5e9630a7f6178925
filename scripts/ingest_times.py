"""Times of the typed input (sift3d_create_typed, sift3d_volume_to_device) beside the float path, on one GPU, in one process.

    python scripts/ingest_times.py [--root DIR] [--sizes 512,256] [--reps 9] [--out FILE.json] [--only ctor|kernels|dvc]

--root: the checkout whose 3dsift_amd is measured (default: this one).  A checkout without the typed entries (the parent commit)
gives the fp32 construction only; run both, alternating, to compare them.
--only kernels: nothing but constructions from device-resident volumes, a few of each kind -- the workload to put under a kernel
trace (rocprofv3 --kernel-trace --stats -- python scripts/ingest_times.py --only kernels), which gives the device time of
k_absmax_t / k_ingest per dtype beside k_absmax / k_scale; the bytes each moves are printed here from the shapes.

Every figure is a median over --reps with the smallest and largest beside it, after one untimed warm-up of the same call; wall
times are host clocks around calls that end in a device synchronisation.  Prints one JSON object (and writes it to --out).
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

COPY_CEILING = 6.29e12  # bytes / s, the measured float4 copy (k_copy16, csrc/kernels_pyramid.hip)


def stats(ms):
    ms = sorted(ms)
    return {"median_ms": round(ms[len(ms) // 2], 3), "min_ms": round(ms[0], 3), "max_ms": round(ms[-1], 3), "n": len(ms)}


def timed(fn, reps):
    fn()  # warm-up: code objects, the staging pool, the allocator
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fn()
        out.append((time.perf_counter() - t0) * 1e3)
        del r
    return stats(out)


def volume(n, dtype):
    """blob-like integer voxels without the cost of rendering blobs at 512^3: a smooth product of sines plus noise, full range"""
    rng = np.random.Generator(np.random.PCG64(7))
    z, y, x = np.ogrid[0:n, 0:n, 0:n]
    v = (np.sin(x * 0.11) * np.sin(y * 0.07) * np.sin(z * 0.05) * 0.45 + 0.5).astype(np.float32)
    v += rng.random((n, n, n), dtype=np.float32) * 0.05
    v /= v.max()
    if np.dtype(dtype) == np.float32:
        return v
    hi = np.iinfo(dtype).max
    return np.round(v * hi).astype(dtype)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--sizes", default="512,256")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default="")
    ap.add_argument("--only", default="", choices=["", "ctor", "kernels", "dvc"])
    a = ap.parse_args()
    sys.path.insert(0, a.root)
    capi = importlib.import_module("3dsift_amd.capi")
    import torch

    if capi.device_count() < 1:
        raise SystemExit("ingest_times.py needs a GPU: a time taken without one says nothing")
    typed = hasattr(capi, "to_device")
    res = {"root": a.root, "typed_entries": typed, "reps": a.reps, "gpu": torch.cuda.get_device_name(0)}
    sizes = [int(s) for s in a.sizes.split(",")]

    def create(v, **kw):
        g = capi.CSIFT3D(v, **kw)
        g.close()

    if a.only in ("", "ctor"):
        for n in sizes:
            f = volume(n, np.float32)
            r = {"create fp32 (host)": timed(lambda: create(f), a.reps)}
            if typed:
                for dt in ("uint16", "uint8"):
                    v = volume(n, dt)
                    r[f"create_typed {dt} (host)"] = timed(lambda: create(v, keep_dtype=True), a.reps)
                r["create fp32 (host), again"] = timed(lambda: create(f), a.reps)
            res[f"construction {n}^3"] = r
            print(json.dumps({f"construction {n}^3": r}), flush=True)

    if a.only == "kernels" and typed:
        n = sizes[0]
        V = n ** 3
        vols = {dt: torch.from_numpy(volume(n, dt).view(np.int16) if dt == "uint16" else volume(n, dt)).cuda()
                for dt in ("float32", "uint16", "int16", "uint8", "int8")}
        torch.cuda.synchronize()
        for _ in range(a.reps):
            for dt, t in vols.items():
                create(None, device_ptr=t.data_ptr(), shape=(n, n, n), dtype=None if dt == "float32" else dt)
        res[f"bytes at {n}^3"] = {
            "k_absmax + k_scale (fp32)": {"k_absmax": 4 * V, "k_scale": 8 * V},
            "k_absmax_t + k_ingest (16-bit)": {"k_absmax_t": 2 * V, "k_ingest": 6 * V},
            "k_absmax_t + k_ingest (8-bit)": {"k_absmax_t": 1 * V, "k_ingest": 5 * V},
            "seconds at the copy ceiling per byte": 1 / COPY_CEILING}

    if a.only in ("", "dvc") and typed:
        n = 256
        ref, tar = volume(n, "uint16"), np.roll(volume(n, "uint16"), 1, axis=2)
        fr, ft = ref.astype(np.float32), tar.astype(np.float32)
        pts = np.array([[n // 2, n // 2, n // 2]], np.int32)
        r = {"icgn, host fp32 volumes (stage_pair upload inside), m = 1": timed(lambda: capi.icgn(fr, ft, pts, subset_radius=8), a.reps)}
        dev = {}

        def up(src_r, src_t):
            dev["r"], dev["t"] = capi.to_device(src_r), capi.to_device(src_t)

        r["to_device x 2, uint16"] = timed(lambda: up(ref, tar), a.reps)
        r["icgn on the device tensors, m = 1"] = timed(lambda: capi.icgn(dev["r"], dev["t"], pts, subset_radius=8), a.reps)
        r["to_device x 2, fp32"] = timed(lambda: up(fr, ft), a.reps)
        ref8 = volume(n, "uint8")
        tar8 = ref8.copy()
        r["to_device x 2, uint8"] = timed(lambda: up(ref8, tar8), a.reps)
        secs = [capi.to_device(ref, with_seconds=True)[1] * 1e3 for _ in range(a.reps)]
        r["k_ingest<uint16, unscaled> device time (events)"] = stats(secs)
        res[f"dvc upload {n}^3"] = r
        print(json.dumps({f"dvc upload {n}^3": r}), flush=True)
        # the same at the first size, where a workflow's volumes are largest
        n = sizes[0]
        if n != 256:
            big = volume(n, "uint16")
            bigf = big.astype(np.float32)
            r = {"to_device uint16": timed(lambda: capi.to_device(big), a.reps), "to_device fp32": timed(lambda: capi.to_device(bigf), a.reps)}
            secs = [capi.to_device(big, with_seconds=True)[1] * 1e3 for _ in range(a.reps)]
            r["k_ingest<uint16, unscaled> device time (events)"] = stats(secs)
            r["k_ingest bytes"] = 6 * n ** 3
            res[f"to_device {n}^3"] = r
            print(json.dumps({f"to_device {n}^3": r}), flush=True)

    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
