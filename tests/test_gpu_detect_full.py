"""GPU tests of the opt-in detection rules (sift3d_set_detect_options): the 80-neighbour extremum test and the sub-voxel refinement.
Every mode's extrema equal a CPU restatement (tests/detect_full_ref.py) on the read-back DoG levels; every mode's keypoints are the
default run's keypoints at the surviving voxels, records and descriptors bit for bit; the default path is untouched."""
import importlib

import numpy as np
import pytest

import detect_full_ref as ref
from hipcheck import bits

pytestmark = pytest.mark.gpu

capi = importlib.import_module("3dsift_amd.capi")


def dog_levels(g, nd):
    return [[g.dog(o, i) for i in range(nd)] for o in range(g.num_octaves)]


def table(e):
    return np.stack([e["octave"], e["level"], e["x"].astype(np.int64), e["y"].astype(np.int64), e["z"].astype(np.int64)], 1).astype(np.int64)


def keyed(kp):
    return {tuple(int(v) for v in r): i for i, r in enumerate(table(kp))}


CASES = [
    ((64, 64, 64), dict(), 0.0),
    ((128, 128, 128), dict(), 0.01),
    ((45, 77, 100), dict(), 0.01),   # (nz, ny, nx) = a 100 x 77 x 45 volume
    ((72, 64, 80), dict(num_kp_levels=2, sigma_default=2.3), 0.01),  # half widths 9 / 11: the separable path
]


@pytest.mark.parametrize("shape,params,noise", CASES)
def test_full_rule_is_exact(synth, shape, params, noise):
    vol = synth.blobs(shape, seed=41, noise=noise)
    g = capi.CSIFT3D(vol, **params).set_detect_options(neighbours=80)
    g.run_stages(3)
    nd = g.levels + 2
    dogs = dog_levels(g, nd)
    pt = params.get("peak_thresh", 0.1)
    got = table(g.extrema())
    want = ref.extrema_table(dogs, pt, 80)
    assert len(want) > 0
    assert np.array_equal(got, want), (len(got), len(want))
    # the 80-neighbour extrema are a subsequence of the reference rule's
    d = capi.CSIFT3D(vol, **params).run_stages(3)
    k8 = keyed(d.extrema())
    idx = [k8[tuple(int(v) for v in r)] for r in got]
    assert idx == sorted(idx)


def test_full_rule_on_oracle_dog(synth, orc):
    vol = synth.blobs((64, 72, 56), seed=21, noise=0.01)
    g = capi.CSIFT3D(vol).set_detect_options(neighbours=80).run_stages(3)
    o = orc.extractor(vol).run(2)
    dogs = [[o.dog(oc, i) for i in range(5)] for oc in range(o.num_octaves)]
    assert np.array_equal(table(g.extrema()), ref.extrema_table(dogs, 0.1, 80))


@pytest.mark.parametrize("neighbours,refine", [(80, False), (8, True), (80, True)])
def test_subsequence_bit_for_bit(synth, neighbours, refine):
    vol = synth.blobs((96, 80, 72), seed=5, noise=0.02)
    d = capi.CSIFT3D(vol).KpSiftAlgorithm()
    dkp, ddesc = d.GetKeypoints()
    dext, dcodes = d.extrema(), d.orientation_codes()
    g = capi.CSIFT3D(vol).set_detect_options(neighbours=neighbours, refine=refine).KpSiftAlgorithm()
    kp, desc = g.GetKeypoints()
    ext, codes = g.extrema(), g.orientation_codes()
    assert 0 < len(kp) <= len(dkp) and len(ext) < len(dext)
    # extrema and their orientation codes: a subsequence of the default run's
    ke = keyed(dext)
    ie = [ke[tuple(int(v) for v in r)] for r in table(ext)]
    assert ie == sorted(ie)
    assert np.array_equal(codes, dcodes[ie])
    # keypoint records and descriptors at the surviving voxels: bit for bit
    kk = keyed(dkp)
    ik = [kk[tuple(int(v) for v in r)] for r in table(kp)]
    assert ik == sorted(ik)
    assert np.array_equal(kp.view(np.uint8).reshape(len(kp), -1), dkp[ik].view(np.uint8).reshape(len(kp), -1))
    assert np.array_equal(bits(desc), bits(ddesc[ik]))
    if refine:
        assert len(g.refined()) == len(kp)


OPTS = [
    dict(max_offset=0.5),
    dict(max_offset=0.0, contrast_thresh=0.03),
    dict(max_offset=0.0, edge_ratio=10.0),
    dict(max_offset=0.5, contrast_thresh=0.03, edge_ratio=10.0),
]


@pytest.mark.parametrize("opts", OPTS)
@pytest.mark.parametrize("neighbours", [8, 80])
def test_refinement_is_exact(synth, opts, neighbours):
    vol = synth.blobs((80, 72, 64), seed=9, noise=0.01)
    g = capi.CSIFT3D(vol).set_detect_options(neighbours=neighbours, refine=True, **opts).KpSiftAlgorithm()
    dogs = dog_levels(g, 5)
    rows = ref.extrema_table(dogs, 0.1, neighbours)
    want = ref.refined_table(dogs, rows, 0.1, neighbours, opts)
    got = table(g.extrema())
    assert len(want) > 0 and len(want) <= len(rows)
    assert np.array_equal(got, want), (len(got), len(want))
    kp, _ = g.GetKeypoints(with_desc=False)
    r = g.refined()
    assert len(r) == len(kp) > 0
    gotv = np.stack([r["rx"], r["ry"], r["rz"], r["scale"], r["offset"][:, 0], r["offset"][:, 1], r["offset"][:, 2], r["offset"][:, 3],
                     r["contrast"]], 1).astype(np.float32)
    wantv = np.stack([ref.refined_record(dogs, k, 3) for k in kp])
    # everything bit for bit; the scale goes through exp2 (device libm vs host libm): at most one fp32 ulp apart
    cols = [0, 1, 2, 4, 5, 6, 7, 8]
    assert np.array_equal(bits(gotv[:, cols]), bits(wantv[:, cols])), int((bits(gotv[:, cols]) != bits(wantv[:, cols])).sum())
    ulp = np.abs(bits(gotv[:, 3]).astype(np.int64) - bits(wantv[:, 3]).astype(np.int64))
    assert ulp.max() <= 1, int(ulp.max())
    if opts.get("max_offset", 0.5) > 0:
        assert np.abs(r["offset"]).max() <= np.float32(opts["max_offset"])


def test_subvoxel_accuracy(synth):
    shape = (256, 256, 256)
    out = []
    for shift in ((0.0, 0.0, 0.0), (0.3, 0.0, 0.0)):
        g = capi.CSIFT3D(synth.blobs(shape, seed=1234, shift=shift)).set_detect_options(neighbours=80, refine=True).KpSiftAlgorithm()
        kp, _ = g.GetKeypoints(with_desc=False)
        out.append((kp, g.refined()))
    (ka, ra), (kb, rb) = out
    sel_a = np.nonzero(ka["octave"] == 0)[0]
    sel_b = np.nonzero(kb["octave"] == 0)[0]
    pos_b = np.stack([kb["x"][sel_b], kb["y"][sel_b], kb["z"][sel_b]], 1)
    dref, dint = [], []
    used = set()
    for i in sel_a:
        p = np.array([ka["x"][i], ka["y"][i], ka["z"][i]])
        cheb = np.abs(pos_b - p).max(axis=1)
        cand = [j for j in np.nonzero((cheb <= 1) & (kb["level"][sel_b] == ka["level"][i]))[0] if sel_b[j] not in used]
        if not cand:
            continue
        j = sel_b[min(cand, key=lambda c: np.abs(pos_b[c] - p).sum())]
        used.add(j)
        dref.append(float(rb["rx"][j]) - float(ra["rx"][i]))
        dint.append(float(kb["rx"][j]) - float(ka["rx"][i]))
    assert len(dref) >= 20, len(dref)
    med, med_int = float(np.median(dref)), float(np.median(dint))
    print(f"sub-voxel: {len(dref)} pairs, median refined dx {med:.4f} (integer {med_int:.4f}), "
          f"refined quartiles {np.percentile(dref, 25):.4f} / {np.percentile(dref, 75):.4f}")
    assert abs(med - 0.3) <= 0.1, (med, med_int, len(dref))


def test_options_leave_no_trace(synth):
    vol = synth.blobs((64, 64, 64), seed=17, noise=0.01)
    fresh = capi.CSIFT3D(vol).KpSiftAlgorithm()
    fkp, fdesc = fresh.GetKeypoints()
    g = capi.CSIFT3D(vol).set_detect_options(neighbours=80, refine=True).KpSiftAlgorithm()
    assert len(g.GetKeypoints()[0]) < len(fkp)
    g.set_detect_options()
    assert g.detect_options() == capi.default_detect_options()
    g.KpSiftAlgorithm()
    kp, desc = g.GetKeypoints()
    assert np.array_equal(kp.view(np.uint8), fkp.view(np.uint8)) and np.array_equal(bits(desc), bits(fdesc))
    with pytest.raises(capi.Sift3dError, match="did not refine"):
        g.refined()


def test_interleaved_handles(synth):
    va = synth.blobs((64, 64, 64), seed=23, noise=0.01)
    vb = synth.blobs((64, 64, 64), seed=24, noise=0.01)
    d = capi.CSIFT3D(va)
    f = capi.CSIFT3D(vb).set_detect_options(neighbours=80, refine=True, edge_ratio=10.0)
    d.KpSiftAlgorithm()
    base = d.GetKeypoints()
    f.KpSiftAlgorithm()
    fbase = f.GetKeypoints()
    for _ in range(2):
        f.KpSiftAlgorithmAsync()
        d.KpSiftAlgorithmAsync(after=f)
        f.Wait(); d.Wait()
        for (a, b), (x, y) in ((d.GetKeypoints(), base), (f.GetKeypoints(), fbase)):
            assert np.array_equal(a.view(np.uint8), x.view(np.uint8)) and np.array_equal(bits(b), bits(y))
        d.KpSiftAlgorithm()
        f.KpSiftAlgorithm()
        assert np.array_equal(d.GetKeypoints()[0].view(np.uint8), base[0].view(np.uint8))


def test_match_handles_full_mode(synth):
    va = synth.blobs((64, 64, 64), seed=1234)
    vb = synth.blobs((64, 64, 64), seed=1234, shift=(1.0, 0.0, 0.0))
    ga = capi.CSIFT3D(va).set_detect_options(neighbours=80, refine=True).KpSiftAlgorithm()
    gb = capi.CSIFT3D(vb).set_detect_options(neighbours=80, refine=True).KpSiftAlgorithm()
    m = capi.muBruteMatcher()
    dev = {k: v.copy() for k, v in m.matchExtractors(ga, gb).items()}
    ka, da = ga.GetKeypoints()
    kb, db = gb.GetKeypoints()
    xa = np.stack([ka["rx"], ka["ry"], ka["rz"]], 1)
    xb = np.stack([kb["rx"], kb["ry"], kb["rz"]], 1)
    host = m.enhancedMatch(da, xa, db, xb, 0.85)
    assert len(dev["pairs"]) > 0
    for k in host:
        assert np.array_equal(dev[k], host[k]), k


def test_refusals(synth):
    vol = synth.blobs((64, 64, 64), seed=3, noise=0.01)
    g = capi.CSIFT3D(vol)
    for bad in (dict(neighbours=26), dict(neighbours=0), dict(max_offset=float("nan")), dict(contrast_thresh=float("inf")),
                dict(edge_ratio=float("-inf"))):
        with pytest.raises(capi.Sift3dError, match="bad argument"):
            g.set_detect_options(**bad)
    o = capi.DetectOptions(8, 0, 0.5, 0.0, 0.0)
    o.reserved[1] = 7
    import ctypes as C
    assert capi.lib().sift3d_set_detect_options(g._h, C.byref(o)) == 1
    assert g.detect_options() == capi.default_detect_options()  # nothing was taken
    g.KpSiftAlgorithm()
    with pytest.raises(capi.Sift3dError, match="call out of order"):
        g.refined()
    g.KpSiftAlgorithmAsync()
    with pytest.raises(capi.Sift3dError, match="call out of order"):
        g.set_detect_options(neighbours=80)
    g.Wait()
    g.set_detect_options(neighbours=80)
    import torch
    arena = torch.zeros(capi.SlabCSIFT3D.arena_floats(64, 64, 64, 0, 32, 40, 4), dtype=torch.float32, device="cuda:0")
    s = capi.SlabCSIFT3D(64, 64, 64, 0, 32, 40, 4, arena.data_ptr(), arena.numel())
    with pytest.raises(capi.Sift3dError, match="bad argument"):
        s.set_detect_options(neighbours=80)
    t = capi.SeededCSIFT3D((32, 32, 32), 1, 4)
    with pytest.raises(capi.Sift3dError, match="bad argument"):
        t.set_detect_options(refine=True)
    s.close(); t.close()
