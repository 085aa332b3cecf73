#!/usr/bin/env python
"""Time the RANSAC line and parabola fits (compvhip_curvefit_*) with HIP events: medians of 10 calls after 3 warm-ups at 2000 tries, 30 % outliers,
noise-free planted curves (tests/curvefit_cases.py), for 2048 sets of 512 points (32 frames x 64 components) and 2048 sets of 128 points --
  * the score and refit kernels apart (the handle's timing mode) and the whole find call (one event pair around it, timing mode off);
  * the share of sets whose mask is exactly the planted inliers;
  * the gather from label maps: 32 frames of 1024 x 1024 with 64 components of about 400 pixels each, a diagonal band in a box of 32 x 32, 64 x 64 or
    128 x 128 pixels -- the kernel walks the box, so its time follows the box AREA, not the pixel count;
  * with --reference, where the reference checkout and oracle/_ref are present (the build container): CompVMathStatsFit::line / ::parabola on ONE core
    for the first 64 sets of each workload, through the shim of tests/golden/make_golden_curvefit.py.  The reference STOPS EARLY (its adaptive try
    count, compv_math_stats_ransac.cxx:240-254 -- on data this clean it stops at the first all-inlier sample) and draws its own random samples, so the
    two columns are not the same amount of work: the device runs all 2000 tries.  --no-gpu skips everything but that column.
Prints one JSON line."""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

import curvefit_cases as cc
import curvefit_model as cm

SETS, TRIES, FRAMES, COMP_CAP = 2048, 2000, 32, 64
WORKLOADS = (("sets_2048_points_512", 512), ("sets_2048_points_128", 128))
MODELS = (("line", cm.LINE), ("parabola", cm.PARABOLA))


def make_sets(model, k, sets=SETS):
    made = [cc.planted(model, k, 0.3, 7000 + s) for s in range(sets)]
    return np.stack([p for p, _, _ in made]), np.stack([i for _, i, _ in made])


def median_ms(h, call, sync, reps=10, warm=3):
    for _ in range(warm):
        call()
    sync()
    h.set_timing(1)
    ms = {}
    for _ in range(reps):
        call()
        sync()
        for name, v in h.get_timing():
            ms.setdefault(name, []).append(v)
    h.set_timing(0)
    return {name: round(float(np.median(v)), 4) for name, v in ms.items()}


def band_labels(side, W=1024, H=1024):
    """64 components of about 400 pixels per frame, one per 128 x 128 cell: the band |y - x| < 256 / side of a side x side box"""
    lab = np.zeros((H, W), np.int32)
    comps = np.zeros(COMP_CAP, cm.COMP_DTYPE)
    yy, xx = np.mgrid[0:side, 0:side]
    band = np.abs(yy - xx) * side < 256
    for c in range(COMP_CAP):
        y0, x0 = (c // 8) * 128, (c % 8) * 128
        lab[y0:y0 + side, x0:x0 + side][band] = c + 1
        ys, xs = np.nonzero(band)
        comps[c] = (x0 + xs[0], y0 + ys[0], x0 + xs.min(), y0 + ys.min(), x0 + xs.max(), y0 + ys.max(), len(ys))
    return lab, comps


def gpu_part(res):
    import torch
    from compv_amd import capi
    dev = torch.device("cuda", 0)
    ctx = capi.Context(0)
    res["device"] = torch.cuda.get_device_properties(0).name
    for name, k in WORKLOADS:
        h = capi.Curvefit(ctx, SETS, k, TRIES)
        d_res = torch.zeros(SETS * capi.CURVEFIT_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        d_mask = torch.zeros(SETS * k, dtype=torch.uint8, device=dev)
        for mname, model in MODELS:
            pts, inl = make_sets(model, k)
            d_pts = torch.from_numpy(pts).to(dev)

            def find():
                h.find(d_pts.data_ptr(), 0, d_res.data_ptr(), d_mask.data_ptr(), model=model, tries=TRIES, threshold=cc.THRESHOLD, seed=1)
            row = median_ms(h, find, torch.cuda.synchronize)
            whole = []
            for _ in range(10):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                find()
                b.record()
                torch.cuda.synchronize()
                whole.append(a.elapsed_time(b))
            row["find_call_ms"] = round(float(np.median(whole)), 4)
            out = np.frombuffer(d_res.cpu().numpy().tobytes(), capi.CURVEFIT_RESULT_DTYPE)
            mask = d_mask.cpu().numpy().reshape(SETS, k)
            row["sets_with_exactly_the_planted_inliers"] = int(((mask != 0) == inl).all(axis=1).sum())
            row["status_0"] = int((out["status"] == 0).sum())
            res.setdefault(name, {})[mname] = row
        h.close()
    h = capi.Curvefit(ctx, FRAMES * COMP_CAP, 512, 1)
    gather = {}
    for side in (32, 64, 128):
        lab, comps = band_labels(side)
        d_lab = torch.from_numpy(np.broadcast_to(lab, (FRAMES,) + lab.shape).copy()).to(dev)
        d_comps = torch.from_numpy(np.broadcast_to(comps, (FRAMES, COMP_CAP)).copy().view(np.uint8).reshape(-1)).to(dev)
        d_n = torch.full((FRAMES,), COMP_CAP, dtype=torch.int32, device=dev)
        row = median_ms(h, lambda: h.points_from_labels(d_lab.data_ptr(), 1024, 1024, 1024, d_comps.data_ptr(), COMP_CAP, d_n.data_ptr(), FRAMES), torch.cuda.synchronize)
        _, got = h.scores(1)
        row["pixels_per_component"], row["points_per_set"] = int(comps["pixels"][0]), int(got[0])
        gather["box_%dx%d" % (side, side)] = row
    res["gather_32_frames_64_components"] = gather
    h.close()
    ctx.close()


def reference_part(res, sets=64):
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_golden_curvefit as g
    from oracle_bindings import RefShim
    RefShim(threads=1)
    with tempfile.TemporaryDirectory() as tmp:
        L = g.build_shim(tmp)
        for name, k in WORKLOADS:
            for mname, model in MODELS:
                pts, inl = make_sets(model, k, sets)
                g.ref_fit(L, pts[0], model, cc.THRESHOLD)
                t0 = time.perf_counter()
                curves = [g.ref_fit(L, pts[s], model, cc.THRESHOLD) for s in range(sets)]
                ms = (time.perf_counter() - t0) * 1e3
                ok = sum(int(((g.ref_distances(L, pts[s], model, curves[s]) < cc.THRESHOLD) == inl[s]).all()) for s in range(sets))
                row = res.setdefault(name, {}).setdefault(mname, {})
                row["reference_ms_%d_sets_one_core" % sets] = round(ms, 2)
                row["reference_sets_with_exactly_the_planted_inliers"] = ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", action="store_true")
    ap.add_argument("--no-gpu", action="store_true")
    a = ap.parse_args()
    res = {"sets": SETS, "tries": TRIES}
    if not a.no_gpu:
        gpu_part(res)
    if a.reference:
        reference_part(res)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
