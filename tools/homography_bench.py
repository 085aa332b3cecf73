#!/usr/bin/env python
"""Time the RANSAC homography (compvhip_homography_points / _find) with HIP events: medians of 10 calls after 3 warm-ups for 32 pairs of 500 and of 2000
points at 2000 tries (30 % outliers, a planted H) --
  * the solve, score and refit kernels apart (the handle's timing mode), and the points gather from a good list of that length;
  * the whole find call (one event pair around it, timing mode off);
  * the distribution of the Jacobi rotation counts of the tries (compvhip_homography_scores);
  * with --reference, where the reference checkout and oracle/_ref are present (the build container): CompVHomography<double>::find on ONE core for
    the same pairs, through the shim of tests/golden/make_golden_homography.py.  The reference STOPS EARLY (its adaptive try count, :318-331 -- a
    handful of tries on data this clean) and draws its own random quads, so the two columns are not the same amount of work: the device runs all
    2000 tries.  --no-gpu skips everything but that column.
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

PAIRS, TRIES = 32, 2000
H_TRUE = np.array([[0.8912, -0.1253, 31.5], [0.1253, 0.8912, -12.25], [0.00011, -0.00007, 1.0]])


def make_pairs(n, seed):
    rng = np.random.default_rng(seed)
    src = np.stack([rng.uniform(20, 620, (PAIRS, n)), rng.uniform(20, 460, (PAIRS, n))], axis=2)
    z = H_TRUE[2, 0] * src[..., 0] + H_TRUE[2, 1] * src[..., 1] + H_TRUE[2, 2]
    dst = np.stack([(H_TRUE[0, 0] * src[..., 0] + H_TRUE[0, 1] * src[..., 1] + H_TRUE[0, 2]) / z, (H_TRUE[1, 0] * src[..., 0] + H_TRUE[1, 1] * src[..., 1] + H_TRUE[1, 2]) / z], axis=2)
    dst += rng.uniform(-0.5, 0.5, dst.shape)
    out = rng.uniform(0, 1, (PAIRS, n)) < 0.3
    dst[out] = np.stack([rng.uniform(0, 640, int(out.sum())), rng.uniform(0, 480, int(out.sum()))], axis=1)
    return src, dst, ~out


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


def gpu_part(res):
    import torch
    from compv_amd import capi
    import homography_model as hm
    dev = torch.device("cuda", 0)
    ctx = capi.Context(0)
    res["device"] = torch.cuda.get_device_properties(0).name
    for n in (500, 2000):
        src, dst, inl = make_pairs(n, n)
        d_src, d_dst = torch.from_numpy(src).to(dev), torch.from_numpy(dst).to(dev)
        d_res = torch.zeros(PAIRS * capi.HOMOGRAPHY_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        d_mask = torch.zeros(PAIRS * n, dtype=torch.uint8, device=dev)
        h = capi.Homography(ctx, PAIRS, n, TRIES)

        def find():
            h.find(d_src.data_ptr(), d_dst.data_ptr(), 0, d_res.data_ptr(), d_mask.data_ptr(), tries=TRIES, seed=1)
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
        out = np.frombuffer(d_res.cpu().numpy().tobytes(), capi.HOMOGRAPHY_RESULT_DTYPE)
        mask = d_mask.cpu().numpy().reshape(PAIRS, n)
        row["pairs_with_exactly_the_planted_inliers"] = int(sum((mask[p] != 0).tolist() == inl[p].tolist() for p in range(PAIRS)))
        row["status_0"] = int((out["status"] == 0).sum())
        _, _, rot = h.scores(TRIES)
        rot = rot[rot > 0]
        row["rotations"] = {"min": int(rot.min()), "p5": int(np.percentile(rot, 5)), "median": int(np.median(rot)), "p95": int(np.percentile(rot, 95)), "max": int(rot.max()),
                            "mean": round(float(rot.mean()), 1), "refit_median": int(np.median(out["rotations"]))}
        # the gather: a good list that names every keypoint once
        good = np.zeros((PAIRS, n), hm.MATCH_DTYPE)
        good["queryIdx"] = good["trainIdx"] = np.arange(n)
        keys_q, keys_t = np.zeros((PAIRS, n), hm.KEYPOINT_DTYPE), np.zeros((PAIRS, n), hm.KEYPOINT_DTYPE)
        keys_q["x"], keys_q["y"], keys_t["x"], keys_t["y"] = dst[..., 0], dst[..., 1], src[..., 0], src[..., 1]
        d_good = torch.from_numpy(good.view(np.uint8).reshape(-1)).to(dev)
        d_kq, d_kt = torch.from_numpy(keys_q.view(np.uint8).reshape(-1)).to(dev), torch.from_numpy(keys_t.view(np.uint8).reshape(-1)).to(dev)
        row.update(median_ms(h, lambda: h.points(d_good.data_ptr(), n, 0, d_kq.data_ptr(), n, d_kt.data_ptr(), n), torch.cuda.synchronize))
        h.close()
        res["points_%d" % n] = row
    ctx.close()


def reference_part(res):
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_golden_homography as g
    from oracle_bindings import RefShim
    RefShim(threads=1)
    with tempfile.TemporaryDirectory() as tmp:
        L = g.build_shim(tmp)
        for n in (500, 2000):
            src, dst, inl = make_pairs(n, n)
            g.ref_find(L, src[0], dst[0], ransac=True)
            t0 = time.perf_counter()
            ok = 0
            for p in range(PAIRS):
                _, count = g.ref_find(L, src[p], dst[p], ransac=True)
                ok += int(count == int(inl[p].sum()))
            res.setdefault("points_%d" % n, {})["reference_find_ms_32_pairs_one_core"] = round((time.perf_counter() - t0) * 1e3, 2)
            res["points_%d" % n]["reference_pairs_with_the_planted_count"] = ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", action="store_true")
    ap.add_argument("--no-gpu", action="store_true")
    a = ap.parse_args()
    res = {"pairs": PAIRS, "tries": TRIES}
    if not a.no_gpu:
        gpu_part(res)
    if a.reference:
        reference_part(res)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
