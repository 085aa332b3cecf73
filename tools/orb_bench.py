#!/usr/bin/env python
"""Time ORB on the GPU (compvhip_plan_orb_keypoints / _describe) with HIP events via the plan's timing mode: medians of 10 calls after 3 warm-ups of
  32 frames of 3840 x 2160 with about 2000 keypoints each (FAST-9, threshold 20, NMS, maxFeatures 2000 on the text-like page of tools/fast_bench.py's kind),
the select, orient, blur and brief kernels apart, and the brief kernel in BOTH byte-read variants: the 37 x 37 patch staged in the LDS, and bytes read
from global memory.  A variant is chosen per plan (the environment variable COMPVHIP_ORB_BRIEF = lds | global, read when a plan first describes), so the
tool makes one plan for each and checks that the two write the same rows.

Beside them the path the GPU replaces, measured in the same run: the download of one frame's corner list (pinned), and -- when oracle/_ref holds the
compiled reference -- the reference's moments + orientation and blur + describe of about 2000 points of one 4K level on one core
(oracle/_ref/headless_samples --orb-only: medians of five calls).  Prints one JSON line."""
import json
import os
import re
import subprocess
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
from compv_amd import capi
from hysteresis_cases import text_frame

W, H, S, F = 3840, 2160, 3840, 32
CAP = 4096


def timed(plan, call, reps=10, warm=3):
    for _ in range(warm):
        call()
    torch.cuda.synchronize()
    plan.set_timing(1)
    ms = {}
    for _ in range(reps):
        call()
        torch.cuda.synchronize()
        for n, v in plan.get_timing():
            ms.setdefault(n, []).append(v)
    plan.set_timing(0)
    return {n: round(float(np.median(v)), 4) for n, v in ms.items()}


def main():
    dev = torch.device("cuda", 0)
    ctx = capi.Context(0)
    res = {"device": torch.cuda.get_device_properties(0).name, "frames": F, "size": [W, H]}
    frames = np.stack([text_frame(W, H, 100 + f) for f in range(4)])
    d_in = torch.from_numpy(np.ascontiguousarray(frames[np.arange(F) % 4])).to(dev)
    d_corners = torch.zeros(F * CAP * 12, dtype=torch.uint8, device=dev)
    d_cc = torch.zeros(F, dtype=torch.int32, device=dev)
    d_keys = torch.zeros(F * CAP * 24, dtype=torch.uint8, device=dev)
    d_kc = torch.zeros(F, dtype=torch.int32, device=dev)
    rows = {}
    for variant in ("lds", "global"):
        os.environ["COMPVHIP_ORB_BRIEF"] = variant
        plan = capi.Plan(ctx, W, H, S, F)
        d_desc = torch.zeros(F * CAP * 32, dtype=torch.uint8, device=dev)
        plan.fast(d_in.data_ptr(), 20, 9, True, 2000, 0, d_corners.data_ptr(), CAP, d_cc.data_ptr())
        torch.cuda.synchronize()
        if variant == "lds":
            res["corners per frame min/max"] = [int(d_cc.min()), int(d_cc.max())]
            res["keypoints_ms"] = timed(plan, lambda: plan.orb_keypoints(d_in.data_ptr(), d_corners.data_ptr(), CAP, d_cc.data_ptr(), 0, 1.0, d_keys.data_ptr(), CAP,
                                                                           d_kc.data_ptr()))
            res["keypoints per frame min/max"] = [int(d_kc.min()), int(d_kc.max())]
        else:
            plan.orb_keypoints(d_in.data_ptr(), d_corners.data_ptr(), CAP, d_cc.data_ptr(), 0, 1.0, d_keys.data_ptr(), CAP, d_kc.data_ptr())
        res["describe_ms brief=%s" % variant] = timed(plan, lambda: plan.orb_describe(d_in.data_ptr(), d_keys.data_ptr(), CAP, d_kc.data_ptr(), 1.0, d_desc.data_ptr(), 32, True))
        n = d_kc.clamp(max=CAP).cpu().numpy()
        d = d_desc.cpu().numpy().reshape(F, CAP, 32)
        rows[variant] = [d[f, :n[f]].copy() for f in range(F)]
        plan.close()
    os.environ.pop("COMPVHIP_ORB_BRIEF")
    res["variants agree"] = all((a == b).all() for a, b in zip(rows["lds"], rows["global"]))
    # the path the GPU replaces: download of one frame's corners, then the reference on one core
    host = torch.empty(2000 * 12, dtype=torch.uint8).pin_memory()
    dl = []
    for i in range(2 + 5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host.copy_(d_corners[:2000 * 12])
        torch.cuda.synchronize()
        if i >= 2:
            dl.append((time.perf_counter() - t0) * 1e3)
    res["download_ms (2000 corners of one frame, pinned, median of 5)"] = round(float(np.median(dl)), 3)
    exe = os.path.join(ROOT, "oracle", "_ref", "headless_samples")
    key = "reference one core, one 4K level, about 2000 points, medians of 5 calls"
    if not os.path.exists(exe):
        res[key] = "oracle/_ref not built: not measured"
    else:
        out = subprocess.run([exe, "--orb-only", str(W), str(H), "2000"], capture_output=True, text=True, timeout=300).stdout
        mt = re.search(r"orb_reference: \[\d+x\d+, (\d+) points \| moments \+ orientation ([\d.]+) ms, blur \+ describe ([\d.]+) ms", out)
        res[key] = {"points": int(mt.group(1)), "orient_ms": float(mt.group(2)), "blur_describe_ms": float(mt.group(3))} if mt else {"error": out[-300:]}
    print(json.dumps(res))
    ctx.close()


if __name__ == "__main__":
    main()
