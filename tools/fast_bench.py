#!/usr/bin/env python
"""Time compvhip_plan_fast on 32 resident 4K frames with HIP events via the plan's timing mode: medians of 10 calls after warm-up, the score
kernel and the list kernels (cut level, row recount, scan, emit) apart, for
  N 9 and 12, NMS on and off, with the caller's score map and with the plan's own, with and without a maxFeatures cut,
  on text-like frames (few candidates: most pixels leave at the opposite-pair test) and on noise (every pixel a candidate),
each beside 1 B/px read at the measured copy rate DESIGN.md uses (5.4 TB/s), and beside the thing the call replaces, measured in the same run on
the same host when oracle/_ref holds the compiled reference: the download of the frames, then CompVCornerDeteFAST on one core
(oracle/_ref/headless_samples --fast-only 3840 2160: the median of five calls on one synthetic 4K frame after a first one; it also checks the point lists
against each other).
"""
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

COPY_TBS = 5.4


def timed(plan, call, reps=10, warm=3):
    for _ in range(warm):
        call()
    torch.cuda.synchronize()
    plan.set_timing(1)
    ms = {}
    for _ in range(reps):
        call()
        torch.cuda.synchronize()
        for n, m in plan.get_timing():
            ms.setdefault(n, []).append(m)
    plan.set_timing(0)
    return {n: round(float(np.median(v)), 4) for n, v in ms.items()}


def main():
    W, H, F = 3840, 2160, 32
    dev = torch.device("cuda", 0)
    ctx = capi.Context(0)
    plan = capi.Plan(ctx, W, H, W, F)
    floor_ms = 1.0 * F * W * H / (COPY_TBS * 1e12) * 1e3
    res = {"frames": F, "W": W, "H": H, "floor_ms (1 B/px at %.1f TB/s)" % COPY_TBS: round(floor_ms, 4)}
    cap = 1 << 20
    d_scores = torch.empty(F * H * W, dtype=torch.uint8, device=dev)
    d_rec = torch.empty(F * cap * capi.CORNER_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    d_counts = torch.zeros(F, dtype=torch.int32, device=dev)
    content = {
        "text": np.stack([text_frame(W, H, 12345 + f % 4) for f in range(4)] * (F // 4)),
        "noise": np.stack([np.random.default_rng(f).integers(0, 256, (H, W), dtype=np.uint8) for f in range(4)] * (F // 4)),
    }
    d_in = None
    for kind, frames in content.items():
        d_in = torch.from_numpy(frames).to(dev)
        for N in (9, 12):
            for nonmax in (True, False):
                for own_map in (False, True):
                    for K in ((-1, 2000) if (N == 9 and nonmax and not own_map) else (-1,)):
                        ms = timed(plan, lambda: plan.fast(d_in.data_ptr(), 20, N, nonmax, K, 0 if own_map else d_scores.data_ptr(), d_rec.data_ptr(), cap, d_counts.data_ptr()))
                        tot = sum(ms.values())
                        name = "%s N%d %s %s%s" % (kind, N, "nms" if nonmax else "all", "plan's map" if own_map else "caller's map", " maxFeatures %d" % K if K > 1 else "")
                        res[name] = {"ms": ms, "ms_total": round(tot, 4), "score_x_floor": round(ms["fast_score_kernel"] / floor_ms, 2), "x_floor": round(tot / floor_ms, 2),
                                     "corners_per_frame min/max": [int(d_counts.min()), int(d_counts.max())]}
    # the yardstick: download + the compiled reference on one core
    host = torch.empty(d_in.shape, dtype=torch.uint8).pin_memory()
    dl = []
    for i in range(2 + 5):          # two warm-up copies, then the median of five
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host.copy_(d_in)
        torch.cuda.synchronize()
        if i >= 2:
            dl.append((time.perf_counter() - t0) * 1e3)
    res["download_ms (32 frames, pinned, median of 5)"] = round(float(np.median(dl)), 2)
    exe = os.path.join(ROOT, "oracle", "_ref", "headless_samples")
    if os.path.exists(exe):
        out = subprocess.run([exe, "--fast-only", str(W), str(H)], capture_output=True, text=True, timeout=300).stdout
        m = re.search(r"fast_corners: (\w+) \[.*?(\d+) points.*CompV CPU ([\d.]+) ms, HIP plugin ([\d.]+) ms", out)
        res["reference one core, one 4K frame, median of 5 calls (N 9, nms, t 20)"] = ({"points": int(m.group(2)), "lists": m.group(1), "compv_cpu_ms": float(m.group(3)), "hip_host_form_ms": float(m.group(4))}
                                                                    if m else {"error": out[-300:]})
    else:
        res["reference one core, one 4K frame, median of 5 calls (N 9, nms, t 20)"] = "oracle/_ref not built: not measured"
    print(json.dumps(res))
    plan.close(); ctx.close()


if __name__ == "__main__":
    main()
