#!/usr/bin/env python
"""Time compvhip_plan_components on 32 resident 4K benchmark frames (seeds 12345 ..), after one pipeline step at the benchmark's thresholds,
with HIP events via the plan's timing mode: medians of 10 calls after warm-up, per kernel and in total, reading the plan's 1-bit masks and
reading the byte edge maps, with and without the label map, minPixels 1 and 10, at 8-connectivity (and once at 4); and once on a single
all-foreground 4K frame, where every pixel lands on one record.

Beside it the thing the call replaces, measured in the same run on the same host: download of the 32 edge maps, then scipy.ndimage.label
and the statistics (tests/components_model.py) on one core.

Also printed, per frame: component count and the largest component's share of the edge pixels, as the device returns them (DESIGN.md 7
argues with a CPU-side 87 %).
"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import numpy as np, torch
from compv_amd import capi
from components_model import components
from oracle_bindings import synth_frame


def main():
    W, H, F, theta, thr = 3840, 2160, 32, 1.0, 100
    line_cap, comp_cap = 1 << 16, 1 << 16
    dev = torch.device("cuda", 0)
    ctx = capi.Context(0)
    plan = capi.Plan(ctx, W, H, W, F, theta)
    d_in = torch.stack([torch.from_numpy(synth_frame(W, H, 12345 + f)) for f in range(F)]).to(dev)
    d_e = torch.empty_like(d_in)
    d_lines = torch.zeros(F * line_cap * 20, dtype=torch.uint8, device=dev)
    d_counts = torch.zeros(F, dtype=torch.int32, device=dev)
    d_labels = torch.zeros((F, H, W), dtype=torch.int32, device=dev)
    d_comps = torch.zeros(F * comp_cap * 28, dtype=torch.uint8, device=dev)
    d_cc = torch.zeros(F, dtype=torch.int32, device=dev)
    plan.pipeline(d_in.data_ptr(), 59.0, 119.0, thr, 0, d_e.data_ptr(), d_lines.data_ptr(), line_cap, d_counts.data_ptr())
    torch.cuda.synchronize()
    res = {"frames": F, "W": W, "H": H}
    for conn, mp, how, labels in [(8, 1, "masks", True), (8, 1, "masks", False), (8, 1, "bytes", True), (8, 1, "bytes", False),
                                  (8, 10, "masks", True), (8, 10, "masks", False), (8, 10, "bytes", True), (8, 10, "bytes", False), (4, 1, "masks", True)]:
        def call():
            plan.components(d_e.data_ptr() if how == "bytes" else 0, conn, mp, d_labels.data_ptr() if labels else 0, W, d_comps.data_ptr(), comp_cap,
                            d_cc.data_ptr())
        for _ in range(3):
            call()
        torch.cuda.synchronize()
        plan.set_timing(1)
        ms = {}
        for _ in range(10):
            call()
            torch.cuda.synchronize()
            for n, m in plan.get_timing():
                ms.setdefault(n, []).append(m)
        plan.set_timing(0)
        med = {n: float(np.median(v)) for n, v in ms.items()}
        res["conn=%d minPixels=%d %s %s" % (conn, mp, how, "labels" if labels else "no-labels")] = {
            "ms": {n: round(v, 4) for n, v in med.items()}, "ms_total": round(sum(med.values()), 4), "components": int(d_cc.cpu().numpy().sum())}
    # component statistics of the benchmark frames, from the device records (8-connectivity, every component)
    plan.components(0, 8, 1, 0, W, d_comps.data_ptr(), comp_cap, d_cc.data_ptr())
    torch.cuda.synchronize()
    cc = d_cc.cpu().numpy()
    recs = d_comps.cpu().numpy().view(capi.COMP_DTYPE).reshape(F, comp_cap)
    res["components_per_frame min/max"] = [int(cc.min()), int(cc.max())]
    res["comp_cap"] = comp_cap
    assert int(cc.max()) <= comp_cap, (int(cc.max()), comp_cap)
    stats = []
    for f in range(F):
        px = recs[f]["pixels"][:int(cc[f])]
        stats.append([int(cc[f]), int(px.sum()), round(float(px.max()) / max(int(px.sum()), 1), 4)])
    res["per_frame [components, edge pixels, largest share]"] = stats
    res["largest_share min/median/max"] = [round(float(np.percentile([s[2] for s in stats], q)), 4) for q in (0, 50, 100)]
    # the worst case of the count / box atomics: ONE all-foreground 4K frame (a single component of W * H pixels), as bytes, with labels
    one = capi.Plan(ctx, W, H, W, 1, theta)
    d_full = torch.full((H, W), 255, dtype=torch.uint8, device=dev)

    def call_full():
        one.components(d_full.data_ptr(), 8, 1, d_labels.data_ptr(), W, d_comps.data_ptr(), comp_cap, d_cc.data_ptr())
    for _ in range(3):
        call_full()
    torch.cuda.synchronize()
    one.set_timing(1)
    ms = {}
    for _ in range(10):
        call_full()
        torch.cuda.synchronize()
        for n, m in one.get_timing():
            ms.setdefault(n, []).append(m)
    one.set_timing(0)
    res["all_foreground one 4K frame bytes labels"] = {"ms": {n: round(float(np.median(v)), 4) for n, v in ms.items()},
                                                       "ms_total": round(sum(float(np.median(v)) for v in ms.values()), 4), "components": int(d_cc.cpu().numpy()[0])}
    one.close()
    # the yardstick: download + scipy.ndimage.label + statistics on one core
    for mp in (1, 10):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        h_e = d_e.cpu().numpy()
        t1 = time.perf_counter()
        n = 0
        same = True
        for f in range(F):
            lab, rec = components(h_e[f], 8, mp)
            n += len(rec)
            if mp == 1:
                same = same and rec.tobytes() == recs[f][:int(cc[f])].tobytes()
        t2 = time.perf_counter()
        res["minPixels=%d cpu_one_core" % mp] = {"download_ms": round((t1 - t0) * 1e3, 1), "label_and_stats_ms": round((t2 - t1) * 1e3, 1), "components": n,
                                                 "records_equal_device": bool(same) if mp == 1 else None}
    print(json.dumps(res))
    plan.close(); ctx.close()


if __name__ == "__main__":
    main()
