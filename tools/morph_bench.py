#!/usr/bin/env python
"""Time the thresholding / morphology calls on 32 resident 4K text-like frames with HIP events via the plan's timing mode: medians of 10 calls
after warm-up, per kernel and in total, for
  the global threshold, the adaptive threshold at blockSize 15 and 31,
  erode rect 3x3, close rect 15x3, close diamond 5x5,
  the full rectangles through the general kernel and the separable one, interleaved call by call in this process,
  the text chain grayscale -> Otsu -> threshold -> close(rect 5x3) -> components(8),
each beside 2 B/px at the measured copy rate DESIGN.md uses (5.4 TB/s), and beside the thing the call replaces, measured in the same run on
the same host: the download of the frames, then scipy.ndimage (or, without scipy, tests/morph_model.py) on one core, timed on CPU_FRAMES frames.
"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import numpy as np, torch
from compv_amd import capi
import morph_model as mm
from hysteresis_cases import text_frame

try:
    from scipy import ndimage
except ImportError:
    ndimage = None

COPY_TBS = 5.4
CPU_FRAMES = 2


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
    # a name that appears twice in a call (the two basic operations of a close) has 2 * reps samples: report the sum per call
    return {n: round(float(np.median(np.array(v).reshape(reps, -1).sum(axis=1))), 4) for n, v in ms.items()}


def cpu_morph(img, se, op):
    fp = se != 0
    if ndimage is None:
        return mm.morph(img, se, op)
    # the reference's anchor: the same offsets for erode and dilate -> scipy's maximum_filter (a correlation) needs no flip either
    lo = lambda a: ndimage.minimum_filter(a, footprint=fp, mode="nearest")
    hi = lambda a: ndimage.maximum_filter(a, footprint=fp, mode="nearest")
    return {mm.ERODE: lambda a: lo(a), mm.DILATE: lambda a: hi(a), mm.OPEN: lambda a: hi(lo(a)), mm.CLOSE: lambda a: lo(hi(a))}[op](img)


def cpu_adaptive(img, bs):
    if ndimage is None:
        return mm.adaptive(img, bs, 5.0)
    mean = ndimage.uniform_filter(img.astype(np.int32), bs, mode="constant")
    return np.where(img.astype(np.int32) - mean + 255 >= 251, 255, 0).astype(np.uint8)


def main():
    W, H, F = 3840, 2160, 32
    dev = torch.device("cuda", 0)
    ctx = capi.Context(0)
    plan = capi.Plan(ctx, W, H, W, F)
    base = [text_frame(W, H, 12345 + f) for f in range(4)]
    gray = np.stack([base[f % 4] for f in range(F)])
    d_in = torch.from_numpy(gray).to(dev)
    d_a, d_b = torch.empty_like(d_in), torch.empty_like(d_in)
    floor_ms = 2.0 * F * W * H / (COPY_TBS * 1e12) * 1e3
    res = {"frames": F, "W": W, "H": H, "floor_ms (2 B/px at %.1f TB/s)" % COPY_TBS: round(floor_ms, 4), "cpu": "scipy.ndimage" if ndimage is not None else "numpy model"}
    rect = lambda w, h: mm.strel(mm.RECT, w, h)
    diamond5 = mm.strel(mm.DIAMOND, 5, 5)
    p_in, p_a, p_b = d_in.data_ptr(), d_a.data_ptr(), d_b.data_ptr()

    def report(name, ms):
        tot = sum(ms.values())
        res[name] = {"ms": ms, "ms_total": round(tot, 4), "x_floor": round(tot / floor_ms, 2)}

    report("threshold 127.5", timed(plan, lambda: plan.threshold(p_in, 127.5, p_a)))
    report("adaptive 15", timed(plan, lambda: plan.threshold_adaptive(p_in, 15, 5.0, 255.0, 0, p_a)))
    report("adaptive 31", timed(plan, lambda: plan.threshold_adaptive(p_in, 31, 5.0, 255.0, 0, p_a)))
    report("erode rect 3x3", timed(plan, lambda: plan.morph(p_in, rect(3, 3), mm.ERODE, mm.BORDER_REPLICATE, p_a)))
    plan.threshold(p_in, 127.5, p_b)           # the binary map the closes work on
    report("close rect 15x3", timed(plan, lambda: plan.morph(p_b, rect(15, 3), mm.CLOSE, mm.BORDER_REPLICATE, p_a)))
    report("close diamond 5x5", timed(plan, lambda: plan.morph(p_b, diamond5, mm.CLOSE, mm.BORDER_REPLICATE, p_a)))
    # general against separable on full rectangles, one basic operation, interleaved call by call
    for (w, h) in ((3, 3), (15, 3), (5, 3), (31, 31)):
        se = rect(w, h)
        t = {capi.MORPH_KERNEL_GENERAL: [], capi.MORPH_KERNEL_SEPARABLE: []}
        for k in t:
            plan.morph(p_in, se, mm.ERODE, mm.BORDER_REPLICATE, p_a, kernel=k)
        torch.cuda.synchronize()
        plan.set_timing(1)
        for _ in range(10):
            for k in t:
                plan.morph(p_in, se, mm.ERODE, mm.BORDER_REPLICATE, p_a, kernel=k)
                torch.cuda.synchronize()
                t[k].append(sum(m for _, m in plan.get_timing()))
        plan.set_timing(0)
        g, s = float(np.median(t[capi.MORPH_KERNEL_GENERAL])), float(np.median(t[capi.MORPH_KERNEL_SEPARABLE]))
        res["erode rect %dx%d general / separable" % (w, h)] = {"general_ms": round(g, 4), "separable_ms": round(s, 4), "ratio": round(g / s, 2), "separable_x_floor": round(s / floor_ms, 2)}
    # the text chain from packed RGBA frames
    rgba = np.repeat(gray[:4, :, :, None], 4, axis=3)
    d_rgba = torch.from_numpy(np.concatenate([rgba] * (F // 4))).to(dev)
    d_lv = torch.zeros(F, dtype=torch.int32, device=dev)
    comp_cap = 1 << 17
    d_comps = torch.zeros(F * comp_cap * 28, dtype=torch.uint8, device=dev)
    d_cc = torch.zeros(F, dtype=torch.int32, device=dev)
    se53 = rect(5, 3)

    def chain():
        plan.grayscale(d_rgba.data_ptr(), capi.FMT_RGBA32, p_a)
        plan.otsu(p_a, d_lv.data_ptr())
        plan.threshold(p_a, 0.0, p_a, d_levels=d_lv.data_ptr())
        plan.morph(p_a, se53, mm.CLOSE, mm.BORDER_REPLICATE, p_b)
        plan.components(p_b, 8, 1, 0, W, d_comps.data_ptr(), comp_cap, d_cc.data_ptr())
    for _ in range(2):
        chain()
    torch.cuda.synchronize()
    wall = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); chain(); e1.record()
        torch.cuda.synchronize()
        wall.append(e0.elapsed_time(e1))
    res["text chain gray->otsu->threshold->close 5x3->components"] = {"ms_total (events around the five calls)": round(float(np.median(wall)), 4),
                                                                       "components_per_frame min/max": [int(d_cc.min()), int(d_cc.max())]}
    # the yardstick: download + one core
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    h_in = d_in.cpu().numpy()
    dl = (time.perf_counter() - t0) * 1e3
    cpu = {"download_ms (32 frames)": round(dl, 1), "frames_timed": CPU_FRAMES}

    def per_frame(fn):
        t0 = time.perf_counter()
        for f in range(CPU_FRAMES):
            fn(h_in[f])
        return round((time.perf_counter() - t0) * 1e3 / CPU_FRAMES, 1)
    cpu["threshold ms/frame"] = per_frame(lambda a: np.where(a > 128, 255, 0).astype(np.uint8))
    cpu["adaptive 15 ms/frame"] = per_frame(lambda a: cpu_adaptive(a, 15))
    cpu["adaptive 31 ms/frame"] = per_frame(lambda a: cpu_adaptive(a, 31))
    cpu["erode rect 3x3 ms/frame"] = per_frame(lambda a: cpu_morph(a, rect(3, 3), mm.ERODE))
    cpu["close rect 15x3 ms/frame"] = per_frame(lambda a: cpu_morph(a, rect(15, 3), mm.CLOSE))
    cpu["close diamond 5x5 ms/frame"] = per_frame(lambda a: cpu_morph(a, diamond5, mm.CLOSE))
    res["cpu_one_core"] = cpu
    print(json.dumps(res))
    plan.close(); ctx.close()


if __name__ == "__main__":
    main()
