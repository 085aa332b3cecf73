#!/usr/bin/env python
"""Time the colour conversion (compvhip_convert_frames) with HIP events on 32 resident frames of 3840 x 2160 --
  * pairs: NV12, YUV420P, YUYV422 -> RGBA32 and -> RGB24; RGB24 -> HSV; NV12 -> HSV; RGBA32 -> YUV444P; dense planes, 16-byte aligned (the word arm);
  * a measurement is one event pair around enough back-to-back calls to fill about a quarter of a second (the count comes from a calibration of 5 calls),
    after 3 warm-up calls; every pair is measured --rounds times (default 5) and reports the median time of a call (32 frames);
  * the yardstick, in the same run: the existing gray_kernel on RGB24 (compvhip_plan_grayscale, unchanged code, a stream of the same kind), measured in the
    same way before every pair of every round, so its own spread over the run is reported beside the pairs (min, median, max);
  * algorithmic bytes: what a pair must read and write, from compvhip_convert_layout -- the source's and the destination's planes once each; grayscale:
    3 + 1 bytes per pixel -- over the call's time;
  * frame 0 of every pair against tests/convert_model.py (bit for bit) before anything is timed;
  * with --reference, where the reference checkout and oracle/_ref are present (the build container): the compiled reference on ONE core through the shim
    of tests/golden/make_golden_convert.py, one 4K frame, scaled to 32.  --no-gpu skips everything but that column.
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

import convert_model as cm

W, H, FRAMES = 3840, 2160, 32
PAIRS = [(cm.NV12, cm.RGBA32), (cm.NV12, cm.RGB24), (cm.YUV420P, cm.RGBA32), (cm.YUV420P, cm.RGB24), (cm.YUYV422, cm.RGBA32), (cm.YUYV422, cm.RGB24),
         (cm.RGB24, cm.HSV), (cm.NV12, cm.HSV), (cm.RGBA32, cm.YUV444P)]
WINDOW_S = 0.25


def image_bytes(fmt):
    n, rb, rows = cm.layout(fmt, W, H)
    return sum(rb[p] * rows[p] for p in range(n))


def source_frame(fmt, seed):
    r = np.random.default_rng(seed)
    return [r.integers(0, 256, s, dtype=np.uint8) for s in cm.plane_shapes(fmt, W, H)]


def gpu_part(res, rounds):
    import torch
    from compv_amd import capi
    dev = torch.device("cuda", 0)
    ctx = capi.Context(0)
    res["device"] = torch.cuda.get_device_properties(0).name
    res["frames"], res["W"], res["H"], res["rounds"] = FRAMES, W, H, rounds

    def device_image(fmt, planes=None):
        """FRAMES dense frames per plane; 4 distinct source frames repeated.  -> (tensors, description)"""
        n, rb, rows = cm.layout(fmt, W, H)
        ts = []
        for p in range(n):
            if planes is None:
                ts.append(torch.zeros(FRAMES * rb[p] * rows[p], dtype=torch.uint8, device=dev))
            else:
                ts.append(torch.from_numpy(np.concatenate([planes[f % len(planes)][p].reshape(-1) for f in range(FRAMES)])).to(dev))
        return ts, capi.Image(fmt, [t.data_ptr() for t in ts], rb[:n], [rb[p] * rows[p] for p in range(n)])

    def measure(call):
        """median-free: one window of back-to-back calls -> ms per call"""
        def window(n):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n):
                call()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / n
        n = max(5, int(WINDOW_S * 1e3 / max(window(5), 1e-3)))
        return window(n), n

    # the yardstick: gray_kernel on RGB24
    rgb = [source_frame(cm.RGB24, 100 + f) for f in range(4)]
    g_in, _ = device_image(cm.RGB24, rgb)
    g_out = torch.zeros(FRAMES * W * H, dtype=torch.uint8, device=dev)
    plan = capi.Plan(ctx, W, H, W, FRAMES)
    gray = lambda: plan.grayscale(g_in[0].data_ptr(), capi.FMT_RGB24, g_out.data_ptr())          # noqa: E731
    gray_bytes = FRAMES * 4 * W * H
    for _ in range(3):
        gray()
    torch.cuda.synchronize()
    yard = []
    rows = {}
    for src, dst in PAIRS:
        name = cm.pair_name(src, dst)
        frames = [source_frame(src, 200 + 10 * src + f) for f in range(4)]
        a_t, a = device_image(src, frames)
        b_t, b = device_image(dst)
        call = lambda: ctx.convert_frames(W, H, FRAMES, a, b)          # noqa: E731
        for _ in range(3):
            call()
        torch.cuda.synchronize()
        exp = cm.convert(src, dst, frames[0], W, H)
        ok = all(t[:e.size].cpu().numpy().tobytes() == e.tobytes() for t, e in zip(b_t, exp))
        nbytes = FRAMES * (image_bytes(src) + image_bytes(dst))
        ms, ycall = [], []
        for _ in range(rounds):          # yardstick, pair, yardstick, pair, ...
            y, _ = measure(gray)
            yard.append(y)
            ycall.append(y)
            m, n = measure(call)
            ms.append(m)
        med = float(np.median(ms))
        rows[name] = {"frame0_equals_model": bool(ok), "bytes_per_px": round(nbytes / FRAMES / (W * H), 2), "call_ms": round(med, 4), "call_ms_min_max": [round(min(ms), 4), round(max(ms), 4)],
                      "calls_per_window": n, "GBps": round(nbytes / (med * 1e-3) / 1e9, 1), "us_per_frame": round(med * 1e3 / FRAMES, 1),
                      "yardstick_GBps_beside": round(gray_bytes / (float(np.median(ycall)) * 1e-3) / 1e9, 1)}
        del a_t, b_t
    ymed = float(np.median(yard))
    res["yardstick_gray_rgb24"] = {"bytes_per_px": 4.0, "call_ms": round(ymed, 4), "call_ms_min_max": [round(min(yard), 4), round(max(yard), 4)], "measurements": len(yard),
                                   "GBps": round(gray_bytes / (ymed * 1e-3) / 1e9, 1), "GBps_min_max": [round(gray_bytes / (max(yard) * 1e-3) / 1e9, 1), round(gray_bytes / (min(yard) * 1e-3) / 1e9, 1)],
                                   "us_per_frame": round(ymed * 1e3 / FRAMES, 1)}
    for r in rows.values():
        r["rate_over_yardstick"] = round(r["GBps"] / res["yardstick_gray_rgb24"]["GBps"], 3)
    res["pairs"] = rows
    plan.close()
    ctx.close()


def reference_part(res):
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_golden_convert as g
    from oracle_bindings import RefShim
    RefShim(threads=1)
    with tempfile.TemporaryDirectory() as tmp:
        L = g.build_shim(tmp)
        for src, dst in PAIRS:
            planes = source_frame(src, 200 + 10 * src)
            c = dict(src=src, W=W, H=H)
            assert not isinstance(g.reference(L, c, planes, dst), str)
            t0 = time.perf_counter()
            g.reference(L, c, planes, dst)          # includes the shim's copies into a CompVMat and out of it
            res.setdefault("pairs", {}).setdefault(cm.pair_name(src, dst), {})["reference_one_core_ms"] = round((time.perf_counter() - t0) * FRAMES * 1e3, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", action="store_true")
    ap.add_argument("--no-gpu", action="store_true")
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    res = {}
    if not a.no_gpu:
        gpu_part(res, a.rounds)
    if a.reference:
        reference_part(res)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
