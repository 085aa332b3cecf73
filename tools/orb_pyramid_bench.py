#!/usr/bin/env python
"""Time the ORB pyramid on the GPU (compvhip_orbpyr_detect / _describe) with HIP events: 32 frames of 3840 x 2160, the defaults (8 levels, 0.83, FAST-9,
threshold 20, maxFeatures 2000), medians of 10 calls after 3 warm-ups.  Per kernel through the object's timing mode -- the scale launch, and per level the
FAST score and list kernels, select, orient, blur, then the one brief launch -- and the whole _detect and _describe between two events of the tool's own
with the timing mode off.  The scale kernel's traffic (the source read once per level, every level written once) over its time is given as a share of the
6.29 TB/s a float4 copy reaches on an MI355X.  Beside them the download of one frame's corner list (pinned): the first step of the host path this replaces.
The compiled reference's full 8-level detect and describe on one core is NOT measured here: oracle/_ref/headless_samples has no mode for it yet.
Prints one JSON line."""
import json
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
from compv_amd import capi
from hysteresis_cases import text_frame

W, H, S, F = 3840, 2160, 3840, 32
KEY_CAP, CORNER_CAP = 4096, 4096
COPY_RATE = 6.29e12          # bytes per second, float4 copy


def per_kernel(pyr, call, reps=10, warm=3):
    for _ in range(warm):
        call()
    torch.cuda.synchronize()
    pyr.set_timing(1)
    runs = []
    for _ in range(reps):
        call()
        torch.cuda.synchronize()
        runs.append(pyr.get_timing())
    pyr.set_timing(0)
    names = [n for n, _ in runs[0]]
    assert all([n for n, _ in r] == names for r in runs)
    return [(n, round(float(np.median([r[i][1] for r in runs])), 4)) for i, n in enumerate(names)]


def whole(call, reps=10, warm=3):
    for _ in range(warm):
        call()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return round(float(np.median(ms)), 4)


def main():
    dev = torch.device("cuda", 0)
    ctx = capi.Context(0)
    res = {"device": torch.cuda.get_device_properties(0).name, "frames": F, "size": [W, H]}
    frames = np.stack([text_frame(W, H, 100 + f) for f in range(4)])
    d_in = torch.from_numpy(np.ascontiguousarray(frames[np.arange(F) % 4])).to(dev)
    d_keys = torch.zeros(F * KEY_CAP * 24, dtype=torch.uint8, device=dev)
    d_kc = torch.zeros(F, dtype=torch.int32, device=dev)
    d_desc = torch.zeros(F * KEY_CAP * 32, dtype=torch.uint8, device=dev)
    before = ctx.live_allocations()
    pyr = capi.OrbPyramid(ctx, W, H, S, F, capi.OrbPyramidOpts(), CORNER_CAP)
    d_lc = torch.zeros(F * pyr.levels, dtype=torch.int32, device=dev)
    d_lk = torch.zeros(F * pyr.levels, dtype=torch.int32, device=dev)
    geo = [pyr.geometry(l) for l in range(pyr.levels)]
    res["levels (W, H, S, quota)"] = [[g[0], g[1], g[2], g[4]] for g in geo]
    s = torch.cuda.current_stream().cuda_stream
    detect = lambda: pyr.detect(d_in.data_ptr(), d_keys.data_ptr(), KEY_CAP, d_kc.data_ptr(), d_lc.data_ptr(), d_lk.data_ptr(), s)          # noqa: E731
    describe = lambda: pyr.describe(d_in.data_ptr(), d_keys.data_ptr(), KEY_CAP, d_kc.data_ptr(), d_desc.data_ptr(), 32, True, s)          # noqa: E731
    res["detect kernels ms"] = per_kernel(pyr, detect)
    res["describe kernels ms (planes reused)"] = per_kernel(pyr, describe)
    res["device allocations of the pyramid"] = ctx.live_allocations() - before
    res["keypoints per frame min/max"] = [int(d_kc.min()), int(d_kc.max())]
    res["keypoints per level, frame 0"] = d_lc.cpu().numpy().reshape(F, -1)[0].tolist()
    res["FAST corners per level, frame 0"] = d_lk.cpu().numpy().reshape(F, -1)[0].tolist()
    res["detect ms (whole call)"] = whole(detect)
    res["describe ms (whole call, planes reused)"] = whole(describe)
    scale_ms = dict(res["detect kernels ms"]).get("scale_bilinear_kernel")
    written = sum(g[0] * g[1] for g in geo[1:] if g[2]) * F
    read = sum(W * H for g in geo[1:] if g[2]) * F
    res["scale traffic"] = {"bytes written": written, "bytes read (the source once per level)": read,
                            "share of the 6.29 TB/s copy rate": round((read + written) / (scale_ms * 1e-3) / COPY_RATE, 3) if scale_ms else None}
    host = torch.empty(2000 * 12, dtype=torch.uint8).pin_memory()
    src = torch.zeros(2000 * 12, dtype=torch.uint8, device=dev)
    dl = []
    for i in range(2 + 5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host.copy_(src)
        torch.cuda.synchronize()
        if i >= 2:
            dl.append((time.perf_counter() - t0) * 1e3)
    res["download_ms (2000 corners of one frame, pinned, median of 5)"] = round(float(np.median(dl)), 3)
    res["reference, 8 levels on one core"] = "not measured: oracle/_ref/headless_samples has no pyramid mode"
    print(json.dumps(res))
    pyr.close()
    ctx.close()


if __name__ == "__main__":
    main()
