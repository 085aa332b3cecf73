#!/usr/bin/env python
"""Time the HOG descriptors (compvhip_plan_hog) with HIP events: medians of 10 calls after 3 warm-ups, seeded noise frames, the reference's defaults
(block 16, stride 8, cell 8, 9 bins, L2HYS, signed, BILINEAR) --
  * 32 frames of 3840 x 2160;
  * 4096 crops of 64 x 128, the shape the reference's text and ADAS users feed it (a plan of 64 x 128 with one frame per crop);
  * the two kernels apart (the plan's timing mode) and the whole call (one event pair around it, timing mode off);
  * beside each time the bytes the call has to move -- frames in, cell map out and in again, descriptors out, counted from the shapes -- over that time,
    as a share of the rate a device-to-device copy of 512 MB reaches in the same process (read + written bytes over its time);
  * the descriptor of frame 0 against tests/hog_model.py (bit for bit) before anything is timed;
  * with --reference, where the reference checkout and oracle/_ref are present (the build container): CompVHOG::process on ONE core, AVX2 + FMA3 off
    (the canonical definition), through the shim of tests/golden/make_golden_hog.py -- one 4K frame and 256 crops, scaled to the workload's count.
    --no-gpu skips everything but that column.
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

WORKLOADS = [("frames_4k", 3840, 2160, 32), ("crops_64x128", 64, 128, 4096)]


def frames(W, H, S, n, seed):
    """n noise frames [n][H][S]; 4 distinct ones repeated (the generator, not the GPU, would otherwise dominate the tool's run time)"""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (min(n, 4), H, S), dtype=np.uint8)
    return np.ascontiguousarray(np.tile(base, ((n + 3) // 4, 1, 1))[:n])


def gpu_part(res):
    import torch
    from compv_amd import capi
    import hog_model as hm
    dev = torch.device("cuda", 0)
    ctx = capi.Context(0)
    res["device"] = torch.cuda.get_device_properties(0).name
    # the copy rate: 512 MB device to device, read + written bytes over the median of 10
    a, b = torch.empty(512 << 20, dtype=torch.uint8, device=dev), torch.empty(512 << 20, dtype=torch.uint8, device=dev)
    ts = []
    for i in range(13):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        b.copy_(a)
        e1.record()
        torch.cuda.synchronize()
        if i >= 3:
            ts.append(e0.elapsed_time(e1))
    copy_rate = 2 * (512 << 20) / (float(np.median(ts)) * 1e-3)
    res["copy_rate_GBps"] = round(copy_rate / 1e9, 1)
    del a, b
    for name, W, H, n in WORKLOADS:
        S = (W + 63) // 64 * 64
        g = capi.hog_geometry(W, H)
        host = frames(W, H, S, n, W)
        d_gray = torch.from_numpy(host).to(dev)
        d_desc = torch.zeros(n * g["descLen"], dtype=torch.float32, device=dev)
        plan = capi.Plan(ctx, W, H, S, n)

        def call():
            plan.hog(d_gray.data_ptr(), d_desc.data_ptr(), g["descLen"])
        for _ in range(3):
            call()
        torch.cuda.synchronize()
        row = {"frames": n, "W": W, "H": H, "descLen": g["descLen"]}
        got = d_desc[:g["descLen"]].cpu().numpy()
        row["frame0_equals_model"] = bool(got.tobytes() == hm.hog(host[0, :, :W])[0].tobytes())
        plan.set_timing(1)
        ms = {}
        for _ in range(10):
            call()
            torch.cuda.synchronize()
            for k, v in plan.get_timing():
                ms.setdefault(k, []).append(v)
        plan.set_timing(0)
        row.update({k + "_ms": round(float(np.median(v)), 4) for k, v in ms.items()})
        whole = []
        for _ in range(10):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            torch.cuda.synchronize()
            whole.append(e0.elapsed_time(e1))
        row["call_ms"] = round(float(np.median(whole)), 4)
        map_bytes = 4 * g["cellsX"] * g["cellsY"] * 9
        by = {"hog_cells_kernel": W * H + map_bytes, "hog_blocks_kernel": map_bytes + 4 * g["descLen"]}          # per frame: what each kernel must read and write once
        row["bytes_per_frame"] = {"frame": W * H, "map": map_bytes, "descriptor": 4 * g["descLen"]}
        for k, nbytes in by.items():
            row[k + "_share_of_copy_rate"] = round(n * nbytes / (row[k + "_ms"] * 1e-3) / copy_rate, 3)
        row["call_share_of_copy_rate"] = round(n * sum(by.values()) / (row["call_ms"] * 1e-3) / copy_rate, 3)
        row["Mpx_per_s"] = round(n * W * H / (row["call_ms"] * 1e-3) / 1e6, 1)
        plan.close()
        res[name] = row
    ctx.close()


def reference_part(res):
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_golden_hog as g
    from oracle_bindings import RefShim
    RefShim(threads=1)
    with tempfile.TemporaryDirectory() as tmp:
        L = g.build_shim(tmp)
        assert L.hogshim_simd(0) == 0
        for name, W, H, n in WORKLOADS:
            m = 1 if W * H > 1 << 16 else 256
            host = frames(W, H, W, m, W)
            g.ref_hog(L, host[0], None)
            t0 = time.perf_counter()
            for f in range(m):
                g.ref_hog(L, host[f], None)
            per_frame = (time.perf_counter() - t0) / m
            res.setdefault(name, {})["reference_one_core_ms"] = round(per_frame * n * 1e3, 1)
            res[name]["reference_frames_timed"] = m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", action="store_true")
    ap.add_argument("--no-gpu", action="store_true")
    a = ap.parse_args()
    res = {}
    if not a.no_gpu:
        gpu_part(res)
    if a.reference:
        reference_part(res)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
