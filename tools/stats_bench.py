#!/usr/bin/env python
"""Time the image statistics (compvhip_plan_integral / _histogram / _equalize / _projections) with HIP events: medians of 10 calls after 3 warm-ups, seeded
noise frames --
  * 32 frames of 3840 x 2160;
  * 4096 crops of 64 x 128 (a plan of 64 x 128 with one frame per crop);
  * every call's kernels apart (the plan's timing mode) and the whole call (one event pair around it, timing mode off): the integral with both outputs,
    with sum only; the histogram; the equalisation with its own histogram, out of place; the projections, both;
  * beside each time the bytes the call has to move at the least, counted from the shapes -- integral: the frame once and 8 bytes per output element;
    histogram and projections: the frame once; equalisation: the frame twice and the output once -- over that time, as a share of the rate a
    device-to-device copy of 512 MB reaches in the same process (read + written bytes over its time);
  * frame 0 of every call against tests/stats_model.py (bit for bit) before anything is timed;
  * with --reference, where the reference checkout and oracle/_ref are present (the build container): the compiled reference on ONE core through the shim
    of tests/golden/make_golden_stats.py -- one 4K frame and 256 crops, scaled to the workload's count.  --no-gpu skips everything but that column.
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
    import stats_model as sm
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
        host = frames(W, H, S, n, W)
        img0 = host[0, :, :W]
        d_gray = torch.from_numpy(host).to(dev)
        plane = (H + 1) * (W + 1)
        d_sum = torch.zeros(n * plane, dtype=torch.float64, device=dev)
        d_sumsq = torch.zeros(n * plane, dtype=torch.float64, device=dev)
        d_hist = torch.zeros(n * 256, dtype=torch.int32, device=dev)
        d_out = torch.zeros(n * H * S, dtype=torch.uint8, device=dev)
        d_px = torch.zeros(n * W, dtype=torch.int32, device=dev)
        d_py = torch.zeros(n * H, dtype=torch.int32, device=dev)
        plan = capi.Plan(ctx, W, H, S, n)
        g = d_gray.data_ptr()
        px = W * H
        calls = {          # name: (the call, bytes per frame at the least)
            "integral_both": (lambda: plan.integral(g, d_sum.data_ptr(), d_sumsq.data_ptr(), W + 1), px + 16 * plane),
            "integral_sum": (lambda: plan.integral(g, d_sum.data_ptr(), 0, W + 1), px + 8 * plane),
            "histogram": (lambda: plan.histogram(g, d_hist.data_ptr()), px),
            "equalize": (lambda: plan.equalize(g, d_out.data_ptr()), 3 * px),
            "projections": (lambda: plan.projections(g, d_px.data_ptr(), d_py.data_ptr()), px),
        }
        row = {"frames": n, "W": W, "H": H}
        # frame 0 against the model before anything is timed
        for c, _ in calls.values():
            c()
        torch.cuda.synchronize()
        s, q = sm.integral(img0)
        ok = d_sum[:plane].cpu().numpy().tobytes() == s.tobytes() and d_sumsq[:plane].cpu().numpy().tobytes() == q.tobytes()
        ok = ok and d_hist[:256].cpu().numpy().view(np.uint32).tobytes() == sm.histogram(img0).tobytes()
        ok = ok and (d_out[:H * S].cpu().numpy().reshape(H, S)[:, :W] == sm.equalize(img0)[0]).all()
        ok = ok and d_px[:W].cpu().numpy().tobytes() == sm.projections(img0)[0].tobytes() and d_py[:H].cpu().numpy().tobytes() == sm.projections(img0)[1].tobytes()
        row["frame0_equals_model"] = bool(ok)
        for cname, (call, nbytes) in calls.items():
            for _ in range(3):
                call()
            torch.cuda.synchronize()
            r = {"bytes_per_px_floor": round(nbytes / px, 2)}
            plan.set_timing(1)
            ms = {}
            for _ in range(10):
                call()
                torch.cuda.synchronize()
                for k, v in plan.get_timing():
                    ms.setdefault(k, []).append(v)
            plan.set_timing(0)
            r.update({k + "_ms": round(float(np.median(v)), 4) for k, v in ms.items()})
            whole = []
            for _ in range(10):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                call()
                e1.record()
                torch.cuda.synchronize()
                whole.append(e0.elapsed_time(e1))
            r["call_ms"] = round(float(np.median(whole)), 4)
            r["call_GBps"] = round(n * nbytes / (r["call_ms"] * 1e-3) / 1e9, 1)
            r["call_share_of_copy_rate"] = round(n * nbytes / (r["call_ms"] * 1e-3) / copy_rate, 3)
            r["Mpx_per_s"] = round(n * px / (r["call_ms"] * 1e-3) / 1e6, 1)
            row[cname] = r
        plan.close()
        res[name] = row
    ctx.close()


def reference_part(res):
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_golden_stats as g
    from oracle_bindings import RefShim
    RefShim(threads=1)
    with tempfile.TemporaryDirectory() as tmp:
        L = g.build_shim(tmp)
        for name, W, H, n in WORKLOADS:
            m = 1 if W * H > 1 << 16 else 256
            host = frames(W, H, W, m, W)
            s, q = np.zeros((H + 1, W + 1)), np.zeros((H + 1, W + 1))
            hist, out = np.zeros(256, np.uint32), np.zeros((H, W), np.uint8)
            px, py = np.zeros(W, np.int32), np.zeros(H, np.int32)
            ref = {
                "integral_both": lambda f: L.statshim_integral(f.ctypes.data, W, H, W, s.ctypes.data, q.ctypes.data),
                "histogram": lambda f: L.statshim_histogram(f.ctypes.data, W, H, W, hist.ctypes.data),
                "equalize": lambda f: L.statshim_equalize(f.ctypes.data, W, H, W, None, -1.0, out.ctypes.data),
                "projections": lambda f: L.statshim_projections(f.ctypes.data, W, H, W, px.ctypes.data, py.ctypes.data),
            }
            for cname, fn in ref.items():
                assert fn(host[0]) == 0
                t0 = time.perf_counter()
                for f in range(m):
                    fn(host[f])
                per_frame = (time.perf_counter() - t0) / m          # includes the shim's copy of the frame into a CompVMat and of the results out of it
                res.setdefault(name, {}).setdefault(cname, {})["reference_one_core_ms"] = round(per_frame * n * 1e3, 1)
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
