#!/usr/bin/env python
"""Time the remap and the inverse warp on the GPU (compvhip_plan_remap / compvhip_plan_warp_inverse) with HIP events: 32 frames of 3840 x 2160 to
3840 x 2160, a shared map, one map per frame, a shared 2 x 3 and a shared 3 x 3 matrix; nearest, bilinear and bicubic with uint8 output, bilinear and
bicubic with float32 output.  Medians of 10 calls after 3 warm-ups; the interpolations of a form are timed ALTERNATELY, one call each per round, so that the
bilinear kernel -- the yardstick of the bicubic one -- sees the same machine state.  The map is a mild radial distortion about the centre (what undistortion with a fixed camera map looks like), the 2 x 3 a rotation by 2 degrees
about the centre, the 3 x 3 the same with a slight perspective: nearly every output pixel is inside and the gathers stay local.

Each form's traffic is counted from the shapes -- every source byte once, every destination byte (1 or 4 per pixel) once, the float32 maps (8 bytes per pixel) once per group of
8 frames when shared and once per frame otherwise; the warp tables are a few kilobytes -- and given over the time as a share of the 6.29 TB/s a float4 copy
reaches on an MI355X.  Beside them the download of one frame (pinned): the first step of the host path this replaces.

--reference times that host path's second step instead, without a GPU: the compiled reference (oracle/_ref, one thread) on one 3840 x 2160 frame through
the shims of tests/golden/make_golden_remap.py and make_golden_bicubic.py (bicubic: median of 3); it needs the reference's headers, so it runs in the build container only.
Prints one JSON line."""
import json
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

W, H, S, F = 3840, 2160, 3840, 32
COPY_RATE = 6.29e12          # bytes per second, float4 copy
GROUP = 8                    # frames a workgroup serves with one read of a shared map (kRemapFramesPerGroup)
NEAREST, BILINEAR, BILINEAR_F32, BICUBIC, BICUBIC_F32 = 0, 1, 2, 4, 5
INTERPS = (("nearest", NEAREST), ("bilinear", BILINEAR), ("bicubic", BICUBIC), ("bilinear_f32", BILINEAR_F32), ("bicubic_f32", BICUBIC_F32))


def radial_map(k1=-0.05):
    """x, y (H, W) float32: a barrel distortion that keeps the corners inside the frame"""
    cx, cy, f = (W - 1) / 2.0, (H - 1) / 2.0, float(W)
    i, j = np.meshgrid(np.arange(W, dtype=np.float32), np.arange(H, dtype=np.float32))
    xn, yn = (i - cx) / f, (j - cy) / f
    g = 1.0 + k1 * (xn * xn + yn * yn)
    return (cx + (i - cx) * g).astype(np.float32), (cy + (j - cy) * g).astype(np.float32)


def matrices():
    a = np.deg2rad(2.0)
    c, s, cx, cy = np.cos(a), np.sin(a), (W - 1) / 2.0, (H - 1) / 2.0
    M2 = np.array([[c, -s, cx - c * cx + s * cy], [s, c, cy - s * cx - c * cy]], np.float32)
    M3 = np.vstack([M2, np.array([[2e-6, -1e-6, 1.0]], np.float32)])
    return M2, M3


def reference_main():
    import tempfile
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_golden_remap as g
    import make_golden_bicubic as gb
    import fast_model as fm
    g.RefShim(threads=1)
    img = np.ascontiguousarray(fm.noise(W, H, 1))
    x, y = radial_map()
    M2, M3 = matrices()
    res = {"what": "compiled reference, one thread, one 3840 x 2160 frame, ms (median of 5 after 1 warm-up)"}
    with tempfile.TemporaryDirectory() as tmp:
        L = g.build_shim(tmp)
        dst = np.zeros((H, W), np.uint8)

        def med(call, reps=5):
            call()
            t = []
            for _ in range(reps):
                t0 = time.perf_counter()
                assert call() == 0
                t.append((time.perf_counter() - t0) * 1e3)
            return round(float(np.median(t)), 2)
        for name, interp in (("nearest", NEAREST), ("bilinear", BILINEAR)):
            res["remap %s" % name] = med(lambda: L.remapshim_remap(img.ctypes.data, W, H, x.ctypes.data, y.ctypes.data, W, H, interp, None, 0, dst.ctypes.data))
            res["warp 2x3 %s" % name] = med(lambda: L.remapshim_warp(img.ctypes.data, W, H, M2.ctypes.data, 2, W, H, interp, 0, dst.ctypes.data))
            res["warp 3x3 %s" % name] = med(lambda: L.remapshim_warp(img.ctypes.data, W, H, M3.ctypes.data, 3, W, H, interp, 0, dst.ctypes.data))
        B = gb.build_shim(tmp)          # its leaf is scalar whatever the CPU flags say; they stay on, as for the forms above
        res["remap bicubic"] = med(lambda: B.bicshim_remap(img.ctypes.data, W, H, x.ctypes.data, y.ctypes.data, W, H, 0, None, 0, dst.ctypes.data), 3)
        res["warp 2x3 bicubic"] = med(lambda: B.bicshim_warp(img.ctypes.data, W, H, M2.ctypes.data, 2, W, H, 0, 0, dst.ctypes.data), 3)
        res["warp 3x3 bicubic"] = med(lambda: B.bicshim_warp(img.ctypes.data, W, H, M3.ctypes.data, 3, W, H, 0, 0, dst.ctypes.data), 3)
    print(json.dumps(res))


def alternately(calls, reps=10, warm=3):
    """calls: name -> call.  Every call `warm` times, then `reps` rounds of one timed call each, in turn; -> name -> median ms"""
    import torch
    for call in calls.values():
        for _ in range(warm):
            call()
    ms = {name: [] for name in calls}
    for _ in range(reps):
        for name, call in calls.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            call()
            b.record()
            torch.cuda.synchronize()
            ms[name].append(a.elapsed_time(b))
    return {name: float(np.median(v)) for name, v in ms.items()}


def main():
    import torch
    from compv_amd import capi
    from hysteresis_cases import text_frame
    dev = torch.device("cuda", 0)
    ctx = capi.Context(0)
    res = {"device": torch.cuda.get_device_properties(0).name, "frames": F, "size": [W, H], "reps": 10, "warm": 3}
    frames = np.stack([text_frame(W, H, 100 + f) for f in range(4)])
    d_in = torch.from_numpy(np.ascontiguousarray(frames[np.arange(F) % 4])).to(dev)
    d_out = torch.zeros(4 * F * H * W, dtype=torch.uint8, device=dev)          # room for float32 output
    x, y = radial_map()
    d_x1, d_y1 = torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)
    d_xf, d_yf = d_x1.unsqueeze(0).repeat(F, 1, 1).contiguous(), d_y1.unsqueeze(0).repeat(F, 1, 1).contiguous()
    M2, M3 = matrices()
    plan = capi.Plan(ctx, W, H, S, F)
    s = torch.cuda.current_stream().cuda_stream
    px = W * H * F
    shared_map_bytes = 8 * W * H * ((F + GROUP - 1) // GROUP)
    forms = (
        ("shared map", lambda i: plan.remap(d_in.data_ptr(), d_x1.data_ptr(), d_y1.data_ptr(), 1, i, d_out.data_ptr(), W, H, W, None, 0, s), shared_map_bytes),
        ("map per frame", lambda i: plan.remap(d_in.data_ptr(), d_xf.data_ptr(), d_yf.data_ptr(), F, i, d_out.data_ptr(), W, H, W, None, 0, s), 8 * px),
        ("2x3", lambda i: plan.warp_inverse(d_in.data_ptr(), M2, i, d_out.data_ptr(), W, H, W, 0, s), 0),
        ("3x3", lambda i: plan.warp_inverse(d_in.data_ptr(), M3, i, d_out.data_ptr(), W, H, W, 0, s), 0),
    )
    rows = []
    for name, call, coord_bytes in forms:
        times = alternately({iname: (lambda interp=interp: call(interp)) for iname, interp in INTERPS})
        for iname, interp in INTERPS:
            ms = times[iname]
            f32 = interp in (BILINEAR_F32, BICUBIC_F32)
            nbytes = px + px * (4 if f32 else 1) + coord_bytes
            call(interp)          # the share below looks at this interpolation's frame 0
            out0 = d_out[:4 * H * W].view(torch.float32) if f32 else d_out[:H * W]
            inside = float((out0 != 0).float().mean())
            rows.append({"form": name, "interp": iname, "ms": round(ms, 4), "bytes read + written": nbytes, "TB/s": round(nbytes / (ms * 1e-3) / 1e12, 3),
                         "share of the 6.29 TB/s copy rate": round(nbytes / (ms * 1e-3) / COPY_RATE, 3), "ms per frame": round(ms / F, 4),
                         "nonzero share of frame 0": round(inside, 3)})
    res["forms"] = rows
    host = torch.empty(H * W, dtype=torch.uint8).pin_memory()
    dl = []
    for i in range(2 + 5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host.copy_(d_in[0].reshape(-1))
        torch.cuda.synchronize()
        if i >= 2:
            dl.append((time.perf_counter() - t0) * 1e3)
    res["download_ms (one frame, pinned, median of 5)"] = round(float(np.median(dl)), 3)
    print(json.dumps(res))
    plan.close()
    ctx.close()


if __name__ == "__main__":
    reference_main() if "--reference" in sys.argv[1:] else main()
