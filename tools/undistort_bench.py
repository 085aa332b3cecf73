#!/usr/bin/env python
"""Time lens undistortion on the GPU (compvhip_undistort_*) with HIP events: 32 frames of 3840 x 2160 to 3840 x 2160, nearest, bilinear and bicubic with
uint8 output.  Medians of 10 calls after 3 warm-ups.  For every interpolation four forms are timed ALTERNATELY, one call each per round, so that each
fused form and the remap form it replaces see the same machine state:

  fused, shared camera        compvhip_undistort_frames, one camera: coordinates in registers, worked out once per group of 8 frames
  remap, shared map           compvhip_plan_remap on the float32 maps compvhip_undistort_maps wrote (the map kernel is NOT in this time)
  fused, camera per frame     compvhip_undistort_frames, 32 cameras
  remap, map per frame        compvhip_plan_remap on 32 pairs of maps from the map kernel

and the map kernel alone (1 camera and 32, float32).  Each form's traffic is counted from the shapes -- every source and destination byte once, the
float32 maps (8 bytes per pixel) once per group of 8 frames when shared and once per frame otherwise -- and given over the time as a share of the
6.29 TB/s a float4 copy reaches on an MI355X.  The camera is a mild barrel distortion: every output pixel is inside and the gathers stay local.

--reference times the host path this replaces instead, without a GPU: the compiled reference (oracle/_ref, one thread) on one 3840 x 2160 frame --
CompVCalibUtils::initUndistMap and undist2DImage (which builds the map again on every call) -- through the shim of
tests/golden/make_golden_undistort.py; it needs the reference's headers, so it runs in the build container only.
Prints one JSON line."""
import ctypes as C
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
GROUP = 8                    # frames a workgroup serves with one set of coordinates when the camera is shared (kRemapFramesPerGroup)
INTERPS = (("nearest", 0), ("bilinear", 1), ("bicubic", 4))
K = np.array([[0.9 * W, 0.0, 0.5 * W - 0.3], [0.0, 0.9 * W, 0.5 * H + 0.45], [0.0, 0.0, 1.0]], np.float32)
D = np.array([-0.05, 0.01, 0.0005, -0.0003], np.float32)


def cameras(n):
    """n cameras of a rig: K (n, 3, 3), d (n, 4) float32, each a little off the first"""
    Ks, ds = np.repeat(K[None], n, axis=0), np.repeat(D[None], n, axis=0)
    for k in range(n):
        Ks[k, 0, 2] += 0.5 * k
        Ks[k, 1, 2] -= 0.25 * k
        ds[k, 0] *= 1.0 - 0.01 * k
    return Ks, ds


def reference_main():
    import tempfile
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_golden_undistort as g
    import fast_model as fm
    g.RefShim(threads=1)
    img = np.ascontiguousarray(fm.noise(W, H, 1))
    res = {"what": "compiled reference, one thread, one 3840 x 2160 frame, ms (median of 5 after 1 warm-up)"}
    with tempfile.TemporaryDirectory() as tmp:
        L = g.build_shim(tmp)
        dst, mx, my, cols = np.zeros((H, W), np.uint8), np.zeros((H, W), np.float32), np.zeros((H, W), np.float32), C.c_size_t()

        def med(call, reps=5):
            call()
            t = []
            for _ in range(reps):
                t0 = time.perf_counter()
                assert call() == 0
                t.append((time.perf_counter() - t0) * 1e3)
            return round(float(np.median(t)), 2)
        res["initUndistMap float32"] = med(lambda: L.undshim_map(0, K.ctypes.data, D.ctypes.data, 4, W, H, None, mx.ctypes.data, my.ctypes.data, C.byref(cols)))
        for name, interp in (("nearest", 0), ("bilinear", 1)):
            res["undist2DImage %s (map + remap)" % name] = med(lambda: L.undshim_image(img.ctypes.data, W, H, K.ctypes.data, D.ctypes.data, 4, interp, dst.ctypes.data))
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
    d_fused = torch.zeros(F * H * W, dtype=torch.uint8, device=dev)
    d_remap = torch.zeros(F * H * W, dtype=torch.uint8, device=dev)
    d_x1, d_y1 = (torch.zeros(H * W, dtype=torch.float32, device=dev) for _ in range(2))
    d_xf, d_yf = (torch.zeros(F * H * W, dtype=torch.float32, device=dev) for _ in range(2))
    s = torch.cuda.current_stream().cuda_stream
    plan = capi.Plan(ctx, W, H, S, F)
    und = capi.Undistort(ctx, W, H, S, F, stream=s)
    Ks, ds = cameras(F)
    und.maps(K, D, d_x1.data_ptr(), d_y1.data_ptr())
    und.maps(Ks, ds, d_xf.data_ptr(), d_yf.data_ptr())
    torch.cuda.synchronize()
    px = W * H * F
    shared_map_bytes = 8 * W * H * ((F + GROUP - 1) // GROUP)
    rows = []
    for iname, interp in INTERPS:
        calls = {
            "fused, shared camera": lambda: und.undistort(d_in.data_ptr(), K, D, interp, d_fused.data_ptr(), W),
            "remap, shared map": lambda: plan.remap(d_in.data_ptr(), d_x1.data_ptr(), d_y1.data_ptr(), 1, interp, d_remap.data_ptr(), W, H, W, None, 0, s),
            "fused, camera per frame": lambda: und.undistort(d_in.data_ptr(), Ks, ds, interp, d_fused.data_ptr(), W),
            "remap, map per frame": lambda: plan.remap(d_in.data_ptr(), d_xf.data_ptr(), d_yf.data_ptr(), F, interp, d_remap.data_ptr(), W, H, W, None, 0, s),
        }
        coord = {"fused, shared camera": 0, "remap, shared map": shared_map_bytes, "fused, camera per frame": 0, "remap, map per frame": 8 * px}
        times = alternately(calls)
        for pair in (("fused, shared camera", "remap, shared map"), ("fused, camera per frame", "remap, map per frame")):
            calls[pair[0]]()
            calls[pair[1]]()
            torch.cuda.synchronize()
            assert torch.equal(d_fused, d_remap), "the fused form and the remap of the device maps differ (%s, %s)" % (iname, pair[0])
        for name in calls:
            ms, nbytes = times[name], 2 * px + coord[name]
            rows.append({"form": name, "interp": iname, "ms": round(ms, 4), "bytes read + written": nbytes, "TB/s": round(nbytes / (ms * 1e-3) / 1e12, 3),
                         "share of the 6.29 TB/s copy rate": round(nbytes / (ms * 1e-3) / COPY_RATE, 3), "ms per frame": round(ms / F, 4)})
        res["nonzero share of frame 0, %s" % iname] = round(float((d_fused[:H * W] != 0).float().mean()), 3)
    res["forms"] = rows
    maps = alternately({"map kernel, 1 camera": lambda: und.maps(K, D, d_x1.data_ptr(), d_y1.data_ptr()),
                        "map kernel, 32 cameras": lambda: und.maps(Ks, ds, d_xf.data_ptr(), d_yf.data_ptr())})
    res["maps"] = [{"form": name, "ms": round(ms, 4), "bytes written": 8 * W * H * n, "TB/s": round(8 * W * H * n / (ms * 1e-3) / 1e12, 3),
                    "share of the 6.29 TB/s copy rate": round(8 * W * H * n / (ms * 1e-3) / COPY_RATE, 3)} for (name, ms), n in zip(maps.items(), (1, F))]
    print(json.dumps(res))
    und.close()
    plan.close()
    ctx.close()


if __name__ == "__main__":
    reference_main() if "--reference" in sys.argv[1:] else main()
