#!/usr/bin/env python
"""Time the image moments on the GPU (compvhip_moments_frames, compvhip_moments_components) with HIP events.  Medians of 10 calls after 3 warm-ups;
calls that are compared are timed ALTERNATELY, one call each per round, so that they see the same machine state.

  frames      32 resident 3840 x 2160 frames (the benchmark's synth_frame seeds) and 4096 crops of 64 x 128: compvhip_moments_frames with VALUE and UNIT
              weights, raw records alone and with shape records, beside compvhip_plan_histogram on the same planes -- the same 1 byte per pixel read
              stream.  Traffic: every source byte once, over the time, as a share of the 6.29 TB/s a float4 copy reaches on an MI355X.
  components  the 32 frames' edge maps of one compvhip_plan_pipeline step at the benchmark's thresholds, labelled by compvhip_plan_components (label map
              33 MB per frame): compvhip_moments_components without gray planes and with them, both origins; and ONE all-foreground 4K frame, where every
              pixel lands on one record.  Traffic: 4 bytes per pixel of labels, plus 1 with gray planes.
  download    what the call replaces on the way to a host implementation: the 32 label maps brought to the host with torch (once, wall clock).

Frame 0 of every form is compared with tests/moments_model.py bit for bit before anything is reported.

--reference times the host path instead, without a GPU: the compiled reference (oracle/_ref, one thread) on one 3840 x 2160 frame and on 256 crops of
64 x 128 -- rawSecondOrder, rawFirstOrder, skewness and orientation, each of which walks the plane again -- through the shim of
tests/golden/make_golden_moments.py; it needs the reference's headers, so it runs in the build container only.
Prints one JSON line."""
import json
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

W, H, F = 3840, 2160, 32
CW, CH, CF = 64, 128, 4096
COPY_RATE = 6.29e12          # bytes per second, float4 copy
RAW, SHAPE = 48, 72


def reference_main():
    import tempfile
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_golden_moments as g
    from oracle_bindings import synth_frame
    g.RefShim(threads=1)
    res = {"what": "compiled reference, one thread, ms (median of 5 after 1 warm-up): rawSecondOrder + rawFirstOrder + skewness + orientation, four walks of the plane"}
    with tempfile.TemporaryDirectory() as tmp:
        L = g.build_shim(tmp)

        def med(planes, reps=5):
            t = []
            for k in range(reps + 1):
                t0 = time.perf_counter()
                for p in planes:
                    g.reference(L, p)
                t.append((time.perf_counter() - t0) * 1e3)
            return round(float(np.median(t[1:])), 2)
        res["one 3840 x 2160 frame"] = med([np.ascontiguousarray(synth_frame(W, H, 12345))])
        crops = np.random.default_rng(5).integers(0, 256, (256, CH, CW), dtype=np.uint8)
        res["256 crops of 64 x 128"] = med(list(crops))
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


def rows_of(times, nbytes):
    return [{"form": name, "ms": round(ms, 4), "bytes read": nbytes[name], "TB/s": round(nbytes[name] / (ms * 1e-3) / 1e12, 3),
             "share of the 6.29 TB/s copy rate": round(nbytes[name] / (ms * 1e-3) / COPY_RATE, 3)} for name, ms in times.items()]


def main():
    import torch
    import moments_model as mm
    from compv_amd import capi
    from oracle_bindings import synth_frame
    dev = torch.device("cuda", 0)
    ctx = capi.Context(0)
    s = torch.cuda.current_stream().cuda_stream
    res = {"device": torch.cuda.get_device_properties(0).name, "reps": 10, "warm": 3}
    d_raw = torch.zeros(max(F * (1 << 16), CF) * RAW, dtype=torch.uint8, device=dev)
    d_shape = torch.zeros(max(F * (1 << 16), CF) * SHAPE, dtype=torch.uint8, device=dev)
    d_hist = torch.zeros(max(F, CF) * 256, dtype=torch.int32, device=dev)

    def raw_of(k):
        return tuple(int(v) for v in np.frombuffer(d_raw[k * RAW:(k + 1) * RAW].cpu().numpy().tobytes(), np.uint64))

    # ---- frames: 32 x 4K, 4096 crops ----
    host = np.stack([synth_frame(W, H, 12345 + f) for f in range(F)])
    d_in = torch.from_numpy(host).to(dev)
    crops = np.random.default_rng(5).integers(0, 256, (CF, CH, CW), dtype=np.uint8)
    d_crops = torch.from_numpy(crops).to(dev)
    for what, d_g, first, (w, h, n) in (("frames 32 x 3840 x 2160", d_in, host[0], (W, H, F)), ("crops 4096 x 64 x 128", d_crops, crops[0], (CW, CH, CF))):
        plan = capi.Plan(ctx, w, h, w, n)
        calls = {
            "moments VALUE, raw": lambda: ctx.moments_frames(d_g.data_ptr(), w, h, w, n, d_raw.data_ptr(), 0, capi.MOMENTS_VALUE, s),
            "histogram": lambda: plan.histogram(d_g.data_ptr(), d_hist.data_ptr(), s),
            "moments UNIT, raw": lambda: ctx.moments_frames(d_g.data_ptr(), w, h, w, n, d_raw.data_ptr(), 0, capi.MOMENTS_UNIT, s),
            "moments VALUE, raw + shape": lambda: ctx.moments_frames(d_g.data_ptr(), w, h, w, n, d_raw.data_ptr(), d_shape.data_ptr(), capi.MOMENTS_VALUE, s),
        }
        for name, weights in (("moments UNIT, raw", mm.UNIT), ("moments VALUE, raw", mm.VALUE)):
            calls[name]()
            torch.cuda.synchronize()
            assert raw_of(0) == mm.raw_sums(first, weights), (what, name)
        res[what] = rows_of(alternately(calls), {name: w * h * n for name in calls})
        plan.close()

    # ---- components: the benchmark's edge maps ----
    line_cap, comp_cap = 1 << 16, 1 << 16
    plan = capi.Plan(ctx, W, H, W, F, 1.0)
    d_e = torch.empty_like(d_in)
    d_lines = torch.zeros(F * line_cap * 20, dtype=torch.uint8, device=dev)
    d_counts = torch.zeros(F, dtype=torch.int32, device=dev)
    d_labels = torch.zeros((F, H, W), dtype=torch.int32, device=dev)
    d_comps = torch.zeros(F * comp_cap * 28, dtype=torch.uint8, device=dev)
    d_cc = torch.zeros(F, dtype=torch.int32, device=dev)
    plan.pipeline(d_in.data_ptr(), 59.0, 119.0, 100, 0, d_e.data_ptr(), d_lines.data_ptr(), line_cap, d_counts.data_ptr())
    plan.components(d_e.data_ptr(), 8, 1, d_labels.data_ptr(), W, d_comps.data_ptr(), comp_cap, d_cc.data_ptr())
    torch.cuda.synchronize()
    cc = d_cc.cpu().numpy()
    assert int(cc.max()) <= comp_cap
    res["components per frame min/max"] = [int(cc.min()), int(cc.max())]

    def comp_call(gray, origin, shape, labels=d_labels, frames=F):
        return lambda: ctx.moments_components(labels.data_ptr(), W, H, W, d_comps.data_ptr(), comp_cap, d_cc.data_ptr(), frames, d_raw.data_ptr(),
                                              d_shape.data_ptr() if shape else 0, d_in.data_ptr() if gray else 0, W, capi.MOMENTS_VALUE, origin, s)
    calls = {
        "no gray, FRAME, raw": comp_call(False, capi.MOMENTS_ORIGIN_FRAME, False),
        "gray VALUE, FRAME, raw": comp_call(True, capi.MOMENTS_ORIGIN_FRAME, False),
        "no gray, BOX, raw": comp_call(False, capi.MOMENTS_ORIGIN_BOX, False),
        "gray VALUE, BOX, raw + shape": comp_call(True, capi.MOMENTS_ORIGIN_BOX, True),
    }
    lab0, recs0 = d_labels[0].cpu().numpy(), np.frombuffer(d_comps[:comp_cap * 28].cpu().numpy().tobytes(), capi.COMP_DTYPE)
    big = int(np.argmax(recs0["pixels"][:int(cc[0])]))          # the component with 87 % of the frame's edge pixels, and the first three
    for name, gray, origin in (("no gray, FRAME, raw", None, mm.ORIGIN_FRAME), ("gray VALUE, BOX, raw + shape", host[0], mm.ORIGIN_BOX)):
        calls[name]()
        torch.cuda.synchronize()
        for cid in (1, 2, 3, big + 1):
            mask = lab0 == cid
            wts = mask.astype(np.int64) if gray is None else gray.astype(np.int64) * mask
            ox, oy = (int(recs0[cid - 1]["x0"]), int(recs0[cid - 1]["y0"])) if origin == mm.ORIGIN_BOX else (0, 0)
            assert raw_of(cid - 1) == mm.weighted_sums(wts, -ox, -oy), (name, cid)
    px = W * H * F
    res["components 32 x 3840 x 2160"] = rows_of(alternately(calls), {name: px * (5 if name.startswith("gray") else 4) for name in calls})
    res["largest component's share of frame 0's edge pixels"] = round(float(recs0["pixels"][big]) / float(recs0["pixels"][:int(cc[0])].sum()), 4)
    # the worst case of the record atomics: one all-foreground frame, a single component of W * H pixels
    d_full = torch.ones((1, H, W), dtype=torch.int32, device=dev)
    d_cc[:1] = 1
    full = alternately({"all-foreground frame, no gray, FRAME, raw": comp_call(False, capi.MOMENTS_ORIGIN_FRAME, False, d_full, 1)})
    torch.cuda.synchronize()
    assert raw_of(0) == mm.weighted_sums(np.ones((H, W), np.int64))
    res["one all-foreground 3840 x 2160 frame"] = rows_of(full, {name: 4 * W * H for name in full})
    # what a host implementation would wait for first
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    d_labels.cpu()
    res["download of the 32 label maps, ms (wall clock, once)"] = round((time.perf_counter() - t0) * 1e3, 1)
    print(json.dumps(res))
    plan.close()
    ctx.close()


if __name__ == "__main__":
    reference_main() if "--reference" in sys.argv[1:] else main()
