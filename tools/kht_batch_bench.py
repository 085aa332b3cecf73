"""Batched KHT (compvhip_plan_houghkht) on one 32-frame 4K batch: ms per frame against the number of host workers.
--order canonical times compvhip_plan_houghkht_ex in the canonical line order (peaks found and sorted on the GPU) on the same batch."""
import argparse, os, sys, time, json
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
ap = argparse.ArgumentParser()
ap.add_argument("threads", nargs="*", type=int, help="host worker counts (default: 4 8 16 24 32 48)")
ap.add_argument("--order", choices=["reference", "canonical"], default="reference")
ap.add_argument("--reps", type=int, default=3, help="timed calls per worker count")
args = ap.parse_args()
import torch
import bench
from compv_amd import capi
W, H, F = 3840, 2160, 32
dev = torch.device("cuda:0")
synth = bench.FrameSynth(torch, dev, W, H)
d_in = synth.batch([12345 + f for f in range(F)])
d_e = torch.empty_like(d_in)
ctx = capi.Context(0); plan = capi.Plan(ctx, W, H, W, F, 1.0)
plan.canny(d_in.data_ptr(), 59.0, 119.0, d_e.data_ptr()); torch.cuda.synchronize()
out = {}
for threads in args.threads or [4, 8, 16, 24, 32, 48]:
    plan.houghkht(d_e.data_ptr(), 1.0, 1.0, 1, threads=threads, order=args.order)
    ts = []
    for _ in range(args.reps):
        t0 = time.perf_counter(); plan.houghkht(d_e.data_ptr(), 1.0, 1.0, 1, threads=threads, order=args.order); ts.append((time.perf_counter() - t0) * 1e3 / F)
    st = plan.houghkht_stage_ms()
    out[threads] = {"order": args.order, "ms_per_frame": [round(t, 3) for t in ts], "stages": st["stages"], "host_share": st["host_share"]}
    print(threads, out[threads], flush=True)
