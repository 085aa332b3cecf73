#!/usr/bin/env python
"""Time the brute-force matcher (compvhip_matcher_knn / _good) with HIP events via the matcher's timing mode: medians of 10 calls after 3 warm-ups,
the slice kernel, the merge and the good list (reverse run of the cross check included) apart, for
  32 pairs of 2000 x 2000 and of 500 x 500 rows of 32 bytes, knn 1 and 2, and one shared-train case of 32 pairs of 8000 queries x 500 train rows,
each beside the instruction floor: Q * T * descBytes / 4 XOR + popcount pairs (2 vector instructions per dword and lane) at the VALU rate of the
device -- compute units x 128 lanes x clock, as the runtime reports them (no docs/kernels file records a measured VALU rate) --, and beside the
path the matcher replaces, measured in the same run when oracle/_ref holds the compiled reference: the download of the descriptors, then
CompVMatcherBruteForce on one core (oracle/_ref/headless_samples --match-only Q T: the median of five calls after a first one; it also compares
the record matrices byte for byte)."""
import json
import os
import re
import subprocess
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import numpy as np, torch
from compv_amd import capi

REC = capi.MATCH_DTYPE.itemsize


def timed(m, call, reps=10, warm=3):
    for _ in range(warm):
        call()
    torch.cuda.synchronize()
    m.set_timing(1)
    ms = {}
    for _ in range(reps):
        call()
        torch.cuda.synchronize()
        for n, v in m.get_timing():
            ms.setdefault(n, []).append(v)
    m.set_timing(0)
    return {n: round(float(np.median(v)), 4) for n, v in ms.items()}


def main():
    dev = torch.device("cuda", 0)
    ctx = capi.Context(0)
    props = torch.cuda.get_device_properties(0)
    clock_hz = getattr(props, "clock_rate", 2400000) * 1e3
    lane_ops = props.multi_processor_count * 128 * clock_hz          # vector lane-instructions per second
    res = {"device": props.name, "compute_units": props.multi_processor_count, "clock_GHz": round(clock_hz / 1e9, 3)}
    B = 32
    for (pairs, Q, T, shared) in ((32, 2000, 2000, False), (32, 500, 500, False), (32, 8000, 500, True)):
        g = torch.Generator(device="cpu").manual_seed(Q + T)
        d_query = torch.randint(0, 256, (pairs, Q, B), dtype=torch.uint8, generator=g).to(dev)
        d_train = torch.randint(0, 256, (1 if shared else pairs, T, B), dtype=torch.uint8, generator=g).to(dev)
        floor_ms = pairs * Q * T * (B // 4) * 2 / lane_ops * 1e3
        for knn in (1, 2):
            m = capi.Matcher(ctx, B, Q, T, pairs, knn)
            d_matches = torch.empty(pairs * knn * Q * REC, dtype=torch.uint8, device=dev)
            d_good = torch.empty(pairs * Q * REC, dtype=torch.uint8, device=dev)
            d_gc = torch.zeros(pairs, dtype=torch.int32, device=dev)
            args = (d_query.data_ptr(), B, 0, d_train.data_ptr(), B, 0, shared)
            k = timed(m, lambda: m.knn(*args, d_matches.data_ptr()))
            opts = dict(ratio=0.8 if knn >= 2 else 0.0, max_distance=100, cross_check=True)
            gd = timed(m, lambda: m.good(d_matches.data_ptr(), *args, d_good.data_ptr(), Q, d_gc.data_ptr(), **opts))
            name = "%d pairs %d x %d%s knn %d" % (pairs, Q, T, " shared train" if shared else "", knn)
            res[name] = {"knn_ms": k, "good_ms": gd, "floor_ms": round(floor_ms, 4), "slice_x_floor": round(k["match_slice_kernel"] / floor_ms, 2),
                         "good per pair min/max": [int(d_gc.min()), int(d_gc.max())]}
            m.close()
    # the path the matcher replaces: download + the compiled reference on one core (one pair)
    host = torch.empty((2000, B), dtype=torch.uint8).pin_memory()
    one = torch.zeros((2000, B), dtype=torch.uint8, device=dev)
    dl = []
    for i in range(2 + 5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host.copy_(one)
        torch.cuda.synchronize()
        if i >= 2:
            dl.append((time.perf_counter() - t0) * 1e3)
    res["download_ms (one 2000 x 32 descriptor set, pinned, median of 5)"] = round(float(np.median(dl)), 3)
    exe = os.path.join(ROOT, "oracle", "_ref", "headless_samples")
    for (Q, T) in ((2000, 2000), (500, 500), (8000, 500)):
        key = "reference one core, one pair %d x %d, knn 2, median of 5 calls" % (Q, T)
        if not os.path.exists(exe):
            res[key] = "oracle/_ref not built: not measured"
            continue
        out = subprocess.run([exe, "--match-only", str(Q), str(T)], capture_output=True, text=True, timeout=300).stdout
        mt = re.search(r"bruteforce_matches: (\w+) \[.*CompV CPU ([\d.]+) ms on (\d+) thread.*HIP plugin ([\d.]+) ms", out)
        res[key] = {"records": mt.group(1), "compv_cpu_ms": float(mt.group(2)), "hip_host_form_ms": float(mt.group(4))} if mt else {"error": out[-300:]}
    print(json.dumps(res))
    ctx.close()


if __name__ == "__main__":
    main()
