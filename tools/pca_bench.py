#!/usr/bin/env python
"""Time the PCA projection (compvhip_pca_project) and the mean / covariance (compvhip_pca_covariance) with HIP events: whole-call medians of 7 after 2
warm-ups, one event pair around each call --
  * projection: 4096 x 3780 -> 92 (the HOG descriptors of 4096 crops of 64 x 128), 4096 x 441 -> 92 and 65 536 x 441 -> 92, with the mean;
  * covariance: 100 x 441 and 10 000 x 441 (mean, centre + transpose and the 441 x 441 product in one call);
  * the float32 operations per second the projection achieves, counting 2 per element pair (multiply, add) -- the subtraction of the mean and the fold are
    not counted;
  * beside it the instruction floor, MEASURED in the same run, alternating with the kernel: a bare loop of independent float32 multiplies and adds without
    memory traffic (tools/microbench/pca_f32_floor.hip, built on first use into tools/_libs/; --build-only builds it and stops);
  * traffic: every input, model and output byte once, over the time, as a share of the 6.29 TB/s a float4 copy reaches on an MI355X;
  * 8 rows of every projection shape and the whole 100 x 441 covariance checked against tests/pca_model.py bit for bit;
  * with --reference, where the reference checkout and oracle/_ref are present (the build container): the product of CompVMathPCA::project --
    CompVMath::mulABt on 64 centred rows -- of the compiled reference on ONE core with its own SIMD leaves, through the shim of
    tests/golden/make_golden_pca.py (the copies into its matrices included, reading the model file not), scaled to n.  --no-gpu skips everything else.
Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

import pca_cases as pc
import pca_model as pm

PROJECT = (("n4096_d3780_m92", 4096, 3780, 92), ("n4096_d441_m92", 4096, 441, 92), ("n65536_d441_m92", 65536, 441, 92))
COVARIANCE = (("n100_d441", 100, 441), ("n10000_d441", 10000, 441))
COPY_RATE = 6.29e12          # bytes per second, float4 copy
FLOOR_SRC = os.path.join(ROOT, "tools", "microbench", "pca_f32_floor.hip")
FLOOR_LIB = os.path.join(ROOT, "tools", "_libs", "libpca_f32_floor.so")
FLOOR_BLOCKS, FLOOR_ITERS = 4096, 4096


def build_floor():
    if os.path.exists(FLOOR_LIB) and os.path.getmtime(FLOOR_LIB) >= os.path.getmtime(FLOOR_SRC):
        return
    os.makedirs(os.path.dirname(FLOOR_LIB), exist_ok=True)
    subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", FLOOR_SRC,
                           "-o", FLOOR_LIB])


def model(D, M):
    """HOG-like: a small non-negative mean, vectors of unit scale"""
    return np.abs(pc.uniform((D,), 11 + D)) * np.float32(0.2), pc.uniform((M, D), 12 + D) * np.float32(0.05)


def rows(n, D):
    return np.abs(pc.uniform((n, D), 13 + D)) * np.float32(0.2)


def timed(call, torch, between=None):
    for _ in range(2):
        call()
    torch.cuda.synchronize()
    ms, other = [], []
    for _ in range(7):
        if between:
            other.append(between())          # alternately, in the same run
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), other


def gpu_part(res):
    import torch
    from compv_amd import capi
    build_floor()
    floor = C.CDLL(FLOOR_LIB)
    floor.pca_f32_floor_ms.argtypes = [C.c_void_p, C.c_int, C.c_int]
    floor.pca_f32_floor_ms.restype = C.c_float
    dev = torch.device("cuda", 0)
    ctx = capi.Context(0)
    res["device"] = torch.cuda.get_device_properties(0).name
    d_floor = torch.zeros(FLOOR_BLOCKS * 256, dtype=torch.float32, device=dev)
    floor_ops = FLOOR_BLOCKS * 256 * FLOOR_ITERS * 32 * 2
    floors = []
    for name, n, D, M in PROJECT:
        mean, vectors = model(D, M)
        x = rows(n, D)
        m = capi.PcaModel(mean, vectors).to_device(dev)
        d_x = torch.from_numpy(x).to(dev)
        d_out = torch.zeros(n * M, dtype=torch.float32, device=dev)
        ms, fl = timed(lambda: ctx.pca_project(m, d_x.data_ptr(), n, D, d_out.data_ptr(), M), torch, lambda: floor.pca_f32_floor_ms(d_floor.data_ptr(), FLOOR_BLOCKS, FLOOR_ITERS))
        floors += fl
        nbytes = 4 * (n * D + M * D + D + n * M)
        row = {"project_call_ms": round(ms, 4), "f32_tops": round(2.0 * n * D * M / (ms * 1e-3) / 1e12, 3),
               "floor_f32_tops": round(floor_ops / (float(np.median(fl)) * 1e-3) / 1e12, 3), "bytes": nbytes,
               "share_of_copy_rate": round(nbytes / (ms * 1e-3) / COPY_RATE, 4)}
        row["share_of_floor"] = round(row["f32_tops"] / row["floor_f32_tops"], 3)
        row["bit_exact_8_rows"] = bool(pm.bits(d_out[:8 * M].cpu().numpy().reshape(8, M)).tobytes() == pm.bits(pm.project(x[:8], mean, vectors)).tobytes())
        res[name] = row
    for name, n, D in COVARIANCE:
        obs = rows(n, D) + pc.uniform((1, D), 14) * np.float32(0.1)
        d_obs = torch.from_numpy(np.ascontiguousarray(obs)).to(dev)
        d_mean, d_cov = torch.zeros(D, dtype=torch.float32, device=dev), torch.zeros(D * D, dtype=torch.float32, device=dev)
        d_scratch = torch.zeros(capi.pca_covariance_scratch(n, D) // 4, dtype=torch.float32, device=dev)
        ms, _ = timed(lambda: ctx.pca_covariance(d_obs.data_ptr(), n, D, D, d_mean.data_ptr(), d_cov.data_ptr(), D, d_scratch.data_ptr()), torch)
        nbytes = 4 * (2 * n * D + D + D * D) + 2 * capi.pca_covariance_scratch(n, D)          # the observations twice, the scratch written and read
        row = {"covariance_call_ms": round(ms, 4), "f32_tops": round(2.0 * n * D * D / (ms * 1e-3) / 1e12, 3), "bytes": nbytes,
               "share_of_copy_rate": round(nbytes / (ms * 1e-3) / COPY_RATE, 4)}
        if n <= 100:
            mean, cov = pm.covariance(obs)
            row["bit_exact"] = bool(pm.bits(d_cov.cpu().numpy().reshape(D, D)).tobytes() == pm.bits(cov).tobytes() and pm.bits(d_mean.cpu().numpy()).tobytes() == pm.bits(mean).tobytes())
        res[name] = row
    res["floor_f32_tops_median"] = round(floor_ops / (float(np.median(floors)) * 1e-3) / 1e12, 3)
    res["floor_ms_min_max"] = [round(float(min(floors)), 4), round(float(max(floors)), 4)]
    ctx.close()


def reference_part(res, nq=64):
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_golden_pca as g
    from oracle_bindings import RefShim
    RefShim(threads=1)
    with tempfile.TemporaryDirectory() as tmp:
        L = g.build_shim(tmp)
        assert L.pcashim_flags(1) == 0          # the reference as its users run it: its own SIMD leaves
        for name, n, D, M in PROJECT:
            mean, vectors = model(D, M)
            x = np.ascontiguousarray(rows(nq, D))
            # mulABt on the centred rows: what project does behind reading the model (the subtraction is not timed)
            c = np.ascontiguousarray(pm.centre(x, mean))
            out = np.zeros((nq, M), np.float32)
            best = 1e30
            for _ in range(3):
                t0 = time.perf_counter()
                assert L.pcashim_mulabt(c.ctypes.data, nq, vectors.ctypes.data, M, D, out.ctypes.data) == 0
                best = min(best, time.perf_counter() - t0)
            row = res.setdefault(name, {})
            row["reference_ms_per_row_one_core"] = round(best * 1e3 / nq, 4)
            row["reference_s_for_n_one_core"] = round(best / nq * n, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", action="store_true")
    ap.add_argument("--no-gpu", action="store_true")
    ap.add_argument("--build-only", action="store_true")
    a = ap.parse_args()
    if a.build_only:
        build_floor()
        return
    res = {}
    if not a.no_gpu:
        gpu_part(res)
    if a.reference:
        reference_part(res)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
