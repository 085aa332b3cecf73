#!/usr/bin/env python
"""Time SVM prediction (compvhip_svm_*) with HIP events: medians of 7 calls after 2 warm-ups, float32 queries, two classes, for
N = 4096, D = 3780 with L = 256 and 1024 (the HOG descriptors of 4096 crops of 64 x 128) and N = 4096, D = 324 with L = 1024, RBF and LINEAR --
  * both kernels apart (the handle's timing mode) and the whole predict call (one event pair around it, timing mode off);
  * the float64 operations per second svm_kvalues_kernel achieves, counting 3 per element pair for RBF (subtract, multiply, add) and 2 for LINEAR;
  * beside it the instruction floor, MEASURED in the same run, alternating with the kernel: a bare loop of independent float64 multiplies and adds without
    memory traffic (tools/microbench/svm_f64_floor.hip, built on first use into tools/_libs/; --build-only builds it and stops);
  * 8 queries of every shape checked against tests/svm_model.py bit for bit;
  * with --reference, where the reference checkout and oracle/_ref are present (the build container): svm_predict_values of the compiled reference on ONE
    core with its own SIMD leaves, 8 queries per shape through the shim of tests/golden/make_golden_svm.py, scaled to N.  --no-gpu skips everything else.
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

import svm_model as sm

N = 4096
SHAPES = (("n4096_d3780_l256", 3780, 256), ("n4096_d3780_l1024", 3780, 1024), ("n4096_d324_l1024", 324, 1024))
KERNELS = (("rbf", sm.RBF), ("linear", sm.LINEAR))
FLOOR_SRC = os.path.join(ROOT, "tools", "microbench", "svm_f64_floor.hip")
FLOOR_LIB = os.path.join(ROOT, "tools", "_libs", "libsvm_f64_floor.so")
FLOOR_BLOCKS, FLOOR_ITERS = 4096, 4096


def build_floor():
    if os.path.exists(FLOOR_LIB) and os.path.getmtime(FLOOR_LIB) >= os.path.getmtime(FLOOR_SRC):
        return
    os.makedirs(os.path.dirname(FLOOR_LIB), exist_ok=True)
    subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", FLOOR_SRC,
                           "-o", FLOOR_LIB])


def make_model(kernel, D, L, seed=1):
    rng = np.random.RandomState(seed + D + L)
    sv = rng.uniform(0.0, 0.2, (L, D)).astype(np.float32).astype(np.float64)          # HOG-like: small non-negative values
    coef = rng.uniform(-1.0, 1.0, (1, L))
    return sm.Model(kernel, 1.0 / D, sv, coef, [0.125], [L // 2, L - L // 2], [1, -1])


def queries(D, n=N, seed=2):
    return np.random.RandomState(seed + D).uniform(0.0, 0.2, (n, D)).astype(np.float32)


def gpu_part(res):
    import torch
    from compv_amd import capi
    build_floor()
    floor = C.CDLL(FLOOR_LIB)
    floor.svm_f64_floor_ms.argtypes = [C.c_void_p, C.c_int, C.c_int]
    floor.svm_f64_floor_ms.restype = C.c_float
    dev = torch.device("cuda", 0)
    ctx = capi.Context(0)
    res["device"] = torch.cuda.get_device_properties(0).name
    d_floor = torch.zeros(FLOOR_BLOCKS * 256, dtype=torch.float64, device=dev)
    floor_ops = FLOOR_BLOCKS * 256 * FLOOR_ITERS * 16 * 2
    floors = []
    for name, D, L in SHAPES:
        X = queries(D)
        d_x = torch.from_numpy(X).to(dev)
        d_lab = torch.zeros(N, dtype=torch.int32, device=dev)
        d_dec = torch.zeros(N, dtype=torch.float64, device=dev)
        d_k = torch.zeros(N * L, dtype=torch.float64, device=dev)
        for kname, kernel in KERNELS:
            m = make_model(kernel, D, L)
            h = capi.Svm(ctx, capi.SvmModel(m.kernel, m.gamma, m.sv, m.sv_coef, m.rho, m.n_sv, m.label), N)

            def call(kv=0):
                h.predict(d_x.data_ptr(), capi.SVM_F32, N, D, d_lab.data_ptr(), d_dec.data_ptr(), kv)
            for _ in range(2):
                call()
            torch.cuda.synchronize()
            ms, whole, fl = {}, [], []
            for _ in range(7):
                h.set_timing(1)
                call()
                torch.cuda.synchronize()
                for n_, v in h.get_timing():
                    ms.setdefault(n_, []).append(v)
                h.set_timing(0)
                fl.append(floor.svm_f64_floor_ms(d_floor.data_ptr(), FLOOR_BLOCKS, FLOOR_ITERS))          # alternately, in the same run
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                call()
                b.record()
                torch.cuda.synchronize()
                whole.append(a.elapsed_time(b))
            row = {n_: round(float(np.median(v)), 4) for n_, v in ms.items()}
            row["predict_call_ms"] = round(float(np.median(whole)), 4)
            ops = N * L * D * (3 if kernel == sm.RBF else 2)
            row["kvalues_f64_tops"] = round(ops / (row["svm_kvalues_kernel"] * 1e-3) / 1e12, 3)
            row["floor_f64_tops"] = round(floor_ops / (float(np.median(fl)) * 1e-3) / 1e12, 3)
            row["share_of_floor"] = round(row["kvalues_f64_tops"] / row["floor_f64_tops"], 3)
            floors += fl
            call(d_k.data_ptr())
            torch.cuda.synchronize()
            labels, dec, K = sm.predict(m, X[:8])
            row["bit_exact_8_queries"] = bool(d_k[:8 * L].cpu().numpy().tobytes() == K.tobytes() and d_dec[:8].cpu().numpy().tobytes() == dec.tobytes()
                                              and d_lab[:8].cpu().numpy().tobytes() == labels.tobytes())
            res.setdefault(name, {})[kname] = row
            h.close()
    res["floor_f64_tops_median"] = round(floor_ops / (float(np.median(floors)) * 1e-3) / 1e12, 3)
    res["floor_ms_min_max"] = [round(float(min(floors)), 4), round(float(max(floors)), 4)]
    ctx.close()


def reference_part(res, nq=8):
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_golden_svm as g
    from oracle_bindings import RefShim
    RefShim(threads=1)
    with tempfile.TemporaryDirectory() as tmp:
        L_ = g.build_shim(tmp, plain_c=False)          # the reference as its users run it: its own SIMD leaves
        for name, D, L in SHAPES:
            X = queries(D, nq).astype(np.float64)
            for kname, kernel in KERNELS:
                m = make_model(kernel, D, L)
                path = os.path.join(tmp, "bench.model")
                sm.write_model_file(path, kernel, "%g" % m.gamma, [["%.8g" % v for v in r] for r in m.sv], [["%.16g" % v for v in r] for r in m.sv_coef], ["0.125"],
                                    m.n_sv.tolist(), m.label.tolist())
                t = g.reference_time(L_, path, X)
                row = res.setdefault(name, {}).setdefault(kname, {})
                row["reference_ms_per_query_one_core"] = round(t * 1e3 / nq, 3)
                row["reference_s_for_4096_one_core"] = round(t / nq * N, 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", action="store_true")
    ap.add_argument("--no-gpu", action="store_true")
    ap.add_argument("--build-only", action="store_true")
    a = ap.parse_args()
    if a.build_only:
        build_floor()
        return
    res = {"n": N}
    if not a.no_gpu:
        gpu_part(res)
    if a.reference:
        reference_part(res)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
