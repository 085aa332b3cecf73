#!/usr/bin/env python
"""Time compvhip_plan_houghsht_segments on 32 resident 4K benchmark frames (seeds 12345 ..), after one pipeline step, with HIP events via
the plan's timing mode: the count walk, the per-frame scan and the write walk, for maxLines in {64, 1024, all}, reading the plan's 1-bit
masks and reading the byte edge maps.  Prints per variant the ms per launch, ns per line-chunk (a chunk = 64 positions of one line, walked
twice) and the mask-read rate on REQUESTED bytes (one 4-byte word -- or one byte -- per lane, chunk and walk: what the lanes ask for, not what
the caches fetch).

The yardstick is what the call replaces: download the edge maps and the lines, then walk the lines on ONE host core.  That loop is plain C
(built with the system compiler into a temporary directory; numpy only carries the buffers), timed on this host in the same run.
"""
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import numpy as np, torch
from compv_amd import capi
from oracle_bindings import synth_frame

CPU_WALK = r"""
#include <stdint.h>
typedef struct { float rho, theta; int32_t strength, row, col; } line_t;
typedef struct { int32_t line, x0, y0, x1, y1, support; } seg_t;
static int64_t fdiv(int64_t a, int64_t b) { int64_t q = a / b; return (a % b != 0 && ((a < 0) != (b < 0))) ? q - 1 : q; }
long walk(const uint8_t* e, int W, int H, int S, const int32_t* sinQ, const int32_t* cosQ, const line_t* ln, int n, int minLength, int maxGap, seg_t* out, long cap)
{
	long found = 0;
	for (int i = 0; i < n; ++i) {
		const int64_t s = sinQ[ln[i].col], c = cosQ[ln[i].col], rhoQ = (int64_t)(W + H - ln[i].row) * 65536;
		const int xm = s >= (c < 0 ? -c : c);
		const int N = xm ? W : H, Nm = xm ? H : W;
		const int64_t cp = xm ? c : s, cm = xm ? s : c;
		int open = 0, p0 = 0, last = 0, sup = 0, p0m = 0, lastM = 0;
		for (int p = 0; p <= N; ++p) {
			int cnt = 0, mf = 0;
			if (p < N) {
				const int64_t A = rhoQ - p * cp, est = fdiv(A, cm);
				for (int k = -1; k <= 2; ++k) {
					const int64_t m = est + k, d = m * cm - A;
					if (d >= 0 && d < 65536 && m >= 0 && m < Nm && (xm ? e[m * S + p] : e[(int64_t)p * S + m])) { if (!cnt) mf = (int)m; ++cnt; }
				}
			}
			if (open && (p == N || (cnt && p - last - 1 > maxGap))) {
				if (last - p0 + 1 >= minLength) {
					if (found < cap) { seg_t g = { i, xm ? p0 : p0m, xm ? p0m : p0, xm ? last : lastM, xm ? lastM : last, sup }; out[found] = g; }
					++found;
				}
				open = 0;
			}
			if (cnt) {
				if (!open) { open = 1; p0 = p; p0m = mf; sup = 0; }
				sup += cnt; last = p; lastM = mf;
			}
		}
	}
	return found;
}
"""


def build_cpu_walk(tmp):
    src = os.path.join(tmp, "walk.c")
    with open(src, "w") as f:
        f.write(CPU_WALK)
    so = os.path.join(tmp, "walk.so")
    subprocess.check_call(["gcc", "-O2", "-shared", "-fPIC", src, "-o", so])
    lib = C.CDLL(so)
    lib.walk.restype = C.c_long
    lib.walk.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_long]
    return lib


def main():
    W, H, F, theta, thr = 3840, 2160, 32, 1.0, 100
    min_length, max_gap = 20, 2
    line_cap, seg_cap = 1 << 16, 1 << 17
    dev = torch.device("cuda", 0)
    ctx = capi.Context(0)
    plan = capi.Plan(ctx, W, H, W, F, theta)
    d_in = torch.stack([torch.from_numpy(synth_frame(W, H, 12345 + f)) for f in range(F)]).to(dev)
    d_e = torch.empty_like(d_in)
    d_lines = torch.zeros(F * line_cap * 20, dtype=torch.uint8, device=dev)
    d_counts = torch.zeros(F, dtype=torch.int32, device=dev)
    d_segs = torch.zeros(F * seg_cap * 24, dtype=torch.uint8, device=dev)
    d_sc = torch.zeros(F, dtype=torch.int32, device=dev)
    plan.pipeline(d_in.data_ptr(), 59.0, 119.0, thr, 0, d_e.data_ptr(), d_lines.data_ptr(), line_cap, d_counts.data_ptr())
    torch.cuda.synchronize()
    counts = d_counts.cpu().numpy()
    lines = d_lines.cpu().numpy().view(capi.LINE_DTYPE).reshape(F, line_cap)
    R, T, step = ctx.houghsht_dims(W, H, theta)
    x_major = np.sin(np.arange(T) * step) >= np.abs(np.cos(np.arange(T) * step))     # close enough to the Q16 rule for counting chunks
    res = {"frames": F, "W": W, "H": H, "minLength": min_length, "maxGap": max_gap, "lines_per_frame": [int(counts.min()), int(counts.max())]}
    for max_lines in (64, 1024, 0):
        chunks = 0
        for f in range(F):
            n = min(int(counts[f]), line_cap, max_lines or line_cap)
            xm = x_major[lines[f]["col"][:n]]
            chunks += int(xm.sum()) * ((W + 63) // 64) + int((~xm).sum()) * ((H + 63) // 64)
        for how, de in (("masks", 0), ("bytes", d_e.data_ptr())):
            def call():
                plan.houghsht_segments(de, d_lines.data_ptr(), d_counts.data_ptr(), line_cap, max_lines, min_length, max_gap, d_segs.data_ptr(), seg_cap,
                                       d_sc.data_ptr())
            for _ in range(3):
                call()
            torch.cuda.synchronize()
            plan.set_timing(1)
            ms = {}
            for _ in range(10):
                call()
                torch.cuda.synchronize()
                for n, m in plan.get_timing():
                    ms.setdefault(n, []).append(m)
            plan.set_timing(0)
            med = {n: float(np.median(v)) for n, v in ms.items()}
            walks = med["sht_segments_count_kernel"] + med["sht_segments_write_kernel"]
            res["maxLines=%s %s" % (max_lines or "all", how)] = {
                "ms": {n: round(v, 4) for n, v in med.items()}, "ms_total": round(sum(med.values()), 4), "segments": int(d_sc.cpu().numpy().sum()),
                "line_chunks": chunks, "ns_per_line_chunk": round(walks * 1e6 / max(2 * chunks, 1), 2),
                "requested_GB/s": round(2 * chunks * 64 * (4 if how == "masks" else 1) / (walks * 1e-3) / 1e9, 1)}
    # the yardstick: download + one-core C walk (tables as the library builds them: float32 running angle, libm sinf / cosf)
    from oracle_bindings import Oracle
    sinQ, cosQ = Oracle().sht_tables(theta, T)
    with tempfile.TemporaryDirectory() as tmp:
        lib = build_cpu_walk(tmp)
        out = np.zeros(seg_cap, capi.SEGMENT_DTYPE)
        for max_lines in (64, 1024, 0):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            h_e = d_e.cpu().numpy()
            h_l = d_lines.cpu().numpy().view(capi.LINE_DTYPE).reshape(F, line_cap)
            h_c = d_counts.cpu().numpy()
            t1 = time.perf_counter()
            total = 0
            walked = F if max_lines else 2          # every line of a frame: two frames are walked and the time is scaled to the batch
            for f in range(walked):
                n = min(int(h_c[f]), line_cap, max_lines or line_cap)
                ln = np.ascontiguousarray(h_l[f][:n])
                total += lib.walk(h_e[f].ctypes.data, W, H, W, sinQ.ctypes.data, cosQ.ctypes.data, ln.ctypes.data, n, min_length, max_gap, out.ctypes.data, seg_cap)
            t2 = time.perf_counter()
            res["maxLines=%s cpu_one_core" % (max_lines or "all")] = {"download_ms": round((t1 - t0) * 1e3, 1), "walk_ms": round((t2 - t1) * 1e3 * F / walked, 1), "frames_walked": walked,
                                                                     "segments_in_walked_frames": int(total)}
    print(json.dumps(res))
    plan.close(); ctx.close()


if __name__ == "__main__":
    main()
