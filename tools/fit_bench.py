#!/usr/bin/env python
"""Time compvhip_plan_houghsht_fit on 32 resident 4K benchmark frames (seeds 12345 ..), after one pipeline step (thresholds 59 / 119, SHT
threshold 100), with HIP events via the plan's timing mode: medians of 10 launches after 3 warm-ups, for maxLines in {64, 1024, all}, half
widths 0 / 2 / 8, reading the plan's 1-bit masks and reading the byte edge maps, per line and per segment (minLength 20, maxGap 2).  Prints
per variant the ms per launch, the records, the band pixels summed, and ns per line-chunk (a chunk = 64 positions of one line).

The yardstick is what the call replaces: download the edge maps and the lines, then fit the lines on ONE host core by the same rules.  That
loop is plain C (built with the system compiler into a temporary directory; numpy only carries the buffers), timed on this host in the same
run.
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

CPU_FIT = r"""
#include <stdint.h>
#include <math.h>
typedef struct { float rho, theta; int32_t strength, row, col; } line_t;
typedef struct { int32_t line, pixels; int64_t sx, sy, sxx, sxy, syy; double nx, ny, rho, rms2; } fit_t;
static int64_t fdiv(int64_t a, int64_t b) { int64_t q = a / b; return (a % b != 0 && ((a < 0) != (b < 0))) ? q - 1 : q; }
long fit(const uint8_t* e, int W, int H, int S, const int32_t* sinQ, const int32_t* cosQ, const line_t* ln, int n, int b, fit_t* out)
{
	long pixels = 0;
	for (int i = 0; i < n; ++i) {
		const int64_t s = sinQ[ln[i].col], c = cosQ[ln[i].col], lo = (int64_t)(W + H - ln[i].row - b) * 65536, span = (int64_t)(2 * b + 1) * 65536;
		const int xm = s >= (c < 0 ? -c : c);
		const int N = xm ? W : H, Nm = xm ? H : W;
		const int64_t cp = xm ? c : s, cm = xm ? s : c;
		int64_t k = 0, sp = 0, sm = 0, spp = 0, spm = 0, smm = 0;
		for (int p = 0; p < N; ++p) {
			const int64_t A = lo - p * cp, e0 = fdiv(A, cm), e1 = fdiv(A + span, cm);
			int64_t m0 = (e0 < e1 ? e0 : e1) - 1, m1 = (e0 < e1 ? e1 : e0) + 1;
			if (m0 < 0) m0 = 0;
			if (m1 > Nm - 1) m1 = Nm - 1;
			for (int64_t m = m0; m <= m1; ++m) {
				const int64_t d = m * cm - A;
				if (d >= 0 && d < span && (xm ? e[m * S + p] : e[(int64_t)p * S + m])) { ++k; sp += p; sm += m; spp += (int64_t)p * p; spm += p * m; smm += m * m; }
			}
		}
		fit_t r = { i, (int32_t)k, xm ? sp : sm, xm ? sm : sp, xm ? spp : smm, spm, xm ? smm : spp, 0, 0, 0, 0 };
		const double a = (double)(k * r.sxx - r.sx * r.sx), bb = (double)(k * r.sxy - r.sx * r.sy), cc = (double)(k * r.syy - r.sy * r.sy);
		const double d = a - cc, q = sqrt(d * d + 4.0 * (bb * bb));
		if (k >= 2 && q != 0.0) {
			double u, v;
			if (d >= 0.0) { u = -(2.0 * bb); v = d + q; } else { u = q - d; v = -(2.0 * bb); }
			const double h = sqrt(u * u + v * v);
			double nx = u / h, ny = v / h;
			if (ny < 0.0 || (ny == 0.0 && nx < 0.0)) { nx = -nx; ny = -ny; }
			const double t = (a + cc) - q;
			r.nx = nx; r.ny = ny; r.rho = (nx * (double)r.sx + ny * (double)r.sy) / (double)k; r.rms2 = (t > 0.0 ? t : 0.0) / (2.0 * (double)k * (double)k);
		}
		out[i] = r;
		pixels += k;
	}
	return pixels;
}
"""


def build_cpu_fit(tmp):
    src = os.path.join(tmp, "fit.c")
    with open(src, "w") as f:
        f.write(CPU_FIT)
    so = os.path.join(tmp, "fit.so")
    subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-shared", "-fPIC", src, "-o", so, "-lm"])
    lib = C.CDLL(so)
    lib.fit.restype = C.c_long
    lib.fit.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
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
    d_fits = torch.zeros(F * seg_cap * 80, dtype=torch.uint8, device=dev)
    d_fc = torch.zeros(F, dtype=torch.int32, device=dev)
    plan.pipeline(d_in.data_ptr(), 59.0, 119.0, thr, 0, d_e.data_ptr(), d_lines.data_ptr(), line_cap, d_counts.data_ptr())
    torch.cuda.synchronize()
    counts = d_counts.cpu().numpy()
    lines = d_lines.cpu().numpy().view(capi.LINE_DTYPE).reshape(F, line_cap)
    R, T, step = ctx.houghsht_dims(W, H, theta)
    x_major = np.sin(np.arange(T) * step) >= np.abs(np.cos(np.arange(T) * step))     # close enough to the Q16 rule for counting chunks
    res = {"frames": F, "W": W, "H": H, "minLength": min_length, "maxGap": max_gap, "lines_per_frame": [int(counts.min()), int(counts.max())]}

    def timed(call):
        for _ in range(3):
            call()
        torch.cuda.synchronize()
        plan.set_timing(1)
        ms = []
        for _ in range(10):
            call()
            torch.cuda.synchronize()
            ms.append(dict(plan.get_timing())["sht_fit_kernel"])
        plan.set_timing(0)
        return float(np.median(ms))

    for max_lines in (64, 1024, 0):
        chunks = 0
        for f in range(F):
            n = min(int(counts[f]), line_cap, max_lines or line_cap)
            xm = x_major[lines[f]["col"][:n]]
            chunks += int(xm.sum()) * ((W + 63) // 64) + int((~xm).sum()) * ((H + 63) // 64)
        plan.houghsht_segments(0, d_lines.data_ptr(), d_counts.data_ptr(), line_cap, max_lines, min_length, max_gap, d_segs.data_ptr(), seg_cap, d_sc.data_ptr())
        torch.cuda.synchronize()
        n_segs = int(np.minimum(d_sc.cpu().numpy(), seg_cap).sum())
        for b in (0, 2, 8):
            for how, de in (("masks", 0), ("bytes", d_e.data_ptr())):
                ms = timed(lambda: plan.houghsht_fit(de, d_lines.data_ptr(), d_counts.data_ptr(), line_cap, max_lines, b, 0, 0, 0, d_fits.data_ptr(), seg_cap,
                                                     d_fc.data_ptr()))
                fc = d_fc.cpu().numpy()
                fits = d_fits.cpu().numpy().view(capi.LINE_FIT_DTYPE).reshape(F, seg_cap)
                pixels = int(sum(int(fits[f]["pixels"][:fc[f]].sum()) for f in range(F)))
                res["per line maxLines=%s b=%d %s" % (max_lines or "all", b, how)] = {
                    "ms": round(ms, 4), "records": int(fc.sum()), "band_pixels": pixels, "line_chunks": chunks, "ns_per_line_chunk": round(ms * 1e6 / max(chunks, 1), 2)}
                ms = timed(lambda: plan.houghsht_fit(de, d_lines.data_ptr(), d_counts.data_ptr(), line_cap, max_lines, b, d_segs.data_ptr(), d_sc.data_ptr(), seg_cap,
                                                     d_fits.data_ptr(), seg_cap, d_fc.data_ptr()))
                res["per segment maxLines=%s b=%d %s" % (max_lines or "all", b, how)] = {"ms": round(ms, 4), "records": int(d_fc.cpu().numpy().sum()), "segments": n_segs}
    # the yardstick: download + one-core C fit (tables as the library builds them)
    from oracle_bindings import Oracle
    sinQ, cosQ = Oracle().sht_tables(theta, T)
    with tempfile.TemporaryDirectory() as tmp:
        lib = build_cpu_fit(tmp)
        out = np.zeros(line_cap, capi.LINE_FIT_DTYPE)
        for max_lines in (64, 1024, 0):
            for b in (0, 2, 8):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                h_e = d_e.cpu().numpy()
                h_l = d_lines.cpu().numpy().view(capi.LINE_DTYPE).reshape(F, line_cap)
                h_c = d_counts.cpu().numpy()
                t1 = time.perf_counter()
                total = 0
                walked = F if max_lines == 64 else (2 if max_lines else 1)      # beyond 64 lines per frame two frames (all lines: one) are fitted and the time is scaled to the batch
                for f in range(walked):
                    n = min(int(h_c[f]), line_cap, max_lines or line_cap)
                    ln = np.ascontiguousarray(h_l[f][:n])
                    total += lib.fit(h_e[f].ctypes.data, W, H, W, sinQ.ctypes.data, cosQ.ctypes.data, ln.ctypes.data, n, b, out.ctypes.data)
                t2 = time.perf_counter()
                res["maxLines=%s b=%d cpu_one_core" % (max_lines or "all", b)] = {
                    "download_ms": round((t1 - t0) * 1e3, 1), "fit_ms": round((t2 - t1) * 1e3 * F / walked, 1), "frames_fitted": walked, "band_pixels_in_fitted_frames": int(total)}
    print(json.dumps(res))
    plan.close(); ctx.close()


if __name__ == "__main__":
    main()
