#!/usr/bin/env python
"""Generate tests/golden/golden_fast.json from the COMPILED REFERENCE (oracle/_ref, built by oracle/build_ref.sh): corner count and MD5 of
the (x, y, strength) int32 triples CompVCornerDeteFAST::process returns, on inputs any box can regenerate (tests/fast_model.py: numpy
default_rng seeds).  Run in the build container only: it compiles the small shim below (our own code: it only CALLS the reference's public
API -- CompVCornerDete::newObj(COMPV_FAST_ID), set, process) into a temporary directory and links it against oracle/_ref/libcompv_ref.so.
The reference runs on one thread (refshim_init(1)), and every case gets a fresh detector: the reference's detector keeps its score map
between frames of equal stride.

Per case the file also holds the reference's maxFeatures = 50 output as a sorted strength list: which corners of a tie survive its
nth_element is unspecified, so only the strengths are recorded."""
import ctypes as C
import hashlib, json, os, subprocess, sys, tempfile
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(HERE, ".."))
from oracle_bindings import RefShim  # noqa: E402
import fast_model as fm  # noqa: E402

SHIM = r"""
#include <compv/base/compv_base.h>
#include <compv/base/compv_features.h>
#include <compv/base/compv_mat.h>
#include <compv/base/image/compv_image.h>
#include <cstring>
using namespace compv;
extern "C" {
int fastshim_enums(int* v)
{
	v[0] = COMPV_FAST_ID; v[1] = COMPV_FAST_TYPE_9; v[2] = COMPV_FAST_TYPE_12;
	return 0;
}
// -> number of corners (all of them, whatever `cap`), or < 0; the first min(n, cap) triples go to out
long fastshim_process(const uint8_t* in, size_t W, size_t H, size_t S, int threshold, int N, int nonmax, int maxFeatures, int32_t* out, size_t cap)
{
	CompVMatPtr img;
	// S == W: the reference's own aligned stride, as its callers get it.  On a stride that is no multiple of its scan width (8, 16 or 32 bytes) the
	// reference's point builder runs past the end of a row into the next one and reports points with x >= W.
	if (COMPV_ERROR_CODE_IS_NOK(CompVImage::newObj8u(&img, COMPV_SUBTYPE_PIXELS_Y, W, H, S == W ? 0 : S))) return -1;
	if (S != W && img->stride() != S) return -2;
	for (size_t j = 0; j < H; ++j) memcpy(img->ptr<uint8_t>(j), in + j * S, S == W ? W : S);
	CompVCornerDetePtr dete;
	if (COMPV_ERROR_CODE_IS_NOK(CompVCornerDete::newObj(&dete, COMPV_FAST_ID))) return -3;
	const int type = N == 9 ? COMPV_FAST_TYPE_9 : COMPV_FAST_TYPE_12;
	const bool nms = nonmax != 0;
	if (COMPV_ERROR_CODE_IS_NOK(dete->set(COMPV_FAST_SET_INT_THRESHOLD, &threshold, sizeof(threshold)))) return -4;
	if (COMPV_ERROR_CODE_IS_NOK(dete->set(COMPV_FAST_SET_INT_FAST_TYPE, &type, sizeof(type)))) return -4;
	if (COMPV_ERROR_CODE_IS_NOK(dete->set(COMPV_FAST_SET_INT_MAX_FEATURES, &maxFeatures, sizeof(maxFeatures)))) return -4;
	if (COMPV_ERROR_CODE_IS_NOK(dete->set(COMPV_FAST_SET_BOOL_NON_MAXIMA_SUPP, &nms, sizeof(nms)))) return -4;
	CompVInterestPointVector pts;
	if (COMPV_ERROR_CODE_IS_NOK(dete->process(img, pts))) return -5;
	for (size_t i = 0; i < pts.size() && i < cap; ++i) {
		out[3 * i] = (int32_t)pts[i].x; out[3 * i + 1] = (int32_t)pts[i].y; out[3 * i + 2] = (int32_t)pts[i].strength;
	}
	return (long)pts.size();
}
}
"""

SIZES = ((7, 7, 7), (20, 20, 20), (130, 17, 160), (642, 31, 704), (200, 258, 200))          # W, H, S
TYPES, NMS, THRESHOLDS = (9, 12), (1, 0), (1, 20, 100)
CONTENT = ("noise", "blocks")
CUT = 50


def frame(kind, W, H, S, seed):
    """[H][S]: the valid region [:, :W] from fast_model, the padding columns random"""
    out = np.random.default_rng(seed + 500000).integers(0, 256, size=(H, S), dtype=np.uint8)
    out[:, :W] = fm.noise(W, H, seed) if kind == "noise" else fm.blocks(W, H, seed)
    return out


def build_shim(tmp):
    ref = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"          # the default of oracle/build_ref.sh
    src = os.path.join(tmp, "fast_shim.cxx")
    so = os.path.join(tmp, "libfast_shim.so")
    with open(src, "w") as f:
        f.write(SHIM)
    refdir = os.path.join(ROOT, "oracle", "_ref")
    subprocess.check_call(["g++", "-include", "limits", "-std=c++11", "-O2", "-fPIC", "-w", "-DCOMPV_ASM=0", "-I%s/base/include" % ref, "-I%s/core/include" % ref,
                           "-shared", "-o", so, src, "-L" + refdir, "-lcompv_ref", "-Wl,-rpath," + refdir, "-ldl", "-lpthread"])
    return C.CDLL(so)


def run(L, img, W, H, S, t, N, nonmax, max_features):
    cap = W * H
    buf = np.zeros(3 * cap, np.int32)
    n = L.fastshim_process(img.ctypes.data, W, H, S, t, N, nonmax, max_features, buf.ctypes.data, cap)
    assert 0 <= n <= cap, n
    return buf[:3 * n].reshape(n, 3)


def main():
    RefShim(threads=1)          # refshim_init(1): the reference on one thread
    vp, sz, i = C.c_void_p, C.c_size_t, C.c_int
    with tempfile.TemporaryDirectory() as tmp:
        L = build_shim(tmp)
        L.fastshim_process.argtypes = [vp, sz, sz, sz, i, i, i, i, vp, sz]
        L.fastshim_process.restype = C.c_long
        L.fastshim_enums.argtypes = [vp]
        ev = np.zeros(3, np.int32)
        L.fastshim_enums(ev.ctypes.data)
        out = {"enums": dict(zip(("FAST_ID", "FAST_TYPE_9", "FAST_TYPE_12"), map(int, ev))), "cut": CUT, "cases": []}
        # one literal of tests/test_fast_model.py put to the reference: a lone pixel of 200 on black, t = 20 -- the pixel itself is a corner
        lone = np.zeros((9, 16), np.uint8)
        lone[4, 5] = 200
        out["lone"] = run(L, lone, 11, 9, 16, 20, 9, 1, -1).tolist()
        seed = 9000
        for (W, H, S) in SIZES:
            for kind in CONTENT:
                for N in TYPES:
                    for nonmax in NMS:
                        for t in THRESHOLDS:
                            seed += 1
                            img = frame(kind, W, H, S, seed)
                            full = run(L, img, W, H, S, t, N, nonmax, -1)
                            best = run(L, img, W, H, S, t, N, nonmax, CUT)
                            out["cases"].append({"W": W, "H": H, "S": S, "seed": seed, "content": kind, "N": N, "nonmax": nonmax, "threshold": t,
                                                 "count": int(len(full)), "md5": hashlib.md5(np.ascontiguousarray(full, "<i4").tobytes()).hexdigest(),
                                                 "cut_strengths": sorted(int(v) for v in best[:, 2])})
    with open(os.path.join(HERE, "golden_fast.json"), "w") as f:
        json.dump(out, f, indent=None, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    print("wrote %d cases, %d corners in all" % (len(out["cases"]), sum(c["count"] for c in out["cases"])))


if __name__ == "__main__":
    main()
