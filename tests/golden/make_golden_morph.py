#!/usr/bin/env python
"""Generate tests/golden/golden_morph.json from the COMPILED REFERENCE (oracle/_ref, built by oracle/build_ref.sh): MD5 of the outputs of
CompVMathMorph::process / buildStructuringElement, CompVImageThreshold::global / adaptive and the tap of CompVKernel::mean, on inputs any
box can regenerate (numpy default_rng seeds).  Run in the build container only: it compiles the small shim below (our own code: it only
CALLS the reference's public API) into a temporary directory and links it against oracle/_ref/libcompv_ref.so.  The reference runs on one
thread (refshim_init(1))."""
import ctypes as C
import hashlib, json, os, subprocess, sys, tempfile
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(HERE, ".."))
from oracle_bindings import RefShim  # noqa: E402

SHIM = r"""
#include <compv/base/compv_base.h>
#include <compv/base/compv_kernel.h>
#include <compv/base/compv_mat.h>
#include <compv/base/image/compv_image_threshold.h>
#include <compv/base/math/compv_math_morph.h>
#include <cstring>
using namespace compv;
static COMPV_ERROR_CODE toMat(const uint8_t* in, size_t W, size_t H, size_t S, CompVMatPtr* mat)
{
	COMPV_CHECK_CODE_RETURN(CompVMat::newObjAligned<uint8_t>(mat, H, W, S == W ? 0 : S));          // S == W: the reference's own aligned stride
	for (size_t j = 0; j < H; ++j) memcpy((*mat)->ptr<uint8_t>(j), in + j * S, W);
	return COMPV_ERROR_CODE_S_OK;
}
static void fromMat(const CompVMatPtr& mat, uint8_t* out)
{
	for (size_t j = 0; j < mat->rows(); ++j) memcpy(out + j * mat->cols(), mat->ptr<const uint8_t>(j), mat->cols());
}
extern "C" {
int morphshim_enums(int* v)
{
	v[0] = COMPV_MATH_MORPH_OP_TYPE_ERODE; v[1] = COMPV_MATH_MORPH_OP_TYPE_DILATE; v[2] = COMPV_MATH_MORPH_OP_TYPE_OPEN; v[3] = COMPV_MATH_MORPH_OP_TYPE_CLOSE;
	v[4] = COMPV_MATH_MORPH_STREL_TYPE_RECT; v[5] = COMPV_MATH_MORPH_STREL_TYPE_DIAMOND; v[6] = COMPV_MATH_MORPH_STREL_TYPE_CROSS;
	v[7] = COMPV_BORDER_TYPE_ZERO; v[8] = COMPV_BORDER_TYPE_REPLICATE;
	return 0;
}
int morphshim_strel(int type, size_t w, size_t h, uint8_t* out)
{
	CompVMatPtr s;
	if (COMPV_ERROR_CODE_IS_NOK(CompVMathMorph::buildStructuringElement(&s, CompVSizeSz(w, h), (COMPV_MATH_MORPH_STREL_TYPE)type))) return -1;
	if (s->cols() != w || s->rows() != h) return -2;
	fromMat(s, out);
	return 0;
}
int morphshim_process(const uint8_t* in, size_t W, size_t H, size_t S, const uint8_t* strel, size_t sw, size_t sh, int op, int border, uint8_t* out)
{
	CompVMatPtr img, s, o;
	if (COMPV_ERROR_CODE_IS_NOK(toMat(in, W, H, S, &img))) return -1;
	if (COMPV_ERROR_CODE_IS_NOK(CompVMat::newObjAligned<uint8_t>(&s, sh, sw))) return -1;
	for (size_t j = 0; j < sh; ++j) memcpy(s->ptr<uint8_t>(j), strel + j * sw, sw);
	if (COMPV_ERROR_CODE_IS_NOK(CompVMathMorph::process(img, s, &o, (COMPV_MATH_MORPH_OP_TYPE)op, (COMPV_BORDER_TYPE)border))) return -3;
	if (o->cols() != W || o->rows() != H) return -2;
	fromMat(o, out);
	return 0;
}
int morphshim_global(const uint8_t* in, size_t W, size_t H, size_t S, double threshold, uint8_t* out)
{
	CompVMatPtr img, o;
	if (COMPV_ERROR_CODE_IS_NOK(toMat(in, W, H, S, &img))) return -1;
	if (COMPV_ERROR_CODE_IS_NOK(CompVImageThreshold::global(img, &o, threshold))) return -3;
	fromMat(o, out);
	return 0;
}
int morphshim_adaptive(const uint8_t* in, size_t W, size_t H, size_t S, size_t blockSize, double delta, double maxVal, int invert, uint8_t* out)
{
	CompVMatPtr img, o;
	if (COMPV_ERROR_CODE_IS_NOK(toMat(in, W, H, S, &img))) return -1;
	if (COMPV_ERROR_CODE_IS_NOK(CompVImageThreshold::adaptive(img, &o, blockSize, delta, maxVal, invert != 0))) return -3;
	if (o->cols() != W || o->rows() != H) return -2;
	fromMat(o, out);
	return 0;
}
int morphshim_mean_tap(size_t blockSize)
{
	CompVMatPtr k;
	if (COMPV_ERROR_CODE_IS_NOK(CompVKernel::mean(blockSize, &k))) return -1;
	const uint16_t* p = k->ptr<const uint16_t>();
	for (size_t i = 1; i < blockSize; ++i) if (p[i] != p[0]) return -2;
	return (int)p[0];
}
}
"""

SIZES = ((20, 20, 20), (130, 17, 160), (642, 31, 704))          # W, H, S
STRELS = (("rect", 0, 3, 3), ("rect", 0, 15, 3), ("rect", 0, 1, 5), ("rect", 0, 5, 1), ("cross", 2, 5, 5), ("diamond", 1, 7, 7))   # name, type, w, h
BUILDER = [(t, w, h) for t in (0, 2, 1) for (w, h) in ((1, 1), (3, 3), (7, 7), (31, 5)) if not (t == 1 and w != h)]
OPS = (("erode", 0), ("dilate", 1), ("open", 2), ("close", 3))
BORDERS = (("replicate", 2), ("zero", 0))
THRESHOLDS = (0.0, 0.4, 127.5, 255.0)
BLOCKS, DELTAS, MAXVALS = (3, 15, 31), (0.0, 5.0, 255.0), (255.0, 100.0)


def frame(W, H, S, seed):
    """[H][S] random bytes (padding columns included); the valid region is [:, :W]."""
    return np.random.default_rng(seed).integers(0, 256, size=(H, S), dtype=np.uint8)


def md5(a):
    return hashlib.md5(np.ascontiguousarray(a).tobytes()).hexdigest()


def build_shim(tmp):
    ref = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"          # the default of oracle/build_ref.sh
    src = os.path.join(tmp, "morph_shim.cxx")
    so = os.path.join(tmp, "libmorph_shim.so")
    with open(src, "w") as f:
        f.write(SHIM)
    refdir = os.path.join(ROOT, "oracle", "_ref")
    subprocess.check_call(["g++", "-include", "limits", "-std=c++11", "-O2", "-fPIC", "-w", "-DCOMPV_ASM=0", "-I%s/base/include" % ref, "-shared", "-o", so, src,
                           "-L" + refdir, "-lcompv_ref", "-Wl,-rpath," + refdir, "-ldl", "-lpthread"])
    return C.CDLL(so)


def main():
    RefShim(threads=1)          # refshim_init(1): the reference on one thread
    vp, sz = C.c_void_p, C.c_size_t
    with tempfile.TemporaryDirectory() as tmp:
        L = build_shim(tmp)
        L.morphshim_strel.argtypes = [C.c_int, sz, sz, vp]
        L.morphshim_process.argtypes = [vp, sz, sz, sz, vp, sz, sz, C.c_int, C.c_int, vp]
        L.morphshim_global.argtypes = [vp, sz, sz, sz, C.c_double, vp]
        L.morphshim_adaptive.argtypes = [vp, sz, sz, sz, sz, C.c_double, C.c_double, C.c_int, vp]
        L.morphshim_mean_tap.argtypes = [sz]
        L.morphshim_enums.argtypes = [vp]
        ev = np.zeros(9, np.int32)
        L.morphshim_enums(ev.ctypes.data)
        out = {"enums": dict(zip(("ERODE", "DILATE", "OPEN", "CLOSE", "RECT", "DIAMOND", "CROSS", "BORDER_ZERO", "BORDER_REPLICATE"), map(int, ev))),
               "strel": [], "morph": [], "threshold": [], "adaptive": [], "mean_tap": {}}
        for (t, w, h) in BUILDER:
            s = np.zeros((h, w), np.uint8)
            assert L.morphshim_strel(t, w, h, s.ctypes.data) == 0
            out["strel"].append({"type": t, "w": w, "h": h, "md5": md5(s)})
        seed = 7000
        for (W, H, S) in SIZES:
            for (name, t, w, h) in STRELS:
                s = np.zeros((h, w), np.uint8)
                assert L.morphshim_strel(t, w, h, s.ctypes.data) == 0
                for (opn, op) in OPS:
                    for (bn, b) in BORDERS:
                        seed += 1
                        img = frame(W, H, S, seed)
                        o = np.zeros((H, W), np.uint8)
                        rc = L.morphshim_process(img.ctypes.data, W, H, S, s.ctypes.data, w, h, op, b, o.ctypes.data)
                        out["morph"].append({"W": W, "H": H, "S": S, "seed": seed, "strel": name, "type": t, "sw": w, "sh": h, "op": op, "border": b,
                                             "md5": md5(o) if rc == 0 else None})
            for thr in THRESHOLDS:
                seed += 1
                img = frame(W, H, S, seed)
                o = np.zeros((H, W), np.uint8)
                assert L.morphshim_global(img.ctypes.data, W, H, S, thr, o.ctypes.data) == 0
                out["threshold"].append({"W": W, "H": H, "S": S, "seed": seed, "threshold": thr, "md5": md5(o)})
            for bs in BLOCKS:
                for delta in DELTAS:
                    for mv in MAXVALS:
                        for inv in (0, 1):
                            seed += 1
                            img = frame(W, H, S, seed)
                            o = np.zeros((H, W), np.uint8)
                            # an image smaller than the block is outside the convolution's domain (compv_math_convlt.h:100): not submitted, md5 null
                            rc = L.morphshim_adaptive(img.ctypes.data, W, H, S, bs, delta, mv, inv, o.ctypes.data) if min(W, H) >= bs else -1
                            out["adaptive"].append({"W": W, "H": H, "S": S, "seed": seed, "blockSize": bs, "delta": delta, "maxVal": mv, "invert": inv,
                                                    "md5": md5(o) if rc == 0 else None})
        for bs in range(3, 33, 2):
            out["mean_tap"][str(bs)] = L.morphshim_mean_tap(bs)
    with open(os.path.join(HERE, "golden_morph.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print("wrote", {k: len(v) for k, v in out.items()})


if __name__ == "__main__":
    main()
