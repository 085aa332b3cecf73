#!/usr/bin/env python
"""Generate tests/golden/golden_stats.json (+ golden_stats.npz) from tests/stats_model.py, held against the COMPILED REFERENCE (oracle/_ref, built by
oracle/build_ref.sh).  Run in the build container only: it compiles the small shim below (our own code: it only CALLS CompVImage::integral,
histogramBuild, both histogramEqualiz overloads, histogramBuildProjectionX and histogramBuildProjectionY) into a temporary directory and links it
against oracle/_ref/libcompv_ref.so.  The reference runs on one thread.

Every case of tests/stats_cases.py is run twice: with the reference's CPU flags as they are, and with SSE2, SSSE3 and AVX2 switched off
(CompVCpu::flagsDisable: the projections have SSE2 leaves).  Asserted in BOTH runs before anything is written: every model array == the reference's, byte
for byte.  Equalisation: the frame's own histogram (first overload) and a caller's (second overload), default scale; every v of these tables is below
256, where the reference's conversion is defined.  The clamped arm (scale 1.0) is the model's alone and is stored with the others.
Stored: an MD5 of every array of every case, the arrays themselves for frames of up to stats_cases.STORE_LIMIT pixels."""
import ctypes as C
import hashlib
import json, os, subprocess, sys, tempfile
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(HERE, ".."))
from oracle_bindings import RefShim  # noqa: E402
import stats_model as sm  # noqa: E402
import stats_cases as sc  # noqa: E402

SHIM = r"""
#include <compv/base/compv_base.h>
#include <compv/base/compv_cpu.h>
#include <compv/base/compv_mat.h>
#include <compv/base/image/compv_image.h>
#include <cstring>
using namespace compv;
static bool frame(CompVMatPtr& img, const uint8_t* gray, size_t W, size_t H, size_t S)
{
	if (COMPV_ERROR_CODE_IS_NOK(CompVImage::newObj8u(&img, COMPV_SUBTYPE_PIXELS_Y, W, H))) return false;
	for (size_t j = 0; j < H; ++j) memcpy(img->ptr<uint8_t>(j), gray + j * S, W);
	return true;
}
extern "C" {
int statshim_simd(int on)
{
	const uint64_t flags = kCpuFlagSSE2 | kCpuFlagSSSE3 | kCpuFlagAVX2;
	return COMPV_ERROR_CODE_IS_NOK(on ? CompVCpu::flagsEnable(flags) : CompVCpu::flagsDisable(flags)) ? -1 : 0;
}
// sum, sumsq: dense (H + 1) x (W + 1)
int statshim_integral(const uint8_t* gray, size_t W, size_t H, size_t S, double* sum, double* sumsq)
{
	CompVMatPtr img, s, q;
	if (!frame(img, gray, W, H, S)) return -1;
	if (COMPV_ERROR_CODE_IS_NOK(CompVImage::integral(img, &s, &q))) return -2;
	if (s->rows() != H + 1 || s->cols() != W + 1 || q->rows() != H + 1 || q->cols() != W + 1) return -3;
	for (size_t j = 0; j <= H; ++j) {
		memcpy(sum + j * (W + 1), s->ptr<const compv_float64_t>(j), (W + 1) * sizeof(double));
		memcpy(sumsq + j * (W + 1), q->ptr<const compv_float64_t>(j), (W + 1) * sizeof(double));
	}
	return 0;
}
int statshim_histogram(const uint8_t* gray, size_t W, size_t H, size_t S, uint32_t* hist)
{
	CompVMatPtr img, h;
	if (!frame(img, gray, W, H, S)) return -1;
	if (COMPV_ERROR_CODE_IS_NOK(CompVImage::histogramBuild(img, &h))) return -2;
	if (h->cols() != 256) return -3;
	memcpy(hist, h->ptr<const uint32_t>(), 256 * sizeof(uint32_t));
	return 0;
}
// hist == NULL: the first overload (the frame's own histogram); out: dense H x W
int statshim_equalize(const uint8_t* gray, size_t W, size_t H, size_t S, const uint32_t* hist, double scale, uint8_t* out)
{
	CompVMatPtr img, h, o;
	if (!frame(img, gray, W, H, S)) return -1;
	if (hist) {
		if (COMPV_ERROR_CODE_IS_NOK(CompVMat::newObjAligned<uint32_t>(&h, 1, 256))) return -1;
		memcpy(h->ptr<uint32_t>(), hist, 256 * sizeof(uint32_t));
		if (COMPV_ERROR_CODE_IS_NOK(CompVImage::histogramEqualiz(img, h, &o, scale))) return -2;
	}
	else if (COMPV_ERROR_CODE_IS_NOK(CompVImage::histogramEqualiz(img, &o, scale))) return -2;
	if (o->cols() != W || o->rows() != H) return -3;
	for (size_t j = 0; j < H; ++j) memcpy(out + j * W, o->ptr<const uint8_t>(j), W);
	return 0;
}
int statshim_projections(const uint8_t* gray, size_t W, size_t H, size_t S, int32_t* projX, int32_t* projY)
{
	CompVMatPtr img, x, y;
	if (!frame(img, gray, W, H, S)) return -1;
	if (COMPV_ERROR_CODE_IS_NOK(CompVImage::histogramBuildProjectionX(img, &x))) return -2;
	if (COMPV_ERROR_CODE_IS_NOK(CompVImage::histogramBuildProjectionY(img, &y))) return -2;
	if (x->cols() != W || y->cols() != H) return -3;
	memcpy(projX, x->ptr<const int32_t>(), W * sizeof(int32_t));
	memcpy(projY, y->ptr<const int32_t>(), H * sizeof(int32_t));
	return 0;
}
}
"""


def build_shim(tmp, ref="/root/reference"):          # the default of oracle/build_ref.sh
    src = os.path.join(tmp, "stats_shim.cxx")
    so = os.path.join(tmp, "libstats_shim.so")
    with open(src, "w") as f:
        f.write(SHIM)
    refdir = os.path.join(ROOT, "oracle", "_ref")
    subprocess.check_call(["g++", "-include", "limits", "-std=c++11", "-O2", "-fPIC", "-w", "-DCOMPV_ASM=0", "-I%s/base/include" % ref, "-shared", "-o", so, src,
                           "-L" + refdir, "-lcompv_ref", "-Wl,-rpath," + refdir, "-ldl", "-lpthread"])
    L = C.CDLL(so)
    vp, sz = C.c_void_p, C.c_size_t
    L.statshim_simd.argtypes = [C.c_int]
    L.statshim_integral.argtypes = [vp, sz, sz, sz, vp, vp]
    L.statshim_histogram.argtypes = [vp, sz, sz, sz, vp]
    L.statshim_equalize.argtypes = [vp, sz, sz, sz, vp, C.c_double, vp]
    L.statshim_projections.argtypes = [vp, sz, sz, sz, vp, vp]
    return L


def reference(L, img, hist):
    """what the compiled reference gives for one frame, with the CPU flags as statshim_simd left them; keys as model_arrays()"""
    img = np.ascontiguousarray(img, np.uint8)
    H, W = img.shape
    g = (img.ctypes.data, W, H, img.strides[0])
    r = dict(sum=np.zeros((H + 1, W + 1)), sumsq=np.zeros((H + 1, W + 1)), hist=np.zeros(256, np.uint32), eq_own=np.zeros((H, W), np.uint8),
             eq_given=np.zeros((H, W), np.uint8), projX=np.zeros(W, np.int32), projY=np.zeros(H, np.int32))
    assert L.statshim_integral(*g, r["sum"].ctypes.data, r["sumsq"].ctypes.data) == 0
    assert L.statshim_histogram(*g, r["hist"].ctypes.data) == 0
    assert L.statshim_equalize(*g, None, -1.0, r["eq_own"].ctypes.data) == 0
    assert L.statshim_equalize(*g, hist.ctypes.data, -1.0, r["eq_given"].ctypes.data) == 0
    assert L.statshim_projections(*g, r["projX"].ctypes.data, r["projY"].ctypes.data) == 0
    return r


def model_arrays(img, hist):
    s, q = sm.integral(img)
    px, py = sm.projections(img)
    own, lut_own = sm.equalize(img)
    given, lut_given = sm.equalize(img, hist)
    clamped, lut_clamped = sm.equalize(img, None, sc.CLAMP_SCALE)
    return dict(sum=s, sumsq=q, hist=sm.histogram(img), eq_own=own, eq_given=given, projX=px, projY=py, lut_own=lut_own, lut_given=lut_given,
                eq_clamped=clamped, lut_clamped=lut_clamped)


def md5(a):
    return hashlib.md5(np.ascontiguousarray(a).tobytes()).hexdigest()


def main():
    RefShim(threads=1)          # refshim_init(1): the reference on one thread
    meta = {"cases": []}
    arrays = {}
    with tempfile.TemporaryDirectory() as tmp:
        L = build_shim(tmp, *sys.argv[1:2])
        for c in sc.CASES:
            img, hist = sc.case_frame(c), sc.other_hist(c)
            m = model_arrays(img, hist)
            assert sm.lut_unclamped_max(sm.histogram(img), 0.0, c["W"], c["H"]) < 256 and sm.lut_unclamped_max(hist, 0.0, c["W"], c["H"]) < 256
            for simd in (1, 0):
                assert L.statshim_simd(simd) == 0
                ref = reference(L, img, hist)
                for k, v in ref.items():
                    assert m[k].dtype == v.dtype and m[k].shape == v.shape and m[k].tobytes() == v.tobytes(), "%s, simd %d: model and reference differ in %s" % (c["id"], simd, k)
            assert L.statshim_simd(1) == 0
            stored = c["W"] * c["H"] <= sc.STORE_LIMIT
            if stored:
                for k, v in m.items():
                    arrays["%s_%s" % (k, c["id"])] = v
            meta["cases"].append(dict(id=c["id"], W=c["W"], H=c["H"], kind=c["kind"], stored=stored, frame_md5=md5(img), md5={k: md5(v) for k, v in m.items()}))
    with open(os.path.join(HERE, "golden_stats.json"), "w") as f:
        json.dump(meta, f, indent=None, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    np.savez_compressed(os.path.join(HERE, "golden_stats.npz"), **arrays)
    print("wrote %d cases, every one model == reference byte for byte, with and without SSE2 / SSSE3 / AVX2" % len(meta["cases"]))


if __name__ == "__main__":
    main()
