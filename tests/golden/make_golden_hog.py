#!/usr/bin/env python
"""Generate tests/golden/golden_hog.json (+ golden_hog.npz) from tests/hog_model.py, held against the COMPILED REFERENCE (oracle/_ref, built by
oracle/build_ref.sh).  Run in the build container only: it compiles the small shim below (our own code: it only CALLS CompVHOG::newObj and process)
into a temporary directory and links it against oracle/_ref/libcompv_ref.so.  The reference runs on one thread.

The reference's AVX2 and FMA3 CPU flags are switched off BEFORE the first HOG object is made (CompVCpu::flagsDisable): oracle/build_ref.sh compiles the
*_avx2.cxx leaves with -mfma, the compiler contracts the two sub(mul()) expressions of compv_core_feature_hog_std_intrin_avx2.cxx:54-55 into fused
operations, and the result then differs from the one-rounding-per-operation definition in the last bits (the reference's own unit test carries an
md5 and an md5_fma column for this); with a cell origin that is no multiple of 8 floats (block 8, stride 4, cell 8) that leaf also loads misaligned
and faults.  The canonical definition is the uncontracted one.

Asserted per case of tests/hog_cases.py before anything is written: model descriptor == reference descriptor, byte for byte.
Stored: the descriptor's bytes for descriptors of up to hog_cases.STORE_LIMIT floats, an MD5 of descriptor and cell map for every case, the frame's MD5.
One case with a cell width of 8 is run once more with AVX2 + FMA3 on: the json records whether the reference differs there and by how much -- for
docs/kernels/hog.md; no test compares against it."""
import ctypes as C
import hashlib
import json, os, subprocess, sys, tempfile
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(HERE, ".."))
from oracle_bindings import RefShim  # noqa: E402
import hog_model as hm  # noqa: E402
import hog_cases as hc  # noqa: E402

SHIM = r"""
#include <compv/base/compv_base.h>
#include <compv/base/compv_cpu.h>
#include <compv/base/compv_mat.h>
#include <compv/base/compv_features.h>
#include <compv/base/image/compv_image.h>
#include <cstring>
using namespace compv;
extern "C" {
// AVX2 + FMA3 leaves of the reference: off (the canonical definition) or back on
int hogshim_simd(int avx2_fma3)
{
	const uint64_t flags = kCpuFlagAVX2 | kCpuFlagFMA3;
	return COMPV_ERROR_CODE_IS_NOK(avx2_fma3 ? CompVCpu::flagsEnable(flags) : CompVCpu::flagsDisable(flags)) ? -1 : 0;
}
// o: blockW, blockH, strideW, strideH, cellW, cellH, nbins, norm (1 none .. 5 L2HYS), gradient (1 signed, 2 unsigned), interp (1 nearest, 2 bilinear).
// -> the descriptor's length, or < 0; at most cap floats are copied
long hogshim_process(const uint8_t* gray, size_t W, size_t H, size_t S, const int* o, float* out, size_t cap)
{
	static const int kNorm[6] = { COMPV_HOG_BLOCK_NORM_L2HYS, COMPV_HOG_BLOCK_NORM_NONE, COMPV_HOG_BLOCK_NORM_L1, COMPV_HOG_BLOCK_NORM_L1SQRT, COMPV_HOG_BLOCK_NORM_L2,
		COMPV_HOG_BLOCK_NORM_L2HYS };
	CompVMatPtr img, desc;
	if (COMPV_ERROR_CODE_IS_NOK(CompVImage::newObj8u(&img, COMPV_SUBTYPE_PIXELS_Y, W, H))) return -1;
	for (size_t j = 0; j < H; ++j) memcpy(img->ptr<uint8_t>(j), gray + j * S, W);
	CompVHOGPtr hog;
	if (COMPV_ERROR_CODE_IS_NOK(CompVHOG::newObj(&hog, COMPV_HOGS_ID, CompVSizeSz(o[0], o[1]), CompVSizeSz(o[2], o[3]), CompVSizeSz(o[4], o[5]), (size_t)o[6], kNorm[o[7]],
		o[8] == 1, o[9] == 1 ? COMPV_HOG_INTERPOLATION_NEAREST : COMPV_HOG_INTERPOLATION_BILINEAR))) return -2;
	if (COMPV_ERROR_CODE_IS_NOK(hog->process(img, &desc))) return -3;
	const size_t n = desc->cols();
	memcpy(out, desc->ptr<const compv_float32_t>(), (n < cap ? n : cap) * sizeof(float));
	return (long)n;
}
}
"""


def build_shim(tmp, ref="/root/reference"):          # the default of oracle/build_ref.sh
    src = os.path.join(tmp, "hog_shim.cxx")
    so = os.path.join(tmp, "libhog_shim.so")
    with open(src, "w") as f:
        f.write(SHIM)
    refdir = os.path.join(ROOT, "oracle", "_ref")
    subprocess.check_call(["g++", "-include", "limits", "-std=c++11", "-O2", "-fPIC", "-w", "-DCOMPV_ASM=0", "-I%s/base/include" % ref, "-I%s/core/include" % ref, "-shared",
                           "-o", so, src, "-L" + refdir, "-lcompv_ref", "-Wl,-rpath," + refdir, "-ldl", "-lpthread"])
    L = C.CDLL(so)
    L.hogshim_simd.argtypes = [C.c_int]
    L.hogshim_process.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t]
    L.hogshim_process.restype = C.c_long
    return L


def ref_hog(L, img, opts):
    """the compiled reference's descriptor of one frame (float32), with the SIMD flags as hogshim_simd left them"""
    o = hm.resolve(opts)
    g = hm.geometry(img.shape[1], img.shape[0], o)
    img = np.ascontiguousarray(img, np.uint8)
    ov = np.array([o[k] for k in hm.FIELDS], np.int32)
    out = np.zeros(g["descLen"], np.float32)
    n = L.hogshim_process(img.ctypes.data, img.shape[1], img.shape[0], img.strides[0], ov.ctypes.data, out.ctypes.data, out.size)
    assert n == g["descLen"], "the reference returns %d floats, the geometry says %d" % (n, g["descLen"])
    return out


def md5(a):
    return hashlib.md5(np.ascontiguousarray(a).tobytes()).hexdigest()


def main():
    RefShim(threads=1)          # refshim_init(1): the reference on one thread
    meta = {"cases": []}
    arrays = {}
    with tempfile.TemporaryDirectory() as tmp:
        L = build_shim(tmp, *sys.argv[1:2])
        assert L.hogshim_simd(0) == 0          # before the first HOG call: newObj picks its leaves from the flags
        for c in hc.CASES:
            img = hc.case_frame(c)
            desc, cells = hm.hog(img, c["opts"])
            ref = ref_hog(L, img, c["opts"])
            assert desc.dtype == np.float32 and desc.tobytes() == ref.tobytes(), "%s: model and reference differ in %d of %d floats (max |d| %g)" % (
                c["id"], int((desc.view(np.uint32) != ref.view(np.uint32)).sum()), desc.size, float(np.abs(desc - ref).max()))
            g = hm.geometry(c["W"], c["H"], c["opts"])
            stored = desc.size <= hc.STORE_LIMIT
            if stored:
                arrays["desc_" + c["id"]] = desc
            meta["cases"].append(dict(id=c["id"], W=c["W"], H=c["H"], kind=c["kind"], opts=c["opts"], geometry=g, stored=stored, frame_md5=md5(img), desc_md5=md5(desc),
                                      cells_md5=md5(cells)))
        c = hc.BY_ID[hc.AVX2_CASE]
        img = hc.case_frame(c)
        desc, _ = hm.hog(img, c["opts"])
        assert L.hogshim_simd(1) == 0
        fused = ref_hog(L, img, c["opts"])
        assert L.hogshim_simd(0) == 0
        meta["avx2_fma3"] = dict(case=c["id"], differs=bool(fused.tobytes() != desc.tobytes()), floats=int(desc.size),
                                 floats_differing=int((fused.view(np.uint32) != desc.view(np.uint32)).sum()), max_abs_difference=float(np.abs(fused - desc).max()))
    with open(os.path.join(HERE, "golden_hog.json"), "w") as f:
        json.dump(meta, f, indent=None, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    np.savez_compressed(os.path.join(HERE, "golden_hog.npz"), **arrays)
    print("wrote %d cases, every one model == reference byte for byte; with AVX2 + FMA3 on, %s: %d of %d floats differ, max |d| %.3g"
          % (len(meta["cases"]), c["id"], meta["avx2_fma3"]["floats_differing"], desc.size, meta["avx2_fma3"]["max_abs_difference"]))


if __name__ == "__main__":
    main()
