#!/usr/bin/env python
"""Generate tests/golden/golden_remap.json (+ golden_remap.npz) from the COMPILED REFERENCE (oracle/_ref, built by oracle/build_ref.sh): what
CompVImageRemap::process writes for float32 maps and what CompVImage::warpInverse writes for 2 x 3 and 3 x 3 float32 matrices, nearest and bilinear.
Run in the build container only: it compiles the small shim below (our own code: it only CALLS the reference's public API) into a temporary directory
and links it against oracle/_ref/libcompv_ref.so.  The reference runs on one thread (refshim_init(1)).

Inputs are what any box can regenerate from seeds (tests/remap_cases.py: frames of tests/fast_model.py, numpy default_rng maps cast to float32, matrices
written out there).  The .json holds, per case and interpolation, the parameters and the MD5 of the reference's plane; the .npz holds the planes.

The generator asserts, before it writes anything, that tests/remap_model.py equals the reference on EVERY byte of every case: the reference is the
definition.  Two limits of the reference shape the cases (include/compv_hip.h, section "remap and inverse warp", E):
  * its float32 output overwrites row tails unless Wout % 8 == 0, so float32 planes are taken (and compared with the model, bit pattern for bit pattern)
    for Wout % 8 == 0 only;
  * its nearest leaf takes a NaN coordinate for inside, so the case whose Z crosses 0 runs through it for the bilinear forms only.
It also reports how many fused multiply-adds of the model needed the exact (fractions) path."""
import ctypes as C
import hashlib, json, os, subprocess, sys, tempfile
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(HERE, ".."))
from oracle_bindings import RefShim  # noqa: E402
import remap_model as rm  # noqa: E402
import remap_cases as rc  # noqa: E402

SHIM = r"""
#include <compv/base/compv_base.h>
#include <compv/base/compv_mat.h>
#include <compv/base/image/compv_image.h>
#include <compv/base/image/compv_image_remap.h>
#include <cstring>
using namespace compv;
static const COMPV_INTERPOLATION_TYPE kInterp[3] = { COMPV_INTERPOLATION_TYPE_NEAREST, COMPV_INTERPOLATION_TYPE_BILINEAR, COMPV_INTERPOLATION_TYPE_BILINEAR_FLOAT32 };
static int makeImage(CompVMatPtr& img, const uint8_t* in, size_t W, size_t H)
{
	if (COMPV_ERROR_CODE_IS_NOK(CompVImage::newObj8u(&img, COMPV_SUBTYPE_PIXELS_Y, W, H, 0))) return -1;   // the reference's own aligned stride
	for (size_t j = 0; j < H; ++j) memcpy(img->ptr<uint8_t>(j), in + j * W, W);
	return 0;
}
static int copyOut(const CompVMatPtr& m, size_t Wout, size_t Hout, int interp, void* out)
{
	if (!m || m->cols() != Wout || m->rows() != Hout) return -3;
	const size_t elem = interp == 2 ? sizeof(compv_float32_t) : 1;
	if (m->elmtInBytes() != elem) return -4;
	for (size_t j = 0; j < Hout; ++j) memcpy(static_cast<uint8_t*>(out) + j * Wout * elem, m->ptr<const uint8_t>(j), Wout * elem);
	return 0;
}
extern "C" {
// CompVImageRemap::process: mx, my of Wout * Hout float32; roi NULL or {left, right, top, bottom}
int remapshim_remap(const uint8_t* in, size_t W, size_t H, const float* mx, const float* my, size_t Wout, size_t Hout, int interp, const float* roi, int def, void* out)
{
	CompVMatPtr img, map, dst;
	if (makeImage(img, in, W, H)) return -1;
	if (COMPV_ERROR_CODE_IS_NOK(CompVMat::newObjAligned<compv_float32_t>(&map, 2, Wout * Hout))) return -1;   // aligned rows: the AVX2 leaf
	memcpy(map->ptr<compv_float32_t>(0), mx, Wout * Hout * sizeof(float));
	memcpy(map->ptr<compv_float32_t>(1), my, Wout * Hout * sizeof(float));
	CompVRectFloat32 r;
	if (roi) { r.left = roi[0]; r.right = roi[1]; r.top = roi[2]; r.bottom = roi[3]; }
	CompVSizeSz size; size.width = Wout; size.height = Hout;
	if (COMPV_ERROR_CODE_IS_NOK(CompVImageRemap::process(img, &dst, map, kInterp[interp], roi ? &r : NULL, &size, (uint8_t)def))) return -2;
	return copyOut(dst, Wout, Hout, interp, out);
}
// CompVImage::warpInverse: M of rows x 3 float32
int remapshim_warp(const uint8_t* in, size_t W, size_t H, const float* M, int rows, size_t Wout, size_t Hout, int interp, int def, void* out)
{
	CompVMatPtr img, mat, dst;
	if (makeImage(img, in, W, H)) return -1;
	if (COMPV_ERROR_CODE_IS_NOK(CompVMat::newObjAligned<compv_float32_t>(&mat, rows, 3))) return -1;
	for (int r = 0; r < rows; ++r) memcpy(mat->ptr<compv_float32_t>(r), M + 3 * r, 3 * sizeof(float));
	CompVSizeSz size; size.width = Wout; size.height = Hout;
	if (COMPV_ERROR_CODE_IS_NOK(CompVImage::warpInverse(img, &dst, mat, size, kInterp[interp], (uint8_t)def))) return -2;
	return copyOut(dst, Wout, Hout, interp, out);
}
}
"""


def build_shim(tmp, ref="/root/reference"):          # the default of oracle/build_ref.sh
    src = os.path.join(tmp, "remap_shim.cxx")
    so = os.path.join(tmp, "libremap_shim.so")
    with open(src, "w") as f:
        f.write(SHIM)
    refdir = os.path.join(ROOT, "oracle", "_ref")
    subprocess.check_call(["g++", "-include", "limits", "-std=c++11", "-O2", "-fPIC", "-w", "-DCOMPV_ASM=0", "-I%s/base/include" % ref, "-shared", "-o", so, src,
                           "-L" + refdir, "-lcompv_ref", "-Wl,-rpath," + refdir, "-ldl", "-lpthread"])
    L = C.CDLL(so)
    vp, sz, i = C.c_void_p, C.c_size_t, C.c_int
    L.remapshim_remap.argtypes = [vp, sz, sz, vp, vp, sz, sz, i, vp, i, vp]
    L.remapshim_warp.argtypes = [vp, sz, sz, vp, i, sz, sz, i, i, vp]
    return L


def bits(a):
    return [int(v) for v in np.asarray(a, np.float32).view(np.uint32).ravel()]


def md5(a):
    return hashlib.md5(np.ascontiguousarray(a).tobytes()).hexdigest()


def same(a, b):
    """byte for byte: float32 planes by bit pattern"""
    return a.dtype == b.dtype and a.shape == b.shape and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def out_plane(w_out, h_out, interp):
    return np.zeros((h_out, w_out), np.float32 if interp == rm.BILINEAR_FLOAT32 else np.uint8)


def main():
    ref = RefShim(threads=1)          # refshim_init(1): the reference on one thread
    assert ref.avx2, "the definition is the AVX2 leaf's arithmetic"
    out = {"remap": [], "warp": []}
    arrays = {}
    pixels = inside_px = 0
    with tempfile.TemporaryDirectory() as tmp:
        L = build_shim(tmp, *sys.argv[1:2])
        for c in rc.remap_cases():
            w, h, wo, ho = c["size"]
            img = np.ascontiguousarray(rc.frame(w, h, c["seed"]))
            x, y = rc.random_map(w, h, wo, ho, c["map_seed"])
            roi = None if c["roi"] is None else np.array(c["roi"], np.float32)
            rec = {"id": c["id"], "size": list(c["size"]), "seed": c["seed"], "map_seed": c["map_seed"], "roi": c["roi"], "default": c["default"], "md5": {}}
            for interp in rc.interps_of(wo):
                dst = out_plane(wo, ho, interp)
                assert L.remapshim_remap(img.ctypes.data, w, h, x.ctypes.data, y.ctypes.data, wo, ho, interp, roi.ctypes.data if roi is not None else None, c["default"],
                                         dst.ctypes.data) == 0
                exp = rm.remap(img, x, y, interp, c["roi"], c["default"])
                assert same(exp, dst), "%s %s: the model differs from the reference in %d elements" % (c["id"], rc.INTERP_NAMES[interp], int((exp != dst).sum()))
                name = rc.INTERP_NAMES[interp]
                arrays["%s_%s" % (c["id"], name)] = dst
                rec["md5"][name] = md5(dst)
                pixels += dst.size
            left, right, top, bottom = rm.clip_roi(c["roi"], w, h)
            rec["outside_share"] = round(1.0 - float(((x >= left) & (x <= right) & (y >= top) & (y <= bottom)).mean()), 4)
            out["remap"].append(rec)
        for c in rc.warp_cases():
            w, h, wo, ho = c["size"]
            img = np.ascontiguousarray(rc.frame(w, h, c["seed"]))
            M = np.ascontiguousarray(c["M"], np.float32)
            rec = {"id": c["id"], "size": list(c["size"]), "seed": c["seed"], "M_bits": bits(M), "rows": int(M.shape[0]), "default": c["default"], "nan": c["nan"], "md5": {}}
            x, y = rm.warp_coords(M, wo, ho)
            if c["nan"]:
                assert np.isnan(x).any() or np.isnan(y).any(), "the Z case holds a NaN"
                assert np.isinf(x).any() and (np.diff(np.sign(rm.warp_tables(M, wo, ho)[2])) != 0).any(), "... infinities, and Z changes sign"
            else:
                assert not (np.isnan(x).any() or np.isnan(y).any()), "only the Z case may hold a NaN (the reference's nearest leaf takes it for inside)"
            for interp in rc.interps_of(wo):
                if c["nan"] and interp == rm.NEAREST:
                    continue
                dst = out_plane(wo, ho, interp)
                assert L.remapshim_warp(img.ctypes.data, w, h, M.ctypes.data, M.shape[0], wo, ho, interp, c["default"], dst.ctypes.data) == 0
                exp = rm.warp_inverse(img, M, wo, ho, interp, c["default"])
                assert same(exp, dst), "%s %s: the model differs from the reference in %d elements" % (c["id"], rc.INTERP_NAMES[interp], int((exp != dst).sum()))
                name = rc.INTERP_NAMES[interp]
                arrays["%s_%s" % (c["id"], name)] = dst
                rec["md5"][name] = md5(dst)
                pixels += dst.size
            ins = (x >= 0) & (x <= w - 1) & (y >= 0) & (y <= h - 1)
            rec["inside_share"] = round(float(ins.mean()), 4)
            inside_px += int(ins.sum())
            out["warp"].append(rec)
    assert any(r["inside_share"] < 0.1 for r in out["warp"]) and any(r["inside_share"] > 0.5 for r in out["warp"])
    out["fma_exact_path"] = rm.fma32.redone
    with open(os.path.join(HERE, "golden_remap.json"), "w") as f:
        json.dump(out, f, indent=None, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    np.savez_compressed(os.path.join(HERE, "golden_remap.npz"), **arrays)
    print("wrote %d remap and %d warp cases, %d planes, %d elements, all equal to the model; %d fused multiply-adds took the exact path"
          % (len(out["remap"]), len(out["warp"]), len(arrays), pixels, rm.fma32.redone))


if __name__ == "__main__":
    main()
