#!/usr/bin/env python
"""Generate tests/golden/golden_bicubic.json (+ golden_bicubic.npz) from tests/bicubic_model.py, held against the COMPILED REFERENCE (oracle/_ref, built by
oracle/build_ref.sh): what CompVImageRemap::process and CompVImage::warpInverse write for COMPV_INTERPOLATION_TYPE_BICUBIC and _BICUBIC_FLOAT32.  Run in
the build container only: it compiles the small shim below (our own code: it only CALLS CompVImage::newObj8u, CompVImageRemap::process -- the call behind
CompVImage::remap, which passes neither an output size nor a default value on -- CompVImage::warpInverse and CompVCpu::flagsDisable / flagsEnable) into a
temporary directory and links it against oracle/_ref/libcompv_ref.so.  The reference runs on one thread.

The parity target is the reference with every SIMD CPU flag switched off: its plain leaves, which are the definition the source states (the policy of
make_golden_convert.py).  Asserted before anything is written: for every case of tests/bicubic_cases.py and both outputs, model == reference (flags off),
uint8 byte for byte and float32 by bit pattern.  Only the cases marked `nan` may miss that and are stored as "model only" with the reason: the reference's
bicubic leaf tests `x < left || x > right || ...`, takes a NaN coordinate for inside and reads wherever the cast lands.
Every case is also run with the flags on; the fixture records, per case and output, how many elements then differ from the plain run and by how much: a
measurement, asserted nowhere.
Stored: the model's plane of every case and output in the .npz, its MD5 in the .json."""
import ctypes as C
import hashlib, json, os, subprocess, sys, tempfile
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(HERE, ".."))
from oracle_bindings import RefShim  # noqa: E402
import bicubic_model as bm  # noqa: E402
import bicubic_cases as bc  # noqa: E402
import remap_cases as rc  # noqa: E402
import remap_model as rm  # noqa: E402

SHIM = r"""
#include <compv/base/compv_base.h>
#include <compv/base/compv_cpu.h>
#include <compv/base/compv_mat.h>
#include <compv/base/image/compv_image.h>
#include <compv/base/image/compv_image_remap.h>
#include <cstring>
using namespace compv;
static COMPV_INTERPOLATION_TYPE interpOf(int f32) { return f32 ? COMPV_INTERPOLATION_TYPE_BICUBIC_FLOAT32 : COMPV_INTERPOLATION_TYPE_BICUBIC; }
static int makeImage(CompVMatPtr& img, const uint8_t* in, size_t W, size_t H)
{
	if (COMPV_ERROR_CODE_IS_NOK(CompVImage::newObj8u(&img, COMPV_SUBTYPE_PIXELS_Y, W, H, 0))) return -1;   // the reference's own aligned stride
	for (size_t j = 0; j < H; ++j) memcpy(img->ptr<uint8_t>(j), in + j * W, W);
	return 0;
}
static int copyOut(const CompVMatPtr& m, size_t Wout, size_t Hout, int f32, void* out)
{
	if (!m || m->cols() != Wout || m->rows() != Hout) return -3;
	const size_t elem = f32 ? sizeof(compv_float32_t) : 1;
	if (m->elmtInBytes() != elem) return -4;
	for (size_t j = 0; j < Hout; ++j) memcpy(static_cast<uint8_t*>(out) + j * Wout * elem, m->ptr<const uint8_t>(j), Wout * elem);
	return 0;
}
extern "C" {
int bicshim_simd(int on)
{
	return COMPV_ERROR_CODE_IS_NOK(on ? CompVCpu::flagsEnable(kCpuFlagAll) : CompVCpu::flagsDisable(kCpuFlagAll)) ? -1 : 0;
}
// CompVImageRemap::process: mx, my of Wout * Hout float32; roi NULL or {left, right, top, bottom}
int bicshim_remap(const uint8_t* in, size_t W, size_t H, const float* mx, const float* my, size_t Wout, size_t Hout, int f32, const float* roi, int def, void* out)
{
	CompVMatPtr img, map, dst;
	if (makeImage(img, in, W, H)) return -1;
	if (COMPV_ERROR_CODE_IS_NOK(CompVMat::newObjAligned<compv_float32_t>(&map, 2, Wout * Hout))) return -1;
	memcpy(map->ptr<compv_float32_t>(0), mx, Wout * Hout * sizeof(float));
	memcpy(map->ptr<compv_float32_t>(1), my, Wout * Hout * sizeof(float));
	CompVRectFloat32 r;
	if (roi) { r.left = roi[0]; r.right = roi[1]; r.top = roi[2]; r.bottom = roi[3]; }
	CompVSizeSz size; size.width = Wout; size.height = Hout;
	if (COMPV_ERROR_CODE_IS_NOK(CompVImageRemap::process(img, &dst, map, interpOf(f32), roi ? &r : NULL, &size, (uint8_t)def))) return -2;
	return copyOut(dst, Wout, Hout, f32, out);
}
// CompVImage::warpInverse: M of rows x 3 float32
int bicshim_warp(const uint8_t* in, size_t W, size_t H, const float* M, int rows, size_t Wout, size_t Hout, int f32, int def, void* out)
{
	CompVMatPtr img, mat, dst;
	if (makeImage(img, in, W, H)) return -1;
	if (COMPV_ERROR_CODE_IS_NOK(CompVMat::newObjAligned<compv_float32_t>(&mat, rows, 3))) return -1;
	for (int r = 0; r < rows; ++r) memcpy(mat->ptr<compv_float32_t>(r), M + 3 * r, 3 * sizeof(float));
	CompVSizeSz size; size.width = Wout; size.height = Hout;
	if (COMPV_ERROR_CODE_IS_NOK(CompVImage::warpInverse(img, &dst, mat, size, interpOf(f32), (uint8_t)def))) return -2;
	return copyOut(dst, Wout, Hout, f32, out);
}
}
"""


def build_shim(tmp, ref="/root/reference"):          # the default of oracle/build_ref.sh
    src = os.path.join(tmp, "bicubic_shim.cxx")
    so = os.path.join(tmp, "libbicubic_shim.so")
    with open(src, "w") as f:
        f.write(SHIM)
    refdir = os.path.join(ROOT, "oracle", "_ref")
    subprocess.check_call(["g++", "-include", "limits", "-std=c++11", "-O2", "-fPIC", "-w", "-DCOMPV_ASM=0", "-I%s/base/include" % ref, "-shared", "-o", so, src,
                           "-L" + refdir, "-lcompv_ref", "-Wl,-rpath," + refdir, "-ldl", "-lpthread"])
    L = C.CDLL(so)
    vp, sz, i = C.c_void_p, C.c_size_t, C.c_int
    L.bicshim_simd.argtypes = [i]
    L.bicshim_remap.argtypes = [vp, sz, sz, vp, vp, sz, sz, i, vp, i, vp]
    L.bicshim_warp.argtypes = [vp, sz, sz, vp, i, sz, sz, i, i, vp]
    return L


def md5(a):
    return hashlib.md5(np.ascontiguousarray(a).tobytes()).hexdigest()


def same(a, b):
    """byte for byte: float32 planes by bit pattern"""
    return a.dtype == b.dtype and a.shape == b.shape and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def out_plane(w_out, h_out, interp):
    return np.zeros((h_out, w_out), np.float32 if interp == bm.BICUBIC_FLOAT32 else np.uint8)


def record(rec, arrays, totals, L, c, interp, model, call):
    """both runs of the reference for one case and output: asserts the plain one against the model, measures the other"""
    name = bc.INTERP_NAMES[interp]
    plain, simd = out_plane(*c["size"][2:], interp), out_plane(*c["size"][2:], interp)
    assert L.bicshim_simd(0) == 0 and call(plain) == 0
    assert L.bicshim_simd(1) == 0 and call(simd) == 0
    if same(model, plain):
        rec["checked"][name] = "reference"
    else:
        bits = np.uint8 if model.dtype == np.uint8 else np.uint32
        bad = int((model.view(bits) != plain.view(bits)).sum()) if model.dtype == plain.dtype else -1
        assert c.get("nan"), "%s %s: the model differs from the reference (SIMD off) in %d elements" % (c["id"], name, bad)
        rec["checked"][name] = "model only: the reference takes a NaN coordinate for inside (%d elements differ)" % bad
    with np.errstate(invalid="ignore"):
        d = np.abs(plain.astype(np.float64) - simd.astype(np.float64))
        d = d[np.isfinite(d)]
    differ = int((plain.view(np.uint8) != simd.view(np.uint8)).sum()) if plain.dtype == np.uint8 else int((plain.view(np.uint32) != simd.view(np.uint32)).sum())
    rec["simd"][name] = {"differ": differ, "max_abs_diff": float(d.max()) if d.size else 0.0, "elements": int(plain.size)}
    totals[name][0] += differ
    totals[name][1] += int(plain.size)
    totals[name][2] = max(totals[name][2], rec["simd"][name]["max_abs_diff"])
    rec["md5"][name] = md5(model)
    arrays[bc.key(c["id"], interp)] = model


def main():
    RefShim(threads=1)          # refshim_init(1): the reference on one thread
    out = {"remap": [], "warp": []}
    arrays = {}
    totals = {n: [0, 0, 0.0] for n in bc.INTERP_NAMES.values()}
    with tempfile.TemporaryDirectory() as tmp:
        L = build_shim(tmp, *sys.argv[1:2])
        for c in bc.all_map_cases():
            w, h, wo, ho = c["size"]
            img = np.ascontiguousarray(rc.frame(w, h, c["seed"]))
            x, y = bc.map_of(c)
            roi = None if c["roi"] is None else np.array(c["roi"], np.float32)
            rec = {"id": c["id"], "size": list(c["size"]), "seed": c["seed"], "map_seed": c["map_seed"], "roi": c["roi"], "default": c["default"], "nan": bool(c.get("nan")),
                   "md5": {}, "checked": {}, "simd": {}}
            if c.get("nan"):
                assert np.isnan(x).any() and np.isinf(y).any()
            else:
                assert np.isfinite(x).all() and np.isfinite(y).all(), "only the NaN case may hold a NaN"
            for interp in bc.INTERPS:
                f32 = int(interp == bm.BICUBIC_FLOAT32)
                record(rec, arrays, totals, L, c, interp, bm.remap(img, x, y, interp, c["roi"], c["default"]),
                       lambda dst: L.bicshim_remap(img.ctypes.data, w, h, x.ctypes.data, y.ctypes.data, wo, ho, f32, roi.ctypes.data if roi is not None else None,
                                                   c["default"], dst.ctypes.data))
            out["remap"].append(rec)
            print(c["id"], rec["checked"], rec["simd"], flush=True)
        for c in bc.warp_cases():
            w, h, wo, ho = c["size"]
            img = np.ascontiguousarray(rc.frame(w, h, c["seed"]))
            M = np.ascontiguousarray(c["M"], np.float32)
            rec = {"id": c["id"], "size": list(c["size"]), "seed": c["seed"], "rows": int(M.shape[0]), "default": c["default"], "nan": c["nan"], "md5": {}, "checked": {}, "simd": {}}
            x, y = rm.warp_coords(M, wo, ho)
            assert bool(np.isnan(x).any() or np.isnan(y).any()) == c["nan"], "only the Z case holds a NaN"
            for interp in bc.INTERPS:
                f32 = int(interp == bm.BICUBIC_FLOAT32)
                record(rec, arrays, totals, L, c, interp, bm.warp_inverse(img, M, wo, ho, interp, c["default"]),
                       lambda dst: L.bicshim_warp(img.ctypes.data, w, h, M.ctypes.data, M.shape[0], wo, ho, f32, c["default"], dst.ctypes.data))
            out["warp"].append(rec)
            print(c["id"], rec["checked"], rec["simd"], flush=True)
    for r in out["remap"] + out["warp"]:          # everything but the NaN cases is reference-checked
        assert r["nan"] or all(v == "reference" for v in r["checked"].values()), r["id"]
    out["simd_total"] = {n: {"differ": t[0], "elements": t[1], "max_abs_diff": t[2]} for n, t in totals.items()}
    with open(os.path.join(HERE, "golden_bicubic.json"), "w") as f:
        json.dump(out, f, indent=None, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    np.savez_compressed(os.path.join(HERE, "golden_bicubic.npz"), **arrays)
    print("wrote %d remap and %d warp cases, %d planes; SIMD on against SIMD off: %s" % (len(out["remap"]), len(out["warp"]), len(arrays), out["simd_total"]))


if __name__ == "__main__":
    main()
