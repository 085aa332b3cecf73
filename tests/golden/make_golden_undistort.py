#!/usr/bin/env python
"""Generate tests/golden/golden_undistort.json (+ golden_undistort.npz) from tests/undistort_cases.py, held against the COMPILED REFERENCE (oracle/_ref,
built by oracle/build_ref.sh).  Run in the build container only: it compiles the small shim below (our own code: it only CALLS the reference --
CompVCalibUtils::initUndistMap, dist2DPoints, proj2D, undist2DImage) into a temporary directory and links it against oracle/_ref/libcompv_ref.so.  The
reference runs on one thread (refshim_init(1)).

Before it writes anything the generator asserts that tests/undistort_model.py equals the reference on EVERY bit of every map (float32 and float64), of
every point case and of every projection case, and that tests/remap_model.py on the model's float32 map equals CompVCalibUtils::undist2DImage for
nearest and bilinear uint8 on the whole-frame cases.  One mismatch fails it; nothing is skipped or retried.  A case that cannot go through the reference
is marked "model only" with its reason; at most two may be.

Stored: the float32 map planes, the point and projection outputs (.npz); the MD5 of the float64 planes and of the model's image for all five
interpolations, the outside shares (.json).  The bicubic and float32 images come from tests/bicubic_model.py / tests/remap_model.py on the pinned map;
those models are pinned against the reference by their own fixtures."""
import ctypes as C
import hashlib, json, os, subprocess, sys, tempfile
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(HERE, ".."))
from oracle_bindings import RefShim  # noqa: E402
import remap_model as rm  # noqa: E402
import undistort_model as um  # noqa: E402
import undistort_cases as uc  # noqa: E402

SHIM = r"""
#include <compv/base/compv_base.h>
#include <compv/base/compv_mat.h>
#include <compv/base/image/compv_image.h>
#include <compv/core/calib/compv_core_calib_utils.h>
#include <cstring>
using namespace compv;
template <typename T> static int mat(CompVMatPtr& m, const T* src, size_t rows, size_t cols)
{
	if (COMPV_ERROR_CODE_IS_NOK(CompVMat::newObjAligned<T>(&m, rows, cols))) return -1;
	for (size_t r = 0; r < rows; ++r) memcpy(m->ptr<T>(r), src + r * cols, cols * sizeof(T));
	return 0;
}
template <typename T> static int camera(CompVMatPtr& K, CompVMatPtr& d, const void* k, const void* dd, int nd)
{
	return mat<T>(K, static_cast<const T*>(k), 3, 3) || mat<T>(d, static_cast<const T*>(dd), (size_t)nd, 1);
}
template <typename T> static void rows2(const CompVMatPtr& m, size_t n, void* a, void* b)
{
	memcpy(a, m->ptr<const T>(0), n * sizeof(T));
	memcpy(b, m->ptr<const T>(1), n * sizeof(T));
}
extern "C" {
// CompVCalibUtils::initUndistMap; roi NULL or {left, right, top, bottom}; mx, my: room for the map's columns
int undshim_map(int f64, const void* k, const void* dd, int nd, size_t W, size_t H, const float* roi, void* mx, void* my, size_t* cols)
{
	CompVMatPtr K, d, map;
	if (f64 ? camera<compv_float64_t>(K, d, k, dd, nd) : camera<compv_float32_t>(K, d, k, dd, nd)) return -1;
	CompVRectFloat32 r;
	if (roi) { r.left = roi[0]; r.right = roi[1]; r.top = roi[2]; r.bottom = roi[3]; }
	if (COMPV_ERROR_CODE_IS_NOK(CompVCalibUtils::initUndistMap(CompVSizeSz(W, H), K, d, &map, roi ? &r : NULL))) return -2;
	if (!map || map->rows() != 3) return -3;
	*cols = map->cols();
	if (f64) rows2<compv_float64_t>(map, map->cols(), mx, my); else rows2<compv_float32_t>(map, map->cols(), mx, my);
	return 0;
}
// CompVCalibUtils::dist2DPoints; x, y: n values each
int undshim_points(int f64, const void* k, const void* dd, int nd, const void* xy, size_t n, void* ox, void* oy)
{
	CompVMatPtr K, d, in, out;
	if (f64 ? camera<compv_float64_t>(K, d, k, dd, nd) : camera<compv_float32_t>(K, d, k, dd, nd)) return -1;
	if (f64 ? mat<compv_float64_t>(in, static_cast<const compv_float64_t*>(xy), 2, n) : mat<compv_float32_t>(in, static_cast<const compv_float32_t*>(xy), 2, n)) return -1;
	if (COMPV_ERROR_CODE_IS_NOK(CompVCalibUtils::dist2DPoints(in, K, d, &out))) return -2;
	if (!out || out->cols() != n || out->rows() < 2) return -3;
	if (f64) rows2<compv_float64_t>(out, n, ox, oy); else rows2<compv_float32_t>(out, n, ox, oy);
	return 0;
}
// CompVCalibUtils::proj2D; xyz: three rows of n values
int undshim_proj(const double* k, const double* dd, int nd, const double* R, const double* t, const double* xyz, size_t n, double* ox, double* oy)
{
	CompVMatPtr K, d, Rm, tm, in, out;
	if (camera<compv_float64_t>(K, d, k, dd, nd) || mat<compv_float64_t>(Rm, R, 3, 3) || mat<compv_float64_t>(tm, t, 1, 3) || mat<compv_float64_t>(in, xyz, 3, n)) return -1;
	if (COMPV_ERROR_CODE_IS_NOK(CompVCalibUtils::proj2D(in, K, d, Rm, tm, &out))) return -2;
	if (!out || out->cols() != n || out->rows() != 3) return -3;
	rows2<compv_float64_t>(out, n, ox, oy);
	return 0;
}
// CompVCalibUtils::undist2DImage(imageIn, K, d, &imageOut, interp): the whole frame, uint8; interp 0 nearest, 1 bilinear
int undshim_image(const uint8_t* in, size_t W, size_t H, const float* k, const float* dd, int nd, int interp, uint8_t* out)
{
	CompVMatPtr K, d, img, dst;
	if (camera<compv_float32_t>(K, d, k, dd, nd)) return -1;
	if (COMPV_ERROR_CODE_IS_NOK(CompVImage::newObj8u(&img, COMPV_SUBTYPE_PIXELS_Y, W, H, 0))) return -1;
	for (size_t j = 0; j < H; ++j) memcpy(img->ptr<uint8_t>(j), in + j * W, W);
	if (COMPV_ERROR_CODE_IS_NOK(CompVCalibUtils::undist2DImage(img, K, d, &dst, interp ? COMPV_INTERPOLATION_TYPE_BILINEAR : COMPV_INTERPOLATION_TYPE_NEAREST))) return -2;
	if (!dst || dst->cols() != W || dst->rows() != H || dst->elmtInBytes() != 1) return -3;
	for (size_t j = 0; j < H; ++j) memcpy(out + j * W, dst->ptr<const uint8_t>(j), W);
	return 0;
}
}
"""


def build_shim(tmp, ref="/root/reference"):          # the default of oracle/build_ref.sh
    src = os.path.join(tmp, "undistort_shim.cxx")
    so = os.path.join(tmp, "libundistort_shim.so")
    with open(src, "w") as f:
        f.write(SHIM)
    refdir = os.path.join(ROOT, "oracle", "_ref")
    subprocess.check_call(["g++", "-include", "limits", "-std=c++11", "-O2", "-fPIC", "-w", "-DCOMPV_ASM=0", "-I%s/base/include" % ref, "-I%s/core/include" % ref, "-shared",
                           "-o", so, src, "-L" + refdir, "-lcompv_ref", "-Wl,-rpath," + refdir, "-ldl", "-lpthread"])
    L = C.CDLL(so)
    vp, sz, i = C.c_void_p, C.c_size_t, C.c_int
    L.undshim_map.argtypes = [i, vp, vp, i, sz, sz, vp, vp, vp, C.POINTER(sz)]
    L.undshim_points.argtypes = [i, vp, vp, i, vp, sz, vp, vp]
    L.undshim_proj.argtypes = [vp, vp, i, vp, vp, vp, sz, vp, vp]
    L.undshim_image.argtypes = [vp, sz, sz, vp, vp, i, i, vp]
    return L


def md5(a):
    return hashlib.md5(np.ascontiguousarray(a).tobytes()).hexdigest()


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def cam(c, T):
    return np.ascontiguousarray(c["K"], T), np.ascontiguousarray(c["d"], T)


def reference_map(L, c, T):
    """initUndistMap of the case's window (its ROI in the reference's terms: left, right, top, bottom of the window, on a frame that holds it)"""
    w, h, wo, ho = c["size"]
    x0, y0 = c["origin"]
    K, d = cam(c, T)
    whole = (x0, y0) == (0, 0)
    roi = None if whole else np.array([x0, x0 + wo - 1, y0, y0 + ho - 1], np.float32)
    mx, my, cols = np.zeros((ho, wo), T), np.zeros((ho, wo), T), C.c_size_t()
    rc = L.undshim_map(int(T is np.float64), K.ctypes.data, d.ctypes.data, d.size, wo if whole else x0 + wo, ho if whole else y0 + ho,
                       None if roi is None else roi.ctypes.data, mx.ctypes.data, my.ctypes.data, C.byref(cols))
    assert rc == 0 and cols.value == wo * ho, (c["id"], rc, cols.value)
    return mx, my


def main():
    ref = RefShim(threads=1)          # refshim_init(1): the reference on one thread
    assert ref.avx2, "the bilinear definition is the AVX2 leaf's arithmetic"
    meta = {"images": [], "points": [], "proj": [], "model_only": []}
    arrays = {}
    elements = 0
    with tempfile.TemporaryDirectory() as tmp:
        L = build_shim(tmp, *sys.argv[1:2])
        for c in uc.image_cases():
            w, h, wo, ho = c["size"]
            x0, y0 = c["origin"]
            rec = {"id": c["id"], "size": list(c["size"]), "origin": [x0, y0], "nd": len(c["d"]), "md5": {}}
            for T, name in ((np.float32, "f32"), (np.float64, "f64")):
                mx, my = um.map_planes(c["K"], c["d"], wo, ho, x0, y0, T)
                rx, ry = reference_map(L, c, T)
                assert same(mx, rx) and same(my, ry), "%s %s: the model's map differs from the reference in %d + %d entries" % (c["id"], name, int((mx != rx).sum()), int((my != ry).sum()))
                rec["md5"]["mapx_" + name], rec["md5"]["mapy_" + name] = md5(rx), md5(ry)
                elements += 2 * rx.size
                if T is np.float32:
                    arrays["mapx_" + c["id"]], arrays["mapy_" + c["id"]] = rx, ry
            mx, my = arrays["mapx_" + c["id"]], arrays["mapy_" + c["id"]]
            rec["outside_share"] = round(um.outside_share(w, h, mx, my, c["roi"]), 4)
            img = uc.frame(c)
            K32, d32 = cam(c, np.float32)
            for interp in um.INTERPS:
                exp = um.remap_on(img, mx, my, interp, c["roi"], c["default"])
                if c["whole"] and c["roi"] is None and interp in (rm.NEAREST, rm.BILINEAR):
                    # undist2DImage has neither a ROI nor a default value: the whole frame, default 0
                    exp0 = um.remap_on(img, mx, my, interp, None, 0)
                    dst = np.zeros((h, w), np.uint8)
                    rc = L.undshim_image(img.ctypes.data, w, h, K32.ctypes.data, d32.ctypes.data, d32.size, int(interp == rm.BILINEAR), dst.ctypes.data)
                    if rc != 0:
                        meta["model_only"].append({"id": c["id"], "interp": um.INTERP_NAMES[interp], "reason": "CompVCalibUtils::undist2DImage returned an error for this shape (%d)" % rc})
                    else:
                        assert same(exp0, dst), "%s %s: remap_model on the model's map differs from undist2DImage in %d bytes" % (c["id"], um.INTERP_NAMES[interp], int((exp0 != dst).sum()))
                        elements += dst.size
                rec["md5"][um.INTERP_NAMES[interp]] = md5(exp)
            meta["images"].append(rec)
            print("%-10s %3d x %-3d -> %3d x %-3d at (%d, %d)  nd %d  outside %.4f" % (c["id"], w, h, wo, ho, x0, y0, len(c["d"]), rec["outside_share"]))
        for c in uc.point_cases():
            T = c["dtype"]
            K, d = cam(uc.case(c["camera"]), T)
            pts = uc.points(c)
            got = um.dist_points(K, d, pts, T)
            planar = np.ascontiguousarray(pts.T)
            ox, oy = np.zeros(c["n"], T), np.zeros(c["n"], T)
            assert L.undshim_points(int(T is np.float64), K.ctypes.data, d.ctypes.data, d.size, planar.ctypes.data, c["n"], ox.ctypes.data, oy.ctypes.data) == 0, c["id"]
            refd = np.stack([ox, oy], axis=1)
            assert same(got, refd), "%s: the model differs from dist2DPoints in %d values" % (c["id"], int((got != refd).sum()))
            arrays[c["id"]] = refd
            elements += refd.size
            meta["points"].append({"id": c["id"], "n": c["n"], "camera": c["camera"], "md5": md5(refd)})
        for c in uc.proj_cases():
            K, d = cam(uc.case(c["camera"]), np.float64)
            R, t, pts = np.ascontiguousarray(c["R"], np.float64), np.ascontiguousarray(c["t"], np.float64), uc.proj_points(c)
            got = um.proj2d(K, d, R, t, pts)
            planar = np.ascontiguousarray(pts.T)
            ox, oy = np.zeros(c["n"]), np.zeros(c["n"])
            assert L.undshim_proj(K.ctypes.data, d.ctypes.data, d.size, R.ctypes.data, t.ctypes.data, planar.ctypes.data, c["n"], ox.ctypes.data, oy.ctypes.data) == 0, c["id"]
            refd = np.stack([ox, oy], axis=1)
            assert same(got, refd), "%s: the model differs from proj2D in %d values" % (c["id"], int((got != refd).sum()))
            z = ((R[2, 0] * pts[:, 0] + R[2, 1] * pts[:, 1]) + R[2, 2] * pts[:, 2]) + t[2]
            zeros = int((z == 0).sum())
            if c["id"] == "proj_z0":
                assert 0 < zeros < c["n"], "the z == 0 branch must be taken by some points and not by all"
            assert np.isfinite(refd).all(), c["id"]
            arrays[c["id"]] = refd
            elements += refd.size
            meta["proj"].append({"id": c["id"], "n": c["n"], "camera": c["camera"], "z_zero": zeros, "md5": md5(refd)})
    shares = [r["outside_share"] for r in meta["images"]]
    assert any(0.05 <= s <= 0.60 for s in shares) and any(s == 0.0 for s in shares), shares          # no test passes on default bytes alone, none on inside bytes alone
    assert len({m["id"] for m in meta["model_only"]}) <= 2, meta["model_only"]
    with open(os.path.join(HERE, "golden_undistort.json"), "w") as f:
        json.dump(meta, f, indent=None, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    np.savez_compressed(os.path.join(HERE, "golden_undistort.npz"), **arrays)
    print("wrote %d image, %d point and %d projection cases, %d elements compared with the reference, 0 mismatches; model only: %s; outside shares %s"
          % (len(meta["images"]), len(meta["points"]), len(meta["proj"]), elements, [(m["id"], m["interp"]) for m in meta["model_only"]] or "none", shares))


if __name__ == "__main__":
    main()
