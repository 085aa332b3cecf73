#!/usr/bin/env python
"""Generate tests/golden/golden_orb_pyramid.json (+ golden_orb_pyramid.npz) from the COMPILED REFERENCE (oracle/_ref, built by oracle/build_ref.sh): what
CompVImage::scale writes for a few downscales, and for whole ORB pyramids the level planes CompVImageScalePyramid holds, the points
CompVCornerDeteORB::process returns per level and the descriptors CompVCornerDescORB::process writes for exactly those points.  Run in the build
container only: it compiles the small shim below (our own code: it only CALLS the reference's public API) into a temporary directory and links it
against oracle/_ref/libcompv_ref.so.  The reference runs on one thread (refshim_init(1)); every case gets a fresh detector and descriptor.

Inputs are frames any box can regenerate (tests/fast_model.py, numpy default_rng seeds).  The .json holds, per case and non-empty level, the size, the
scale factor's bits, the MD5 of the plane, the quota and the counts; the .npz holds the bulky arrays: the scaled planes of the direct downscales and of
the 100 x 90 pyramid, and per level the points sorted by (y, x) -- the level's integer coordinates (the generator asserts that the reference's x, y,
level and size are exactly what they give with sf[level]), the strength, the orientation's bits -- with their 32 descriptor bytes and the packed
`libm_exact` flags (tests/golden/make_golden_orb.py says what they mean).

The generator asserts what lets the reference stand for the definition: every neighbour the reference's scaler reads lies inside the plane (no upscale is
ever run through it); in each cut case no two strengths tie at a level's quota boundary, so the reference's selectBest (an unspecified nth_element pivot,
scrambled order) yields the same SET as the definition's cut; no level has more than 2000 corners and no level kept fewer points than the definition keeps
(two habits of the reference's inner FAST detector, see check_level); every point fed to the descriptor lies 18 pixels inside its level, so the
reference refuses none and its rows stay aligned; at least 95 % of the points have a libm cosf / sinf equal to the canonical value."""
import ctypes as C
import hashlib, json, os, subprocess, sys, tempfile
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(HERE, ".."))
from oracle_bindings import RefShim  # noqa: E402
import fast_model as fm  # noqa: E402
import orb_model as om  # noqa: E402
import orb_pyramid_model as pm  # noqa: E402
from make_golden_orb import libm_exact  # noqa: E402

SHIM = r"""
#include <compv/base/compv_base.h>
#include <compv/base/compv_features.h>
#include <compv/base/compv_mat.h>
#include <compv/base/image/compv_image.h>
#include <compv/base/image/compv_image_scale_pyramid.h>
#include <cstring>
using namespace compv;
static int makeImage(CompVMatPtr& img, const uint8_t* in, size_t W, size_t H)
{
	if (COMPV_ERROR_CODE_IS_NOK(CompVImage::newObj8u(&img, COMPV_SUBTYPE_PIXELS_Y, W, H, 0))) return -1;   // the reference's own aligned stride
	for (size_t j = 0; j < H; ++j) memcpy(img->ptr<uint8_t>(j), in + j * W, W);
	return 0;
}
static void copyPlane(const CompVMatPtr& m, uint8_t* out)
{
	for (size_t j = 0; j < m->rows(); ++j) memcpy(out + j * m->cols(), m->ptr<const uint8_t>(j), m->cols());
}
extern "C" {
// CompVImage::scale, bilinear: in (H rows of W bytes) -> out (Hout rows of Wout bytes)
int pyrshim_scale(const uint8_t* in, size_t W, size_t H, size_t Wout, size_t Hout, uint8_t* out)
{
	CompVMatPtr img, dst;
	if (makeImage(img, in, W, H)) return -1;
	if (COMPV_ERROR_CODE_IS_NOK(CompVImage::scale(img, &dst, Wout, Hout, COMPV_INTERPOLATION_TYPE_BILINEAR))) return -2;
	if (!dst || dst->cols() != Wout || dst->rows() != Hout) return -3;
	copyPlane(dst, out);
	return 0;
}
// An ORB detector with the given pyramid runs on the frame; its points (24-byte CompVInterestPoint records, all levels, the detector's order) go to
// pts; the level planes, copied BEFORE the descriptor blurs them in place, go to planes one behind the other (dims: cols, rows per level); then an ORB
// descriptor attached to the detector describes exactly those points.  -> number of points, or < 0.
long pyrshim_run(const uint8_t* in, size_t W, size_t H, int levels, float sf, int maxFeatures, int threshold, uint8_t* planes, size_t planesCap, int32_t* dims, float* scales,
                 float* sfs, void* pts, size_t ptsCap, uint8_t* desc)
{
	CompVMatPtr img;
	if (makeImage(img, in, W, H)) return -1;
	CompVCornerDetePtr det;
	if (COMPV_ERROR_CODE_IS_NOK(CompVCornerDete::newObj(&det, COMPV_ORB_ID))) return -2;
	if (COMPV_ERROR_CODE_IS_NOK(det->set(COMPV_ORB_SET_INT_PYRAMID_LEVELS, &levels, sizeof(levels)))) return -3;
	if (COMPV_ERROR_CODE_IS_NOK(det->set(COMPV_ORB_SET_FLT32_PYRAMID_SCALE_FACTOR, &sf, sizeof(sf)))) return -3;   // after the levels: that call rebuilds the pyramid
	if (COMPV_ERROR_CODE_IS_NOK(det->set(COMPV_ORB_SET_INT_MAX_FEATURES, &maxFeatures, sizeof(maxFeatures)))) return -3;
	if (COMPV_ERROR_CODE_IS_NOK(det->set(COMPV_ORB_SET_INT_FAST_THRESHOLD, &threshold, sizeof(threshold)))) return -3;
	CompVInterestPointVector found;
	if (COMPV_ERROR_CODE_IS_NOK(det->process(img, found))) return -4;
	const void* vp = NULL;
	if (COMPV_ERROR_CODE_IS_NOK(det->get(COMPV_FEATURE_GET_PTR_PYRAMID, &vp, sizeof(CompVImageScalePyramid))) || !vp) return -5;
	CompVImageScalePyramidPtr pyr = reinterpret_cast<CompVImageScalePyramid*>(const_cast<void*>(vp));
	if ((int)pyr->levels() != levels) return -6;
	*sfs = pyr->scaleFactorsSum();
	size_t off = 0;
	for (int l = 0; l < levels; ++l) {
		CompVMatPtr lv;
		if (COMPV_ERROR_CODE_IS_NOK(pyr->image(l, &lv)) || !lv) return -7;
		dims[2 * l] = (int32_t)lv->cols(); dims[2 * l + 1] = (int32_t)lv->rows();
		scales[l] = pyr->scaleFactor(l);
		if (off + lv->cols() * lv->rows() > planesCap) return -8;
		copyPlane(lv, planes + off);
		off += lv->cols() * lv->rows();
	}
	if (found.size() > ptsCap) return -9;
	memcpy(pts, found.data(), found.size() * sizeof(CompVInterestPoint));
	CompVCornerDescPtr dsc;
	if (COMPV_ERROR_CODE_IS_NOK(CompVCornerDesc::newObj(&dsc, COMPV_ORB_ID, det))) return -10;
	CompVMatPtr rows;
	if (COMPV_ERROR_CODE_IS_NOK(dsc->process(img, found, &rows))) return -11;
	if (!found.empty() && (!rows || rows->rows() != found.size() || rows->cols() != 32)) return -12;
	for (size_t i = 0; i < found.size(); ++i) memcpy(desc + 32 * i, rows->ptr<const uint8_t>(i), 32);
	return (long)found.size();
}
}
"""

SCALES = ((9, 7, 7, 5), (64, 41, 53, 34), (1100, 5, 1021, 4), (300, 8, 2, 1))          # Win, Hin, Wout, Hout: downscales only
# W, H, content, seed, levels, scale factor, maxFeatures, FAST threshold.  The uncut noise frame of 200 x 258 takes threshold 70, which keeps every level below
# the 2000 corners at which the reference's INNER FAST detector cuts by a default of its own (compv_core_feature_fast_dete.cxx:79,418) whatever the ORB
# detector was told.  The seeds of the cut cases were searched, with the assertions of check_level below, until every level passed: blocks at 500 (all 8
# levels cut) after 6848 seeds, 100 x 90 at 60 (5 levels cut) after 24.  Noise of 200 x 258 at 500 has so many corners of so few strengths that about
# 135 000 seeds at thresholds 70, 80 and 90 left none whose levels were all free of ties and of stale corners; at threshold 100 level 0 alone is cut
# (its quota of 110 among several hundred corners) and the 79th seed passed.
PYRAMIDS = (
    (200, 258, "blocks", 41006, 8, 0.83, 0, 20), (200, 258, "noise", 41001, 8, 0.83, 0, 70),
    (200, 258, "blocks", 47847, 8, 0.83, 500, 20), (200, 258, "noise", 600078, 8, 0.83, 500, 100),
    (100, 90, "noise", 41023, 8, 0.83, 60, 20), (96, 80, "blocks", 41007, 3, 0.5, 2000, 20))
FULL_PLANES = (100, 90)          # the case whose planes go to the .npz whole
PTS_CAP = 1 << 15
FAST_TYPE, NONMAX = 9, True          # the reference detector's defaults
INNER_FAST_CUT = 2000


def frame(kind, W, H, seed):
    return fm.noise(W, H, seed) if kind == "noise" else fm.blocks(W, H, seed)


def build_shim(tmp):
    ref = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"          # the default of oracle/build_ref.sh
    src = os.path.join(tmp, "pyr_shim.cxx")
    so = os.path.join(tmp, "libpyr_shim.so")
    with open(src, "w") as f:
        f.write(SHIM)
    refdir = os.path.join(ROOT, "oracle", "_ref")
    subprocess.check_call(["g++", "-include", "limits", "-std=c++11", "-O2", "-fPIC", "-w", "-DCOMPV_ASM=0", "-I%s/base/include" % ref, "-I%s/core/include" % ref,
                           "-shared", "-o", so, src, "-L" + refdir, "-lcompv_ref", "-Wl,-rpath," + refdir, "-ldl", "-lpthread"])
    return C.CDLL(so)


def bits(a):
    return [int(v) for v in np.asarray(a, np.float32).view(np.uint32).ravel()]


def md5(a):
    return hashlib.md5(np.ascontiguousarray(a).tobytes()).hexdigest()


def bind(L):
    vp, sz, i = C.c_void_p, C.c_size_t, C.c_int
    L.pyrshim_scale.argtypes = [vp, sz, sz, sz, sz, vp]
    L.pyrshim_run.argtypes = [vp, sz, sz, i, C.c_float, i, i, vp, sz, vp, vp, vp, vp, sz, vp]
    L.pyrshim_run.restype = C.c_long
    return L


def check_level(p, g, n_kept, max_features, threshold):
    """What lets the reference's level stand for the definition; -> (None, the level was cut) or (the reason it does not, _).  p: the reference's plane,
    n_kept: the points the reference returned for the level."""
    corners, _ = fm.fast(p, threshold, FAST_TYPE, NONMAX, -1)
    if len(corners) > INNER_FAST_CUT:
        return "more than 2000 corners: the inner FAST detector's own default cut", False
    cut = max_features > 0 and len(corners) > g["quota"]
    if cut:
        s = np.sort(corners["strength"])[::-1]
        if s[g["quota"] - 1] == s[g["quota"]]:
            return "tie at the quota boundary", True
        corners = fm.cut(corners, g["quota"])
    # The reference's ORB detector runs ONE inner FAST detector over all levels, and that detector keeps its strength map while the stride stays the same
    # (compv_core_feature_fast_dete.cxx:192-197): on such a level it reports stale corners of the wider level before at x >= W - 3.  The border erase
    # removes them all, but in a cut level they take places of the quota first.  A level where that happened keeps fewer points than the definition.
    if n_kept != int(om.admissible(corners["x"], corners["y"], g["W"], g["H"]).sum()):
        return "stale corners of the reused inner detector took places of the quota", cut
    return None, cut


def run_pyramid(L, img, levels, sf, max_features, threshold):
    H, W = img.shape
    img = np.ascontiguousarray(img)
    planes = np.zeros(W * H * levels, np.uint8)
    dims, scales, sfs = np.zeros(2 * levels, np.int32), np.zeros(levels, np.float32), C.c_float(0)
    pts, desc = np.zeros(PTS_CAP, om.KEYPOINT_DTYPE), np.zeros((PTS_CAP, 32), np.uint8)
    n = L.pyrshim_run(img.ctypes.data, W, H, levels, sf, max_features, threshold, planes.ctypes.data, planes.size, dims.ctypes.data, scales.ctypes.data, C.byref(sfs),
                      pts.ctypes.data, PTS_CAP, desc.ctypes.data)
    assert n >= 0, n
    out, off = [], 0
    for l in range(levels):
        w, h = int(dims[2 * l]), int(dims[2 * l + 1])
        out.append(planes[off:off + w * h].reshape(h, w).copy())
        off += w * h
    return out, scales, np.float32(sfs.value), pts[:n], desc[:n]


def main():
    RefShim(threads=1)          # refshim_init(1): the reference on one thread
    out = {"scales": [], "pyramids": [], "fast_type": FAST_TYPE, "nonmax": NONMAX}
    arrays = {}
    exact_all = []
    with tempfile.TemporaryDirectory() as tmp:
        L = bind(build_shim(tmp))
        for k, (W, H, Wo, Ho) in enumerate(SCALES):
            assert Wo <= W and Ho <= H and pm.reads_inside(W, H, Wo, Ho), "the reference is never run where it reads outside the plane"
            seed = 51000 + k
            img = np.ascontiguousarray(fm.noise(W, H, seed))
            dst = np.zeros((Ho, Wo), np.uint8)
            assert L.pyrshim_scale(img.ctypes.data, W, H, Wo, Ho, dst.ctypes.data) == 0
            arrays["scale_%d" % k] = dst
            out["scales"].append({"W": W, "H": H, "Wout": Wo, "Hout": Ho, "content": "noise", "seed": seed, "md5": md5(dst)})
        for c, (W, H, kind, seed, levels, sf, mf, thr) in enumerate(PYRAMIDS):
            img = frame(kind, W, H, seed)
            planes, scales, sfs, pts, desc = run_pyramid(L, img, levels, sf, mf, thr)
            geo = pm.geometry(W, H, levels, sf, mf)
            case = {"W": W, "H": H, "content": kind, "seed": seed, "levels": levels, "scale_factor_bits": bits([sf])[0], "max_features": mf, "threshold": thr, "sfs_bits": bits([sfs])[0],
                    "level": []}
            assert (planes[0] == img).all(), "level 0 is the input"
            cuts = 0
            for l, g in enumerate(geo):
                p = planes[l]
                assert p.shape == (g["H"], g["W"]) and bits([scales[l]]) == bits([g["scale"]]), (l, p.shape, g)
                if g["empty"]:
                    assert not (pts["level"] == l).any(), "an empty level contributes nothing in the reference either"
                    case["level"].append({"W": g["W"], "H": g["H"], "empty": True})
                    continue
                assert l == 0 or pm.reads_inside(W, H, g["W"], g["H"])
                sel = np.nonzero(pts["level"] == l)[0]
                why, was_cut = check_level(p, g, len(sel), mf, thr)          # on the reference's own plane
                assert why is None, "level %d of case %d: %s: pick another seed" % (l, c, why)
                cuts += was_cut
                k, d = pts[sel], desc[sel]
                sfl = np.float32(scales[l])
                xi, ok_x = om.centre(k["x"], sfl)
                yi, ok_y = om.centre(k["y"], sfl)
                assert ok_x.all() and ok_y.all() and om.admissible(xi, yi, g["W"], g["H"]).all(), "a fed point inside the 18-pixel margin: pick another seed"
                order = np.lexsort((xi, yi))
                k, d, xi, yi = k[order], d[order], xi[order], yi[order]
                # the record is what the level's integers give (so the integers are all the file needs)
                x, y = xi.astype(np.float32), yi.astype(np.float32)
                if l:
                    sfi = np.float32(1.0) / sfl
                    x, y = x * sfi, y * sfi
                assert bits(k["x"]) == bits(x) and bits(k["y"]) == bits(y) and (k["size"] == np.float32(31.0) / sfl).all()
                assert (k["strength"] == np.rint(k["strength"])).all() and k["strength"].max(initial=0) < 256
                ex = libm_exact(k["orient"])
                exact_all += ex
                pre = "c%d_l%d_" % (c, l)
                arrays[pre + "xy"] = np.stack([xi, yi], axis=1).astype(np.int16)
                arrays[pre + "strength"] = k["strength"].astype(np.uint8)
                arrays[pre + "orient"] = k["orient"].view(np.uint32).copy()
                arrays[pre + "desc"] = d
                arrays[pre + "exact"] = np.packbits(np.array(ex, bool))
                if (W, H) == FULL_PLANES and l:
                    arrays[pre + "plane"] = p
                case["level"].append({"W": g["W"], "H": g["H"], "empty": False, "scale_bits": bits([scales[l]])[0], "plane_md5": md5(p), "quota": g["quota"], "points": len(k)})
            assert mf <= 0 or mf >= 2000 or cuts > 0, "a cut case cuts at least one level"
            out["pyramids"].append(case)
    inexact = 1.0 - sum(exact_all) / len(exact_all)
    assert inexact <= 0.05, inexact
    with open(os.path.join(HERE, "golden_orb_pyramid.json"), "w") as f:
        json.dump(out, f, indent=None, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    np.savez_compressed(os.path.join(HERE, "golden_orb_pyramid.npz"), **arrays)
    print("wrote %d scales, %d pyramids, %d points (%.2f %% with a libm cosf / sinf off the canonical value)" % (len(SCALES), len(PYRAMIDS), len(exact_all), 100 * inexact))


if __name__ == "__main__":
    main()
