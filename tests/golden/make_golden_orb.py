#!/usr/bin/env python
"""Generate tests/golden/golden_orb.json (+ golden_orb.npz) from the COMPILED REFERENCE (oracle/_ref, built by oracle/build_ref.sh): the patch
moments CompVPatch::moments0110 returns, the descriptors CompVCornerDescORB::process writes for keypoints fed to it, the MD5 of the level plane it
blurred, and the points its ORB detector found.  Run in the build container only: it compiles the small shim below (our own code: it only CALLS the
reference's public API -- CompVPatch, CompVCornerDete / CompVCornerDesc with COMPV_ORB_ID, the detector's pyramid) into a temporary directory and
links it against oracle/_ref/libcompv_ref.so.  The reference runs on one thread (refshim_init(1)); every case gets a fresh detector and descriptor,
because the descriptor blurs the detector's pyramid in place.

Inputs are frames any box can regenerate (tests/fast_model.py, numpy default_rng seeds).  The plane of a case is what the reference's pyramid holds
for the level after dete->process and before desc->process: for level 0 the generator asserts it equals the input (so only the seed is recorded), the
level-1 plane -- data the reference's scaler wrote -- goes to golden_orb.npz.

Per fed keypoint the file holds the 32 descriptor bytes and `libm_exact`: whether THIS glibc's cosf / sinf of the fed angle (called through ctypes on
the same libm the reference calls) equal the canonical float32 of the binary64 cos / sin.  Where they do not, the reference's descriptor may differ
from the definition in the bits whose rotated coordinates sit on a rounding boundary; tests/test_orb_model.py compares the others bit for bit."""
import ctypes as C
import hashlib, json, os, subprocess, sys, tempfile
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(HERE, ".."))
from oracle_bindings import RefShim  # noqa: E402
import fast_model as fm  # noqa: E402
import orb_model as om  # noqa: E402

SHIM = r"""
#include <compv/base/compv_base.h>
#include <compv/base/compv_features.h>
#include <compv/base/compv_mat.h>
#include <compv/base/compv_patch.h>
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
// m[2 * i] = m01, m[2 * i + 1] = m10 of the patch of diameter 31 around (xs[i], ys[i]); in: H rows of W bytes
int orbshim_moments(const uint8_t* in, size_t W, size_t H, const int32_t* xs, const int32_t* ys, size_t n, int32_t* m)
{
	CompVMatPtr img;
	if (makeImage(img, in, W, H)) return -1;
	CompVPatchPtr patch;
	if (COMPV_ERROR_CODE_IS_NOK(CompVPatch::newObj(&patch, 31))) return -2;
	for (size_t i = 0; i < n; ++i) {
		int m01 = 0, m10 = 0;
		if (COMPV_ERROR_CODE_IS_NOK(patch->moments0110(img->ptr<const uint8_t>(), xs[i], ys[i], W, H, img->stride(), &m01, &m10))) return -3;
		m[2 * i] = m01; m[2 * i + 1] = m10;
	}
	return 0;
}
// An ORB detector with `levels` pyramid levels runs on the frame; the plane of `level` is copied out (dims: cols, rows), then an ORB descriptor attached to
// the detector describes `nFeed` keypoints {x, y, orient} of that level (nFeed < 0: the detector's own points of the level, at most -nFeed) and the
// blurred plane is copied out.  dete: the detector's points of the level as 24-byte CompVInterestPoint records, *nDete of them (at most deteCap).
// fedOut: the records fed to the descriptor.  -> number of described points, or < 0.
long orbshim_describe(const uint8_t* in, size_t W, size_t H, int levels, int level, const float* feed, long nFeed, uint8_t* plane, uint8_t* blurred,
                      int32_t* dims, float* scale, uint8_t* desc, void* dete, size_t deteCap, size_t* nDete, void* fedOut)
{
	CompVMatPtr img;
	if (makeImage(img, in, W, H)) return -1;
	CompVCornerDetePtr det;
	if (COMPV_ERROR_CODE_IS_NOK(CompVCornerDete::newObj(&det, COMPV_ORB_ID))) return -2;
	if (COMPV_ERROR_CODE_IS_NOK(det->set(COMPV_ORB_SET_INT_PYRAMID_LEVELS, &levels, sizeof(levels)))) return -3;
	CompVInterestPointVector pts;
	if (COMPV_ERROR_CODE_IS_NOK(det->process(img, pts))) return -4;
	const void* vp = NULL;
	if (COMPV_ERROR_CODE_IS_NOK(det->get(COMPV_FEATURE_GET_PTR_PYRAMID, &vp, sizeof(CompVImageScalePyramid))) || !vp) return -5;
	CompVImageScalePyramidPtr pyr = reinterpret_cast<CompVImageScalePyramid*>(const_cast<void*>(vp));
	CompVMatPtr lv;
	if (COMPV_ERROR_CODE_IS_NOK(pyr->image(level, &lv))) return -6;
	dims[0] = (int32_t)lv->cols(); dims[1] = (int32_t)lv->rows();
	copyPlane(lv, plane);
	const float sf = pyr->scaleFactor(level);
	*scale = sf;
	CompVInterestPointVector own, fed;
	for (size_t i = 0; i < pts.size(); ++i) if (pts[i].level == level) own.push_back(pts[i]);
	*nDete = own.size() < deteCap ? own.size() : deteCap;
	memcpy(dete, own.data(), *nDete * sizeof(CompVInterestPoint));
	if (nFeed < 0) { for (size_t i = 0; i < own.size() && i < (size_t)-nFeed; ++i) fed.push_back(own[i]); }
	else for (long i = 0; i < nFeed; ++i) fed.push_back(CompVInterestPoint(feed[3 * i], feed[3 * i + 1], 1.f, feed[3 * i + 2], level, 31.f / sf));
	memcpy(fedOut, fed.data(), fed.size() * sizeof(CompVInterestPoint));
	CompVCornerDescPtr dsc;
	if (COMPV_ERROR_CODE_IS_NOK(CompVCornerDesc::newObj(&dsc, COMPV_ORB_ID, det))) return -7;
	CompVMatPtr rows;
	if (COMPV_ERROR_CODE_IS_NOK(dsc->process(img, fed, &rows))) return -8;
	if (!fed.empty() && (!rows || rows->rows() != fed.size() || rows->cols() != 32)) return -9;
	for (size_t i = 0; i < fed.size(); ++i) memcpy(desc + 32 * i, rows->ptr<const uint8_t>(i), 32);
	if (COMPV_ERROR_CODE_IS_NOK(pyr->image(level, &lv))) return -10;
	copyPlane(lv, blurred);
	return (long)fed.size();
}
}
"""

MOMENT_SIZES = ((37, 37), (64, 41), (200, 258))          # W, H
DESC_CASES = (          # W, H, content, positions
    (37, 37, "noise", 1), (64, 41, "noise", 12), (64, 41, "blocks", 12), (200, 258, "noise", 40), (200, 258, "blocks", 40))
LEVEL1 = (200, 258, "blocks", 150)          # W, H, content, detector points described at most
DETE_CAP = 4096


def frame(kind, W, H, seed):
    return fm.noise(W, H, seed) if kind == "noise" else fm.blocks(W, H, seed)


def build_shim(tmp):
    ref = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"          # the default of oracle/build_ref.sh
    src = os.path.join(tmp, "orb_shim.cxx")
    so = os.path.join(tmp, "liborb_shim.so")
    with open(src, "w") as f:
        f.write(SHIM)
    refdir = os.path.join(ROOT, "oracle", "_ref")
    subprocess.check_call(["g++", "-include", "limits", "-std=c++11", "-O2", "-fPIC", "-w", "-DCOMPV_ASM=0", "-I%s/base/include" % ref, "-I%s/core/include" % ref,
                           "-shared", "-o", so, src, "-L" + refdir, "-lcompv_ref", "-Wl,-rpath," + refdir, "-ldl", "-lpthread"])
    return C.CDLL(so)


def bits(a):
    return [int(v) for v in np.asarray(a, np.float32).view(np.uint32)]


def libm_exact(orient):
    """does this glibc's cosf / sinf of the fed angle equal the canonical float32 of the binary64 cos / sin"""
    libm = C.CDLL("libm.so.6")
    libm.cosf.restype = libm.sinf.restype = C.c_float
    libm.cosf.argtypes = libm.sinf.argtypes = [C.c_float]
    fcos, fsin, a = om.canonical_cos_sin(orient)
    return [bool(np.float32(libm.cosf(float(v))) == c and np.float32(libm.sinf(float(v))) == s) for v, c, s in zip(a, fcos, fsin)]


def describe(L, img, levels, level, feed, n_feed):
    H, W = img.shape
    img = np.ascontiguousarray(img)
    plane, blurred = np.zeros(W * H, np.uint8), np.zeros(W * H, np.uint8)
    dims, scale = np.zeros(2, np.int32), C.c_float(0)
    cap = max(abs(n_feed), 1)
    desc, fed = np.zeros((cap, 32), np.uint8), np.zeros(cap, om.KEYPOINT_DTYPE)
    dete, n_dete = np.zeros(DETE_CAP, om.KEYPOINT_DTYPE), C.c_size_t(0)
    feed = np.ascontiguousarray(feed, np.float32)
    n = L.orbshim_describe(img.ctypes.data, W, H, levels, level, feed.ctypes.data, n_feed, plane.ctypes.data, blurred.ctypes.data, dims.ctypes.data, C.byref(scale),
                           desc.ctypes.data, dete.ctypes.data, DETE_CAP, C.byref(n_dete), fed.ctypes.data)
    assert n >= 0, n
    w, h = int(dims[0]), int(dims[1])
    return plane[:w * h].reshape(h, w), blurred[:w * h].reshape(h, w), np.float32(scale.value), desc[:n], fed[:n], dete[:n_dete.value]


def main():
    RefShim(threads=1)          # refshim_init(1): the reference on one thread
    vp, sz, i, lg = C.c_void_p, C.c_size_t, C.c_int, C.c_long
    out = {"moments": [], "descriptors": []}
    arrays = {}
    all_desc, exact = [], []
    with tempfile.TemporaryDirectory() as tmp:
        L = build_shim(tmp)
        L.orbshim_moments.argtypes = [vp, sz, sz, vp, vp, sz, vp]
        L.orbshim_describe.argtypes = [vp, sz, sz, i, i, vp, lg, vp, vp, vp, vp, vp, vp, sz, vp, vp]
        L.orbshim_describe.restype = lg
        seed = 31000
        for (W, H) in MOMENT_SIZES:
            for kind in ("noise", "blocks"):
                seed += 1
                img = np.ascontiguousarray(frame(kind, W, H, seed))
                rng = np.random.default_rng(seed + 700000)
                n = min(40, (W - 30) * (H - 30))
                xs = rng.integers(15, W - 15, n).astype(np.int32)          # the disc fits: the reference's interior path
                ys = rng.integers(15, H - 15, n).astype(np.int32)
                m = np.zeros((n, 2), np.int32)
                assert L.orbshim_moments(img.ctypes.data, W, H, xs.ctypes.data, ys.ctypes.data, n, m.ctypes.data) == 0
                out["moments"].append({"W": W, "H": H, "content": kind, "seed": seed, "x": xs.tolist(), "y": ys.tolist(), "m01": m[:, 0].tolist(), "m10": m[:, 1].tolist()})
        for (W, H, kind, npos) in DESC_CASES:
            seed += 1
            img = frame(kind, W, H, seed)
            rng = np.random.default_rng(seed + 700000)
            xs = rng.integers(om.BORDER, W - om.BORDER, npos)
            ys = rng.integers(om.BORDER, H - om.BORDER, npos)
            m01, m10 = om.moments(img, xs, ys)
            canon = om.orient_of(m01, m10)
            if npos == 1:          # the one admissible position of 37 x 37: every fixed orientation
                feed = [(xs[0], ys[0], canon[0])] + [(xs[0], ys[0], o) for o in om.FIXED_ORIENTS]
            else:
                feed = [(x, y, o) for x, y, o in zip(xs, ys, canon)] + [(x, y, om.FIXED_ORIENTS[k % len(om.FIXED_ORIENTS)]) for k, (x, y) in enumerate(zip(xs, ys))]
            feed = np.array(feed, np.float32)
            plane, blurred, scale, desc, fed, dete = describe(L, img, 1, 0, feed, len(feed))
            assert (plane == img).all() and scale == 1.0, "level 0 is the input"
            ex = libm_exact(fed["orient"])
            case = {"W": W, "H": H, "content": kind, "seed": seed, "level": 0, "scale_bits": bits([scale])[0], "x_bits": bits(fed["x"]), "y_bits": bits(fed["y"]),
                    "orient_bits": bits(fed["orient"]), "desc": desc.tobytes().hex(), "libm_exact": "".join("1" if e else "0" for e in ex),
                    "blurred_md5": hashlib.md5(blurred.tobytes()).hexdigest()}
            if (W, H, kind) == (200, 258, "blocks"):          # the detector's own level-0 points, for the orientation bound
                case["dete"] = {"x_bits": bits(dete["x"]), "y_bits": bits(dete["y"]), "orient_bits": bits(dete["orient"])}
            out["descriptors"].append(case)
            all_desc.append(desc); exact += ex
        W, H, kind, cap = LEVEL1
        seed += 1
        img = frame(kind, W, H, seed)
        plane, blurred, scale, desc, fed, dete = describe(L, img, 2, 1, np.zeros(3, np.float32), -cap)
        assert len(fed) > 20, len(fed)
        ex = libm_exact(fed["orient"])
        arrays["level1_plane"] = plane
        out["descriptors"].append({"W": int(plane.shape[1]), "H": int(plane.shape[0]), "content": "level1_plane", "seed": seed, "level": 1, "scale_bits": bits([scale])[0],
                                   "x_bits": bits(fed["x"]), "y_bits": bits(fed["y"]), "orient_bits": bits(fed["orient"]), "desc": desc.tobytes().hex(),
                                   "libm_exact": "".join("1" if e else "0" for e in ex), "blurred_md5": hashlib.md5(blurred.tobytes()).hexdigest(),
                                   "dete": {"x_bits": bits(dete["x"]), "y_bits": bits(dete["y"]), "orient_bits": bits(dete["orient"])}})
        all_desc.append(desc); exact += ex
    every = np.unpackbits(np.concatenate(all_desc), axis=1)
    assert every.any(axis=0).all() and (~every.astype(bool)).any(axis=0).all(), "every one of the 256 bits takes both values"
    inexact = 1.0 - sum(exact) / len(exact)
    assert inexact <= 0.05, inexact
    with open(os.path.join(HERE, "golden_orb.json"), "w") as f:
        json.dump(out, f, indent=None, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    np.savez_compressed(os.path.join(HERE, "golden_orb.npz"), **arrays)
    print("wrote %d moment points, %d descriptors (%.2f %% with a libm cosf / sinf off the canonical value)" %
          (sum(len(c["x"]) for c in out["moments"]), len(exact), 100 * inexact))


if __name__ == "__main__":
    main()
