#!/usr/bin/env python
"""Generate tests/golden/golden_moments.json (+ golden_moments.npz) from tests/moments_cases.py, held against the COMPILED REFERENCE (oracle/_ref,
built by oracle/build_ref.sh).  Run in the build container only: it compiles the small shim below (our own code: it only CALLS the reference --
CompVMathMoments::rawFirstOrder, rawSecondOrder, skewness, orientation on uint8 mats) into a temporary directory and links it against
oracle/_ref/libcompv_ref.so.  The reference runs on one thread (refshim_init(1)).

Before it writes anything the generator asserts, for every case whose six sums stay below 2^53, that tests/moments_model.py equals the reference on
EVERY bit of all six sums (and of the three of rawFirstOrder) and of skew, and measures the angle distance |atan2(sn, cs) - theta| on the cases where
the -0 branch of atan2 plays no part (2 * u11 != 0 or den > 0).  One mismatch fails it; nothing is skipped or retried.  UNIT weights go through the
reference as the 0 / 1 plane; a component goes through it as the frame (ORIGIN_FRAME) or the blob's crop (ORIGIN_BOX) with every foreign pixel zeroed.
A case that cannot be held against the reference is marked "model only" with its reason; at most two may be.

Stored: the raw records (.npz, uint64), the reference's skew and theta, the largest angle distance seen (.json)."""
import ctypes as C
import json, os, subprocess, sys, tempfile
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(HERE, ".."))
from oracle_bindings import RefShim  # noqa: E402
import moments_cases as mc  # noqa: E402
import moments_model as mm  # noqa: E402

SHIM = r"""
#include <compv/base/compv_base.h>
#include <compv/base/compv_mat.h>
#include <compv/base/image/compv_image.h>
#include <compv/base/math/compv_math_moments.h>
#include <cstring>
using namespace compv;
extern "C" {
// one uint8 plane of W x H (rows of W bytes): rawSecondOrder -> m6, rawFirstOrder -> m3, skewness, orientation
int momshim_frame(const uint8_t* in, size_t W, size_t H, int binar, double* m6, double* m3, double* skew, double* theta)
{
	CompVMatPtr img;
	if (COMPV_ERROR_CODE_IS_NOK(CompVImage::newObj8u(&img, COMPV_SUBTYPE_PIXELS_Y, W, H, 0))) return -1;
	for (size_t j = 0; j < H; ++j) memcpy(img->ptr<uint8_t>(j), in + j * W, W);
	double a[6], b[3];
	if (COMPV_ERROR_CODE_IS_NOK(CompVMathMoments::rawSecondOrder(img, a, binar != 0))) return -2;
	if (COMPV_ERROR_CODE_IS_NOK(CompVMathMoments::rawFirstOrder(img, b, binar != 0))) return -3;
	if (COMPV_ERROR_CODE_IS_NOK(CompVMathMoments::skewness(img, *skew, binar != 0))) return -4;
	if (COMPV_ERROR_CODE_IS_NOK(CompVMathMoments::orientation(img, *theta, binar != 0))) return -5;
	memcpy(m6, a, sizeof(a)); memcpy(m3, b, sizeof(b));
	return 0;
}
}
"""


def build_shim(tmp, ref="/root/reference"):          # the default of oracle/build_ref.sh
    src = os.path.join(tmp, "moments_shim.cxx")
    so = os.path.join(tmp, "libmoments_shim.so")
    with open(src, "w") as f:
        f.write(SHIM)
    refdir = os.path.join(ROOT, "oracle", "_ref")
    subprocess.check_call(["g++", "-include", "limits", "-std=c++11", "-O2", "-fPIC", "-w", "-DCOMPV_ASM=0", "-I%s/base/include" % ref, "-shared",
                           "-o", so, src, "-L" + refdir, "-lcompv_ref", "-Wl,-rpath," + refdir, "-ldl", "-lpthread"])
    L = C.CDLL(so)
    L.momshim_frame.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    return L


def reference(L, plane, binar=0):
    """(the six sums, the three of rawFirstOrder, skew, theta) of a uint8 plane, doubles"""
    plane = np.ascontiguousarray(plane, np.uint8)
    h, w = plane.shape
    m6, m3, skew, theta = np.zeros(6), np.zeros(3), C.c_double(), C.c_double()
    rc = L.momshim_frame(plane.ctypes.data, w, h, binar, m6.ctypes.data, m3.ctypes.data, C.byref(skew), C.byref(theta))
    assert rc == 0, rc
    return m6, m3, skew.value, theta.value


def bits(x):
    return np.float64(x).tobytes()


class Pin:
    """holds the model against the reference, case by case"""

    def __init__(self, L):
        self.L, self.compared, self.angle, self.angle_cases = L, 0, 0.0, 0

    def check(self, what, plane, sums, binar=0):
        """plane: what the reference gets; sums: the model's record.  -> (skew, theta) of the reference"""
        assert max(sums) < 2 ** 53, what
        m6, m3, skew, theta = reference(self.L, plane, binar)
        for k in range(6):
            assert bits(m6[k]) == bits(float(sums[k])), "%s: %s is %r in the reference, %d in the model" % (what, mm.NAMES[k], m6[k], sums[k])
        assert m3.tobytes() == m6[:3].tobytes(), what
        s = mm.shape(sums)
        assert bits(skew) == bits(s["skew"]), "%s: skew is %r in the reference, %r in the model" % (what, skew, s["skew"])
        if mm.angle_case(s):
            self.angle = max(self.angle, abs(mm.theta(s) - theta))
            self.angle_cases += 1
        elif s["status"] == 1 or abs(s["u20"] - s["u02"]) <= mm.EPS:
            assert theta == 0.0 and (s["cs"], s["sn"]) == (1.0, 0.0), what
        self.compared += 1
        return skew, theta


def main():
    ref = RefShim(threads=1)          # refshim_init(1): the reference on one thread
    assert ref.threads == 1
    meta = {"frames": [], "components": [], "model_only": []}
    arrays = {}
    with tempfile.TemporaryDirectory() as tmp:
        pin = Pin(build_shim(tmp, *sys.argv[1:2]))
        for c in mc.frame_cases():
            img = mc.frame(c)
            for weights in c["weights"]:
                name = "%s_%s" % (c["id"], ("value", "unit")[weights])
                sums = mm.raw_sums(img, weights)
                rec = {"id": name, "case": c["id"], "weights": weights, "size": list(c["size"]), "sums": [int(v) for v in sums]}
                if max(sums) >= 2 ** 53:
                    big = [mm.NAMES[k] for k in range(6) if sums[k] >= 2 ** 53]
                    m6 = reference(pin.L, img)[0]
                    differ = [mm.NAMES[k] for k in range(6) if int(m6[k]) != sums[k]]
                    meta["model_only"].append({"id": name, "reason": "%s above 2^53: the reference's double partial sums round (its %s differ from the exact sums)"
                                               % (", ".join(big), ", ".join(differ) or "sums happen not to")})
                    rec["model_only"] = True
                else:
                    # UNIT: what `binar` promises is the reference on the 0 / 1 plane (binar itself is accepted and ignored: passed along all the same)
                    plane = (img != 0).astype(np.uint8) if weights == mm.UNIT else img
                    skew, theta = pin.check(name, plane, sums, int(weights == mm.UNIT))
                    rec["skew"], rec["theta"] = float(skew).hex(), float(theta).hex()
                    if weights == mm.VALUE and c["kind"] == "bin01":
                        assert sums == mm.raw_sums(img, mm.UNIT)
                arrays["raw_" + name] = mm.raw_array([sums])[0]
                meta["frames"].append(rec)
                print("%-18s %5d x %-5d m00 %d" % (name, c["size"][0], c["size"][1], sums[0]))
        for c in mc.component_cases():
            labels, comps = mc.labelled(c)
            gray = mc.component_frame(c)[1] if c["gray"] else None
            assert len(comps) >= 3, c["id"]
            sums = mm.component_sums(labels, comps, len(comps), len(comps), gray, c["weights"], c["origin"])
            skews, thetas = [], []
            for k, s in enumerate(sums):
                cid = k + 1
                if c["origin"] == mm.ORIGIN_BOX:
                    plane = mm.crop_of(labels, comps[k], cid, gray, c["weights"])
                else:
                    mask = labels == cid
                    plane = mask.astype(np.uint8) if gray is None else (mm.pixel_weights(gray, c["weights"]) * mask).astype(np.uint8)
                skew, theta = pin.check("%s component %d" % (c["id"], cid), plane, s)
                skews.append(skew); thetas.append(theta)
            if gray is not None and c["weights"] == mm.VALUE:
                assert any(((labels == k + 1) & (gray == 0)).any() for k in range(len(comps))), "no zero-valued pixel inside a blob"
            arrays["raw_" + c["id"]] = mm.raw_array(sums)
            arrays["skew_" + c["id"]], arrays["theta_" + c["id"]] = np.array(skews), np.array(thetas)
            meta["components"].append({"id": c["id"], "components": len(comps)})
            print("%-22s %d components" % (c["id"], len(comps)))
    assert len(meta["model_only"]) <= 2 and [m["id"] for m in meta["model_only"]] == [mc.BIG + "_value"], meta["model_only"]
    assert pin.angle_cases >= 20, pin.angle_cases
    meta["max_angle_distance"], meta["angle_cases"], meta["compared"] = pin.angle, pin.angle_cases, pin.compared
    with open(os.path.join(HERE, "golden_moments.json"), "w") as f:
        json.dump(meta, f, indent=None, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    np.savez_compressed(os.path.join(HERE, "golden_moments.npz"), **arrays)
    print("wrote %d frame and %d component cases; %d planes compared with the reference, 0 mismatches; largest angle distance %.3g over %d planes; model only: %s"
          % (len(meta["frames"]), len(meta["components"]), pin.compared, pin.angle, pin.angle_cases, [m["id"] for m in meta["model_only"]]))


if __name__ == "__main__":
    main()
