#!/usr/bin/env python
"""Generate tests/golden/golden_curvefit.json (+ golden_curvefit.npz) from tests/curvefit_model.py, held against the COMPILED REFERENCE (oracle/_ref,
built by oracle/build_ref.sh).  Run in the build container only: it compiles the small shim below (our own code: it only CALLS the reference's
public API -- CompVMathStatsFit::line / ::parabola, CompVMathDistance::line / ::parabola, CompVCpu::flagsDisable) into a temporary directory and
links it against oracle/_ref/libcompv_ref.so.  The reference runs on one thread.

Asserted before anything is written:
 1. item B bit for bit: the public fit calls with exactly 2 (line) or 3 (parabolas) float64 points take the direct path of
    compv_math_stats_fit.cxx:53-65 / :101-114, no random number; rejected sets (zeros) included.
 2. item C bit for bit: CompVMathDistance on float64 points (plain C leaves) -- vertical, horizontal and slanted lines, both parabola types.
 3. noise-free planted sets (tests/curvefit_cases.py: integer coordinates, 30 % outliers at least 4 x threshold off the curve): the model's mask at 200
    tries is the planted set; the points within the threshold of the reference's returned curve (its own CompVMathDistance) are the planted set --
    the public call returns no count, this is how its inlier set is read, and a run that misses it fails the generator outright, it is not retried --;
    model and reference curves lie within 1e-6 px of each other over the set's extent.
 4. noisy sets: the model's refit lies within 1e-6 px of an independent least-squares solve of the same inliers in longdouble (parabola: QR by modified
    Gram-Schmidt; line: the total-least-squares angle by libm's atan2l).  The reference's result on the same set is compared with that solve too; its
    distance is RECORDED (reference_px), asserted nowhere: the stopping rule of its Levenberg-Marquardt is the reference's business.
Stored: the point sets, the planted flags, per case the record bytes, the mask, the per-try counts and the samples' first rows."""
import ctypes as C
import json, os, subprocess, sys, tempfile
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(HERE, ".."))
from oracle_bindings import RefShim  # noqa: E402
import curvefit_model as cm  # noqa: E402
import curvefit_cases as cc  # noqa: E402

SHIM = r"""
#include <compv/base/compv_base.h>
#include <compv/base/compv_cpu.h>
#include <compv/base/compv_mat.h>
#include <compv/base/math/compv_math_distance.h>
#include <compv/base/math/compv_math_stats_fit.h>
using namespace compv;
static int points(CompVMatPtr& m, const double* xy, size_t n)
{
	if (COMPV_ERROR_CODE_IS_NOK(CompVMat::newObjAligned<compv_float64_t>(&m, 2, n))) return -1;
	for (size_t i = 0; i < n; ++i) { *m->ptr<compv_float64_t>(0, i) = xy[2 * i]; *m->ptr<compv_float64_t>(1, i) = xy[2 * i + 1]; }
	return 0;
}
extern "C" {
int cfshim_plain_c(void) { return COMPV_ERROR_CODE_IS_NOK(CompVCpu::flagsDisable(kCpuFlagAll)) ? -1 : 0; }
// model 0: CompVMathStatsFit::line; 1 / 2: ::parabola REGULAR / SIDEWAYS -> params[3]
int cfshim_fit(const double* xy, size_t n, int model, double threshold, double* params)
{
	CompVMatPtr p, r;
	if (points(p, xy, n)) return -1;
	const COMPV_ERROR_CODE e = model == 0 ? CompVMathStatsFit::line(p, threshold, &r)
		: CompVMathStatsFit::parabola(p, threshold, &r, model == 2 ? COMPV_MATH_PARABOLA_TYPE_SIDEWAYS : COMPV_MATH_PARABOLA_TYPE_REGULAR);
	if (COMPV_ERROR_CODE_IS_NOK(e)) return -2;
	for (int i = 0; i < 3; ++i) params[i] = *r->ptr<const compv_float64_t>(0, i);
	return 0;
}
int cfshim_distances(const double* xy, size_t n, int model, const double* params, double* dist)
{
	CompVMatPtr p, d;
	if (points(p, xy, n)) return -1;
	const double eq[3] = { params[0], params[1], params[2] };
	const COMPV_ERROR_CODE e = model == 0 ? CompVMathDistance::line(p, eq, &d)
		: CompVMathDistance::parabola(p, eq, &d, model == 2 ? COMPV_MATH_PARABOLA_TYPE_SIDEWAYS : COMPV_MATH_PARABOLA_TYPE_REGULAR);
	if (COMPV_ERROR_CODE_IS_NOK(e)) return -2;
	for (size_t i = 0; i < n; ++i) dist[i] = d->ptr<const compv_float64_t>()[i];
	return 0;
}
}
"""


def build_shim(tmp, ref="/root/reference"):          # the default of oracle/build_ref.sh
    src = os.path.join(tmp, "curvefit_shim.cxx")
    so = os.path.join(tmp, "libcurvefit_shim.so")
    with open(src, "w") as f:
        f.write(SHIM)
    refdir = os.path.join(ROOT, "oracle", "_ref")
    subprocess.check_call(["g++", "-include", "limits", "-std=c++11", "-O2", "-fPIC", "-w", "-DCOMPV_ASM=0", "-I%s/base/include" % ref, "-shared", "-o", so, src,
                           "-L" + refdir, "-lcompv_ref", "-Wl,-rpath," + refdir, "-ldl", "-lpthread"])
    L = C.CDLL(so)
    vp, sz = C.c_void_p, C.c_size_t
    L.cfshim_fit.argtypes = [vp, sz, C.c_int, C.c_double, vp]
    L.cfshim_distances.argtypes = [vp, sz, C.c_int, vp, vp]
    assert L.cfshim_plain_c() == 0
    return L


def ref_fit(L, pts, model, threshold):
    pts = np.ascontiguousarray(pts, np.float64)
    out = np.zeros(3)
    assert L.cfshim_fit(pts.ctypes.data, len(pts), model, threshold, out.ctypes.data) == 0
    return out


def ref_distances(L, pts, model, params):
    pts, params = np.ascontiguousarray(pts, np.float64), np.ascontiguousarray(params, np.float64)
    out = np.zeros(len(pts))
    assert L.cfshim_distances(pts.ctypes.data, len(pts), model, params.ctypes.data, out.ctypes.data) == 0
    return out


def curve_px(model, a, b, pts):
    """the largest distance between two curves (A, B, C) over the set's extent, 257 abscissas"""
    x, _ = cm.xy_of(model, pts[:, 0], pts[:, 1])
    if model == cm.LINE and abs(a[0]) > abs(a[1]):
        x = pts[:, 1]
    t = np.linspace(x.min(), x.max(), 257)
    return float(np.abs(cm.curve_y(model, a[0], a[1], a[2], t) - cm.curve_y(model, b[0], b[1], b[2], t)).max())


def independent(model, sel):
    """the least-squares curve of the points in longdouble"""
    L = np.longdouble
    if model == cm.LINE:
        x, y = sel[:, 0].astype(L), sel[:, 1].astype(L)
        mx, my = x.sum() / len(x), y.sum() / len(y)
        a, b = x - mx, y - my
        phi = L(0.5) * np.arctan2(L(-2) * (a * b).sum(), (b * b - a * a).sum())
        cs, sn = np.cos(phi), np.sin(phi)
        return np.array([cs, sn, -(mx * cs + my * sn)], np.float64)
    x, y = cm.xy_of(model, sel[:, 0], sel[:, 1])
    x, y = x.astype(L), y.astype(L)
    mean = x.sum() / len(x)
    u = x - mean
    cols = [u * u, u, np.ones(len(u), L)]
    Q, R = [], np.zeros((3, 3), L)
    for j in range(3):          # modified Gram-Schmidt
        v = cols[j].copy()
        for i in range(j):
            R[i, j] = (Q[i] * v).sum()
            v = v - R[i, j] * Q[i]
        R[j, j] = np.sqrt((v * v).sum())
        Q.append(v / R[j, j])
    rhs = [(q * y).sum() for q in Q]
    c = rhs[2] / R[2, 2]
    b = (rhs[1] - R[1, 2] * c) / R[1, 1]
    a = (rhs[0] - R[0, 1] * b - R[0, 2] * c) / R[0, 0]
    return np.array([a, b - 2 * a * mean, c - b * mean + a * mean * mean], np.float64)


def store(arrays, cid, out):
    arrays["result_" + cid] = np.frombuffer(out["result"].tobytes(), np.uint8)
    arrays["mask_" + cid] = np.asarray(out["mask"], np.uint8)
    if out["counts"] is not None:
        arrays["counts_" + cid] = out["counts"].astype(np.int16)
        arrays["samples_" + cid] = out["samples"].astype(np.int16)


DIRECT = {          # item B: the points of the direct path, rejected ones included
    cm.LINE: [[(0, 0), (3, 4)], [(5, 1), (5, 9)], [(-2, 7), (11, 7)], [(0.1, 0.7), (1e6, -3.3)], [(4, 4), (4, 4)]],
    cm.PARABOLA: [[(0, 1), (1, 3), (2, 9)], [(-3.5, 2.25), (0.1, 7), (8, -1)], [(1e3, 5), (1e3 + 1, 6), (1e3 - 1, 9)], [(1, 1), (1, 2), (3, 4)], [(1, 1), (2, 2), (2, 4)]],
}
DIRECT[cm.PARABOLA_SIDEWAYS] = [[(y, x) for x, y in s] for s in DIRECT[cm.PARABOLA]]
CURVES = {          # item C: vertical, horizontal, slanted lines; parabolas
    cm.LINE: [(1.0, 0.0, -5.0), (0.0, 1.0, 3.0), (3.0, -4.0, 2.5), (-0.001, 1e3, 7.0)],
    cm.PARABOLA: [(1.0, 0.0, 0.0), (-0.25, 3.5, 17.0), (1e-3, -2.0, 400.0)],
}
CURVES[cm.PARABOLA_SIDEWAYS] = CURVES[cm.PARABOLA]


def main():
    RefShim(threads=1)          # refshim_init(1): the reference on one thread
    meta = {"cases": [], "direct": [], "distances": 0}
    arrays = {}
    with tempfile.TemporaryDirectory() as tmp:
        L = build_shim(tmp, *sys.argv[1:2])
        # 1. item B
        for model in cm.MODELS:
            for i, s in enumerate(DIRECT[model]):
                pts = np.array(s, np.float64)
                ref = ref_fit(L, pts, model, cc.THRESHOLD)
                out = cm.find(pts, len(pts), model, 1, cc.THRESHOLD)
                got = np.array([out["result"]["A"], out["result"]["B"], out["result"]["C"]])
                assert got.tobytes() == ref.tobytes(), ("item B", model, i, got, ref)
                cid = "direct_m%d_%d" % (model, i)
                arrays["pts_" + cid] = pts
                store(arrays, cid, out)
                meta["direct"].append(dict(id=cid, model=model, status=int(out["result"]["status"])))
        assert sorted({d["status"] for d in meta["direct"]}) == [0, 1]
        # 2. item C
        rng = np.random.RandomState(3)
        cloud = np.concatenate([rng.uniform(-500, 500, (200, 2)), rng.randint(-50, 50, (57, 2)).astype(np.float64)])
        arrays["cloud"] = cloud
        for model in cm.MODELS:
            for i, p in enumerate(CURVES[model]):
                ref = ref_distances(L, cloud, model, p)
                got = cm.residuals(model, p[0], p[1], p[2], cloud)[0]
                assert got.tobytes() == ref.tobytes(), ("item C", model, p)
                arrays["dist_m%d_%d" % (model, i)] = got
                meta["distances"] += 1
        # 3. and 4.
        worst = {"planted_px": 0.0, "noisy_px": 0.0, "reference_px": 0.0}
        for model in cm.MODELS:
            for k in cc.KS:
                for share in cc.SHARES:
                    for kind, make in (("planted", cc.planted), ("noisy", cc.noisy)):
                        pts, inl, coef = make(model, k, share, 1)
                        out = cm.find(pts, k, model, 200, cc.THRESHOLD, seed=k, set_index=0)
                        res = out["result"]
                        assert res["status"] == 0
                        mine = np.array([res["A"], res["B"], res["C"]])
                        ref = ref_fit(L, pts, model, cc.THRESHOLD)
                        rec = dict(id="%s_m%d_k%d_s%d" % (kind, model, k, int(share * 100)), kind=kind, model=model, k=k, share=share, tries=200, seed=k,
                                   threshold=cc.THRESHOLD, inliers=int(res["inliers"]), planted=int(inl.sum()))
                        if kind == "planted":
                            assert (out["mask"] != 0).tolist() == inl.tolist(), (rec["id"], "the model misses the planted set")
                            ref_in = ref_distances(L, pts, model, ref) < cc.THRESHOLD
                            assert ref_in.tolist() == inl.tolist(), (rec["id"], "the reference's curve does not select the planted set")
                            rec["px"] = curve_px(model, mine, ref, pts)
                            assert rec["px"] <= 1e-6, (rec["id"], rec["px"])
                            worst["planted_px"] = max(worst["planted_px"], rec["px"])
                        else:
                            solve = independent(model, pts[out["mask"] != 0])
                            rec["px"] = curve_px(model, mine, solve, pts)
                            assert rec["px"] <= 1e-6, (rec["id"], rec["px"])
                            rec["reference_px"] = curve_px(model, ref, solve, pts)          # recorded, asserted nowhere
                            worst["noisy_px"] = max(worst["noisy_px"], rec["px"])
                            worst["reference_px"] = max(worst["reference_px"], rec["reference_px"])
                        arrays["pts_" + rec["id"]] = pts
                        arrays["inl_" + rec["id"]] = inl.astype(np.uint8)
                        store(arrays, rec["id"], out)
                        meta["cases"].append(rec)
    meta["worst"] = worst
    with open(os.path.join(HERE, "golden_curvefit.json"), "w") as f:
        json.dump(meta, f, indent=None, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    np.savez_compressed(os.path.join(HERE, "golden_curvefit.npz"), **arrays)
    print("wrote %d direct sets, %d distance curves, %d cases; worst: %s" % (len(meta["direct"]), meta["distances"], len(meta["cases"]), worst))


if __name__ == "__main__":
    main()
