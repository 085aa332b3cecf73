#!/usr/bin/env python
"""Generate tests/golden/golden_homography.json (+ golden_homography.npz) from tests/homography_model.py, held against the COMPILED REFERENCE
(oracle/_ref, built by oracle/build_ref.sh).  Run in the build container only: it compiles the small shim below (our own code: it only CALLS the
reference's public API) into a temporary directory and links it against oracle/_ref/libcompv_ref.so.  The reference runs on one thread.

The shim calls CompVHomography<double>::find(..., COMPV_MODELEST_TYPE_NONE) -- computeH of the points it is given --, the same with
COMPV_MODELEST_TYPE_RANSAC, and CompVMatrix::mulAB / invA3x3 with CompVMathStats::mse2D_homogeneous in countInliers' sequence (item E).

Cases (tests/homography_cases.py): a known H maps k points of a 640 x 480 frame, inliers with at most 0.05 px of noise, gross outliers; k 4, 5, 9, 63,
64, 65, 129 x outlier shares 0, 30, 60 % x tries 1, 63, 64, 65, 200; a collinear quad, a repeated-index (singular) quad, an out-of-range quad, an
all-outlier pair, a pair whose sources all lie on one line (no try scores: the status 1 path -- an all-outlier pair does NOT take it, because a quad
always fits its own four points), k = 3, a negative count, a count beyond pointCap.

Asserted per case before anything is written (a failing case is reseeded, never weakened):
 (a) model and reference agree on every try's inlier set; no d of any try, the model's or the reference's, lies within 0.1 % of the threshold; the best
     try is unique: no other try with a DIFFERENT inlier set has its count and a variance within 1e-6 relative (tries that reach the best's own
     inlier set -- 200 tries over the 5 quads of k = 5 must repeat them -- lead to the same result, and item F takes the first).  A try on which the
     reference's eigen solver gives up (its H misses the very four points it was computed from; it prints "ops >= maxops") is counted, not compared:
     there the model must fit its quad;
 (b) computeH of the model and of the reference (the final fit) move the four frame corners apart by at most 1e-6 px; the measured value is stored;
 (c) on the planted cases the reference's own RANSAC and the model at 200 tries both return exactly the planted inliers.
Stored: inputs, quads, per-try (count, variance bits, rotations), the result records as bytes, the masks."""
import ctypes as C
import json, os, subprocess, sys, tempfile
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(HERE, ".."))
from oracle_bindings import RefShim  # noqa: E402
import homography_model as hm  # noqa: E402
import homography_cases as hc  # noqa: E402

SHIM = r"""
#include <compv/base/compv_base.h>
#include <compv/base/compv_mat.h>
#include <compv/base/math/compv_math_matrix.h>
#include <compv/base/math/compv_math_stats.h>
#include <compv/core/calib/compv_core_calib_homography.h>
#include <cstring>
using namespace compv;
static int points(CompVMatPtr& m, const double* xy, size_t n)
{
	if (COMPV_ERROR_CODE_IS_NOK(CompVMat::newObjAligned<compv_float64_t>(&m, 3, n))) return -1;
	for (size_t i = 0; i < n; ++i) { *m->ptr<compv_float64_t>(0, i) = xy[2 * i]; *m->ptr<compv_float64_t>(1, i) = xy[2 * i + 1]; *m->ptr<compv_float64_t>(2, i) = 1.0; }
	return 0;
}
static int matrix(CompVMatPtr& m, const double* h)
{
	if (COMPV_ERROR_CODE_IS_NOK(CompVMat::newObjAligned<compv_float64_t>(&m, 3, 3))) return -1;
	for (int i = 0; i < 9; ++i) *m->ptr<compv_float64_t>(i / 3, i % 3) = h[i];
	return 0;
}
extern "C" {
// CompVHomography<double>::find: ransac == 0: COMPV_MODELEST_TYPE_NONE (computeH of all n points); else the reference's RANSAC.  -> H[9], *inliers
int hgshim_find(const double* src, const double* dst, size_t n, int ransac, double* H, size_t* inliers)
{
	CompVMatPtr s, d, h;
	if (points(s, src, n) || points(d, dst, n)) return -1;
	CompVHomographyResult r; r.reset();
	if (COMPV_ERROR_CODE_IS_NOK(CompVHomography<compv_float64_t>::find(s, d, &h, &r, ransac ? COMPV_MODELEST_TYPE_RANSAC : COMPV_MODELEST_TYPE_NONE))) return -2;
	for (int i = 0; i < 9; ++i) H[i] = *h->ptr<const compv_float64_t>(i / 3, i % 3);
	*inliers = r.inlinersCount;
	return 0;
}
// countInliers' sequence for one H: d[i] = mse(Hinv dst, src) + mse(H src, dst); returns 1 when the reference calls H singular
int hgshim_distances(const double* H, const double* src, const double* dst, size_t n, double* dist)
{
	CompVMatPtr h, s, d, b, a, hinv, mseb, msea;
	if (matrix(h, H) || points(s, src, n) || points(d, dst, n)) return -1;
	if (COMPV_ERROR_CODE_IS_NOK(CompVMatrix::mulAB(h, s, &b))) return -2;
	if (COMPV_ERROR_CODE_IS_NOK(CompVMathStats::mse2D_homogeneous<compv_float64_t>(&mseb, b->ptr<compv_float64_t>(0), b->ptr<compv_float64_t>(1), b->ptr<compv_float64_t>(2),
		d->ptr<compv_float64_t>(0), d->ptr<compv_float64_t>(1), n))) return -3;
	bool singular = false;
	if (COMPV_ERROR_CODE_IS_NOK(CompVMatrix::invA3x3(h, &hinv, false, &singular))) return -4;
	if (singular) return 1;
	if (COMPV_ERROR_CODE_IS_NOK(CompVMatrix::mulAB(hinv, d, &a))) return -5;
	if (COMPV_ERROR_CODE_IS_NOK(CompVMathStats::mse2D_homogeneous<compv_float64_t>(&msea, a->ptr<compv_float64_t>(0), a->ptr<compv_float64_t>(1), a->ptr<compv_float64_t>(2),
		s->ptr<compv_float64_t>(0), s->ptr<compv_float64_t>(1), n))) return -6;
	for (size_t i = 0; i < n; ++i) dist[i] = msea->ptr<const compv_float64_t>()[i] + mseb->ptr<const compv_float64_t>()[i];
	return 0;
}
}
"""


def build_shim(tmp, ref="/root/reference"):          # the default of oracle/build_ref.sh
    src = os.path.join(tmp, "homography_shim.cxx")
    so = os.path.join(tmp, "libhomography_shim.so")
    with open(src, "w") as f:
        f.write(SHIM)
    refdir = os.path.join(ROOT, "oracle", "_ref")
    subprocess.check_call(["g++", "-include", "limits", "-std=c++11", "-O2", "-fPIC", "-w", "-DCOMPV_ASM=0", "-I%s/base/include" % ref, "-I%s/core/include" % ref, "-shared",
                           "-o", so, src, "-L" + refdir, "-lcompv_ref", "-Wl,-rpath," + refdir, "-ldl", "-lpthread"])
    L = C.CDLL(so)
    vp, sz = C.c_void_p, C.c_size_t
    L.hgshim_find.argtypes = [vp, vp, sz, C.c_int, vp, C.POINTER(sz)]
    L.hgshim_distances.argtypes = [vp, vp, vp, sz, vp]
    return L


CORNERS = np.array([[0.0, 0.0], [639.0, 0.0], [639.0, 479.0], [0.0, 479.0]])


def ref_find(L, src, dst, ransac=False):
    src, dst = np.ascontiguousarray(src, np.float64), np.ascontiguousarray(dst, np.float64)
    H = np.zeros(9)
    n = C.c_size_t(0)
    assert L.hgshim_find(src.ctypes.data, dst.ctypes.data, len(src), int(ransac), H.ctypes.data, C.byref(n)) == 0
    return H, n.value


def ref_distances(L, H, src, dst):
    H, src, dst = np.ascontiguousarray(H, np.float64), np.ascontiguousarray(src, np.float64), np.ascontiguousarray(dst, np.float64)
    d = np.zeros(len(src))
    rc = L.hgshim_distances(H.ctypes.data, src.ctypes.data, dst.ctypes.data, len(src), d.ctypes.data)
    assert rc in (0, 1), rc
    return None if rc else d


stats = {"compared": 0, "reference_gave_up": 0}


def check_case(L, src, dst, out, threshold, planted=None, tries=0):
    """assertions (a) - (c); returns the corner distance of (b), or raises AssertionError (the caller reseeds)"""
    k = out["k"]
    src, dst = src[:k], dst[:k]
    counts, var = out["counts"], out["variances"]
    for t in range(len(counts)):
        q = out["quads"][t]
        if ((q < 0) | (q >= k)).any() or hm.collinear(src[q][None, :, 0], src[q][None, :, 1])[0]:
            assert counts[t] == 0
            continue
        Href, _ = ref_find(L, src[q], dst[q])          # the reference's computeH of the quad
        d_ref = ref_distances(L, Href, src, dst)
        d_mod = out["distances"][t]
        distinct = len(set(q.tolist())) == 4
        if distinct and (d_ref is None or not (d_ref[q] < 1e-6).all()):
            # The reference's own eigen solver gave up on this quad: its H does not even map the four points it was computed from (findSymm reports
            # "ops >= maxops": its cached row maxima go stale and it rotates about entries that are already zero).  Such a try says nothing about the
            # model, which must then fit the quad itself; it is counted, not compared.
            assert np.isfinite(d_mod).all() and (d_mod[q] < 1e-6).all(), "try %d: neither side fits its own quad" % t
            stats["reference_gave_up"] += 1
            continue
        stats["compared"] += 1
        if d_ref is None or not np.isfinite(d_mod).any():
            assert counts[t] == 0 and (d_ref is None or not distinct), "try %d: singular for one side only" % t
            continue
        both = np.concatenate([d_ref, d_mod[np.isfinite(d_mod)]])
        assert not (np.abs(both - threshold) <= 1e-3 * threshold).any(), "try %d: a distance within 0.1 %% of the threshold" % t
        if distinct:
            assert ((d_ref < threshold) == (d_mod < threshold)).all(), "try %d: inlier sets differ" % t
    res = out["result"]
    if res["status"] == 0:
        bt = int(res["bestTry"])
        for t in range(len(counts)):
            if t != bt and counts[t] == counts[bt] and (out["inlier_sets"][t] != out["inlier_sets"][bt]).any():
                assert abs(var[t] - var[bt]) > 1e-6 * abs(var[bt]), "tries %d and %d tie" % (t, bt)
        sel = np.nonzero(out["mask"])[0]
    else:
        sel = np.arange(k)
    Href, _ = ref_find(L, src[sel], dst[sel])
    corner_px = float(np.abs(hm.project(Href, CORNERS) - hm.project(res["H"], CORNERS)).max())
    if res["status"] == 0:          # (a degenerate point set has no H to compare)
        assert corner_px <= 1e-6, "computeH: model and reference move a corner apart by %g px" % corner_px
    if planted is not None and tries == 200:
        assert (out["mask"] != 0).tolist() == planted.tolist(), "the model at 200 tries misses the planted inliers"
        _, n_ref = ref_find(L, src, dst, ransac=True)
        assert n_ref == int(planted.sum()), "the reference's RANSAC returns %d inliers, planted %d" % (n_ref, int(planted.sum()))
    return corner_px


def store(arrays, cid, out):
    arrays["result_" + cid] = np.frombuffer(out["result"].tobytes(), np.uint8)
    arrays["mask_" + cid] = np.asarray(out["mask"], np.uint8)
    if out["counts"] is not None:
        arrays["quads_" + cid] = out["quads"].astype(np.int16)
        arrays["counts_" + cid] = out["counts"].astype(np.int16)
        arrays["varbits_" + cid] = np.ascontiguousarray(out["variances"], np.float64).view(np.uint64)
        arrays["rot_" + cid] = out["rotations"].astype(np.int16)


def main():
    RefShim(threads=1)          # refshim_init(1): the reference on one thread
    meta = {"cases": []}
    arrays = {}
    worst = 0.0
    reseeded = 0
    with tempfile.TemporaryDirectory() as tmp:
        L = build_shim(tmp, *sys.argv[1:2])
        for k in hc.KS:
            for share in hc.SHARES:
                seed = 100
                while True:
                    src, dst, inl = hc.planted(k, share, seed)
                    try:
                        outs = []
                        for tries in hc.TRIES:
                            o = hm.find(src, dst, k, tries, seed=seed + tries, pair=0)
                            o["corner_px"] = check_case(L, src, dst, o, hm.DEFAULT_THRESHOLD, inl, tries)
                            outs.append((tries, o))
                        break
                    except AssertionError as e:
                        print("k %d share %g seed %d: %s -> reseeding" % (k, share, seed, e))
                        seed += 1
                        reseeded += 1
                        assert seed < 500
                pid = "k%d_s%d" % (k, int(share * 100))
                arrays["src_" + pid], arrays["dst_" + pid] = src, dst
                for tries, o in outs:
                    cid = "%s_t%d" % (pid, tries)
                    store(arrays, cid, o)
                    worst = max(worst, o["corner_px"])
                    meta["cases"].append(dict(id=cid, kind="planted", points=pid, k=k, share=share, tries=tries, seed=seed + tries, points_seed=seed, threshold=hm.DEFAULT_THRESHOLD,
                                              count=k, point_cap=k, given_quads=True, status=int(o["result"]["status"]), inliers=int(o["result"]["inliers"]),
                                              planted_inliers=int(inl.sum()), corner_px=o["corner_px"]))
        edge = []
        s, d, _ = hc.collinear_case()
        edge.append(("collinear_quad", s, d, 9, 9, np.array([[0, 1, 2, 3], [3, 2, 1, 0], [4, 5, 6, 8]], np.int32), 3, 0, 30.0))
        s, d, _ = hc.planted(9, 0.0, 2)
        edge.append(("singular_and_out_of_range_quads", s, d, 9, 9, hc.edge_quads(9), len(hc.edge_quads(9)), 0, 30.0))
        s, d, _ = hc.planted(20, 1.0, 3)
        edge.append(("all_outliers", s, d, 20, 20, None, 64, 11, 30.0))
        s, d = hc.line_case(20)
        edge.append(("no_best", s, d, 20, 20, None, 64, 12, 30.0))
        s, d, _ = hc.planted(9, 0.0, 4)
        edge.append(("k3", s, d, 3, 9, None, 8, 13, 30.0))
        edge.append(("negative_count", s, d, -2, 9, None, 8, 14, 30.0))
        edge.append(("count_beyond_cap", s, d, 14, 9, None, 65, 15, 30.0))
        for cid, s, d, count, cap, quads, tries, seed, thr in edge:
            o = hm.find(s[:cap], d[:cap], count, tries, threshold=thr, seed=seed, pair=0, quad_list=quads)
            px = check_case(L, s, d, o, thr) if o["result"]["status"] != 2 else 0.0
            arrays["src_" + cid], arrays["dst_" + cid] = s[:cap], d[:cap]
            store(arrays, cid, o)
            meta["cases"].append(dict(id=cid, kind="edge", points=cid, k=o["k"], tries=tries, seed=seed, threshold=thr, count=count, point_cap=cap, given_quads=quads is not None,
                                      status=int(o["result"]["status"]), inliers=int(o["result"]["inliers"]), corner_px=px))
    by = {c["id"]: c for c in meta["cases"]}
    assert by["no_best"]["status"] == 1 and by["all_outliers"]["status"] == 0 and by["k3"]["status"] == by["negative_count"]["status"] == 2 and by["count_beyond_cap"]["status"] == 0
    meta["worst_corner_px"] = worst
    meta["reseeded"] = reseeded
    meta["tries_compared"], meta["tries_reference_gave_up"] = stats["compared"], stats["reference_gave_up"]
    with open(os.path.join(HERE, "golden_homography.json"), "w") as f:
        json.dump(meta, f, indent=None, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    np.savez_compressed(os.path.join(HERE, "golden_homography.npz"), **arrays)
    print("wrote %d cases (%d reseeded), %d tries compared, the reference gave up on %d, worst corner distance model vs reference %.3g px"
          % (len(meta["cases"]), reseeded, stats["compared"], stats["reference_gave_up"], worst))


if __name__ == "__main__":
    main()
