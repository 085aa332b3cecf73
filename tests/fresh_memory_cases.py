"""First calls on fresh, poisoned allocations (tests/test_gpu_fresh_memory.py; docs/dispatch_coverage.md, "Fresh allocations"): the cases that are not
the stream-order rig's.  hipMalloc and hipHostMalloc promise nothing about what a block holds; compvhip_debug_alloc_fill (gpu_support.alloc_fill) makes
every block the library allocates hold one byte, and every case here makes the FIRST call of a handle or of a context's staging inside such a block and
holds it, bit for bit, against the model or oracle of the stage's own GPU test.

  HOST_CALLS    name -> fn(ctx, orc, W, H, k): one call of a host entry family on a context of the test's own, at the k-th of SIZES (the second is larger in
                both directions: the cached single-frame plan and the staging are allocated at the first and reallocated at the second)
  FAMILIES      name -> fn(ctx): the first calls of the handles that carry their stream in a descriptor (curve fit, SVM, undistort), on handles of their own
  handle_cases  opaque handle type of include/compv_hip.h -> the cold cases that create one (tests/test_fresh_memory_cases.py: none is left out)

Importing this module loads neither torch nor the library."""
import re

import numpy as np

FILLS = (0xFF, 0x01)          # NaN / 65 535 / -1 / every flag and mask bit; and 16 843 009: a positive count that clamps to the capacity, small non-zero sums
FILL_IDS = {0xFF: "ff", 0x01: "01"}
SIZES = ((61, 47), (130, 70))

HOST_CALLS = {}
FAMILIES = {}


def host_call(fn):
    HOST_CALLS[fn.__name__] = fn
    return fn


def family(fn):
    FAMILIES[fn.__name__] = fn
    return fn


def same(got, exp, what):
    got, exp = np.ascontiguousarray(got), np.ascontiguousarray(exp)
    assert got.dtype == exp.dtype and got.shape == exp.shape, "%s: %s %s, expected %s %s" % (what, got.dtype, got.shape, exp.dtype, exp.shape)
    if got.tobytes() != exp.tobytes():
        bad = np.flatnonzero(got.view(np.uint8).reshape(-1) != exp.view(np.uint8).reshape(-1))
        raise AssertionError("%s: %d of %d bytes differ, first at byte %d" % (what, bad.size, got.nbytes, bad[0]))


# ---- content ------------------------------------------------------------------------------------------------------------------------------------
def gray(W, H, k):
    """a text frame: at these sizes it has tens of lines and components (a synthetic scene of 61 x 47 has four edge pixels)"""
    from gpu_support import make_frame
    return make_frame("text", W, H, 31 + k)


def corners_frame(W, H, k):
    import fast_model as fm
    return fm.blocks(W, H, 5 + k)


def edge_map(orc, W, H, k):
    from compv_amd import capi
    from gpu_support import T_HIGH, T_LOW, canny_expect
    return canny_expect(orc, gray(W, H, k), 3, capi.THRESHOLD_COMPARE_TO_GRADIENT, T_LOW, T_HIGH)


def line_threshold(W, H):
    return max(3, min(W, H) // 3)


# ---- the host entry families --------------------------------------------------------------------------------------------------------------------
@host_call
def canny(ctx, orc, W, H, k):
    """the three threshold modes: the mean's sums and the Otsu histogram are first-use scratch of the cached plan"""
    from gpu_support import canny_expect, canny_modes
    img = gray(W, H, k)
    for m in canny_modes():
        same(ctx.canny(img, m[2], m[3], m[0], m[1]), canny_expect(orc, img, *m), "canny %r" % (m,))


@host_call
def edge_dete(ctx, orc, W, H, k):
    from compv_amd import capi
    img = gray(W, H, k)
    for op in (capi.OP_SCHARR, capi.OP_SOBEL, capi.OP_PREWITT):          # the largest weights first: a maximum left behind would show in the next
        same(ctx.edge_dete(img, op), orc.edge_dete(img, op)[0], "edge_dete %d" % op)


@host_call
def grayscale(ctx, orc, W, H, k):
    from compv_amd import capi
    from gpu_support import rgb_of
    rgb = rgb_of(gray(W, H, k)).reshape(H, W * 3)
    same(ctx.grayscale(rgb, capi.FMT_RGB24, W), orc.grayscale(rgb, capi.FMT_RGB24, W), "grayscale")


@host_call
def otsu(ctx, orc, W, H, k):
    img = gray(W, H, k)
    got, exp = ctx.otsu(img), float(orc.otsu(img))
    assert got == exp, "otsu: %r, expected %r" % (got, exp)


@host_call
def convlt_fixedpoint(ctx, orc, W, H, k):
    from compv_amd import capi
    img, kern = gray(W, H, k), capi.gauss_kernel_fixedpoint(5, 1.0)
    rc, exp = orc.convlt_fxp(img, kern, kern)
    assert rc == 0, "oracle convlt_fxp returned %d" % rc
    same(ctx.convlt_fixedpoint(img, kern, kern), exp, "convlt_fixedpoint")


def _sht(ctx, orc, W, H, k):
    e, thr = edge_map(orc, W, H, k), line_threshold(W, H)
    lines, acc = ctx.houghsht(e, 1.0, thr, want_acc=True)
    exp_acc = orc.sht_acc(e, 1.0)
    assert acc.shape == exp_acc.shape and (acc == exp_acc).all(), "houghsht: %d accumulator cells differ" % int((acc != exp_acc).sum())
    exp = orc.sht_lines_from_acc_reference_order(exp_acc, W, H, 1.0, thr)
    assert len(exp) >= 2, "houghsht: the case has %d lines" % len(exp)
    assert [(int(l["row"]), int(l["col"]), int(l["strength"])) for l in lines] == [(l[3], l[4], l[2]) for l in exp], "houghsht: lines"
    return e, lines


@host_call
def houghsht(ctx, orc, W, H, k):
    _sht(ctx, orc, W, H, k)


@host_call
def houghkht(ctx, orc, W, H, k):
    """both orders: the reference order sweeps on the host, the canonical one sorts on the GPU (the group's pinned arenas and line buffers)"""
    from kht_canon_model import CanonModel, line_bits, model_line_bits
    e = edge_map(orc, W, H, k)
    exp, gs_exp = orc.kht(e, 1.0, 1.0, 12)
    got, gs = ctx.houghkht(e, 1.0, 1.0, 12)
    assert len(exp) >= 2, "houghkht: the case has %d lines" % len(exp)
    assert gs == gs_exp, "houghkht: gs %r, expected %r" % (gs, gs_exp)
    assert [(float(l["rho"]), float(l["theta"]), int(l["strength"])) for l in got] == [(float(np.float32(l[0])), float(np.float32(l[1])), int(l[2])) for l in exp], "houghkht: lines"
    el, egs = CanonModel(orc).lines(e, 1.0, 1.0, 12)[:2]
    got, gs = ctx.houghkht(e, 1.0, 1.0, 12, order="canonical")
    assert line_bits(got) == model_line_bits(el) and gs == egs, "houghkht, canonical order"


@host_call
def houghsht_segments(ctx, orc, W, H, k):
    import sht_segments_rig as sr
    from sht_segments_model import frame_segments
    e, lines = _sht(ctx, orc, W, H, k)
    sinQ, cosQ = sr.tables(orc, W, H, 1.0)
    want = frame_segments(e, sinQ, cosQ, sr.cells_of(lines), 3, 1)
    assert len(want) >= 2, "houghsht_segments: the case has %d segments" % len(want)
    same(ctx.houghsht_segments(e, lines, 1.0, 3, 1, cap=2), want, "houghsht_segments")          # grows through E_OUT_OF_BOUND


@host_call
def houghsht_fit(ctx, orc, W, H, k):
    import sht_fit_rig as fr
    from sht_fit_model import frame_fits
    from sht_segments_rig import cells_of
    e, lines = _sht(ctx, orc, W, H, k)
    R, (sinQ, cosQ) = fr.tables(orc, W, H, 1.0)
    want, valid = frame_fits(e, sinQ, cosQ, cells_of(lines), 2, R)
    got, refined = ctx.houghsht_fit(e, lines, 1.0, 2, want_refined=True)
    fr.same_records(got, want, "houghsht_fit")
    fr.assert_refined(refined, lines, want, valid, "houghsht_fit, refined lines")


@host_call
def components(ctx, orc, W, H, k):
    from components_model import components as model
    e = edge_map(orc, W, H, k)
    for conn in (8, 4):
        exp_lab, exp_rec = model(e, conn, 1)
        assert len(exp_rec) >= 2, "components: the case has %d components" % len(exp_rec)
        lab, rec = ctx.components(e, conn, 1, cap=2)          # grows through E_OUT_OF_BOUND
        assert np.array_equal(lab, exp_lab), "components %d: labels" % conn
        same(rec, exp_rec, "components %d: records" % conn)
        same(ctx.components(e, conn, 1, want_labels=False)[1], exp_rec, "components %d without a label map" % conn)          # the plan's own parent plane


@host_call
def threshold(ctx, orc, W, H, k):
    import morph_model as mm
    img = gray(W, H, k)
    same(ctx.threshold(img, 127.5), mm.threshold(img, 127.5), "threshold")


@host_call
def threshold_adaptive(ctx, orc, W, H, k):
    import morph_model as mm
    img = gray(W, H, k)
    same(ctx.threshold_adaptive(img, 15, 5.0, 100.0, True), mm.adaptive(img, 15, 5.0, 100.0, True), "threshold_adaptive")


@host_call
def morph(ctx, orc, W, H, k):
    """CLOSE and OPEN: two passes through the plan's plane"""
    import morph_model as mm
    img, se = gray(W, H, k), mm.strel(mm.CROSS, 5, 5)
    for op in (mm.CLOSE, mm.OPEN):
        same(ctx.morph(img, se, op, mm.BORDER_ZERO), mm.morph(img, se, op, mm.BORDER_ZERO), "morph %d" % op)


@host_call
def fast(ctx, orc, W, H, k):
    import fast_model as fm
    img = corners_frame(W, H, k)
    exp_rec, exp_map = fm.fast(img, 20, 9, True)
    assert len(exp_rec) > 7, "fast: the case has %d corners" % len(exp_rec)
    rec, smap = ctx.fast(img, 20, 9, True, want_scores=True, cap=3)          # grows through E_OUT_OF_BOUND
    same(rec, exp_rec, "fast: corners")
    same(smap, exp_map, "fast: score map")
    same(ctx.fast(img, 20, 9, True, max_features=7), fm.cut(exp_rec, 7), "fast: the strongest 7")          # the histogram and the cut level


@host_call
def orb(ctx, orc, W, H, k):
    import orb_model as om
    from orb_rig import corner_list
    img = corners_frame(W, H, k)
    corners = corner_list(W, H, 65, 50 + k)
    keys, desc = ctx.orb(img, corners, 0, 1.0)
    exp_k, _ = om.keypoints(img, corners, 0, np.float32(1.0))
    assert len(exp_k) == 65, "orb: %d survivors" % len(exp_k)
    same(keys, exp_k, "orb: keypoints")
    same(desc, om.describe(om.blur(img), exp_k, np.float32(1.0)), "orb: descriptors")


@host_call
def orb_pyramid(ctx, orc, W, H, k):
    import orb_pyramid_model as pm
    from compv_amd import capi
    import fast_model as fm
    levels, sf, mf = 3, 0.83, 60
    img = fm.noise(W, H, 6 + k)          # (blocks of 61 x 47 leave no corner 18 pixels from every border)
    keys, _, _, planes = pm.detect(img, levels, sf, 20, 9, True, mf, None)
    assert len(keys) >= 8, "orb_pyramid: the case has %d keypoints" % len(keys)
    rows = pm.describe(planes, pm.geometry(W, H, levels, sf, mf), keys)
    gk, gd = ctx.orb_pyramid(img, capi.OrbPyramidOpts(levels, sf, 20, 9, True, mf), cap=3)          # the binding repeats the call with the reported size
    same(gk, keys, "orb_pyramid: keypoints")
    same(gd, rows, "orb_pyramid: descriptors")


def _out_size(W, H):
    return (2 * W) // 3 + 1, H // 2 + 2


@host_call
def scale(ctx, orc, W, H, k):
    import orb_pyramid_model as pm
    img = gray(W, H, k)
    wo, ho = _out_size(W, H)
    same(ctx.scale(img, wo, ho), pm.scale(img, wo, ho), "scale")


@host_call
def remap(ctx, orc, W, H, k):
    import remap_cases as rc
    import remap_model as rm
    img = gray(W, H, k)
    wo, ho = _out_size(W, H)
    x, y = rc.random_map(W, H, wo, ho, 62000 + k)
    roi = (-5.0, 30.25, 3.5, 400.0)
    same(ctx.remap(img, x, y, rm.BILINEAR, roi, 9), rm.remap(img, x, y, rm.BILINEAR, roi, 9), "remap")


@host_call
def warp_inverse(ctx, orc, W, H, k):
    import remap_cases as rc
    import remap_model as rm
    img = gray(W, H, k)
    wo, ho = _out_size(W, H)
    M = rc.matrices(W, H, wo, ho)["affine"]
    same(ctx.warp_inverse(img, M, wo, ho, rm.BILINEAR, 9), rm.warp_inverse(img, M, wo, ho, rm.BILINEAR, 9), "warp_inverse")


@host_call
def hog(ctx, orc, W, H, k):
    import hog_model as hm
    img = gray(W, H, k)
    same(ctx.hog(img), hm.hog(img)[0], "hog")


@host_call
def integral(ctx, orc, W, H, k):
    import stats_model as sm
    img = gray(W, H, k)
    s, q = ctx.integral(img)
    es, eq = sm.integral(img)
    same(s, np.asarray(es, np.float64), "integral: sum")
    same(q, np.asarray(eq, np.float64), "integral: sumsq")


@host_call
def histogram(ctx, orc, W, H, k):
    import stats_model as sm
    img = gray(W, H, k)
    same(ctx.histogram(img), np.asarray(sm.histogram(img), np.uint32), "histogram")


@host_call
def equalize(ctx, orc, W, H, k):
    import stats_model as sm
    img = gray(W, H, k)
    out, lut = ctx.equalize(img)          # the frame's own histogram: the context's partial histograms and table
    eo, el = sm.equalize(img, None, 0.0)
    same(out, eo, "equalize: frame")
    same(lut, np.asarray(el, np.uint8), "equalize: table")


@host_call
def projections(ctx, orc, W, H, k):
    import stats_model as sm
    img = gray(W, H, k)
    px, py = ctx.projections(img)
    ex, ey = sm.projections(img)
    same(px, np.asarray(ex, np.int32), "projections: x")
    same(py, np.asarray(ey, np.int32), "projections: y")


@host_call
def convert(ctx, orc, W, H, k):
    import convert_model as cm
    planes = [np.random.default_rng(500 + 10 * k + p).integers(0, 256, s, dtype=np.uint8) for p, s in enumerate(cm.plane_shapes(cm.NV12, W, H))]
    got, exp = ctx.convert(planes, cm.NV12, cm.RGBA32, W, H), cm.convert(cm.NV12, cm.RGBA32, planes, W, H)
    assert len(got) == len(exp), "convert: %d planes, expected %d" % (len(got), len(exp))
    for p, (g, e) in enumerate(zip(got, exp)):
        same(g, e, "convert: plane %d" % p)


@host_call
def match_hamming(ctx, orc, W, H, k):
    """cols = 30: two zero bytes pad every staged row to a dword multiple (the staging's per-call clear)"""
    import match_model as mm
    rng = np.random.default_rng(3 + k)
    Q, T = (70, 131) if k == 0 else (140, 300)
    q, t = rng.integers(0, 256, (Q, 30), dtype=np.uint8), rng.integers(0, 256, (T, 30), dtype=np.uint8)
    same(ctx.match_hamming(q, t, 2), mm.knn_reference(q, t, 2), "match_hamming")


@host_call
def homography_find_f64(ctx, orc, W, H, k):
    import homography_cases as hc
    import homography_model as hm
    n = (65, 129)[k]
    src, dst, _ = hc.planted(n, 0.3, 85 + k)
    e = hm.find(src, dst, n, 64, seed=6)
    res, mask = ctx.homography_find(src, dst, tries=64, seed=6)
    assert res.tobytes() == e["result"].tobytes(), "homography_find_f64: record %r, model %r" % (res, e["result"])
    same(mask, np.asarray(e["mask"], np.uint8), "homography_find_f64: mask")


@host_call
def curvefit_find_f64(ctx, orc, W, H, k):
    import curvefit_cases as cc
    import curvefit_model as cm
    n = (65, 129)[k]
    for model, call in ((cm.LINE, ctx.fit_line), (cm.PARABOLA, ctx.fit_parabola)):
        pts = cc.noisy(model, n, 0.3, 9 + k)[0]
        e = cm.find(pts, n, model, 64, 1.0, seed=12)
        res, mask = call(pts, threshold=1.0, tries=64, seed=12)
        assert res.tobytes() == e["result"].tobytes(), "curvefit_find_f64, model %d: record %r, model %r" % (model, res, e["result"])
        same(mask, np.asarray(e["mask"], np.uint8), "curvefit_find_f64, model %d: mask" % model)


@host_call
def undistort_u8(ctx, orc, W, H, k):
    import undistort_cases as uc
    from undistort_rig import model_image
    c = uc.case(("pin40", "pin61")[k])
    wo, ho = c["size"][2:]
    for interp in (1, 4):          # bilinear, bicubic
        got = ctx.undistort(uc.frame(c), c["K"], c["d"], wo, ho, *c["origin"], interp=interp, roi=c["roi"], default=c["default"])
        same(got, model_image(c, interp), "undistort_u8 %s, interpolation %d" % (c["id"], interp))


# ---- the handles that carry their stream in a descriptor ----------------------------------------------------------------------------------------------
@family
def curvefit(ctx):
    """points_from_labels -> find -> distances at 37 x 29 with cap 16 (test_gpu_curvefit.py::test_gather_from_label_maps, one turn), then find on the
    caller's points at k = 257 (the 256-point round and one more)"""
    import curvefit_cases as cc
    import curvefit_model as cm
    from compv_amd import capi
    from curvefit_rig import REC, SENT64, Rig, gather_case
    from gpu_support import SENTINEL, Arena, d2h, ptr, u8
    W, H, cap, frames, comp_cap = 37, 29, 16, 2, 5
    n = frames * comp_cap
    labels, comps, counts, exp_pts, exp_k = gather_case(W, H, cap)
    ar = Arena()
    d_lab, d_comps, d_counts = ar.new(labels.nbytes, u8(labels)), ar.new(comps.nbytes, u8(comps)), ar.new(8, u8(counts))
    for d, h in ((d_lab, labels), (d_comps, comps), (d_counts, counts)):
        ar.keep(d, u8(h))
    d_res, d_mask, d_dist = ar.new(n * REC), ar.new(n * cap), ar.new(n * cap * 8)
    params = np.tile(np.array([1.0, -2.0, 3.0]), (n, 1))
    d_params = ar.new(params.nbytes, u8(params))
    h = capi.Curvefit(ctx, n, cap, 64)
    try:
        h.points_from_labels(ptr(d_lab), W, H, W + 3, ptr(d_comps), comp_cap, ptr(d_counts), frames)
        _, got_k = h.scores(1)
        ar.check("gather")
        assert got_k.tolist() == exp_k.tolist(), "curvefit: gathered counts %r, expected %r" % (got_k.tolist(), exp_k.tolist())
        p_pts, _ = h.gathered()
        got = np.frombuffer(d2h(p_pts, n * cap * 16).tobytes(), np.float64).reshape(n, cap, 2)
        for s in range(n):
            assert got[s, :exp_k[s]].tobytes() == exp_pts[s, :exp_k[s]].tobytes(), "curvefit: set %d gathered points" % s
        for model in cm.MODELS:
            exp = [cm.find(exp_pts[s], exp_k[s], model, 64, seed=6, set_index=s) for s in range(n)]
            d_res.fill_(SENTINEL)
            d_mask.fill_(SENTINEL)
            h.find(0, 0, ptr(d_res), ptr(d_mask), model=model, tries=64, seed=6)
            tries_counts, _ = h.scores(64)
            ar.check("find on gathered points")
            res = np.frombuffer(d_res.cpu().numpy().tobytes(), cm.RESULT_DTYPE)
            mask = d_mask.cpu().numpy().reshape(n, cap)
            for s, e in enumerate(exp):
                assert res[s].tobytes() == e["result"].tobytes(), "curvefit: model %d set %d record %r, model %r" % (model, s, res[s], e["result"])
                assert mask[s, :exp_k[s]].tobytes() == e["mask"].tobytes() and (mask[s, exp_k[s]:] == SENTINEL).all(), "curvefit: model %d set %d mask" % (model, s)
                assert e["counts"] is None or tries_counts[s].tolist() == e["counts"].tolist(), "curvefit: model %d set %d per-try counts" % (model, s)
        h.distances(0, 0, cm.LINE, ptr(d_params), ptr(d_dist))
        h.scores(1)
        ar.check("distances")
        got = np.frombuffer(d_dist.cpu().numpy().tobytes(), np.float64).reshape(n, cap)
        for s in range(n):
            assert got[s, :exp_k[s]].tobytes() == cm.residuals(cm.LINE, 1.0, -2.0, 3.0, exp_pts[s, :exp_k[s]])[0].tobytes(), "curvefit: set %d distances" % s
            assert got[s, exp_k[s]:].tobytes() == np.full(cap - exp_k[s], SENT64).tobytes(), "curvefit: set %d wrote distances at or behind k" % s
    finally:
        h.close()
    for model in (cm.LINE, cm.PARABOLA):
        rig = Rig(ctx, [cc.planted(model, 257, 0.3, 277)[0]], 257, 257)
        try:
            rig.run(model, 257, seed=257)
            res = rig.check("curvefit: caller's points, model %d" % model, model, 257, rig.model(model, 257, seed=257))
            assert res[0]["status"] == 0 and res[0]["k"] == 257, "curvefit: caller's points, model %d: record %r" % (model, res[0])
        finally:
            rig.close()


@family
def svm(ctx):
    """predict with d_kvalues == NULL (the handle's own kernel-value scratch) at n = 65 on an RBF and a LINEAR fixture case, then predict_host across a
    slice boundary (maxVectors 100, 257 queries: the handle's host staging)"""
    import svm_cases as sc
    from compv_amd import capi
    from svm_rig import PAD, Rig
    by_id = {c["id"]: c for c in sc.all_cases()}
    _, A = sc.golden()
    for cid in ("rbf_d33_c2", "lin_d21_c3"):
        c = by_id[cid]
        rig = Rig(ctx, c, 65)
        try:
            rig.load(sc.queries(c, rig.m)[:65])
            rig.run(65, True, False)
            rig.check("svm %s, n 65, no kernel values" % cid, 65, A["lab_" + cid], A["dec_" + cid], A["K_" + cid], True, False)
        finally:
            rig.close()
        h = capi.Svm(ctx, sc.model_path(cid), 100)
        try:
            x = sc.queries(c, sc.recorded_model(c))
            wide = sc.padded(x, c["D"] + 2, PAD)
            labels, dec = h.predict_host(wide[:, :c["D"]], want_dec=True)
            same(labels, A["lab_" + cid], "svm %s: predict_host labels" % cid)
            same(dec, A["dec_" + cid], "svm %s: predict_host decision values" % cid)
        finally:
            h.close()


@family
def undistort(ctx):
    """frames with a shared camera and with a camera each, maps, points and project at the pin40 case: the coefficient staging (device block and the
    pinned ring) is what the handle allocates"""
    import undistort_cases as uc
    import undistort_model as um
    from compv_amd import capi
    from gpu_support import SENTINEL, ptr, u8
    from undistort_rig import Rig, layouts, maps_of, model_image
    c = uc.case("pin40")
    wo, ho = c["size"][2:]
    K3, d3 = uc.cameras_for_frames(c, 3)
    rig = Rig(ctx, c, 3, max_sets=3, max_points=80)
    try:
        name, Sout, off = layouts(wo, 1)[0]
        rig.run(1, c["K"], c["d"], Sout, off)
        rig.check("undistort: shared camera", [model_image(c, 1, k) for k in range(3)], Sout, off)
        K, d = K3.astype(np.float32), d3.astype(np.float32)
        for interp in (1, 4):
            name, Sout, off = layouts(wo, interp)[1]
            rig.run(interp, K, d, Sout, off)
            rig.check("undistort: a camera each, interpolation %d" % interp, [model_image(c, interp, k, K[k], d[k]) for k in range(3)], Sout, off)
        for T in (np.float32, np.float64):
            x, y, _, _ = maps_of(rig, K3, d3, 3, T, rig.ar)
            ex, ey = zip(*[um.map_planes(K3[k].astype(T), d3[k].astype(T), wo, ho, dtype=T) for k in range(3)])
            assert x.tobytes() == np.stack(ex).tobytes() and y.tobytes() == np.stack(ey).tobytes(), "undistort: maps of %s" % T.__name__
        ar = rig.ar
        pts = np.random.default_rng(9).uniform(-3, 64, (3, 65, 2))
        counts = np.array([65, 0, 17], np.int32)
        exp = np.full(pts.shape, np.frombuffer(bytes([SENTINEL] * 8), np.float64)[0])
        for s in range(3):
            exp[s, :counts[s]] = um.dist_points(K3[s], d3[s], pts[s, :counts[s]], np.float64)
        d_pts, d_out, d_cnt = ar.new(pts.nbytes, u8(pts)), ar.new(pts.nbytes), ar.new(12, u8(counts))
        ar.keep(d_pts, u8(pts))
        ar.keep(d_cnt, u8(counts))
        rig.h.points(K3, d3, ptr(d_pts), 3, 65, ptr(d_out), capi.UNDISTORT_F64, ptr(d_cnt))
        ar.check("undistort: points")
        assert d_out.cpu().numpy().tobytes() == exp.tobytes(), "undistort: points"
        p = uc.proj_cases()[1]
        cam = uc.case(p["camera"])
        pose = np.concatenate([np.asarray(p["R"], np.float64).ravel(), np.asarray(p["t"], np.float64)])
        obj = uc.proj_points(p)
        d_obj, d_img = ar.new(obj.nbytes, u8(obj)), ar.new(p["n"] * 16)
        ar.keep(d_obj, u8(obj))
        rig.h.project(cam["K"], cam["d"], pose[None], ptr(d_obj), 1, p["n"], ptr(d_img))
        ar.check("undistort: project")
        exp = um.proj2d(np.asarray(cam["K"], np.float64), np.asarray(cam["d"], np.float64), pose[:9], pose[9:], obj)
        assert d_img.cpu().numpy().tobytes() == exp.tobytes(), "undistort: project"
    finally:
        rig.close()


# ---- which handle type has a cold case ---------------------------------------------------------------------------------------------------------------
# the stream-order rig's cases by the handle they create (stream_order_rig.CASES: everything else there runs on a plan)
RIG_HANDLES = {
    "matcher": ("matcher_knn", "matcher_good"),
    "orbpyr": ("orbpyr_detect", "orbpyr_describe"),
    "homography": ("homography_find", "homography_scores", "homography_points", "homography_project"),
}


def handle_cases(rig_cases):
    """opaque handle type -> ids of the cold cases that create one; rig_cases: the ids of stream_order_rig.CASES"""
    rig_cases = set(rig_cases)
    elsewhere = {c for ids in RIG_HANDLES.values() for c in ids}
    out = {"ctx": ["host:" + n for n in HOST_CALLS], "plan": sorted("rig:" + c for c in rig_cases - elsewhere)}
    for handle, ids in RIG_HANDLES.items():
        out[handle] = ["rig:" + c for c in ids if c in rig_cases]
    for name in FAMILIES:
        out[name] = ["family:" + name]
    return out


def handle_types(header_text):
    """the opaque handle types a header declares: `typedef struct compvhip_X compvhip_X;` -> X"""
    return sorted({a for a, b in re.findall(r"typedef\s+struct\s+compvhip_(\w+)\s+compvhip_(\w+)\s*;", header_text) if a == b})


def handles_without_a_case(header_text, cases):
    return [t for t in handle_types(header_text) if not cases.get(t)]
