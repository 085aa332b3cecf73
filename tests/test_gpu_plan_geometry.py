"""The batched plan API (compvhip_plan_*) at ragged widths, padded row strides and large batches, frame by frame against the oracle.

Every device buffer sits between two 4096-byte guards holding a fixed pattern (the Arena of tests/gpu_support.py); outputs start
filled with a sentinel over their valid region too (so every valid pixel, count and accumulator cell must be written), and the
input's padding columns [W, S) hold seeded random bytes, 255 included.  After every call the guards must be intact and, for
out-of-place calls, the input unchanged.  Output padding [W, S) is not asserted on: kernels may write it, as the reference's SIMD
does.  The bar is the suite's: bit-exact maps, accumulators cell by cell, line sets in canonical order, counts, Otsu levels, KHT
GS.

The geometry table lives in tests/plan_geometries.py (checked on the CPU by tests/test_plan_geometries.py).
"""
import numpy as np
import pytest

from gpu_support import (KINDS, LINE_CAP, SENTINEL, T_HIGH, T_LOW, Arena, assert_lines, assert_maps, canny_expect, canny_modes, check_accs, edge_counts,
                         frame_expectations, frames_view, lines_of, make_batch, make_frame, pad_frames, pool, ptr, rgb565le_of, rgb_of, sht_expect, sht_threshold)
from plan_geometries import GEOMETRIES, XCH_GEOMETRY, XCH_MARGIN, XCH_MIN_WAVES, swar_waves

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------------------
# the geometry sweep
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H,S,F,theta", GEOMETRIES, ids=lambda v: str(v))
def test_plan_geometry_sweep(hip_ctx, oracle, W, H, S, F, theta):
    from compv_amd import capi
    seed = W * 7 + H * 3 + F
    rng = np.random.default_rng(seed)
    imgs = make_batch(W, H, F, seed)
    gauss = capi.gauss_kernel_fixedpoint(5, 1.0)
    want_kht = F <= 9
    with pool() as ex:
        exp = list(ex.map(lambda img: frame_expectations(oracle, img, theta, want_kht, gauss), imgs))
    thr = sht_threshold(W, H)
    R, T, _ = oracle.sht_dims(W, H, theta)
    A = Arena()
    n = F * H * S
    host_in = pad_frames(imgs, S, rng)
    d_in = A.new(n, host_in)
    A.keep(d_in, host_in)
    d_out = A.new(n)
    d_lines = A.new(F * LINE_CAP * 20)
    d_counts = A.new(F * 4)
    plan = capi.Plan(hip_ctx, W, H, S, F, theta)
    try:
        def out_frames(buf=d_out):
            return frames_view(buf, F, H, S, W)

        def counts_of():
            return d_counts.cpu().numpy().view(np.int32)

        def raw_lines():
            return d_lines.cpu().numpy().reshape(F, LINE_CAP, 20)

        # Sobel / Scharr / Prewitt detectors
        for op in (capi.OP_SOBEL, capi.OP_SCHARR, capi.OP_PREWITT):
            A.refill(d_out)
            plan.edge_dete(ptr(d_in), op, ptr(d_out))
            A.check("edge_dete %d" % op)
            assert_maps(out_frames(), [x["dete"][op] for x in exp], "edge_dete %d" % op)

        # Canny: kernel sizes 3 / 5 x the three threshold modes, out of place; the gradient 3x3 run last (its masks feed the SHT below)
        modes = canny_modes()
        for ks, mode, tl, th in modes[1:] + modes[:1]:
            A.refill(d_out)
            plan.canny(ptr(d_in), tl, th, ptr(d_out), ks, mode)
            A.check("canny %d/%d" % (ks, mode))
            e = [x["canny"][(ks, mode)] for x in exp]
            assert_maps(out_frames(), e, "canny %d/%d" % (ks, mode))
        e3 = [x["canny"][(3, capi.THRESHOLD_COMPARE_TO_GRADIENT)] for x in exp]

        # SHT on the plan's own bit masks of that Canny run
        plan.houghsht(0, thr, 0, ptr(d_lines), LINE_CAP, ptr(d_counts))
        A.check("houghsht(masks)")
        assert_lines(raw_lines(), counts_of(), [x["sht"][1] for x in exp], "houghsht(masks)")
        assert edge_counts(plan, F).tolist() == [int((m != 0).sum()) for m in e3], "edge counts (masks)"
        check_accs(plan, A, F, R, T, [x["sht"][0] for x in exp], "houghsht(masks)")

        # KHT on the device edge maps of that run (their padding holds whatever the kernels left there)
        if want_kht:
            lines, gs = plan.houghkht(ptr(d_out), 1.0, theta, 12)
            A.check("houghkht")
            for f in range(F):
                el, egs = exp[f]["kht"]
                assert [(float(l["rho"]), float(l["theta"]), int(l["strength"])) for l in lines[f]] == \
                       [(float(np.float32(l[0])), float(np.float32(l[1])), int(l[2])) for l in el], ("kht", f)
                assert (gs[f] == egs) if len(el) else (gs[f] is None), ("kht gs", f)

        # SHT on foreign edge maps: the oracle's maps with 255 in their padding
        host_e = np.full((F, H, S), 255, np.uint8)
        host_e[:, :, :W] = np.stack(e3)
        d_fe = A.new(n, host_e)
        A.keep(d_fe, host_e)
        A.refill(d_lines); A.refill(d_counts)
        plan.houghsht(ptr(d_fe), thr, 0, ptr(d_lines), LINE_CAP, ptr(d_counts))
        A.check("houghsht(foreign)")
        assert_lines(raw_lines(), counts_of(), [x["sht"][1] for x in exp], "houghsht(foreign)")
        assert edge_counts(plan, F).tolist() == [int((m != 0).sum()) for m in e3], "edge counts (foreign)"
        check_accs(plan, A, F, R, T, [x["sht"][0] for x in exp], "houghsht(foreign)")

        # in place: d_edges == d_in
        d_alias = A.new(n, host_in)
        plan.canny(ptr(d_alias), T_LOW, T_HIGH, ptr(d_alias))
        A.check("canny in place")
        assert_maps(out_frames(d_alias), e3, "canny in place")

        # the pipeline: synchronous, asynchronous + wait, and the general step (5x5, mean thresholds)
        for how in ("sync", "async", "ex"):
            A.refill(d_out); A.refill(d_lines); A.refill(d_counts)
            if how == "sync":
                plan.pipeline(ptr(d_in), T_LOW, T_HIGH, thr, 0, ptr(d_out), ptr(d_lines), LINE_CAP, ptr(d_counts))
                e, lx = e3, [x["sht"][1] for x in exp]
            elif how == "async":
                plan.wait(plan.pipeline_async(ptr(d_in), T_LOW, T_HIGH, thr, 0, ptr(d_out), ptr(d_lines), LINE_CAP, ptr(d_counts)))
                e, lx = e3, [x["sht"][1] for x in exp]
            else:
                plan.pipeline_ex(ptr(d_in), 0.68, 1.36, thr, 0, ptr(d_out), ptr(d_lines), LINE_CAP, ptr(d_counts), ksize=5,
                                 threshold_type=capi.THRESHOLD_PERCENT_OF_MEAN)
                e, lx = [x["canny"][(5, capi.THRESHOLD_PERCENT_OF_MEAN)] for x in exp], [x["sht5"] for x in exp]
            A.check("pipeline " + how)
            assert_maps(out_frames(), e, "pipeline " + how)
            assert_lines(raw_lines(), counts_of(), lx, "pipeline " + how)
            assert edge_counts(plan, F).tolist() == [int((m != 0).sum()) for m in e], ("edge counts", how)

        # the general step on packed RGB24 frames, with the luma planes, the Otsu levels and the Cartesian endpoints
        host_rgb = pad_frames(np.stack([rgb_of(i).reshape(H, W * 3) for i in imgs]), S * 3, rng)
        d_rgb = A.new(n * 3, host_rgb)
        A.keep(d_rgb, host_rgb)
        d_gray = A.new(n)
        d_otsu = A.new(F * 4)
        d_cart = A.new(F * LINE_CAP * 16)
        A.refill(d_out); A.refill(d_lines); A.refill(d_counts)
        plan.pipeline_ex(ptr(d_rgb), 0.5, 1.0, thr, 0, ptr(d_out), ptr(d_lines), LINE_CAP, ptr(d_counts), threshold_type=capi.THRESHOLD_OTSU,
                         pixfmt=capi.FMT_RGB24, d_gray=ptr(d_gray), d_otsu=ptr(d_otsu), d_cart=ptr(d_cart))
        A.check("pipeline_ex rgb24")
        assert_maps(frames_view(d_gray, F, H, S, W), [x["rgb"][0] for x in exp], "pipeline_ex gray")
        assert d_otsu.cpu().numpy().view(np.int32).tolist() == [x["rgb"][1] for x in exp]
        assert_maps(out_frames(), [x["rgb"][2] for x in exp], "pipeline_ex rgb24 edges")
        raw, counts = raw_lines(), counts_of()
        assert_lines(raw, counts, [x["rgb"][3] for x in exp], "pipeline_ex rgb24")
        cart = d_cart.cpu().numpy().view(np.float32).reshape(F, LINE_CAP, 4)
        for f in range(F):
            k = min(int(counts[f]), LINE_CAP)
            got = lines_of(raw[f], k)
            ce = oracle.sht_to_cartesian(W, H, [(float(l["rho"]), float(l["theta"])) for l in got])
            assert (cart[f][:k].view(np.uint32) == ce.view(np.uint32)).all(), ("cartesian", f)

        # grayscale + Otsu: one packed format and the Y plane
        host_565 = pad_frames(np.stack([rgb565le_of(i).reshape(H, W * 2) for i in imgs]), S * 2, rng)
        d_565 = A.new(n * 2, host_565)
        A.keep(d_565, host_565)
        for fmt, src, xg in ((capi.FMT_RGB565LE, d_565, [x["565"] for x in exp]), (capi.FMT_Y, d_in, [(i, x["otsu_y"]) for i, x in zip(imgs, exp)])):
            A.refill(d_gray); A.refill(d_otsu)
            plan.grayscale(ptr(src), fmt, ptr(d_gray))
            plan.otsu(ptr(d_gray), ptr(d_otsu))
            A.check("grayscale + otsu %d" % fmt)
            assert_maps(frames_view(d_gray, F, H, S, W), [g for g, _ in xg], "grayscale %d" % fmt)
            assert d_otsu.cpu().numpy().view(np.int32).tolist() == [t for _, t in xg], ("otsu", fmt)

        # fixed-point Gaussian, out of place and in place
        A.refill(d_out)
        plan.convlt_fixedpoint(ptr(d_in), gauss, gauss, ptr(d_out))
        A.check("convlt")
        assert_maps(out_frames(), [x["gauss"] for x in exp], "convlt")
        d_alias = A.new(n, host_in)
        plan.convlt_fixedpoint(ptr(d_alias), gauss, gauss, ptr(d_alias))
        A.check("convlt in place")
        assert_maps(out_frames(d_alias), [x["gauss"] for x in exp], "convlt in place")
    finally:
        plan.close()


def test_second_sht_on_the_plans_masks_clears_the_counters_itself(hip_ctx, oracle):
    """compvhip_plan_canny zeroes the plan's edge, line and tile counts in its tile kernel, and the compvhip_plan_houghsht(d_edges = 0)
    behind it relies on that and skips its own fill (countersFresh).  A second SHT on the same masks finds the first one's counts
    there: it has to clear them itself and return the same lines, counts, edge counts and accumulators.  The smallest two-frame
    geometry of the table whose frames have edges at all (at W = 17 the reference's column coverage [1, 1) + [16, 16) is empty)."""
    from compv_amd import capi
    W, H, S, F, theta = next(g for g in GEOMETRIES if g[3] == 2 and g[0] != 17)
    assert (W, H) == (13, 70)
    imgs = make_batch(W, H, F, W * 7 + H * 3 + F)
    thr = sht_threshold(W, H)
    e3 = [canny_expect(oracle, img, 3, capi.THRESHOLD_COMPARE_TO_GRADIENT, T_LOW, T_HIGH) for img in imgs]
    exp = [sht_expect(oracle, m, theta, thr) for m in e3]
    assert all(len(x[1]) > 0 for x in exp) and all((m != 0).any() for m in e3)   # counts that a missing fill would double
    R, T, _ = oracle.sht_dims(W, H, theta)
    A = Arena()
    host_in = pad_frames(imgs, S, np.random.default_rng(W + H))
    d_in = A.new(F * H * S, host_in)
    A.keep(d_in, host_in)
    d_out = A.new(F * H * S)
    d_lines = A.new(F * LINE_CAP * 20)
    d_counts = A.new(F * 4)
    plan = capi.Plan(hip_ctx, W, H, S, F, theta)
    try:
        plan.canny(ptr(d_in), T_LOW, T_HIGH, ptr(d_out))
        A.check("canny")
        assert_maps(frames_view(d_out, F, H, S, W), e3, "canny")
        for what in ("first houghsht(masks)", "second houghsht(masks)"):
            A.refill(d_lines); A.refill(d_counts)
            plan.houghsht(0, thr, 0, ptr(d_lines), LINE_CAP, ptr(d_counts))
            A.check(what)
            assert_lines(d_lines.cpu().numpy().reshape(F, LINE_CAP, 20), d_counts.cpu().numpy().view(np.int32), [x[1] for x in exp], what)
            assert edge_counts(plan, F).tolist() == [int((m != 0).sum()) for m in e3], what
            check_accs(plan, A, F, R, T, [x[0] for x in exp], what)
    finally:
        plan.close()


# ---------------------------------------------------------------------------------------------------------------
# the exchange-path batch
# ---------------------------------------------------------------------------------------------------------------
def test_plan_canny_exchange_path_batch_with_gap(hip_ctx, oracle):
    """canny_swar_tile_kernel<GAP = true, XCH = true>: a GAP width (W = 1 mod 16) in a launch over the exchange-path threshold of
    launch_swar (canny_swar_kernels.hip:522: frames * tilesY * tilesX >= 4 * 8192 waves).  The whole batch against the oracle, its
    first 64 frames through a second plan under the threshold (the three-loads path) byte for byte, then the pipeline."""
    from compv_amd import capi
    W, H, S, F, theta = XCH_GEOMETRY
    waves = F * ((H + 23) // 24) * ((W + 239) // 240)
    assert waves == swar_waves(W, H, F)
    assert waves >= XCH_MARGIN * XCH_MIN_WAVES, "retune the batch: it no longer reaches the exchange path with margin"
    F_small = 64
    assert swar_waves(W, H, F_small) < XCH_MIN_WAVES
    c = oracle.canny_coverage(W)
    assert not (c[0] >= W - 1 or c[1] <= c[0]), "W must leave a coverage gap"
    rng = np.random.default_rng(2731)
    kinds = [make_frame(k, W, H, 500 + i) for i, k in enumerate(KINDS)]
    # per-frame variation without generating 2731 text frames: shift the five base frames and add a frame-dependent offset
    imgs = np.empty((F, H, W), np.uint8)
    for f in range(F):
        b = kinds[f % len(kinds)]
        imgs[f] = b if f % len(kinds) == 2 else np.roll(b, (f * 7) % W, axis=1) ^ np.uint8(f & 0x1f)
    thr = sht_threshold(W, H)
    with pool() as ex:
        e3 = list(ex.map(lambda img: canny_expect(oracle, img, 3, capi.THRESHOLD_COMPARE_TO_GRADIENT, T_LOW, T_HIGH), imgs))
    A = Arena()
    n = F * H * S
    host_in = pad_frames(imgs, S, rng)
    d_in = A.new(n, host_in)
    A.keep(d_in, host_in)
    d_out = A.new(n)
    plan = capi.Plan(hip_ctx, W, H, S, F, theta)
    small = capi.Plan(hip_ctx, W, H, S, F_small, theta)
    try:
        plan.canny(ptr(d_in), T_LOW, T_HIGH, ptr(d_out))
        A.check("canny (exchange path)")
        big = frames_view(d_out, F, H, S, W)
        assert_maps(big, e3, "canny (exchange path)")
        d_small = A.new(F_small * H * S)
        small.canny(ptr(d_in), T_LOW, T_HIGH, ptr(d_small))
        A.check("canny (three loads)")
        assert (frames_view(d_small, F_small, H, S, W) == big[:F_small]).all()

        line_cap = 1024
        d_lines = A.new(F * line_cap * 20)
        d_counts = A.new(F * 4)
        A.refill(d_out)
        plan.pipeline(ptr(d_in), T_LOW, T_HIGH, thr, 0, ptr(d_out), ptr(d_lines), line_cap, ptr(d_counts))
        A.check("pipeline (exchange path)")
        assert_maps(frames_view(d_out, F, H, S, W), e3, "pipeline (exchange path)")
        assert edge_counts(plan, F).tolist() == [int((m != 0).sum()) for m in e3]
        counts = d_counts.cpu().numpy().view(np.int32)
        raw = d_lines.cpu().numpy().reshape(F, line_cap, 20)
        subset = sorted(set(range(0, F, 97)) | {F - 1})
        with pool() as ex:
            lx = list(ex.map(lambda f: oracle.sht(e3[f], theta, thr), subset))
        assert_lines(raw[subset], counts[subset], lx, "pipeline (exchange path)")
        assert sum(len(x) for x in lx) > 0
    finally:
        small.close()
        plan.close()


# ---------------------------------------------------------------------------------------------------------------
# grid and grouping variants
# ---------------------------------------------------------------------------------------------------------------
def _sht_on_foreign_maps(hip_ctx, oracle, W, H, S, F, theta, imgs, thr):
    """A fresh plan's SHT on the oracle's Canny maps of imgs (255 in the padding): accumulator cell by cell and lines vs the oracle."""
    from compv_amd import capi
    e = [canny_expect(oracle, img, 3, capi.THRESHOLD_COMPARE_TO_GRADIENT, T_LOW, T_HIGH) for img in imgs]
    R, T, _ = oracle.sht_dims(W, H, theta)
    host_e = np.full((F, H, S), 255, np.uint8)
    host_e[:, :, :W] = np.stack(e)
    A = Arena()
    d_e = A.new(F * H * S, host_e)
    A.keep(d_e, host_e)
    d_lines = A.new(F * LINE_CAP * 20)
    d_counts = A.new(F * 4)
    plan = capi.Plan(hip_ctx, W, H, S, F, theta)
    try:
        plan.houghsht(ptr(d_e), thr, 0, ptr(d_lines), LINE_CAP, ptr(d_counts))
        A.check("houghsht")
        exp = [sht_expect(oracle, m, theta, thr) for m in e]
        assert_lines(d_lines.cpu().numpy().reshape(F, LINE_CAP, 20), d_counts.cpu().numpy().view(np.int32), [x[1] for x in exp], "houghsht")
        check_accs(plan, A, F, R, T, [x[0] for x in exp], "houghsht")
        assert sum(len(x[1]) for x in exp) > 0
    finally:
        plan.close()


@pytest.mark.parametrize("W,H,S,F,theta", [(241, 25, 248, 3, 0.5), (641, 480, 648, 2, 1.0), (481, 97, 488, 3, 1.5), (100, 1537, 104, 2, 2.0)],
                         ids=lambda v: str(v))
def test_vote_window_knob_is_bit_exact(hip_ctx, oracle, monkeypatch, W, H, S, F, theta):
    """COMPVHIP_VOTE_MAX_WINDOW (api.cpp, read when a plan is made) forces finer vote tile grids; the voting is exact on any grid
    (border tiles are not clipped, the 16-row window alignment follows the grid)."""
    from compv_amd import capi
    imgs = make_batch(W, H, F, W + H)
    thr = sht_threshold(W, H)
    grids = []
    for win in (None, 640, 200, 96, 64):
        if win is None:
            monkeypatch.delenv("COMPVHIP_VOTE_MAX_WINDOW", raising=False)
        else:
            monkeypatch.setenv("COMPVHIP_VOTE_MAX_WINDOW", str(win))
        nx, ny, rows = capi.houghsht_vote_grid(W, H, theta, F)
        if win is not None:
            assert rows <= win
        grids.append(nx * ny)
        _sht_on_foreign_maps(hip_ctx, oracle, W, H, S, F, theta, imgs, thr)
    assert grids == sorted(grids) and grids[-1] > grids[0], grids    # the knob made the grid finer


def test_vote_grid_that_does_not_fit_is_refused(hip_ctx, monkeypatch):
    """With a 64-row window a 32 x 20000 frame needs more tiles than the grid search tries: the geometry helper and the plan's SHT
    refuse with E_NOT_IMPLEMENTED and write nothing."""
    from compv_amd import capi
    W, H, S, F = 32, 20000, 32, 1
    monkeypatch.setenv("COMPVHIP_VOTE_MAX_WINDOW", "64")
    with pytest.raises(capi.CompvHipError) as err:
        capi.houghsht_vote_grid(W, H, 1.0, F)
    assert err.value.code == capi.E_NOT_IMPLEMENTED
    A = Arena()
    host_e = np.zeros((F, H, S), np.uint8)
    host_e[:, ::7, 3] = 255
    d_e = A.new(F * H * S, host_e)
    d_lines = A.new(F * LINE_CAP * 20)
    d_counts = A.new(F * 4)
    plan = capi.Plan(hip_ctx, W, H, S, F, 1.0)
    try:
        with pytest.raises(capi.CompvHipError) as err:
            plan.houghsht(ptr(d_e), 5, 0, ptr(d_lines), LINE_CAP, ptr(d_counts))
        assert err.value.code == capi.E_NOT_IMPLEMENTED
        A.check("refused houghsht")
        assert (d_lines.cpu().numpy() == SENTINEL).all() and (d_counts.cpu().numpy() == SENTINEL).all()
    finally:
        plan.close()
    monkeypatch.delenv("COMPVHIP_VOTE_MAX_WINDOW")
    assert capi.houghsht_vote_grid(W, H, 1.0, F)[0] >= 1


def test_vote_grid_depends_on_the_frame_count(hip_ctx, oracle):
    """planVoteTiles prices finer grids only for plans that leave the chip nearly empty ("starved": frames x tiles x theta groups < 64),
    so one geometry votes on different grids with 1 and with 16 frames; both exact."""
    from compv_amd import capi
    W, H, S, theta = 201, 150, 208, 1.0
    g1, g16 = capi.houghsht_vote_grid(W, H, theta, 1), capi.houghsht_vote_grid(W, H, theta, 16)
    assert g1 != g16, (g1, g16)
    imgs = make_batch(W, H, 16, 16)
    thr = sht_threshold(W, H)
    _sht_on_foreign_maps(hip_ctx, oracle, W, H, S, 1, theta, imgs[:1], thr)
    _sht_on_foreign_maps(hip_ctx, oracle, W, H, S, 16, theta, imgs, thr)


def test_plan_houghkht_group_knob(hip_ctx, oracle, monkeypatch):
    """COMPVHIP_KHT_GROUP (frames per stage group, read on every compvhip_plan_houghkht call) at 1, 3 and 8 on 11 frames of a ragged
    S > W geometry: per-frame lines, counts and GS equal the default run and the oracle."""
    from compv_amd import capi
    W, H, S, F = 321, 243, 336, 11
    imgs = make_batch(W, H, F, 11)
    e3 = [canny_expect(oracle, img, 3, capi.THRESHOLD_COMPARE_TO_GRADIENT, T_LOW, T_HIGH) for img in imgs]
    with pool() as ex:
        exp = list(ex.map(lambda e: oracle.kht(e, 1.0, 1.0, 12), e3))
    assert sum(len(el) for el, _ in exp) > 0
    A = Arena()
    rng = np.random.default_rng(11)
    host_in = pad_frames(imgs, S, rng)
    d_in = A.new(F * H * S, host_in)
    A.keep(d_in, host_in)
    d_out = A.new(F * H * S)
    plan = capi.Plan(hip_ctx, W, H, S, F, 1.0)
    try:
        plan.canny(ptr(d_in), T_LOW, T_HIGH, ptr(d_out))
        A.check("canny")
        assert_maps(frames_view(d_out, F, H, S, W), e3, "canny")
        A.keep(d_out, d_out.cpu().numpy())                              # the KHT only reads the edge maps
        monkeypatch.delenv("COMPVHIP_KHT_GROUP", raising=False)
        default = plan.houghkht(ptr(d_out), 1.0, 1.0, 12)
        A.check("houghkht default")
        for g in (1, 3, 8):
            monkeypatch.setenv("COMPVHIP_KHT_GROUP", str(g))
            lines, gs = plan.houghkht(ptr(d_out), 1.0, 1.0, 12)
            A.check("houghkht group %d" % g)
            for f in range(F):
                el, egs = exp[f]
                assert lines[f].tobytes() == default[0][f].tobytes() and gs[f] == default[1][f], (g, f)
                assert [(float(l["rho"]), float(l["theta"]), int(l["strength"])) for l in lines[f]] == \
                       [(float(np.float32(l[0])), float(np.float32(l[1])), int(l[2])) for l in el], (g, f)
                assert (gs[f] == egs) if len(el) else (gs[f] is None), (g, f)
    finally:
        plan.close()
