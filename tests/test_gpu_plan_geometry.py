"""The batched plan API (compvhip_plan_*) at ragged widths, padded row strides and large batches, frame by frame against the oracle.

Every device buffer sits between two 4096-byte guards holding a fixed pattern; outputs start filled with a sentinel over their valid
region too (so every valid pixel, count and accumulator cell must be written), and the input's padding columns [W, S) hold seeded
random bytes, 255 included.  After every call the guards must be intact and, for out-of-place calls, the input unchanged.  Output
padding [W, S) is not asserted on: kernels may write it, as the reference's SIMD does.  The bar is the suite's: bit-exact maps,
accumulators cell by cell, line sets in canonical order, counts, Otsu levels, KHT GS.

The geometry table lives in tests/plan_geometries.py (checked on the CPU by tests/test_plan_geometries.py).
"""
import concurrent.futures as cf

import numpy as np
import pytest

from hysteresis_cases import text_frame   # the text-like page, shared with the hysteresis cases
from oracle_bindings import synth_frame
from plan_geometries import GEOMETRIES, XCH_GEOMETRY, XCH_MARGIN, XCH_MIN_WAVES, swar_waves

pytestmark = pytest.mark.gpu

GUARD = 4096
SENTINEL = 0xA5
LINE_CAP = 4096
KEY_CAP = 65536          # lines beyond max(lineCap, 65536) per frame make the plan's line set an arbitrary subset (compv_hip.h)
T_LOW, T_HIGH = 59.0, 119.0


# ---------------------------------------------------------------------------------------------------------------
# guarded, poisoned device buffers
# ---------------------------------------------------------------------------------------------------------------
class Arena:
    """Device buffers as uint8 tensors with a guard pattern before and after; check() verifies every guard and every input
    registered with keep() (which must be unchanged)."""

    def __init__(self):
        import torch
        self.torch = torch
        self.dev = torch.device("cuda:0")
        self.pattern = ((torch.arange(GUARD, dtype=torch.int32) * 167 + 89) & 0xff).to(torch.uint8).to(self.dev)
        self.bufs = []
        self.kept = []

    def new(self, nbytes, fill=SENTINEL):
        raw = self.torch.empty(nbytes + 2 * GUARD, dtype=self.torch.uint8, device=self.dev)
        raw[:GUARD] = self.pattern
        raw[GUARD + nbytes:] = self.pattern
        body = raw[GUARD:GUARD + nbytes]
        if isinstance(fill, np.ndarray):
            assert fill.dtype == np.uint8 and fill.size == nbytes
            body.copy_(self.torch.from_numpy(np.ascontiguousarray(fill).reshape(-1)))
        else:
            body.fill_(fill)
        self.bufs.append(raw)
        return body

    def keep(self, body, host):
        self.kept.append((body, np.ascontiguousarray(host).reshape(-1).copy()))

    def refill(self, body, fill=SENTINEL):
        body.fill_(fill)

    def reload(self, body, host):
        """new content for a buffer registered with keep(): the device bytes, and the copy check() holds them against"""
        h = np.ascontiguousarray(host).view(np.uint8).reshape(-1).copy()
        assert h.size == body.numel() and any(b is body for b, _ in self.kept)
        body.copy_(self.torch.from_numpy(h))
        self.torch.cuda.synchronize()
        self.kept = [(b, h if b is body else old) for b, old in self.kept]

    def check(self, what):
        self.torch.cuda.synchronize()
        for raw in self.bufs:
            assert self.torch.equal(raw[:GUARD], self.pattern), "%s: guard before a buffer overwritten" % what
            assert self.torch.equal(raw[-GUARD:], self.pattern), "%s: guard after a buffer overwritten" % what
        for body, host in self.kept:
            assert (body.cpu().numpy() == host).all(), "%s: input modified" % what


def ptr(t):
    return t.data_ptr()


def frames_view(body, F, H, S, W):
    """(F, H, W) host copy of the valid region of a [F][H][S] device buffer."""
    return body.cpu().numpy().reshape(F, H, S)[:, :, :W]


def d2h(dptr, nbytes):
    """Device -> host copy of memory the plan owns (the edge counts)."""
    import ctypes as C
    import torch
    from compv_amd import capi
    L = capi.load()
    L.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    out = np.empty(nbytes, np.uint8)
    torch.cuda.synchronize()
    assert L.hipMemcpy(out.ctypes.data, dptr, nbytes, 2) == 0          # hipMemcpyDeviceToHost
    return out


def pad_frames(valid, row_bytes, rng):
    """[F][H][Wb] valid bytes -> [F][H][row_bytes] whose padding holds seeded random bytes, with a 255 in one padding column of every row."""
    F, H, Wb = valid.shape
    out = rng.integers(0, 256, (F, H, row_bytes), dtype=np.uint8)
    if row_bytes > Wb:
        out[:, :, Wb + rng.integers(0, row_bytes - Wb)] = 255
    out[:, :, :Wb] = valid
    return out


# ---------------------------------------------------------------------------------------------------------------
# frame content
# ---------------------------------------------------------------------------------------------------------------
def checker_frame(W, H, seed):
    c = 3 + seed % 7
    x = np.arange(W)[None, :] // c
    y = np.arange(H)[:, None] // c
    return (((x + y) & 1) * 255).astype(np.uint8)


KINDS = ("synth", "noise", "zero", "text", "checker")   # the all-zero frame sits between two dense ones


def make_frame(kind, W, H, seed):
    if kind == "synth":
        return synth_frame(W, H, seed)
    if kind == "noise":
        return np.random.default_rng(seed).integers(0, 256, (H, W), dtype=np.uint8)
    if kind == "zero":
        return np.zeros((H, W), np.uint8)
    if kind == "text":
        return text_frame(W, H, seed)
    return checker_frame(W, H, seed)


def make_batch(W, H, F, seed):
    return np.stack([make_frame(KINDS[(seed + f) % len(KINDS)], W, H, seed * 1000 + f) for f in range(F)])


def rgb_of(img):
    b = img.astype(np.int32)
    return np.stack([np.clip(b + 20, 0, 255), b * 3 // 4, 255 - b], axis=-1).astype(np.uint8)


def rgb565le_of(img):
    b = img.astype(np.uint16)
    v = ((b >> 3) << 11) | ((b >> 2) << 5) | ((255 - b) >> 3)
    return np.stack([v & 0xff, v >> 8], axis=-1).astype(np.uint8)


# ---------------------------------------------------------------------------------------------------------------
# oracle side, one frame at a time on a thread pool (ctypes releases the GIL inside the oracle)
# ---------------------------------------------------------------------------------------------------------------
def pool():
    from compv_amd import capi
    return cf.ThreadPoolExecutor(max_workers=max(1, min(16, capi.host_cpu_budget())))


def canny_expect(orc, img, ksize, mode, tl, th):
    from compv_amd import capi
    if mode == capi.THRESHOLD_OTSU:
        lo, hi = orc.otsu_canny_thresholds(orc.otsu(img), tl, th)
        rc, e = orc.canny(img, float(lo), float(hi), ksize)
    else:
        rc, e = orc.canny(img, tl, th, ksize, mode)
    assert rc == 0, rc
    return e


def sht_expect(orc, edges, theta, thr):
    H, W = edges.shape
    acc = orc.sht_acc(edges, theta)
    return acc, orc.sht_lines_from_acc(acc, W, H, theta, thr)


def canny_modes():
    from compv_amd import capi
    return [(3, capi.THRESHOLD_COMPARE_TO_GRADIENT, T_LOW, T_HIGH), (3, capi.THRESHOLD_PERCENT_OF_MEAN, 0.68, 1.36), (3, capi.THRESHOLD_OTSU, 0.5, 1.0),
            (5, capi.THRESHOLD_COMPARE_TO_GRADIENT, 400.0, 900.0), (5, capi.THRESHOLD_PERCENT_OF_MEAN, 0.68, 1.36), (5, capi.THRESHOLD_OTSU, 0.5, 1.0)]


def sht_threshold(W, H):
    return max(3, min(W, H) // 2)


def frame_expectations(orc, img, theta, want_kht, gauss):
    from compv_amd import capi
    H, W = img.shape
    thr = sht_threshold(W, H)
    x = {"dete": {op: orc.edge_dete(img, op)[0] for op in (capi.OP_SOBEL, capi.OP_SCHARR, capi.OP_PREWITT)}}
    x["canny"] = {m[:2]: canny_expect(orc, img, *m) for m in canny_modes()}
    e3 = x["canny"][(3, capi.THRESHOLD_COMPARE_TO_GRADIENT)]
    x["sht"] = sht_expect(orc, e3, theta, thr)
    x["sht5"] = sht_expect(orc, x["canny"][(5, capi.THRESHOLD_PERCENT_OF_MEAN)], theta, thr)[1]
    x["otsu_y"] = int(orc.otsu(img))
    gray = orc.grayscale(rgb_of(img).reshape(H, W * 3), capi.FMT_RGB24, W)
    lo, hi = orc.otsu_canny_thresholds(orc.otsu(gray), 0.5, 1.0)
    rc, eg = orc.canny(gray, float(lo), float(hi))
    assert rc == 0
    x["rgb"] = (gray, int(orc.otsu(gray)), eg, sht_expect(orc, eg, theta, thr)[1])
    g565 = orc.grayscale(rgb565le_of(img).reshape(H, W * 2), capi.FMT_RGB565LE, W)
    x["565"] = (g565, int(orc.otsu(g565)))
    rc, x["gauss"] = orc.convlt_fxp(img, gauss, gauss)
    assert rc == 0
    if want_kht:
        x["kht"] = orc.kht(e3, 1.0, theta, 12)
    return x


def lines_of(raw_f, n):
    from compv_amd import capi
    return np.frombuffer(raw_f[:n].tobytes(), dtype=capi.LINE_DTYPE)


def assert_lines(raw, counts, exp, what):
    """raw: (F, cap, 20) bytes; counts: int32[F]; exp: per-frame oracle lines in canonical order."""
    for f, e in enumerate(exp):
        assert int(counts[f]) == len(e), (what, f, int(counts[f]), len(e))
        assert len(e) <= KEY_CAP, (what, f, len(e))                      # otherwise the test itself would be out of contract
        n = min(len(e), raw.shape[1])
        got = lines_of(raw[f], n)
        assert [(float(l["rho"]), float(l["theta"]), int(l["strength"]), int(l["row"]), int(l["col"])) for l in got] == \
               [(float(np.float32(l[0])), float(np.float32(l[1])), int(l[2]), int(l[3]), int(l[4])) for l in e[:n]], (what, f)


def assert_maps(got, exp, what):
    for f, e in enumerate(exp):
        if not (got[f] == e).all():
            ys, xs = np.nonzero(got[f] != e)
            raise AssertionError("%s: frame %d differs at %d pixels, first (y=%d, x=%d): got %d, expected %d"
                                 % (what, f, len(ys), ys[0], xs[0], got[f][ys[0], xs[0]], e[ys[0], xs[0]]))


def check_accs(plan, arena, F, R, T, exp_accs, what):
    d_acc = arena.new(R * T * 4)
    for f in range(F):
        arena.refill(d_acc)
        plan.acc_export(f, ptr(d_acc), T)
        arena.check("%s acc_export %d" % (what, f))
        got = d_acc.cpu().numpy().view(np.int32).reshape(R, T)
        assert (got == exp_accs[f]).all(), (what, f, int((got != exp_accs[f]).sum()))


def edge_counts(plan, F):
    """compvhip_plan_edge_counts: counted by the SHT's voting kernel, so meaningful after an SHT or a pipeline step."""
    return d2h(plan.edge_counts_ptr(), 4 * F).view(np.int32)


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
