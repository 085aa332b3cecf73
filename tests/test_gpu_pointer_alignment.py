"""Every plan call at device pointers off their natural alignment: served bit for bit, or refused with nothing written (include/compv_hip.h, "Alignment
of device pointers"; the contract table is tests/alignment_cases.py, the coverage table docs/dispatch_coverage.md, "Pointer alignment").

Buffers.  Every buffer is one uint8 torch allocation (256-byte aligned, asserted) filled with a sentinel; its payload starts 64 + off bytes in and at least
64 sentinel bytes follow it.  Both bands must hold the sentinel after every call, an input must come back unchanged, and where the header promises that
columns >= W are never written those must hold the sentinel too.

Served pointers.  F = 3 frames, so frames 1 and 2 inherit the misalignment through S * H.  Geometries (W, H, S): (43, 49, 48) -- one Canny tile column,
three row tiles; (515, 67, 520) -- three tile columns with a ragged last one, past one resolve band and one 512-column mask word row, S % 16 == 8; and
(64, 33, 64) for bytes_to_bits' 16-byte arm (S % 16 == 0, x + 32 <= W) at offsets 1, 4 and 8.  Offset pairs (input, output): (1, 0), (0, 1), (3, 2),
(4, 4), (8, 12): 4 reaches the 8-byte groups, 8 and 12 the 16-byte groups.  Every result is compared, by bit pattern and on all frames, with the model or
oracle the stage's own GPU test uses; the expectations are computed once per geometry.

Refused pointers.  One call per row of the table with that pointer alone moved by 1 byte (for N = 8 also by 4, for N = 16 also by 8), everything else
valid, on a handle that has run nothing: the return code, a compvhip_last_error that speaks of alignment, every buffer still the sentinel,
compvhip_live_allocations unchanged.  No kernel is ever launched on a typed array off its alignment.

The exchange arm of the 3 x 3 Canny (plan_geometries.XCH_GEOMETRY, about 128 MB) is left out: it reads through the same buffer descriptor as the arm
that runs here."""
import functools

import numpy as np
import pytest

import alignment_cases as ac
import components_rig as tgc
import morph_model as mm
import orb_pyramid_model as pm
import remap_cases as rc
import remap_model as rm
import sht_fit_rig as tgf
import sht_segments_rig as tgs
from gpu_support import (BAND, FIT_BYTES, LINE_CAP, SEG_BYTES, SENTINEL, T_HIGH, T_LOW, assert_lines, assert_maps, canny_modes, check_accs, edge_counts,
                         frame_expectations, frames_view, lines_of, make_batch, pad_frames, ptr, rgb_of, sht_expect, sht_threshold)
from kht_canon_model import line_bits, model_line_bits

pytestmark = pytest.mark.gpu

F = 3
THETA = 1.0
GEOMETRIES = ((43, 49, 48), (515, 67, 520))
BITS16 = (64, 33, 64)                      # bytes_to_bits' 16-byte arm
PAIRS = ((1, 0), (0, 1), (3, 2), (4, 4), (8, 12))
IN_OFFSETS = tuple(sorted({p[0] for p in PAIRS}))          # 0, 1, 3, 4, 8
GID = lambda g: "%dx%d_S%d" % g          # noqa: E731
MAX_LINES = 12                             # lines per frame the segment and fit models walk (the calls' maxLines)


class Bands:
    """Arena of tests/gpu_support.py with 64-byte sentinel bands and a payload that starts `off` bytes behind the first one"""

    def __init__(self):
        import torch
        self.torch = torch
        self.dev = torch.device("cuda:0")
        self.bufs, self.kept = [], []

    def new(self, nbytes, fill=SENTINEL, off=0):
        tail = BAND + (-(off + nbytes)) % 16
        raw = self.torch.full((BAND + off + nbytes + tail,), SENTINEL, dtype=self.torch.uint8, device=self.dev)
        assert raw.data_ptr() % 256 == 0, "the allocation itself must be aligned for `off` to mean anything"
        body = raw[BAND + off:BAND + off + nbytes]
        assert body.data_ptr() == raw.data_ptr() + BAND + off
        if isinstance(fill, np.ndarray):
            assert fill.dtype == np.uint8 and fill.size == nbytes
            body.copy_(self.torch.from_numpy(np.ascontiguousarray(fill).reshape(-1)))
        elif fill != SENTINEL:
            body.fill_(fill)
        self.bufs.append((raw, BAND + off, nbytes))
        return body

    def keep(self, body, host):
        self.kept.append((body, np.ascontiguousarray(host).reshape(-1).copy()))

    def refill(self, body, fill=SENTINEL):
        body.fill_(fill)

    def check(self, what):
        self.torch.cuda.synchronize()
        for raw, start, n in self.bufs:
            assert bool((raw[:start] == SENTINEL).all()), "%s: bytes in front of a buffer written" % what
            assert bool((raw[start + n:] == SENTINEL).all()), "%s: bytes behind a buffer written" % what
        for body, host in self.kept:
            assert (body.cpu().numpy() == host).all(), "%s: input modified" % what

    def all_sentinel(self):
        self.torch.cuda.synchronize()
        return all(bool((raw == SENTINEL).all()) for raw, _, _ in self.bufs)


# ---- content and expectations, once per geometry -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def frames_of(g):
    W, H, _ = g
    out = make_batch(W, H, F, W * 7 + H * 3 + F)          # synth / noise / zero / text / checker frames, three different ones
    out.setflags(write=False)
    return out


def gauss5():
    from compv_amd import capi
    return capi.gauss_kernel_fixedpoint(5, 1.0)


_EXPECT = {}


def expectations(orc, g):
    """per frame: the dictionary of gpu_support.frame_expectations (detectors, the six Canny modes, SHT, Otsu, RGB24 chain, K = 5 blur, KHT)"""
    if g not in _EXPECT:
        _EXPECT[g] = [frame_expectations(orc, img, THETA, True, gauss5()) for img in frames_of(g)]
    return _EXPECT[g]


def upload(A, valid, S, off, seed, keep=True):
    """[F][H][W * bpp] -> a device batch at stride S * bpp, `off` bytes into its buffer, random bytes in the padding"""
    host = pad_frames(valid, S, np.random.default_rng(seed))
    d = A.new(host.size, host.reshape(-1), off)
    if keep:
        A.keep(d, host)
    return d


def edge_maps(orc, g):
    from compv_amd import capi
    return [x["canny"][(3, capi.THRESHOLD_COMPARE_TO_GRADIENT)] for x in expectations(orc, g)]


def upload_edges(A, e3, g, off):
    W, H, S = g
    host = np.full((F, H, S), 255, np.uint8)          # 255 in the padding: columns >= W are never edges
    host[:, :, :W] = np.stack(e3)
    d = A.new(host.size, host.reshape(-1), off)
    A.keep(d, host)
    return d


def untouched_padding(d_out, g, what):
    W, H, S = g
    assert (d_out.cpu().numpy().reshape(F, H, S)[:, :, W:] == SENTINEL).all(), "%s: columns >= W written" % what


# ---- served: Canny, the detectors, the blur ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", GEOMETRIES, ids=GID)
def test_canny_at_unaligned_frames_and_edge_maps(hip_ctx, oracle, g):
    """canny_swar_tile_kernel<KS = 3, 5> (the frame through a buffer descriptor built on the raw pointer, the edge bytes through 16-byte stores), the resolve
    rounds' byte patches, frame_sum_kernel (PERCENT_OF_MEAN) and the Otsu histogram (OTSU) on the caller's frame; in place at base + 3"""
    from compv_amd import capi
    W, H, S = g
    exp = expectations(oracle, g)
    plan = capi.Plan(hip_ctx, W, H, S, F, THETA)
    try:
        for oi, oo in PAIRS:
            A = Bands()
            d_in = upload(A, frames_of(g), S, oi, W + oi)
            d_out = A.new(F * H * S, off=oo)
            for ks, mode, tl, th in canny_modes():
                what = "canny %d/%d at +%d -> +%d" % (ks, mode, oi, oo)
                A.refill(d_out)
                plan.canny(ptr(d_in), tl, th, ptr(d_out), ks, mode)
                A.check(what)
                assert_maps(frames_view(d_out, F, H, S, W), [x["canny"][(ks, mode)] for x in exp], what)
        A = Bands()
        d_io = upload(A, frames_of(g), S, 3, W, keep=False)
        for ks, mode, tl, th in (canny_modes()[0], canny_modes()[4]):
            d_io.copy_(A.torch.from_numpy(pad_frames(frames_of(g), S, np.random.default_rng(W)).reshape(-1)))
            plan.canny(ptr(d_io), tl, th, ptr(d_io), ks, mode)
            A.check("canny in place at +3")
            assert_maps(frames_view(d_io, F, H, S, W), [x["canny"][(ks, mode)] for x in exp], "canny %d/%d in place at +3" % (ks, mode))
    finally:
        plan.close()


@pytest.mark.parametrize("g", GEOMETRIES, ids=GID)
def test_detectors_and_blur_at_unaligned_frames(hip_ctx, oracle, g):
    """edge_dete_kernels for the three operators (descriptor reads, dword stores); convlt_fxp_fused_kernel<5> out of place and the two-pass path
    (convlt_fxp_hz_kernel / _vt_kernel through the plan's scratch) in place at base + 3"""
    from compv_amd import capi
    W, H, S = g
    exp = expectations(oracle, g)
    plan = capi.Plan(hip_ctx, W, H, S, F, THETA)
    try:
        for oi, oo in PAIRS:
            A = Bands()
            d_in = upload(A, frames_of(g), S, oi, W + oi)
            d_out = A.new(F * H * S, off=oo)
            for op in (capi.OP_SOBEL, capi.OP_SCHARR, capi.OP_PREWITT):
                what = "edge_dete %d at +%d -> +%d" % (op, oi, oo)
                A.refill(d_out)
                plan.edge_dete(ptr(d_in), op, ptr(d_out))
                A.check(what)
                assert_maps(frames_view(d_out, F, H, S, W), [x["dete"][op] for x in exp], what)
            A.refill(d_out)
            plan.convlt_fixedpoint(ptr(d_in), gauss5(), gauss5(), ptr(d_out))
            A.check("blur at +%d -> +%d" % (oi, oo))
            assert_maps(frames_view(d_out, F, H, S, W), [x["gauss"] for x in exp], "blur (fused) at +%d -> +%d" % (oi, oo))
        A = Bands()
        d_io = upload(A, frames_of(g), S, 3, W, keep=False)
        plan.convlt_fixedpoint(ptr(d_io), gauss5(), gauss5(), ptr(d_io))
        A.check("blur in place at +3")
        assert_maps(frames_view(d_io, F, H, S, W), [x["gauss"] for x in exp], "blur (two passes) in place at +3")
    finally:
        plan.close()


# ---- served: grayscale, Otsu, thresholds -------------------------------------------------------------------------------------------------------
def packed_of(img, fmt):
    """(H, W * bpp) samples of a gray frame in one format of each load shape of gray_kernel"""
    from compv_amd import capi
    H, W = img.shape
    rgb = rgb_of(img)
    if fmt == capi.FMT_RGBA32:
        return np.concatenate([rgb, (img ^ 0x5a)[:, :, None]], axis=-1).reshape(H, W * 4)
    if fmt == capi.FMT_RGB24:
        return rgb.reshape(H, W * 3)
    if fmt == capi.FMT_RGB565LE:
        b = img.astype(np.uint16)
        v = ((b >> 3) << 11) | ((b >> 2) << 5) | ((255 - b) >> 3)
        return np.stack([v & 0xff, v >> 8], axis=-1).astype(np.uint8).reshape(H, W * 2)
    assert fmt == capi.FMT_Y
    return img


@pytest.mark.parametrize("g", GEOMETRIES, ids=GID)
def test_grayscale_and_otsu_at_unaligned_frames(hip_ctx, oracle, g):
    """gray_kernel<FMT>: the uint4 pair (RGBA32), the uint2 triple (RGB24), the single uint4 (RGB565LE), the single uint2 (Y), and its 8-byte store; then
    hist256_kernel's 8-byte loads on the plane it wrote"""
    from compv_amd import capi
    W, H, S = g
    plan = capi.Plan(hip_ctx, W, H, S, F, THETA)
    try:
        for fmt in (capi.FMT_RGBA32, capi.FMT_RGB24, capi.FMT_RGB565LE, capi.FMT_Y):
            bpp = capi.FMT_BYTES[fmt]
            valid = np.stack([packed_of(img, fmt) for img in frames_of(g)])
            gray = [oracle.grayscale(v, fmt, W) for v in valid]
            levels = [int(oracle.otsu(x)) for x in gray]
            for oi, oo in PAIRS:
                what = "format %d at +%d -> +%d" % (fmt, oi, oo)
                A = Bands()
                d_in = upload(A, valid, S * bpp, oi, fmt + oi)
                d_gray = A.new(F * H * S, off=oo)
                d_lv = A.new(F * 4)
                plan.grayscale(ptr(d_in), fmt, ptr(d_gray))
                plan.otsu(ptr(d_gray), ptr(d_lv))
                A.check(what)
                assert_maps(frames_view(d_gray, F, H, S, W), gray, "grayscale " + what)
                assert d_lv.cpu().numpy().view(np.int32).tolist() == levels, "otsu " + what
    finally:
        plan.close()


@pytest.mark.parametrize("g", GEOMETRIES, ids=GID)
def test_thresholds_at_unaligned_frames(hip_ctx, g):
    """threshold_kernel with a level array (8-byte loads and stores, the byte tail at W % 8 != 0); threshold_adaptive_kernel at block sizes 3 and 9, out of
    place and, through the plan's plane and the 2-D copy, in place at base + 3"""
    from compv_amd import capi
    W, H, S = g
    imgs = frames_of(g)
    levels = np.array([97, 300, -4], np.int32)          # clipped to 0 .. 255 by the kernel
    exp_t = [mm.threshold(img, float(min(max(int(t), 0), 255))) for img, t in zip(imgs, levels)]
    exp_a = {bs: [mm.adaptive(img, bs, 7.0, 200.0, bs == 9) for img in imgs] for bs in (3, 9)}
    plan = capi.Plan(hip_ctx, W, H, S, F, THETA)
    try:
        for oi, oo in PAIRS:
            A = Bands()
            d_in = upload(A, imgs, S, oi, W + oi)
            d_out = A.new(F * H * S, off=oo)
            d_lv = A.new(F * 4, levels.view(np.uint8))
            what = "threshold at +%d -> +%d" % (oi, oo)
            plan.threshold(ptr(d_in), 0.0, ptr(d_out), ptr(d_lv))
            A.check(what)
            assert_maps(frames_view(d_out, F, H, S, W), exp_t, what)
            untouched_padding(d_out, g, what)
            for bs in (3, 9):
                what = "adaptive %d at +%d -> +%d" % (bs, oi, oo)
                A.refill(d_out)
                plan.threshold_adaptive(ptr(d_in), bs, 7.0, 200.0, bs == 9, ptr(d_out))
                A.check(what)
                assert_maps(frames_view(d_out, F, H, S, W), exp_a[bs], what)
                untouched_padding(d_out, g, what)
        for bs in (3, 9):
            A = Bands()
            host = pad_frames(imgs, S, np.random.default_rng(W + bs))
            d_io = A.new(host.size, host.reshape(-1), 3)
            plan.threshold_adaptive(ptr(d_io), bs, 7.0, 200.0, bs == 9, ptr(d_io))
            A.check("adaptive in place at +3")
            got = d_io.cpu().numpy().reshape(F, H, S)
            assert_maps(got[:, :, :W], exp_a[bs], "adaptive %d in place at +3" % bs)
            assert (got[:, :, W:] == host[:, :, W:]).all(), "adaptive in place: columns >= W written"
    finally:
        plan.close()


# ---- served: morphology ---------------------------------------------------------------------------------------------------------------------------
def morph_arms():
    from compv_amd import capi
    return (("rect15x3 separable", mm.strel(mm.RECT, 15, 3), capi.MORPH_KERNEL_SEPARABLE), ("cross5x5 separable", mm.strel(mm.CROSS, 5, 5), capi.MORPH_KERNEL_SEPARABLE),
            ("random5x7 general", (np.random.default_rng(57).random((7, 5)) < 0.4).astype(np.uint8) * 255, capi.MORPH_KERNEL_GENERAL))


@pytest.mark.parametrize("g", GEOMETRIES, ids=GID)
def test_morph_at_unaligned_frames(hip_ctx, g):
    """morph_separable_kernel<rect>, <cross> and morph_general_kernel, each with erode (one launch) and close (two, through the plan's plane)"""
    from compv_amd import capi
    W, H, S = g
    imgs = frames_of(g)
    plan = capi.Plan(hip_ctx, W, H, S, F, THETA)
    try:
        for name, se, kernel in morph_arms():
            for op in (mm.ERODE, mm.CLOSE):
                exp = [mm.morph(img, se, op, mm.BORDER_REPLICATE) for img in imgs]
                for oi, oo in PAIRS:
                    what = "morph %s op %d at +%d -> +%d" % (name, op, oi, oo)
                    A = Bands()
                    d_in = upload(A, imgs, S, oi, W + oi)
                    d_out = A.new(F * H * S, off=oo)
                    plan.morph(ptr(d_in), se, op, capi.BORDER_REPLICATE, ptr(d_out), kernel)
                    A.check(what)
                    assert_maps(frames_view(d_out, F, H, S, W), exp, what)
                    untouched_padding(d_out, g, what)
    finally:
        plan.close()


# ---- served: scale, remap, inverse warp ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", GEOMETRIES, ids=GID)
def test_scale_at_unaligned_frames_and_destinations(hip_ctx, g):
    """scale_bilinear_kernel once down and once up; the destination pointer moves while its stride stays a multiple of 4: the dword-store arm needs pointer,
    stride and frame size aligned, so at +1 and +2 the launcher has to pick the byte arm by the pointer alone (test_gpu_scale.py varies only the stride)"""
    from compv_amd import capi
    W, H, S = g
    imgs = frames_of(g)
    plan = capi.Plan(hip_ctx, W, H, S, F, THETA)
    try:
        for wo, ho in ((W * 3 // 4, H * 2 // 3), (W + W // 3 + 1, H + 5)):
            So = (wo + 3) // 4 * 4 + 4
            exp = np.stack([pm.scale(v, wo, ho) for v in imgs])
            for oi, oo in PAIRS:
                what = "scale to %dx%d at +%d -> +%d" % (wo, ho, oi, oo)
                A = Bands()
                d_in = upload(A, imgs, S, oi, W + oi)
                d_out = A.new(F * ho * So, off=oo)
                plan.scale(ptr(d_in), ptr(d_out), wo, ho, So)
                A.check(what)
                body = d_out.cpu().numpy().reshape(F, ho, So)
                assert (body[:, :, :wo] == exp).all(), what
                assert (body[:, :, wo:] == SENTINEL).all(), what + ": columns >= Wout written"
    finally:
        plan.close()


@pytest.mark.parametrize("g", GEOMETRIES, ids=GID)
def test_remap_and_warp_at_unaligned_frames_and_destinations(hip_ctx, g):
    """remap_kernel<kRemapMap> and <kRemapWarp2> in the three interpolations, the destination offset at an aligned stride.  A float32 destination is REFUSED
    below 4 bytes: the pairs whose output offset is odd or 2 must be refused there, with nothing written"""
    from compv_amd import capi
    W, H, S = g
    imgs = frames_of(g)
    wo, ho, So = 37, 11, 40
    x, y = rc.random_map(W, H, wo, ho, 62000 + W)
    M = rc.matrices(W, H, wo, ho)["affine"]
    plan = capi.Plan(hip_ctx, W, H, S, F, THETA)
    try:
        for interp in (rm.NEAREST, rm.BILINEAR, rm.BILINEAR_FLOAT32):
            e = 4 if interp == rm.BILINEAR_FLOAT32 else 1
            dt = np.float32 if e == 4 else np.uint8
            exp_r = np.stack([rm.remap(v, x, y, interp, None, 9) for v in imgs])
            exp_w = np.stack([rm.warp_inverse(v, M, wo, ho, interp, 9) for v in imgs])
            for oi, oo in PAIRS:
                A = Bands()
                d_in = upload(A, imgs, S, oi, W + oi)
                d_x, d_y = (A.new(m.size * 4, np.ascontiguousarray(m, np.float32).view(np.uint8).reshape(-1)) for m in (x, y))
                d_out = A.new(F * ho * So * e, off=oo)
                calls = (("remap", exp_r, lambda: plan.remap(ptr(d_in), ptr(d_x), ptr(d_y), 1, interp, ptr(d_out), wo, ho, So, None, 9)),
                         ("warp", exp_w, lambda: plan.warp_inverse(ptr(d_in), M, interp, ptr(d_out), wo, ho, So, 9)))
                for name, exp, call in calls:
                    what = "%s interp %d at +%d -> +%d" % (name, interp, oi, oo)
                    A.refill(d_out)
                    if e == 4 and oo % 4:
                        with pytest.raises(capi.CompvHipError) as err:
                            call()
                        assert err.value.code == capi.E_INVALID_PARAMETER and "align" in hip_ctx.last_error(), what
                        A.check(what)
                        assert (d_out.cpu().numpy() == SENTINEL).all(), what + ": a refused call wrote"
                        continue
                    call()
                    A.check(what)
                    body = d_out.cpu().numpy().view(dt).reshape(F, ho, So)
                    assert np.ascontiguousarray(body[:, :, :wo]).tobytes() == np.ascontiguousarray(exp).tobytes(), what
                    assert (body[:, :, wo:].view(np.uint8) == SENTINEL).all(), what + ": elements >= Wout written"
    finally:
        plan.close()


# ---- served: the SHT, segments, fits, components and the KHT on the caller's bytes ------------------------------------------------------------
@pytest.mark.parametrize("g,offsets", [(GEOMETRIES[0], IN_OFFSETS[1:]), (GEOMETRIES[1], IN_OFFSETS[1:]), (BITS16, (1, 4, 8))], ids=[GID(GEOMETRIES[0]), GID(GEOMETRIES[1]), GID(BITS16)])
def test_sht_segments_fits_and_components_on_unaligned_edge_bytes(hip_ctx, oracle, g, offsets):
    """bytes_to_bits_kernel (the byte arm; the two 16-byte loads per lane at 64 x 33), then the vote on its masks; sht_segments and sht_fit kernels reading
    the caller's bytes pixel by pixel; bytes_to_bits again in front of the components.  Every typed array stays aligned"""
    from compv_amd import capi
    W, H, S = g
    e3 = edge_maps(oracle, g)
    thr = sht_threshold(W, H)
    sht = [sht_expect(oracle, m, THETA, thr) for m in e3]
    R, T, _ = oracle.sht_dims(W, H, THETA)
    sinQ, cosQ = oracle.sht_tables(THETA, T)
    comp = tgc.model(e3, 8, 1)
    cap = 64
    plan = capi.Plan(hip_ctx, W, H, S, F, THETA)
    try:
        for off in offsets:
            what = "edge bytes at +%d" % off
            A = Bands()
            d_e = upload_edges(A, e3, g, off)
            d_lines, d_counts = A.new(F * LINE_CAP * 20), A.new(F * 4)
            plan.houghsht(ptr(d_e), thr, 0, ptr(d_lines), LINE_CAP, ptr(d_counts))
            A.check("houghsht " + what)
            assert_lines(d_lines.cpu().numpy().reshape(F, LINE_CAP, 20), d_counts.cpu().numpy().view(np.int32), [x[1] for x in sht], "houghsht " + what)
            assert edge_counts(plan, F).tolist() == [int((m != 0).sum()) for m in e3], "edge counts " + what
            check_accs(plan, A, F, R, T, [x[0] for x in sht], "houghsht " + what)

            lines, _ = tgs.lines_of(d_lines, d_counts, F, LINE_CAP)
            d_segs, d_sc = A.new(F * cap * SEG_BYTES), A.new(F * 4)
            plan.houghsht_segments(ptr(d_e), ptr(d_lines), ptr(d_counts), LINE_CAP, MAX_LINES, 3, 1, ptr(d_segs), cap, ptr(d_sc))
            A.check("segments " + what)
            tgs.assert_segments(d_segs, d_sc, F, cap, tgs.model_frames(e3, sinQ, cosQ, lines, [(3, 1)], MAX_LINES)[(3, 1)], "segments " + what)

            d_fits, d_fc, d_ref = A.new(F * cap * FIT_BYTES), A.new(F * 4), A.new(F * LINE_CAP * 20)
            plan.houghsht_fit(ptr(d_e), ptr(d_lines), ptr(d_counts), LINE_CAP, MAX_LINES, 2, 0, 0, 0, ptr(d_fits), cap, ptr(d_fc), ptr(d_ref))
            A.check("fits " + what)
            fits, valid = tgf.model_fits(e3, sinQ, cosQ, R, lines, 2, MAX_LINES)
            tgf.assert_fits(d_fits, d_fc, F, cap, fits, "fits " + what)
            raw = d_ref.cpu().numpy().reshape(F, LINE_CAP * 20)
            for f in range(F):
                n = len(fits[f])
                tgf.assert_refined(np.frombuffer(raw[f][:n * 20].tobytes(), capi.LINE_DTYPE), lines[f][:n], fits[f], valid[f], "refined %s frame %d" % (what, f))
                assert (raw[f][n * 20:] == SENTINEL).all()
            segs = tgf.segs_of(d_segs, d_sc, F, cap)
            A.refill(d_fits); A.refill(d_fc)
            plan.houghsht_fit(ptr(d_e), ptr(d_lines), ptr(d_counts), LINE_CAP, MAX_LINES, 1, ptr(d_segs), ptr(d_sc), cap, ptr(d_fits), cap, ptr(d_fc))
            A.check("fits per segment " + what)
            tgf.assert_fits(d_fits, d_fc, F, cap, tgf.model_fits(e3, sinQ, cosQ, R, lines, 1, MAX_LINES, segs)[0], "fits per segment " + what)

            out = tgc.Out(A, F, H, W + 3, 4096)
            out.call(plan, ptr(d_e), 8, 1)
            A.check("components " + what)
            tgc.assert_result(out, W, comp, "components " + what)
        assert sum(len(x[1]) for x in sht) > 0 and sum(len(c[1]) for c in comp) > 0
    finally:
        plan.close()


@pytest.mark.parametrize("g", GEOMETRIES, ids=GID)
def test_batched_kht_on_unaligned_edge_bytes_in_both_orders(hip_ctx, oracle, g):
    """the batched KHT's own bytes_to_bits launch (api_kht.cpp) on d_edges + off: reference order against the oracle, canonical order against the model"""
    from compv_amd import capi
    from kht_canon_model import CanonModel
    W, H, S = g
    e3 = edge_maps(oracle, g)
    ref = [x["kht"] for x in expectations(oracle, g)]
    canon = [CanonModel(oracle).lines(e, 1.0, THETA, 12)[:2] for e in e3]
    plan = capi.Plan(hip_ctx, W, H, S, F, THETA)
    try:
        for off in IN_OFFSETS[1:]:
            A = Bands()
            d_e = upload_edges(A, e3, g, off)
            lines, gs = plan.houghkht(ptr(d_e), 1.0, THETA, 12)
            A.check("kht at +%d" % off)
            for f in range(F):
                el, egs = ref[f]
                assert [(float(l["rho"]), float(l["theta"]), int(l["strength"])) for l in lines[f]] == \
                    [(float(np.float32(l[0])), float(np.float32(l[1])), int(l[2])) for l in el], ("kht at +%d" % off, f)
                assert (gs[f] == egs) if len(el) else (gs[f] is None), ("kht gs at +%d" % off, f)
            lines, gs = plan.houghkht(ptr(d_e), 1.0, THETA, 12, order="canonical")
            A.check("canonical kht at +%d" % off)
            for f in range(F):
                assert line_bits(lines[f]) == model_line_bits(canon[f][0]), ("canonical kht at +%d" % off, f)
                assert gs[f] == canon[f][1], ("canonical kht gs at +%d" % off, f)
    finally:
        plan.close()


# ---- served: the pipeline -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", GEOMETRIES, ids=GID)
def test_pipeline_at_unaligned_frames_and_edge_maps(hip_ctx, oracle, g):
    """compvhip_plan_pipeline, one compvhip_plan_pipeline_async step with its wait, and compvhip_plan_pipeline_ex on packed RGB24 input (gray_kernel into a
    d_gray that is off alignment as well, OTSU thresholds, toCartesian)"""
    from compv_amd import capi
    W, H, S = g
    imgs = frames_of(g)
    exp = expectations(oracle, g)
    thr = sht_threshold(W, H)
    e3 = edge_maps(oracle, g)
    rgb = np.stack([rgb_of(i).reshape(H, W * 3) for i in imgs])
    plan = capi.Plan(hip_ctx, W, H, S, F, THETA)
    try:
        for oi, oo in PAIRS:
            A = Bands()
            d_in = upload(A, imgs, S, oi, W + oi)
            d_rgb = upload(A, rgb, S * 3, oi, W + 3 + oi)
            d_out, d_gray = A.new(F * H * S, off=oo), A.new(F * H * S, off=oi)
            d_lines, d_counts, d_otsu, d_cart = A.new(F * LINE_CAP * 20), A.new(F * 4), A.new(F * 4), A.new(F * LINE_CAP * 16)
            for how in ("sync", "async", "rgb24"):
                what = "pipeline %s at +%d -> +%d" % (how, oi, oo)
                for b in (d_out, d_lines, d_counts):
                    A.refill(b)
                if how == "sync":
                    plan.pipeline(ptr(d_in), T_LOW, T_HIGH, thr, 0, ptr(d_out), ptr(d_lines), LINE_CAP, ptr(d_counts))
                elif how == "async":
                    plan.wait(plan.pipeline_async(ptr(d_in), T_LOW, T_HIGH, thr, 0, ptr(d_out), ptr(d_lines), LINE_CAP, ptr(d_counts)))
                else:
                    plan.pipeline_ex(ptr(d_rgb), 0.5, 1.0, thr, 0, ptr(d_out), ptr(d_lines), LINE_CAP, ptr(d_counts), threshold_type=capi.THRESHOLD_OTSU,
                                     pixfmt=capi.FMT_RGB24, d_gray=ptr(d_gray), d_otsu=ptr(d_otsu), d_cart=ptr(d_cart))
                A.check(what)
                raw, counts = d_lines.cpu().numpy().reshape(F, LINE_CAP, 20), d_counts.cpu().numpy().view(np.int32)
                if how != "rgb24":
                    assert_maps(frames_view(d_out, F, H, S, W), e3, what)
                    assert_lines(raw, counts, [x["sht"][1] for x in exp], what)
                    assert edge_counts(plan, F).tolist() == [int((m != 0).sum()) for m in e3], what
                    continue
                assert_maps(frames_view(d_gray, F, H, S, W), [x["rgb"][0] for x in exp], what + " gray")
                assert d_otsu.cpu().numpy().view(np.int32).tolist() == [x["rgb"][1] for x in exp], what
                assert_maps(frames_view(d_out, F, H, S, W), [x["rgb"][2] for x in exp], what + " edges")
                assert_lines(raw, counts, [x["rgb"][3] for x in exp], what)
                cart = d_cart.cpu().numpy().view(np.float32).reshape(F, LINE_CAP, 4)
                for f in range(F):
                    k = min(int(counts[f]), LINE_CAP)
                    ce = oracle.sht_to_cartesian(W, H, [(float(l["rho"]), float(l["theta"])) for l in lines_of(raw[f], k)])
                    assert (cart[f][:k].view(np.uint32) == ce.view(np.uint32)).all(), (what, "cartesian", f)
    finally:
        plan.close()


# ---- refused ------------------------------------------------------------------------------------------------------------------------------------------
RW, RH, RS = GEOMETRIES[0]
CAP = 8


class Handles:
    """the handle an export is called on, created on demand: a plan, a pyramid, a matcher or a homography that has run nothing"""

    def __init__(self, ctx):
        self.ctx, self.made = ctx, {}

    def get(self, kind):
        from compv_amd import capi
        if kind not in self.made:
            self.made[kind] = {"plan": lambda: capi.Plan(self.ctx, RW, RH, RS, F, THETA), "pyr": lambda: capi.OrbPyramid(self.ctx, RW, RH, RS, F, corner_cap=CAP),
                               "matcher": lambda: capi.Matcher(self.ctx, 32, CAP, CAP, pairs=F, knn=2), "hom": lambda: capi.Homography(self.ctx, F, CAP, 16)}[kind]()
        return self.made[kind]

    def close(self):
        for h in self.made.values():
            h.close()


def refused_call(export, H, p):
    """the export with the pointers p[name] (everything else valid): a function that makes the call through the capi wrapper"""
    from compv_amd import capi
    plan, pyr, mt, hom = (lambda: H.get("plan")), (lambda: H.get("pyr")), (lambda: H.get("matcher")), (lambda: H.get("hom"))
    thr = sht_threshold(RW, RH)
    per_segment = p.get("_per_segment", False)
    table = {
        "compvhip_plan_otsu": lambda: plan().otsu(p["d_gray"], p["d_thresholds"]),
        "compvhip_plan_to_cartesian": lambda: plan().to_cartesian(p["d_lines"], p["d_counts"], CAP, p["d_cart"]),
        "compvhip_plan_houghsht": lambda: plan().houghsht(p["d_edges"], thr, 0, p["d_lines"], CAP, p["d_counts"]),
        "compvhip_plan_pipeline": lambda: plan().pipeline(p["d_in"], T_LOW, T_HIGH, thr, 0, p["d_edges"], p["d_lines"], CAP, p["d_counts"]),
        "compvhip_plan_pipeline_async": lambda: plan().pipeline_async(p["d_in"], T_LOW, T_HIGH, thr, 0, p["d_edges"], p["d_lines"], CAP, p["d_counts"]),
        "compvhip_plan_pipeline_ex": lambda: plan().pipeline_ex(p["d_in"], T_LOW, T_HIGH, thr, 0, p["d_edges"], p["d_lines"], CAP, p["d_counts"]),
        "compvhip_plan_acc_export": lambda: plan().acc_export(0, p["d_out"], 180),
        "compvhip_plan_houghsht_segments": lambda: plan().houghsht_segments(p["d_edges"], p["d_lines"], p["d_counts"], CAP, 0, 3, 1, p["d_segs"], CAP, p["d_segCounts"]),
        "compvhip_plan_houghsht_fit": lambda: plan().houghsht_fit(p["d_edges"], p["d_lines"], p["d_counts"], CAP, 0, 2, p["d_segs"] if per_segment else 0,
                                                                  p["d_segCounts"] if per_segment else 0, CAP, p["d_fits"], CAP, p["d_fitCounts"],
                                                                  0 if per_segment else p["d_refined"]),
        "compvhip_plan_components": lambda: plan().components(p["d_edges"], 8, 1, p["d_labels"], RW, p["d_comps"], CAP, p["d_compCounts"]),
        "compvhip_plan_threshold": lambda: plan().threshold(p["d_in"], 0.0, p["d_out"], p["d_levels"]),
        "compvhip_plan_fast": lambda: plan().fast(p["d_gray"], 20, 9, True, -1, p["d_scores"], p["d_corners"], CAP, p["d_counts"]),
        "compvhip_plan_orb_keypoints": lambda: plan().orb_keypoints(p["d_gray"], p["d_corners"], CAP, p["d_cornerCounts"], 0, 1.0, p["d_keypoints"], CAP, p["d_keyCounts"],
                                                                    p["d_moments"]),
        "compvhip_plan_orb_describe": lambda: plan().orb_describe(p["d_gray"], p["d_keypoints"], CAP, p["d_keyCounts"], 1.0, p["d_desc"], 32),
        "compvhip_plan_remap": lambda: plan().remap(p["d_in"], p["d_mapX"], p["d_mapY"], 1, rm.BILINEAR_FLOAT32, p["d_out"], 8, 8, 8),
        "compvhip_plan_warp_inverse": lambda: plan().warp_inverse(p["d_in"], np.eye(3, dtype=np.float32)[:2], rm.BILINEAR_FLOAT32, p["d_out"], 8, 8, 8),
        "compvhip_plan_hog": lambda: plan().hog(p["d_gray"], p["d_desc"], 1024, p["d_cells"]),
        "compvhip_plan_integral": lambda: plan().integral(p["d_gray"], p["d_sum"], p["d_sumsq"], RW + 1),
        "compvhip_plan_histogram": lambda: plan().histogram(p["d_gray"], p["d_hist"]),
        "compvhip_plan_equalize": lambda: plan().equalize(p["d_gray"], p["d_out"], p["d_hist"], 0.0, p["d_lut"]),
        "compvhip_plan_projections": lambda: plan().projections(p["d_gray"], p["d_projX"], p["d_projY"]),
        "compvhip_orbpyr_detect": lambda: pyr().detect(p["d_gray"], p["d_keypoints"], CAP, p["d_keyCounts"], p["d_levelCounts"], p["d_levelCorners"]),
        "compvhip_orbpyr_describe": lambda: pyr().describe(p["d_gray"], p["d_keypoints"], CAP, p["d_keyCounts"], p["d_desc"], 32),
        "compvhip_matcher_knn": lambda: mt().knn(p["d_query"], 32, p["d_queryCounts"], p["d_train"], 32, p["d_trainCounts"], False, p["d_matches"]),
        "compvhip_matcher_good": lambda: mt().good(p["d_matches"], p["d_query"], 32, p["d_queryCounts"], p["d_train"], 32, p["d_trainCounts"], False, p["d_good"], CAP,
                                                   p["d_goodCounts"], ratio=0.8),
        "compvhip_homography_points": lambda: hom().points(p["d_good"], CAP, p["d_goodCounts"], p["d_query"], CAP, p["d_train"], CAP),
        "compvhip_homography_find": lambda: hom().find(p["d_src"], p["d_dst"], p["d_counts"], p["d_results"], p["d_mask"], tries=8, d_quads=p["d_quads"]),
        "compvhip_homography_project": lambda: hom().project(p["d_results"], p["d_points"], 4, False, p["d_out"]),
    }
    return table[export]


REFUSED_EXPORTS = sorted({r.export for r in ac.refused_rows()})


def test_every_refused_row_has_a_call_here():
    assert all(r.test == ac.HERE for r in ac.refused_rows())
    for export in REFUSED_EXPORTS:
        refused_call(export, None, {})          # KeyError: an export of the table without a call below


@pytest.mark.parametrize("export", REFUSED_EXPORTS)
def test_refused_pointer(hip_ctx, export):
    """every REFUSED row of the export: that pointer alone moved off its alignment -> E_INVALID_PARAMETER that speaks of alignment, every buffer (all of them
    hold nothing but the sentinel) untouched, no allocation on a handle that has run nothing.  The call with nothing moved is NOT made: the buffers hold no
    content, and the served tests make it"""
    from compv_amd import capi
    rows = [r for r in ac.ROWS if r.export == export]
    A = Bands()
    base = {r.param: ptr(A.new(1 << 16)) for r in rows}
    H = Handles(hip_ctx)
    try:
        call0 = refused_call(export, H, dict(base))
        kind = "pyr" if "orbpyr" in export else "matcher" if "matcher" in export else "hom" if "homography" in export else "plan"
        H.get(kind)
        live = hip_ctx.live_allocations()
        tried = 0
        for r in (x for x in ac.refused_rows() if x.export == export):
            for move in ac.moves(r.n):
                p = dict(base)
                p[r.param] += move
                p["_per_segment"] = r.param in ("d_segs", "d_segCounts") and export.endswith("_fit")
                what = "%s(%s + %d)" % (export, r.param, move)
                with pytest.raises(capi.CompvHipError) as err:
                    refused_call(export, H, p)()
                assert err.value.code == capi.E_INVALID_PARAMETER, what
                assert "align" in hip_ctx.last_error(), (what, hip_ctx.last_error())
                assert A.all_sentinel(), what + ": a refused call wrote"
                assert hip_ctx.live_allocations() == live, what + ": a refused call allocated"
                tried += 1
        assert tried >= len([x for x in rows if x.cls == ac.REFUSED]) and call0 is not None
    finally:
        H.close()


# ---- host forms ---------------------------------------------------------------------------------------------------------------------------------------
def test_host_forms_take_any_host_pointer(hip_ctx):
    """compvhip_canny_u8, compvhip_morph_u8 and compvhip_histogram_u8 copy into buffers of their own: a numpy view that starts one byte into its buffer
    gives what an aligned copy gives"""
    W, H = 43, 49
    img = frames_of(GEOMETRIES[0])[1]
    raw = np.zeros(W * H + 65, np.uint8)
    base = (-raw.ctypes.data) % 64          # a 64-byte aligned start inside raw ...
    odd = raw[base + 1:base + 1 + W * H].reshape(H, W)          # ... and the view one byte behind it
    odd[:] = img
    even = np.ascontiguousarray(img)
    assert odd.ctypes.data % 2 == 1 and odd.flags["C_CONTIGUOUS"]
    se = mm.strel(mm.CROSS, 5, 5)
    assert (hip_ctx.canny(odd, T_LOW, T_HIGH) == hip_ctx.canny(even, T_LOW, T_HIGH)).all()
    assert (hip_ctx.morph(odd, se, mm.CLOSE) == hip_ctx.morph(even, se, mm.CLOSE)).all()
    assert (hip_ctx.histogram(odd) == hip_ctx.histogram(even)).all()
    assert (hip_ctx.morph(even, se, mm.CLOSE) == mm.morph(img, se, mm.CLOSE, mm.BORDER_REPLICATE)).all() and (hip_ctx.histogram(even) == np.bincount(img.reshape(-1), minlength=256)).all()
