"""GPU thresholding and morphology (compvhip_plan_threshold / _threshold_adaptive / _morph and their host forms) against tests/morph_model.py,
byte for byte, every frame of every case.

Harness of tests/gpu_support.py: every device buffer sits between two guards; outputs start filled with a sentinel, their padding
columns [W, S) included, and must still hold it there afterwards (the kernels never write columns >= W); the input's padding columns hold
seeded random bytes.  Inputs of out-of-place calls must come back unchanged.

Geometries (W, H, S, F) and what they reach.  The morphology kernels work on 256 x 32 tiles (one dword column of 8 rows per thread), the
adaptive threshold on 128 x 32 tiles (16-column / 16-row segments per thread), the global threshold on 8-pixel groups:
  (9, 9, 16, 3)         the smallest frame; one ragged dword (W % 4 == 1); every 5- and 7-tall strel makes most rows border rows
  (17, 9, 24, 2)        W % 8 == 1: the threshold's byte-wise tail store; S % 16 == 8
  (13, 70, 24, 2)       three row tiles, the last 6 rows tall
  (239, 24, 240, 5)     W % 4 == 3, one tile wide, S - W = 1: the tile's last dword is ragged
  (241, 25, 248, 3)     the adaptive kernel's second column tile is ragged
  (257, 33, 264, 2)     one column past the morphology tile width, one row past the tile height (both kernels): 1-wide / 1-tall tiles whose
                        whole content is halo of the neighbour
  (513, 65, 576, 9)     three column tiles, the last one column wide; three row tiles; 9 frames
  (1001, 333, 1008, 33) F = 33 frames (blockIdx.z), 11 row tiles
  (100, 1537, 104, 3)   tall: 49 row tiles
  (129, 40, 136, 2)     one column past the adaptive tile width (128)
"""
import numpy as np
import pytest

import morph_model as mm
from components_model import COMP_DTYPE, components
from gpu_support import SENTINEL, Arena, pad_frames, ptr
from morph_rig import STRELS, strokes
from plan_geometries import GEOMETRIES

pytestmark = pytest.mark.gpu

WANTED = [(9, 9, 16, 3), (17, 9, 24, 2), (13, 70, 24, 2), (239, 24, 240, 5), (241, 25, 248, 3), (513, 65, 576, 9), (1001, 333, 1008, 33), (100, 1537, 104, 3)]
SWEEP = [g[:4] for g in GEOMETRIES if g[:4] in WANTED] + [(257, 33, 264, 2), (129, 40, 136, 2)]
assert len(SWEEP) == len(WANTED) + 2
OPS = (mm.ERODE, mm.DILATE, mm.OPEN, mm.CLOSE)
BORDERS = (mm.BORDER_REPLICATE, mm.BORDER_ZERO)


# ---- frame content ---------------------------------------------------------------------------------------------------------------------
def seam(W, H, seed):
    """mid-gray everywhere; the extremes 0 and 255 sit only in the columns and rows either side of the 256 x 32 (and 128 x 32) tile seams, which
    are halo cells of the neighbouring tile"""
    rng = np.random.default_rng(seed)
    img = np.full((H, W), 128, np.uint8)
    for x0 in range(128, W + 1, 128):
        for x in range(max(0, x0 - 2), min(W, x0 + 2)):
            img[:, x] = np.where(rng.random(H) < 0.5, 0, 255)
    for y0 in range(32, H + 1, 32):
        for y in range(max(0, y0 - 2), min(H, y0 + 2)):
            img[y, :] = np.where(rng.random(W) < 0.5, 0, 255)
    return img


def batch(W, H, F, seed):
    """frames cycle through: random bytes, strokes, a constant frame, tile-seam extremes"""
    out = []
    for f in range(F):
        k = (seed + f) % 4
        if k == 0:
            out.append(np.random.default_rng(seed * 100 + f).integers(0, 256, (H, W), dtype=np.uint8))
        elif k == 1:
            out.append(strokes(W, H, seed * 100 + f))
        elif k == 2:
            out.append(np.full((H, W), (37 * (seed + f)) & 0xff, np.uint8))
        else:
            out.append(seam(W, H, seed * 100 + f))
    return np.stack(out)


class Rig:
    """A plan, a guarded input batch and a guarded output of one geometry."""

    def __init__(self, hip_ctx, W, H, S, F, seed):
        from compv_amd import capi
        self.W, self.H, self.S, self.F = W, H, S, F
        self.ar = Arena()
        self.valid = batch(W, H, F, seed)
        self.host_in = pad_frames(self.valid, S, np.random.default_rng(seed + 1))
        self.d_in = self.ar.new(F * H * S, self.host_in)
        self.ar.keep(self.d_in, self.host_in)
        self.d_out = self.ar.new(F * H * S)
        self.plan = capi.Plan(hip_ctx, W, H, S, F)

    def check(self, what, expect, d_out=None):
        """expect(f) -> (H, W) model output of frame f"""
        self.ar.check(what)
        got = (self.d_out if d_out is None else d_out).cpu().numpy().reshape(self.F, self.H, self.S)
        assert (got[:, :, self.W:] == SENTINEL).all(), "%s: padding columns written" % what
        for f in range(self.F):
            assert got[f, :, :self.W].tobytes() == expect(f).tobytes(), "%s: frame %d" % (what, f)
        self.ar.refill(self.d_out)

    def close(self):
        self.plan.close()


# ---- morphology ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", SWEEP, ids=lambda g: "%dx%d_S%d_F%d" % g)
def test_morph_geometry_sweep(hip_ctx, geom):
    """every strel x op x border on every geometry it fits; full rectangles and crosses through the separable AND the general kernel by name,
    and through the one compvhip_plan_morph picks (the general one up to 15 members)"""
    from compv_amd import capi
    W, H, S, F = geom
    rig = Rig(hip_ctx, W, H, S, F, seed=W + H)
    big = W * H * F > 2_000_000      # the two large batches: one border and two ops per strel (the small ones cover the full product)
    try:
        for name, se in STRELS.items():
            sh, sw = se.shape
            if W < sw or H < sh:
                continue
            separable = name.startswith(("rect", "cross"))
            for border in (BORDERS[:1] if big else BORDERS):
                for op in ((mm.ERODE, mm.CLOSE) if big else OPS):
                    exp = [mm.morph(rig.valid[f], se, op, border) for f in range(F)]
                    for kernel in ((capi.MORPH_KERNEL_AUTO, capi.MORPH_KERNEL_SEPARABLE, capi.MORPH_KERNEL_GENERAL) if separable else (capi.MORPH_KERNEL_AUTO,)):
                        rig.plan.morph(ptr(rig.d_in), se, op, border, ptr(rig.d_out), kernel=kernel)
                        rig.check("%s op %d border %d kernel %d" % (name, op, border, kernel), lambda f: exp[f])
    finally:
        rig.close()


@pytest.mark.parametrize("W,H,S", [(31, 31, 32), (40, 37, 40)])
def test_morph_rect31(hip_ctx, W, H, S):
    """31 x 31 rectangle: on a 31 x 31 frame every cell is a border cell; on 40 x 37 the interior is 10 x 5 (hb = 16 leaves rows 16..20)"""
    from compv_amd import capi
    se = mm.strel(mm.RECT, 31, 31)
    rig = Rig(hip_ctx, W, H, S, 2, seed=31)
    try:
        for border in BORDERS:
            for op in OPS:
                exp = [mm.morph(rig.valid[f], se, op, border) for f in range(2)]
                for kernel in (capi.MORPH_KERNEL_SEPARABLE, capi.MORPH_KERNEL_GENERAL):
                    rig.plan.morph(ptr(rig.d_in), se, op, border, ptr(rig.d_out), kernel=kernel)
                    rig.check("rect31 op %d border %d kernel %d" % (op, border, kernel), lambda f: exp[f])
    finally:
        rig.close()


# ---- thresholds --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", SWEEP, ids=lambda g: "%dx%d_S%d_F%d" % g)
def test_threshold_geometry_sweep(hip_ctx, geom):
    """the fixture's parameter grid: fixed levels, per-frame Otsu levels computed on the same stream, in place"""
    import torch
    W, H, S, F = geom
    rig = Rig(hip_ctx, W, H, S, F, seed=2 * W + H)
    try:
        for thr in (0.0, 0.4, 127.5, 255.0):
            rig.plan.threshold(ptr(rig.d_in), thr, ptr(rig.d_out))
            rig.check("threshold %g" % thr, lambda f: mm.threshold(rig.valid[f], thr))
        # Otsu levels, never seen by the host before the threshold runs
        d_lv = rig.ar.new(4 * F)
        rig.plan.otsu(ptr(rig.d_in), ptr(d_lv))
        rig.plan.threshold(ptr(rig.d_in), 999.0, ptr(rig.d_out), d_levels=ptr(d_lv))
        torch.cuda.synchronize()
        lv = np.frombuffer(d_lv.cpu().numpy().tobytes(), np.int32)
        rig.check("threshold at the Otsu levels", lambda f: mm.threshold(rig.valid[f], float(lv[f])))
        # levels outside 0..255 are clipped
        wild = np.array([(-5, 300, 128)[f % 3] for f in range(F)], np.int32)
        d_lv.copy_(torch.from_numpy(wild.view(np.uint8)))
        rig.plan.threshold(ptr(rig.d_in), 0.0, ptr(rig.d_out), d_levels=ptr(d_lv))
        rig.check("clipped levels", lambda f: mm.threshold(rig.valid[f], float(min(max(int(wild[f]), 0), 255))))
        # in place: the padding columns keep the input's bytes
        d_io = rig.ar.new(F * H * S, rig.host_in)
        rig.plan.threshold(ptr(d_io), 100.0, ptr(d_io))
        rig.ar.check("threshold in place")
        got = d_io.cpu().numpy().reshape(F, H, S)
        assert (got[:, :, W:] == rig.host_in[:, :, W:]).all()
        for f in range(F):
            assert got[f, :, :W].tobytes() == mm.threshold(rig.valid[f], 100.0).tobytes(), f
    finally:
        rig.close()


ADAPTIVE_GRID = [(bs, d, mv, inv) for bs in (3, 15, 31) for d in (0.0, 5.0, 255.0) for mv in (255.0, 100.0) for inv in (0, 1)]


@pytest.mark.parametrize("geom", SWEEP, ids=lambda g: "%dx%d_S%d_F%d" % g)
def test_adaptive_geometry_sweep(hip_ctx, geom):
    from compv_amd import capi
    W, H, S, F = geom
    rig = Rig(hip_ctx, W, H, S, F, seed=3 * W + H)
    big = W * H * F > 2_000_000
    try:
        means = {}
        for (bs, d, mv, inv) in ADAPTIVE_GRID:
            if big and (mv != 255.0 or inv):
                continue
            if min(W, H) < bs:
                with pytest.raises(capi.CompvHipError) as e:
                    rig.plan.threshold_adaptive(ptr(rig.d_in), bs, d, mv, inv, ptr(rig.d_out))
                assert e.value.code == capi.E_INVALID_PARAMETER
                continue
            if bs not in means:      # the model's mean once per block size; the decision is re-derived per parameter set
                means[bs] = [mm.box_mean(rig.valid[f], bs).astype(np.int32) for f in range(F)]

            def expect(f):
                hit = (rig.valid[f].astype(np.int32) - means[bs][f] + 255) >= (256 - mm.round_u8(d))
                return np.where(hit != bool(inv), mm.round_u8(mv), 0).astype(np.uint8)
            rig.plan.threshold_adaptive(ptr(rig.d_in), bs, d, mv, inv, ptr(rig.d_out))
            rig.check("adaptive %s" % ((bs, d, mv, inv),), expect)
        # in place, through the plan's plane
        bs = 3 if min(W, H) < 15 else 15
        d_io = rig.ar.new(F * H * S, rig.host_in)
        rig.plan.threshold_adaptive(ptr(d_io), bs, 5.0, 255.0, 0, ptr(d_io))
        rig.ar.check("adaptive in place")
        got = d_io.cpu().numpy().reshape(F, H, S)
        assert (got[:, :, W:] == rig.host_in[:, :, W:]).all()
        for f in range(F):
            assert got[f, :, :W].tobytes() == mm.adaptive(rig.valid[f], bs, 5.0).tobytes(), f
    finally:
        rig.close()


def test_adaptive_matches_model_function(hip_ctx):
    """the sweep re-derives the decision from box_mean; this pins it to morph_model.adaptive itself, and runs blockSize 31 on a 31 x 31 frame
    (one interior cell)"""
    rig = Rig(hip_ctx, 31, 31, 32, 3, seed=5)
    try:
        for (bs, d, mv, inv) in ((31, 5.0, 255.0, 0), (31, 0.0, 100.0, 1), (15, 5.0, 255.0, 0), (3, 255.0, 255.0, 1)):
            rig.plan.threshold_adaptive(ptr(rig.d_in), bs, d, mv, inv, ptr(rig.d_out))
            rig.check("adaptive %s" % ((bs, d, mv, inv),), lambda f: mm.adaptive(rig.valid[f], bs, d, mv, inv))
    finally:
        rig.close()


# ---- the text chain ------------------------------------------------------------------------------------------------------------------------
def words_frame(W, H, seed):
    """drawn 'words': rectangles filled with vertical strokes 2 px wide and 2 px apart, dark ink (30) on light paper (200)"""
    rng = np.random.default_rng(seed)
    img = np.full((H, W), 200, np.uint8)
    for _ in range(12):
        x0, y0 = int(rng.integers(2, W - 30)), int(rng.integers(2, H - 12))
        w, h = int(rng.integers(10, 28)), int(rng.integers(5, 10))
        for x in range(x0, x0 + w, 4):
            img[y0:y0 + h, x:x + 2] = 30
    return img


def test_text_chain(hip_ctx):
    """otsu -> threshold at the device levels -> close(rect 5x3) -> components(8): the records equal components_model on the model's closed map.
    Ink is dark: the binarised paper is foreground, so the frame is inverted first (255 - gray) to make the strokes the blobs."""
    import torch
    from compv_amd import capi
    W, H, S, F = 166, 89, 176, 3
    valid = np.stack([255 - words_frame(W, H, 70 + f) for f in range(F)])
    ar = Arena()
    host_in = pad_frames(valid, S, np.random.default_rng(9))
    d_in = ar.new(F * H * S, host_in)
    ar.keep(d_in, host_in)
    d_bin, d_closed, d_lv = ar.new(F * H * S), ar.new(F * H * S), ar.new(4 * F)
    cap = 256
    d_comps, d_counts = ar.new(F * cap * COMP_DTYPE.itemsize), ar.new(4 * F)
    plan = capi.Plan(hip_ctx, W, H, S, F)
    se = mm.strel(mm.RECT, 5, 3)
    try:
        plan.otsu(ptr(d_in), ptr(d_lv))
        plan.threshold(ptr(d_in), 0.0, ptr(d_bin), d_levels=ptr(d_lv))
        plan.morph(ptr(d_bin), se, mm.CLOSE, mm.BORDER_REPLICATE, ptr(d_closed))
        plan.components(ptr(d_closed), 8, 1, 0, 0, ptr(d_comps), cap, ptr(d_counts))
        ar.check("text chain")
        lv = np.frombuffer(d_lv.cpu().numpy().tobytes(), np.int32)
        counts = np.frombuffer(d_counts.cpu().numpy().tobytes(), np.int32)
        raw = d_comps.cpu().numpy().reshape(F, cap * COMP_DTYPE.itemsize)
        closed = d_closed.cpu().numpy().reshape(F, H, S)
        for f in range(F):
            exp_closed = mm.morph(mm.threshold(valid[f], float(lv[f])), se, mm.CLOSE, mm.BORDER_REPLICATE)
            assert closed[f, :, :W].tobytes() == exp_closed.tobytes(), f
            _, rec = components(exp_closed, 8, 1)
            assert 2 <= len(rec) <= 12 and counts[f] == len(rec), (f, counts[f], len(rec))     # the 2-px gaps are closed: words, not strokes
            assert np.frombuffer(raw[f][:len(rec) * COMP_DTYPE.itemsize].tobytes(), COMP_DTYPE).tobytes() == rec.tobytes(), f
    finally:
        plan.close()


# ---- contract ------------------------------------------------------------------------------------------------------------------------------
def test_host_entry_points_equal_plan_and_model(hip_ctx):
    rng = np.random.default_rng(11)
    img = rng.integers(0, 256, (45, 77), dtype=np.uint8)
    padded = np.ascontiguousarray(rng.integers(0, 256, (45, 96), dtype=np.uint8))
    padded[:, :77] = img
    view = padded[:, :77]                                   # a host image with a row stride
    assert hip_ctx.threshold(view, 127.5).tobytes() == mm.threshold(img, 127.5).tobytes()
    assert hip_ctx.threshold_adaptive(view, 15, 5.0, 100.0, True).tobytes() == mm.adaptive(img, 15, 5.0, 100.0, True).tobytes()
    for name in ("rect15x3", "cross5x5", "diamond7x7", "single"):
        for op in OPS:
            assert hip_ctx.morph(view, STRELS[name], op, mm.BORDER_ZERO).tobytes() == mm.morph(img, STRELS[name], op, mm.BORDER_ZERO).tobytes(), (name, op)


def test_refusals(hip_ctx):
    from compv_amd import capi
    img = np.zeros((40, 40), np.uint8)

    def code(fn, *a, **k):
        with pytest.raises(capi.CompvHipError) as e:
            fn(*a, **k)
        return e.value.code
    assert code(hip_ctx.threshold, img, -1.0) == capi.E_INVALID_PARAMETER
    assert code(hip_ctx.threshold_adaptive, img, 4, 5.0) == capi.E_INVALID_PARAMETER
    assert code(hip_ctx.threshold_adaptive, img, 1, 5.0) == capi.E_INVALID_PARAMETER
    assert code(hip_ctx.threshold_adaptive, img, 33, 5.0) == capi.E_NOT_IMPLEMENTED
    assert code(hip_ctx.threshold_adaptive, img[:20], 31, 5.0) == capi.E_INVALID_PARAMETER
    assert code(hip_ctx.threshold_adaptive, img, 3, 5.0, -1.0) == capi.E_INVALID_PARAMETER
    assert code(hip_ctx.morph, img, np.ones((3, 4), np.uint8), mm.ERODE) == capi.E_NOT_IMPLEMENTED
    assert code(hip_ctx.morph, img, np.ones((33, 3), np.uint8), mm.ERODE) == capi.E_NOT_IMPLEMENTED
    assert code(hip_ctx.morph, img, np.zeros((3, 3), np.uint8), mm.ERODE) == capi.E_INVALID_PARAMETER
    assert code(hip_ctx.morph, img[:9], np.ones((11, 3), np.uint8), mm.ERODE) == capi.E_INVALID_PARAMETER
    assert code(hip_ctx.morph, img, np.ones((3, 3), np.uint8), 4) == capi.E_NOT_IMPLEMENTED          # the gradient is compiled out of the reference
    assert code(hip_ctx.morph, img, np.ones((3, 3), np.uint8), mm.ERODE, 1) == capi.E_NOT_IMPLEMENTED
    # aliasing: host and plan
    L = hip_ctx.lib
    se = np.ones((3, 3), np.uint8)
    assert L.compvhip_morph_u8(hip_ctx.h, img.ctypes.data, 40, 40, 40, se.ctypes.data, 3, 3, 0, 2, img.ctypes.data, 40) == capi.E_INVALID_PARAMETER
    ar = Arena()
    d = ar.new(2 * 40 * 40)
    plan = capi.Plan(hip_ctx, 40, 40, 40, 1)
    try:
        assert code(plan.morph, ptr(d), se, mm.ERODE, mm.BORDER_ZERO, ptr(d)) == capi.E_INVALID_PARAMETER
        assert code(plan.morph, ptr(d), se, mm.ERODE, mm.BORDER_ZERO, ptr(d) + 40 * 39) == capi.E_INVALID_PARAMETER      # overlapping by one row
        assert code(plan.threshold_adaptive, ptr(d), 3, 5.0, 255.0, 0, ptr(d) + 8) == capi.E_INVALID_PARAMETER
        assert code(plan.morph, ptr(d), STRELS["diamond7x7"], mm.ERODE, mm.BORDER_ZERO, ptr(d) + 1600, kernel=capi.MORPH_KERNEL_SEPARABLE) == capi.E_INVALID_PARAMETER
        assert code(plan.threshold, ptr(d), -0.5, ptr(d)) == capi.E_INVALID_PARAMETER
        ar.check("refusals")
    finally:
        plan.close()


def test_plan_scratch_streams_and_allocations(hip_ctx):
    """a second call with another strel size on the same plan, a call on a non-default stream, and the allocation balance: the plan's plane is
    allocated on first use (one allocation, counted) and released with the plan"""
    import torch
    from compv_amd import capi
    torch.cuda.synchronize()
    start = hip_ctx.live_allocations()
    rig = Rig(hip_ctx, 70, 50, 72, 2, seed=4)
    try:
        base = hip_ctx.live_allocations()
        rig.plan.morph(ptr(rig.d_in), STRELS["rect3x3"], mm.ERODE, mm.BORDER_REPLICATE, ptr(rig.d_out))
        assert hip_ctx.live_allocations() == base                     # a basic operation needs no scratch
        rig.check("erode", lambda f: mm.morph(rig.valid[f], STRELS["rect3x3"], mm.ERODE))
        rig.plan.morph(ptr(rig.d_in), STRELS["rect3x3"], mm.CLOSE, mm.BORDER_REPLICATE, ptr(rig.d_out))
        assert hip_ctx.live_allocations() == base + 1
        rig.check("close 3x3", lambda f: mm.morph(rig.valid[f], STRELS["rect3x3"], mm.CLOSE))
        rig.plan.morph(ptr(rig.d_in), STRELS["rect3x15"], mm.OPEN, mm.BORDER_ZERO, ptr(rig.d_out))
        assert hip_ctx.live_allocations() == base + 1
        rig.check("open 3x15", lambda f: mm.morph(rig.valid[f], STRELS["rect3x15"], mm.OPEN, mm.BORDER_ZERO))
        st = torch.cuda.Stream()
        st.wait_stream(torch.cuda.current_stream())
        rig.plan.morph(ptr(rig.d_in), STRELS["diamond7x7"], mm.CLOSE, mm.BORDER_REPLICATE, ptr(rig.d_out), stream=st.cuda_stream)
        rig.plan.threshold(ptr(rig.d_out), 90.0, ptr(rig.d_out), stream=st.cuda_stream)
        st.synchronize()
        rig.check("close + threshold on a stream", lambda f: mm.threshold(mm.morph(rig.valid[f], STRELS["diamond7x7"], mm.CLOSE), 90.0))
    finally:
        rig.close()
    assert hip_ctx.live_allocations() == start
