"""Batches beyond 65 535 frames (compv_amd/csrc/frame_slices.hpp: the frame index rides in blockIdx.y / .z, limited to 65 535 per launch).

Every plan-form call is in one of three classes (include/compv_hip.h, "Batches beyond 65 535 frames"; docs/dispatch_coverage.md has the table):

  sliced             the launcher goes through for_frame_slices: the tests here run 65 541 frames (one full slice and a last one of 6), the threshold
                     131 073 as well (the slice start advances twice), the shared-map remap 524 285 (it packs 8 frames into a group: 8 * 65 535 + 5), and
                     check EVERY frame, so what a kernel does with a non-zero frame0 / group0 / offset base pointer is executed and compared;
  frames only in x   compvhip_plan_edge_dete: one positive case against the oracle;
  refused            E_INVALID_PARAMETER with the limit in the message, before anything is allocated or enqueued.

A batch cycles through 7 distinct small frames; per-frame parameters (levels, matrices) through 11, line lists and their counts through 4.  None of the
periods divides 65 535 = 3 * 5 * 17 * 257 (test_no_period_divides_a_slice), so a slice that started at the wrong frame -- at frame 0 again, say -- would
read or write another pattern than the model expects: Cycle.check asserts, for every expectation that has teeth, that the slots at the start of every
later slice differ from slot 0.  The models run once per distinct (content, parameter) combination; the expectation of the whole batch is that table
indexed by frame, built and compared on the device, byte for byte, unwritten bytes (padding columns, record slots beyond a count) included: they must
still hold the sentinel.  Every case runs on the default stream and on a caller's stream.
"""
import math

import numpy as np
import pytest

import morph_model as mm
import remap_cases as rc
import remap_model as rm
from components_model import COMP_DTYPE, components
from gpu_support import COMP_BYTES, FIT_BYTES, LINE_BYTES, SEG_BYTES, SENTINEL, Arena, pad_frames, ptr
from morph_rig import STRELS, strokes
from sht_fit_model import FIT_DTYPE, frame_fits, refine_lines
from sht_segments_model import SEG_DTYPE, frame_segments

pytestmark = pytest.mark.gpu

LIMIT = 65535                       # kMaxFramesPerLaunch
F_BIG = LIMIT + 6                   # one full slice, a last slice of 6
F_TWICE = 2 * LIMIT + 3             # two full slices: the slice start advances twice
F_GROUPS = 8 * LIMIT + 5            # the shared-map remap packs 8 frames into a group: a second slice of one ragged group
CONTENT, PARAM, COUNT = 7, 11, 4    # periods of the frame content, of per-frame parameters, of line lists and their counts
FIT_INTS, FIT_DOUBLES = ("line", "pixels", "sx", "sy", "sxx", "sxy", "syy"), ("nx", "ny", "rho", "rms2")


def test_no_period_divides_a_slice():
    """the premise of every positive test below: no slice of 65 535 frames (or of 65 535 groups of 8) starts where the cycle starts"""
    assert LIMIT == 3 * 5 * 17 * 257
    for p in (CONTENT, PARAM, COUNT, CONTENT * PARAM, CONTENT * COUNT):
        assert math.gcd(p, LIMIT) == 1 and LIMIT % p != 0 and (2 * LIMIT) % p != 0, p
    assert (8 * LIMIT) % CONTENT != 0          # the shared-map remap: slices of 65 535 groups of 8 frames
    assert F_BIG > LIMIT and F_BIG - LIMIT == 6 and F_TWICE == 2 * LIMIT + 3 and F_GROUPS == 8 * LIMIT + 5


# ---------------------------------------------------------------------------------------------------------------
# the batch as a table of slots indexed by frame
# ---------------------------------------------------------------------------------------------------------------
class Cycle:
    """Frame f of a batch of F frames holds slot (f % p for p in periods) of a table [periods...][bytes].  unit: frames per grid index of the sliced
    launch (8 for the shared-map remap)."""

    def __init__(self, F, *periods, unit=1):
        self.F, self.periods, self.unit = F, periods, unit
        f = np.arange(F)
        self.lin = np.ravel_multi_index(tuple(f % p for p in periods), periods)
        # the slot of the first frame of every slice behind the first
        self.starts = [tuple((k * LIMIT * unit) % p for p in periods) for k in range(1, (F + LIMIT * unit - 1) // (LIMIT * unit))]
        assert self.starts and all(any(s) for s in self.starts)

    def table(self, slots):
        a = np.ascontiguousarray(slots)
        assert a.shape[:len(self.periods)] == self.periods, (a.shape, self.periods)
        return a.reshape((int(np.prod(self.periods)),) + a.shape[len(self.periods):])

    def host(self, slots):
        """[F][...] host array of the batch"""
        return self.table(slots)[self.lin]

    def has_teeth(self, slots):
        t = self.table(slots)
        zero = t[0].tobytes()
        return all(t[np.ravel_multi_index(s, self.periods)].tobytes() != zero for s in self.starts)

    def check(self, body, slots, what, teeth=True):
        """body: device bytes [F][n]; slots: uint8 [periods...][n].  Compared on the device; the first wrong frame is named."""
        import torch
        t = self.table(slots)
        assert t.dtype == np.uint8 and t.ndim == 2 and body.numel() == self.F * t.shape[1], (what, t.dtype, t.shape, body.numel())
        if teeth:
            assert self.has_teeth(slots), "%s: a slice that started at frame 0 again would pass" % what
        dev = body.device
        exp = torch.from_numpy(t).to(dev)[torch.from_numpy(self.lin).to(dev)]
        got = body.view(self.F, t.shape[1])
        if torch.equal(got, exp):
            return
        bad = (got != exp).any(dim=1).nonzero().reshape(-1)
        f = int(bad[0])
        at = int((got[f] != exp[f]).nonzero()[0])
        raise AssertionError("%s: %d of %d frames differ, the first is frame %d (slice %d, frame %d of it) at byte %d: got %d, expected %d"
                             % (what, bad.numel(), self.F, f, f // (LIMIT * self.unit), f % (LIMIT * self.unit), at, int(got[f][at]), int(exp[f][at])))


def plane_slot(valid, S):
    """[H][S] bytes of an output plane: the model's pixels, the sentinel in the padding columns"""
    H, W = valid.shape
    out = np.full((H, S), SENTINEL, np.uint8)
    out[:, :W] = valid
    return out.reshape(-1)


def record_slot(rec, cap):
    """cap record slots: the first min(len, cap) hold the model's, the others were never written"""
    out = np.full(cap * rec.dtype.itemsize, SENTINEL, np.uint8)
    n = min(len(rec), cap)
    out[:n * rec.dtype.itemsize] = np.frombuffer(rec[:n].tobytes(), np.uint8)
    return out


def i32_slot(v):
    return np.array([v], np.int32).view(np.uint8)


def upload(ar, host):
    host = np.ascontiguousarray(host)
    raw = host.view(np.uint8).reshape(-1)
    d = ar.new(raw.size, raw)
    ar.keep(d, raw)
    return d


def each_stream(run):
    """run(name, stream handle): the default stream, then a caller's (what the buffers hold was written on the default stream: drained first)"""
    import torch
    run("default stream", 0)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    run("caller's stream", side.cuda_stream)


def noise_frames(W, H, seed, n=CONTENT):
    return np.stack([np.random.default_rng(seed + d).integers(0, 256, (H, W), dtype=np.uint8) for d in range(n)])


# ---------------------------------------------------------------------------------------------------------------
# the text chain: otsu -> threshold at the device levels -> close -> components of the caller's bytes
# ---------------------------------------------------------------------------------------------------------------
CHAIN_W, CHAIN_H, CHAIN_S = 24, 9, 24
CHAIN_SE = mm.strel(mm.RECT, 5, 3)


def glyphs(W, H, seed):
    """words_frame of tests/test_gpu_morph.py at the size of a crop, inverted: strokes 2 px wide and 2 px apart, light (225) on dark (55)"""
    rng = np.random.default_rng(seed)
    img = np.full((H, W), 55, np.uint8)
    for _ in range(2):
        x0, y0 = int(rng.integers(1, W - 10)), int(rng.integers(1, H - 4))
        w, h = int(rng.integers(5, 10)), int(rng.integers(2, 5))
        for x in range(x0, x0 + w, 4):
            img[y0:y0 + h, x:x + 2] = 225
    return img


def chain_frames():
    W, H = CHAIN_W, CHAIN_H
    gray_strokes = (strokes(W, H, 3).astype(np.int32) * 140 // 255 + 60).astype(np.uint8)
    return np.stack([glyphs(W, H, 1), strokes(W, H, 7), gray_strokes, np.full((H, W), 90, np.uint8),
                     np.random.default_rng(5).integers(0, 256, (H, W), dtype=np.uint8), glyphs(W, H, 6), glyphs(W, H, 2)])


def chain_slots(oracle, frames):
    """per distinct frame: Otsu level, binary plane, closed plane (S == W: no padding)"""
    lv = [int(oracle.otsu(f)) for f in frames]
    binary = [mm.threshold(f, float(t)) for f, t in zip(frames, lv)]
    closed = [mm.morph(b, CHAIN_SE, mm.CLOSE, mm.BORDER_REPLICATE) for b in binary]
    return lv, binary, closed


def component_slots(closed, min_pixels, cap):
    exp = [components(c, 8, min_pixels) for c in closed]
    labels = np.stack([np.ascontiguousarray(l, np.int32).view(np.uint8).reshape(-1) for l, _ in exp])
    records = np.stack([record_slot(r, cap) for _, r in exp]) if cap else None
    counts = np.stack([i32_slot(len(r)) for _, r in exp])
    return labels, records, counts, [len(r) for _, r in exp]


@pytest.mark.parametrize("F", [F_BIG, LIMIT, LIMIT + 1], ids=["65541", "65535_one_slice", "65536_last_slice_of_one"])
def test_text_chain(hip_ctx, oracle, F):
    """The text-detection front end on crops of 24 x 9: levels, binary planes, closed planes, labels, records and counts of every frame.  With
    65 541 frames the chain also runs with minPixels = 3 and with compCap = 0 and no label map (counts only: the calls that skip phases 7 / 8)."""
    from compv_amd import capi
    W, H, S = CHAIN_W, CHAIN_H, CHAIN_S
    frames = chain_frames()
    lv, binary, closed = chain_slots(oracle, frames)
    cap = max(len(components(c, 8, 1)[1]) for c in closed) + 1
    labels, records, counts, n = component_slots(closed, 1, cap)
    assert len(set(lv)) >= 4 and len(set(n)) >= 3 and max(n) >= 2, (lv, n)
    cyc = Cycle(F, CONTENT) if F > LIMIT else None
    idx = np.arange(F) % CONTENT

    def check(body, slots, what):
        """(up to the limit there is one slice and no later slice start to have teeth for)"""
        slots = np.ascontiguousarray(slots)
        if cyc is not None:
            return cyc.check(body, slots, what)
        import torch
        exp = torch.from_numpy(slots).to(body.device)[torch.from_numpy(idx).to(body.device)]
        assert torch.equal(body.view(F, -1), exp), what

    ar = Arena()
    d_in = upload(ar, frames[idx])
    n_px = F * H * S
    d_lv, d_bin, d_closed = ar.new(4 * F), ar.new(n_px), ar.new(n_px)
    d_labels, d_comps, d_cc = ar.new(4 * n_px), ar.new(F * cap * COMP_BYTES), ar.new(4 * F)
    plan = capi.Plan(hip_ctx, W, H, S, F)
    try:
        def run(name, st):
            import torch
            for d in (d_lv, d_bin, d_closed, d_labels, d_comps, d_cc):
                ar.refill(d)
            torch.cuda.synchronize()
            plan.otsu(ptr(d_in), ptr(d_lv), stream=st)
            plan.threshold(ptr(d_in), 0.0, ptr(d_bin), d_levels=ptr(d_lv), stream=st)
            plan.morph(ptr(d_bin), CHAIN_SE, mm.CLOSE, mm.BORDER_REPLICATE, ptr(d_closed), stream=st)
            plan.components(ptr(d_closed), 8, 1, ptr(d_labels), W, ptr(d_comps), cap, ptr(d_cc), stream=st)
            ar.check("text chain, " + name)
            check(d_lv, np.stack([i32_slot(t) for t in lv]), "Otsu levels, " + name)
            check(d_bin, np.stack([b.reshape(-1) for b in binary]), "binary planes, " + name)
            check(d_closed, np.stack([c.reshape(-1) for c in closed]), "closed planes, " + name)
            check(d_cc, counts, "component counts, " + name)
            check(d_comps, records, "component records, " + name)
            check(d_labels, labels, "label maps, " + name)
            if F != F_BIG:
                return
            # minPixels > 1: labels and records of the survivors only
            labels3, records3, counts3, n3 = component_slots(closed, 3, cap)
            assert n3 != n
            for d in (d_labels, d_comps, d_cc):
                ar.refill(d)
            plan.components(ptr(d_closed), 8, 3, ptr(d_labels), W, ptr(d_comps), cap, ptr(d_cc), stream=st)
            ar.check("components minPixels 3, " + name)
            check(d_cc, counts3, "counts, minPixels 3, " + name)
            check(d_comps, records3, "records, minPixels 3, " + name)
            check(d_labels, labels3, "labels, minPixels 3, " + name)
            # counts only: neither a label map nor records
            for d in (d_labels, d_comps, d_cc):
                ar.refill(d)
            plan.components(ptr(d_closed), 8, 1, 0, 0, 0, 0, ptr(d_cc), stream=st)
            ar.check("components, counts only, " + name)
            check(d_cc, counts, "counts only, " + name)
            assert bool((d_labels == SENTINEL).all()) and bool((d_comps == SENTINEL).all()), "counts only: a label map or records written"
        each_stream(run)
    finally:
        plan.close()


# ---------------------------------------------------------------------------------------------------------------
# grayscale, thresholds, morphology
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt_name", ["FMT_RGB24", "FMT_YUYV422"])
def test_grayscale(hip_ctx, oracle, fmt_name):
    """16 x 3: a 3-byte and a 2-byte format, two different source frame strides"""
    from compv_amd import capi
    fmt = getattr(capi, fmt_name)
    bpp = capi.FMT_BYTES[fmt]
    W, H, S, F = 16, 3, 16, F_BIG
    packed = noise_frames(S * bpp, H, 400 + fmt)
    exp = np.stack([oracle.grayscale(p, fmt, W).reshape(-1) for p in packed])
    cyc = Cycle(F, CONTENT)
    ar = Arena()
    d_in = upload(ar, cyc.host(packed))
    d_out = ar.new(F * H * S)
    plan = capi.Plan(hip_ctx, W, H, S, F)
    try:
        def run(name, st):
            import torch
            ar.refill(d_out)
            torch.cuda.synchronize()
            plan.grayscale(ptr(d_in), fmt, ptr(d_out), stream=st)
            ar.check("grayscale, " + name)
            cyc.check(d_out, exp, "grayscale %s, %s" % (fmt_name, name))
        each_stream(run)
    finally:
        plan.close()


LEVELS = np.array([-5, 300, 128, 0, 255, 17, 99, 200, 64, 1, 254], np.int32)      # per frame, clipped to 0 .. 255 by the kernel


@pytest.mark.parametrize("F", [F_BIG, F_TWICE], ids=["65541", "131073"])
def test_threshold_with_a_level_per_frame(hip_ctx, F):
    """8 x 3; the level array is offset per slice like the planes"""
    from compv_amd import capi
    assert len(LEVELS) == PARAM and LEVELS.min() < 0 and LEVELS.max() > 255
    W, H, S = 8, 3, 8
    frames = noise_frames(W, H, 31)
    exp = np.stack([np.stack([mm.threshold(f, float(min(max(int(t), 0), 255))).reshape(-1) for t in LEVELS]) for f in frames])      # [7][11][24]
    cyc = Cycle(F, CONTENT, PARAM)
    ar = Arena()
    d_in = upload(ar, frames[np.arange(F) % CONTENT])
    d_lv = upload(ar, LEVELS[np.arange(F) % PARAM])
    d_out = ar.new(F * H * S)
    plan = capi.Plan(hip_ctx, W, H, S, F)
    try:
        def run(name, st):
            import torch
            ar.refill(d_out)
            torch.cuda.synchronize()
            plan.threshold(ptr(d_in), 999.0, ptr(d_out), d_levels=ptr(d_lv), stream=st)
            ar.check("threshold, " + name)
            cyc.check(d_out, exp, "threshold with per-frame levels, " + name)
        each_stream(run)
    finally:
        plan.close()


@pytest.mark.parametrize("bs,W,H,S", [(3, 8, 3, 8), (9, 13, 12, 16)], ids=["block3_8x3", "block9_13x12"])
def test_adaptive_threshold(hip_ctx, bs, W, H, S):
    """out of place.  Block 3 on the smallest frame; block 9 on 13 x 12 at S = 16: on the 9 x 9 it accepts the mean is 0 everywhere but at the centre
    pixel and seven random frames give one and the same plane, so the frame has an interior of 5 x 4, and padding columns that must keep the sentinel"""
    from compv_amd import capi
    F = F_BIG
    frames = noise_frames(W, H, 50 + bs)
    exp = np.stack([plane_slot(mm.adaptive(f, bs, 5.0, 200.0, False), S) for f in frames])
    cyc = Cycle(F, CONTENT)
    ar = Arena()
    d_in = upload(ar, cyc.host(pad_frames(frames, S, np.random.default_rng(bs))))
    d_out = ar.new(F * H * S)
    plan = capi.Plan(hip_ctx, W, H, S, F)
    try:
        def run(name, st):
            import torch
            ar.refill(d_out)
            torch.cuda.synchronize()
            plan.threshold_adaptive(ptr(d_in), bs, 5.0, 200.0, False, ptr(d_out), stream=st)
            ar.check("adaptive, " + name)
            cyc.check(d_out, exp, "adaptive threshold %d, %s" % (bs, name))
        each_stream(run)
    finally:
        plan.close()


MORPH_STRELS = {"rect3x3": STRELS["rect3x3"], "random5x3": (np.random.default_rng(53).random((3, 5)) < 0.5).astype(np.uint8) * 255}


def test_morph(hip_ctx):
    """9 x 9 at S = 16 (the smallest geometry of tests/test_gpu_morph.py): the separable and the general kernel by name, one strel each, erode and
    close (the scratch plane between its two operations is offset like the caller's), both borders.  The strels are 3 rows tall: a taller one leaves
    a 9-row frame one interior row, and a close with a zero border nothing at all."""
    from compv_amd import capi
    W, H, S, F = 9, 9, 16, F_BIG
    frames = np.concatenate([noise_frames(W, H, 90, 4), np.stack([strokes(W, H, 91), np.full((H, W), 77, np.uint8), strokes(W, H, 92)])])
    assert len(frames) == CONTENT
    cyc = Cycle(F, CONTENT)
    ar = Arena()
    d_in = upload(ar, cyc.host(pad_frames(frames, S, np.random.default_rng(9))))
    d_out = ar.new(F * H * S)
    cases = [(capi.MORPH_KERNEL_SEPARABLE, "rect3x3"), (capi.MORPH_KERNEL_GENERAL, "random5x3")]
    expect = {(k, op, b): np.stack([plane_slot(mm.morph(f, MORPH_STRELS[s], op, b), S) for f in frames])
              for k, s in cases for op in (mm.ERODE, mm.CLOSE) for b in (mm.BORDER_REPLICATE, mm.BORDER_ZERO)}
    plan = capi.Plan(hip_ctx, W, H, S, F)
    try:
        def run(name, st):
            import torch
            for kernel, sname in cases:
                for op in (mm.ERODE, mm.CLOSE):
                    for border in (mm.BORDER_REPLICATE, mm.BORDER_ZERO):
                        what = "morph %s op %d border %d kernel %d, %s" % (sname, op, border, kernel, name)
                        ar.refill(d_out)
                        torch.cuda.synchronize()
                        plan.morph(ptr(d_in), MORPH_STRELS[sname], op, border, ptr(d_out), kernel=kernel, stream=st)
                        ar.check(what)
                        cyc.check(d_out, expect[(kernel, op, border)], what)
        each_stream(run)
    finally:
        plan.close()


# ---------------------------------------------------------------------------------------------------------------
# frames only in x: the Sobel / Scharr / Prewitt detector
# ---------------------------------------------------------------------------------------------------------------
def test_edge_dete_has_its_frames_in_x(hip_ctx, oracle):
    """compvhip_plan_edge_dete rides frames in the x extent (launch_op, sobel_kernels.hip): no slicing, no refusal, 8 x 3.  The per-frame
    maximum that scales the output sits at gmax[frame * 32]."""
    from compv_amd import capi
    W, H, S, F = 8, 3, 8, F_BIG
    frames = noise_frames(W, H, 120)
    cyc = Cycle(F, CONTENT)
    ar = Arena()
    d_in = upload(ar, cyc.host(frames))
    d_out = ar.new(F * H * S)
    plan = capi.Plan(hip_ctx, W, H, S, F)
    try:
        def run(name, st):
            import torch
            for op in (capi.OP_SOBEL, capi.OP_SCHARR, capi.OP_PREWITT):
                exp = np.stack([oracle.edge_dete(f, op)[0].reshape(-1) for f in frames])
                ar.refill(d_out)
                torch.cuda.synchronize()
                plan.edge_dete(ptr(d_in), op, ptr(d_out), stream=st)
                ar.check("edge_dete %d, %s" % (op, name))
                cyc.check(d_out, exp, "edge_dete %d, %s" % (op, name))
        each_stream(run)
    finally:
        plan.close()


# ---------------------------------------------------------------------------------------------------------------
# Hough line segments and line fits on caller's edge bytes and caller's line lists
# ---------------------------------------------------------------------------------------------------------------
SEG_W, SEG_H, SEG_S, SEG_THETA, LINE_CAP = 9, 9, 16, 30.0, 4
LINE_COUNTS = (3, 0, 6, 1)          # per frame, period 4: none, fewer than the capacity, more than it


def segment_inputs(oracle):
    """7 edge maps of 9 x 9; 4 line lists of LINE_CAP made-up lines (the calls read only row / col): the strongest accumulator cells of map k"""
    from compv_amd import capi
    W, H = SEG_W, SEG_H
    R, T, step = oracle.sht_dims(W, H, SEG_THETA)
    assert T == 6
    sinQ, cosQ = oracle.sht_tables(SEG_THETA, T)
    maps = np.zeros((CONTENT, H, W), np.uint8)
    i = np.arange(W)
    maps[0, 4, :] = 255; maps[0, :, 2] = 255
    maps[1, i, i] = 255; maps[1, 7, 1:6] = 255
    maps[2] = (np.random.default_rng(2).random((H, W)) < 0.35) * 255
    maps[4, :, 6] = 255; maps[4, 1, 3:] = 255; maps[4, 8 - i, i] = 255
    maps[5, 2, :4] = 255; maps[5, 2, 6:] = 255; maps[5, 6, :] = 255
    maps[6] = (np.random.default_rng(6).random((H, W)) < 0.6) * 255          # maps[3] stays empty
    lists = np.zeros((COUNT, LINE_CAP), capi.LINE_DTYPE)
    for k in range(COUNT):
        acc = oracle.sht_acc(maps[(0, 1, 4, 5)[k]], SEG_THETA)
        for j, cell in enumerate(np.argsort(-acc, axis=None, kind="stable")[:LINE_CAP]):
            row, col = divmod(int(cell), T)
            lists[k][j] = (float(row), float(np.float32(col) * np.float32(step)), int(acc[row, col]), row, col)
    return maps, lists, R, sinQ, cosQ


def cells_of(lines, count):
    n = min(count, LINE_CAP)
    return list(zip(lines["row"][:n].tolist(), lines["col"][:n].tolist()))


def fit_compare(cyc, d_fits, d_counts, recs, cap, what):
    """recs[d][k]: FIT_DTYPE records of slot (d, k).  Integers bit for bit, the doubles as VALUES (tests/test_gpu_sht_fit.py: the sign of a zero
    is not part of the contract), counts exact, record slots beyond the count unwritten."""
    F = cyc.F
    exp = np.zeros(cyc.periods + (cap,), FIT_DTYPE)
    n = np.zeros(cyc.periods, np.int64)
    for d in range(CONTENT):
        for k in range(COUNT):
            m = min(len(recs[d][k]), cap)
            exp[d, k, :m] = recs[d][k][:m]
            n[d, k] = m
    counts = np.array([[len(recs[d][k]) for k in range(COUNT)] for d in range(CONTENT)], np.int32)
    cyc.check(d_counts, counts.view(np.uint8).reshape(CONTENT, COUNT, 4), what + ": counts")
    assert cyc.has_teeth(np.frombuffer(exp.tobytes(), np.uint8).reshape(CONTENT, COUNT, -1)), what
    raw = d_fits.cpu().numpy().reshape(F, cap, FIT_BYTES)
    got = raw.view(FIT_DTYPE).reshape(F, cap)
    e, m = cyc.host(exp), np.arange(cap)[None, :] < cyc.host(n)[:, None]
    for k in FIT_INTS:
        assert (got[k] == e[k])[m].all(), (what, k, int(np.flatnonzero(((got[k] != e[k]) & m).any(axis=1))[0]))
    for k in FIT_DOUBLES:
        same = (got[k] == e[k]) | (np.isnan(got[k]) & np.isnan(e[k]))
        assert same[m].all(), (what, k, int(np.flatnonzero((~same & m).any(axis=1))[0]))
    assert (raw[~m] == SENTINEL).all(), (what, "records beyond the count were written")


def test_segments_and_fits(hip_ctx, oracle):
    """9 x 9 at S = 16 with thetaDeg = 30 (T = 6: the accumulators a plan of 65 541 frames allocates stay small).  Caller's edge bytes (random
    bytes in their padding columns), caller's line lists with counts 3, 0, 6, 1 at lineCap 4.  The three segment phases (count, scan, write) show
    in the counts, in where a line's segments start, and in the records; the fits run per line (with refined lines) and per segment."""
    from compv_amd import capi
    W, H, S, F = SEG_W, SEG_H, SEG_S, F_BIG
    maps, lists, R, sinQ, cosQ = segment_inputs(oracle)
    min_length, max_gap, b = 2, 1, 1
    segs = [[frame_segments(maps[d], sinQ, cosQ, cells_of(lists[k], LINE_COUNTS[k]), min_length, max_gap) for k in range(COUNT)] for d in range(CONTENT)]
    seg_cap = max(len(s) for row in segs for s in row)          # the fullest frame fills the capacity ...
    assert seg_cap >= 3 and sum(len(s) > 0 for row in segs for s in row) >= 8
    seg_cap -= 1                                                # ... and one more: clipped
    seg_slots = np.stack([np.stack([record_slot(s, seg_cap) for s in row]) for row in segs])
    seg_counts = np.stack([np.stack([i32_slot(len(s)) for s in row]) for row in segs])
    per_line = [[frame_fits(maps[d], sinQ, cosQ, cells_of(lists[k], LINE_COUNTS[k]), b, R) for k in range(COUNT)] for d in range(CONTENT)]
    per_seg = [[frame_fits(maps[d], sinQ, cosQ, cells_of(lists[k], LINE_COUNTS[k]), b, R, segs=segs[d][k][:seg_cap])[0] for k in range(COUNT)] for d in range(CONTENT)]
    cyc = Cycle(F, CONTENT, COUNT)
    ar = Arena()
    d_e = upload(ar, pad_frames(maps, S, np.random.default_rng(16))[np.arange(F) % CONTENT])
    d_lines = upload(ar, lists[np.arange(F) % COUNT])
    d_counts = upload(ar, np.array(LINE_COUNTS, np.int32)[np.arange(F) % COUNT])
    d_segs, d_sc = ar.new(F * seg_cap * SEG_BYTES), ar.new(4 * F)
    d_fits, d_fc, d_ref = ar.new(F * seg_cap * FIT_BYTES), ar.new(4 * F), ar.new(F * LINE_CAP * LINE_BYTES)
    plan = capi.Plan(hip_ctx, W, H, S, F, SEG_THETA)
    try:
        def run(name, st):
            import torch
            for d in (d_segs, d_sc, d_fits, d_fc, d_ref):
                ar.refill(d)
            torch.cuda.synchronize()
            plan.houghsht_segments(ptr(d_e), ptr(d_lines), ptr(d_counts), LINE_CAP, 0, min_length, max_gap, ptr(d_segs), seg_cap, ptr(d_sc), stream=st)
            ar.check("segments, " + name)
            cyc.check(d_sc, seg_counts, "segment counts, " + name)
            cyc.check(d_segs, seg_slots, "segments, " + name)
            # per line, with the refined lines
            plan.houghsht_fit(ptr(d_e), ptr(d_lines), ptr(d_counts), LINE_CAP, 0, b, 0, 0, 0, ptr(d_fits), seg_cap, ptr(d_fc), ptr(d_ref), stream=st)
            ar.check("fit per line, " + name)
            fit_compare(cyc, d_fits, d_fc, [[pl[0] for pl in row] for row in per_line], seg_cap, "fit per line, " + name)
            got = d_ref.cpu().numpy().reshape(F, LINE_CAP, LINE_BYTES)
            ref = np.zeros((CONTENT, COUNT, LINE_CAP), capi.LINE_DTYPE)
            valid = np.zeros((CONTENT, COUNT, LINE_CAP), bool)
            n = np.array([min(c, LINE_CAP) for c in LINE_COUNTS])
            for d in range(CONTENT):
                for k in range(COUNT):
                    ref[d, k, :n[k]] = refine_lines(lists[k][:n[k]], per_line[d][k][0], per_line[d][k][1])
                    valid[d, k, :n[k]] = per_line[d][k][1]
            assert valid.any() and not valid.all()
            e, v, m = cyc.host(ref), cyc.host(valid), np.arange(LINE_CAP)[None, :] < cyc.host(np.tile(n, (CONTENT, 1)))[:, None]
            g = got.view(capi.LINE_DTYPE).reshape(F, LINE_CAP)
            for k in ("rho", "strength", "row", "col"):
                assert (g[k].view(np.uint32) == e[k].view(np.uint32))[m].all(), ("refined lines", k, name)
            # theta of a fitted line goes through atan2: within 1 float32 ulp (tests/test_gpu_sht_fit.py); every other line keeps its own
            lo, hi = np.nextafter(e["theta"], np.float32(-np.inf)), np.nextafter(e["theta"], np.float32(np.inf))
            assert ((g["theta"] >= lo) & (g["theta"] <= hi))[m & v].all() and (g["theta"] == e["theta"])[m & ~v].all(), ("refined theta", name)
            assert (got[~m] == SENTINEL).all(), "refined lines beyond the count were written"
            # per segment, on the segments the device has just written
            for d in (d_fits, d_fc):
                ar.refill(d)
            plan.houghsht_fit(ptr(d_e), ptr(d_lines), ptr(d_counts), LINE_CAP, 0, b, ptr(d_segs), ptr(d_sc), seg_cap, ptr(d_fits), seg_cap, ptr(d_fc), stream=st)
            ar.check("fit per segment, " + name)
            fit_compare(cyc, d_fits, d_fc, per_seg, seg_cap, "fit per segment, " + name)
        each_stream(run)
    finally:
        plan.close()


# ---------------------------------------------------------------------------------------------------------------
# remap and inverse warp
# ---------------------------------------------------------------------------------------------------------------
INTERPS = (rm.NEAREST, rm.BILINEAR, rm.BILINEAR_FLOAT32)          # three kernels


def remap_slot(plane):
    return np.ascontiguousarray(plane).view(np.uint8).reshape(-1)


def test_remap_with_a_map_per_frame(hip_ctx):
    """8 x 4 -> 8 x 4, frame f through map f % 7: the coordinate offset f0 * coordFrameStride of the later slice"""
    from compv_amd import capi
    w, h, wo, ho, S, F = 8, 4, 8, 4, 8, F_BIG
    frames = noise_frames(w, h, 700)
    xs, ys = zip(*[rc.random_map(w, h, wo, ho, 710 + d) for d in range(CONTENT)])
    cyc = Cycle(F, CONTENT)
    ar = Arena()
    d_in = upload(ar, cyc.host(frames))
    d_x, d_y = upload(ar, cyc.host(np.stack(xs))), upload(ar, cyc.host(np.stack(ys)))
    exp = {i: np.stack([remap_slot(rm.remap(frames[d], xs[d], ys[d], i, None, 201)) for d in range(CONTENT)]) for i in INTERPS}
    outs = {i: ar.new(F * ho * wo * (4 if i == rm.BILINEAR_FLOAT32 else 1)) for i in INTERPS}
    plan = capi.Plan(hip_ctx, w, h, S, F)
    try:
        def run(name, st):
            import torch
            for i in INTERPS:
                ar.refill(outs[i])
                torch.cuda.synchronize()
                plan.remap(ptr(d_in), ptr(d_x), ptr(d_y), F, i, ptr(outs[i]), wo, ho, wo, None, 201, stream=st)
                ar.check("remap per frame %s, %s" % (rc.INTERP_NAMES[i], name))
                cyc.check(outs[i], exp[i], "remap per frame %s, %s" % (rc.INTERP_NAMES[i], name))
        each_stream(run)
    finally:
        plan.close()


@pytest.mark.parametrize("rows", [2, 3], ids=["2x3", "3x3"])
def test_warp_inverse_with_a_matrix_per_frame(hip_ctx, rows):
    """8 x 4 -> 8 x 4, frame f (content f % 7) through matrix f % 11: the table offset of the later slice"""
    from compv_amd import capi
    w, h, wo, ho, S, F = 8, 4, 8, 4, 8, F_BIG
    frames = noise_frames(w, h, 800 + rows)
    base = rc.matrices(w, h, wo, ho)["affine" if rows == 2 else "homography"]
    Ms = np.stack([base] * PARAM)
    for k in range(PARAM):
        Ms[k, 0, 2] += np.float32(0.375 * k)
        Ms[k, 1, 0] += np.float32(0.03 * k)
    cyc = Cycle(F, CONTENT, PARAM)
    ar = Arena()
    d_in = upload(ar, frames[np.arange(F) % CONTENT])
    all_M = np.ascontiguousarray(Ms[np.arange(F) % PARAM])
    exp = {i: np.stack([np.stack([remap_slot(rm.warp_inverse(frames[d], Ms[k], wo, ho, i, 17)) for k in range(PARAM)]) for d in range(CONTENT)]) for i in INTERPS}
    outs = {i: ar.new(F * ho * wo * (4 if i == rm.BILINEAR_FLOAT32 else 1)) for i in INTERPS}
    plan = capi.Plan(hip_ctx, w, h, S, F)
    try:
        def run(name, st):
            import torch
            for i in INTERPS:
                ar.refill(outs[i])
                torch.cuda.synchronize()
                plan.warp_inverse(ptr(d_in), all_M, i, ptr(outs[i]), wo, ho, wo, 17, stream=st)
                ar.check("warp per frame %s, %s" % (rc.INTERP_NAMES[i], name))
                cyc.check(outs[i], exp[i], "warp %d x 3 per frame %s, %s" % (rows, rc.INTERP_NAMES[i], name))
        each_stream(run)
    finally:
        plan.close()


def test_remap_with_a_shared_map_crosses_the_group_limit(hip_ctx):
    """A shared map serves 8 frames per workgroup, so group0 != 0 needs 8 * 65 535 + 5 = 524 285 frames: 8 x 3 at S = 8, 12.6 MB of frames each
    way.  The plan's own edge masks (16 words a row, two planes) take 2 * 524 285 * 3 * 64 bytes = 201 MB.  The second slice is one ragged
    group of 5 frames."""
    from compv_amd import capi
    w, h, wo, ho, S, F = 8, 3, 8, 3, 8, F_GROUPS
    assert F % 8 == 5 and (F + 7) // 8 == LIMIT + 1
    frames = noise_frames(w, h, 900)
    x, y = rc.random_map(w, h, wo, ho, 901)
    cyc = Cycle(F, CONTENT, unit=8)
    ar = Arena()
    d_in = upload(ar, cyc.host(frames))
    d_x, d_y = upload(ar, x), upload(ar, y)
    exp = {i: np.stack([remap_slot(rm.remap(f, x, y, i, None, 3)) for f in frames]) for i in INTERPS}
    outs = {i: ar.new(F * ho * wo * (4 if i == rm.BILINEAR_FLOAT32 else 1)) for i in INTERPS}
    plan = capi.Plan(hip_ctx, w, h, S, F)
    try:
        def run(name, st):
            import torch
            for i in INTERPS:
                ar.refill(outs[i])
                torch.cuda.synchronize()
                plan.remap(ptr(d_in), ptr(d_x), ptr(d_y), 1, i, ptr(outs[i]), wo, ho, wo, None, 3, stream=st)
                ar.check("remap shared %s, %s" % (rc.INTERP_NAMES[i], name))
                cyc.check(outs[i], exp[i], "remap shared %s, %s" % (rc.INTERP_NAMES[i], name))
        each_stream(run)
    finally:
        plan.close()


# ---------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------
def refused(hip_ctx, ar, outputs, what, call):
    """E_INVALID_PARAMETER naming the limit; nothing allocated; every output still the sentinel"""
    import torch
    from compv_amd import capi
    live = hip_ctx.live_allocations()
    with pytest.raises(capi.CompvHipError) as err:
        call()
    assert err.value.code == capi.E_INVALID_PARAMETER, (what, err.value)
    assert str(LIMIT) in str(err.value), (what, str(err.value))
    assert hip_ctx.live_allocations() == live, (what, "the refused call allocated")
    ar.check(what)
    for o in outputs:
        if isinstance(o, np.ndarray):
            assert (o.view(np.uint8) == SENTINEL).all(), (what, "a host output was written")
        else:
            assert bool((o == SENTINEL).all()), (what, "an output was written")
    torch.cuda.synchronize()


def test_unsliced_calls_refuse_beyond_the_limit(hip_ctx):
    """65 536 frames of 8 x 3 (FAST: 8 x 7, its minimum; ORB: 40 x 37).  Every buffer has its full size and holds the sentinel, inputs included: a
    call that failed to refuse could touch nothing it does not own."""
    from compv_amd import capi
    F = LIMIT + 1
    gauss = capi.gauss_kernel_fixedpoint(3, 1.0)

    def plan_calls(W, H, S, make):
        ar = Arena()
        plan = capi.Plan(hip_ctx, W, H, S, F)
        try:
            n = F * H * S
            for what, outputs, call in make(plan, ar, n):
                refused(hip_ctx, ar, outputs, what, call)
        finally:
            plan.close()

    def small(plan, ar, n):
        d_in, d_out = ar.new(n), ar.new(n)
        d_lines, d_counts, d_cart = ar.new(F * LINE_BYTES), ar.new(4 * F), ar.new(F * 16)
        R, T, _ = hip_ctx.houghsht_dims(plan.W, plan.H, 1.0)
        d_acc = ar.new(R * T * 4)
        io = (d_in, d_out, d_lines, d_counts, d_cart, d_acc)
        yield "canny", io, lambda: plan.canny(ptr(d_in), 59.0, 119.0, ptr(d_out))
        yield "canny, Otsu thresholds", io, lambda: plan.canny(ptr(d_in), 0.5, 1.0, ptr(d_out), threshold_type=capi.THRESHOLD_OTSU)
        yield "convlt_fixedpoint", io, lambda: plan.convlt_fixedpoint(ptr(d_in), gauss, gauss, ptr(d_out))
        yield "houghsht", io, lambda: plan.houghsht(ptr(d_in), 2, 0, ptr(d_lines), 1, ptr(d_counts))
        yield "pipeline", io, lambda: plan.pipeline(ptr(d_in), 59.0, 119.0, 2, 0, ptr(d_out), ptr(d_lines), 1, ptr(d_counts))
        yield "pipeline_async", io, lambda: plan.pipeline_async(ptr(d_in), 59.0, 119.0, 2, 0, ptr(d_out), ptr(d_lines), 1, ptr(d_counts))
        yield "pipeline_ex", io, lambda: plan.pipeline_ex(ptr(d_in), 0.5, 1.0, 2, 0, ptr(d_out), ptr(d_lines), 1, ptr(d_counts), threshold_type=capi.THRESHOLD_OTSU,
                                                          d_cart=ptr(d_cart))
        yield "pipeline_ex, asynchronous", io, lambda: plan.pipeline_ex(ptr(d_in), 59.0, 119.0, 2, 0, ptr(d_out), ptr(d_lines), 1, ptr(d_counts), asynchronous=True)
        yield "to_cartesian", io, lambda: plan.to_cartesian(ptr(d_lines), ptr(d_counts), 1, ptr(d_cart))
        yield "acc_export", io, lambda: plan.acc_export(0, ptr(d_acc), T)
        yield "scale", io, lambda: plan.scale(ptr(d_in), ptr(d_out), plan.W, plan.H, plan.S)
        # the batched KHT writes host arrays
        lines, counts, gs = (np.full(F * 2 * LINE_BYTES, SENTINEL, np.uint8), np.full(F * 8, SENTINEL, np.uint8), np.full(F * 8, SENTINEL, np.uint8))
        host = io + (lines, counts, gs)
        L = plan.lib
        yield "houghkht", host, lambda: hip_ctx._chk(L.compvhip_plan_houghkht(plan.h, ptr(d_in), 1.0, 1.0, 1, 0, 2.0, 10, 0.002, capi._ptr(lines), 2, capi._ptr(counts),
                                                                                 capi._ptr(gs), 0))
        opts = capi.KhtOpts(1.0, 1.0, 1, 0, 2.0, 10, 0.002, 0, capi.KHT_ORDER_CANONICAL)
        import ctypes as C
        yield "houghkht_ex", host, lambda: hip_ctx._chk(L.compvhip_plan_houghkht_ex(plan.h, ptr(d_in), C.byref(opts), capi._ptr(lines), 2, capi._ptr(counts), capi._ptr(gs)))

    def fast(plan, ar, n):
        d_in, d_scores, d_corners, d_counts = ar.new(n), ar.new(n), ar.new(F * 12), ar.new(4 * F)
        yield "fast", (d_in, d_scores, d_corners, d_counts), lambda: plan.fast(ptr(d_in), 20, 9, True, -1, ptr(d_scores), ptr(d_corners), 1, ptr(d_counts))

    def orb(plan, ar, n):
        d_in = ar.new(n)
        d_corners, d_cc, d_keys, d_kc, d_desc = ar.new(F * 12), ar.new(4 * F), ar.new(F * 24), ar.new(4 * F), ar.new(F * 32)
        io = (d_in, d_corners, d_cc, d_keys, d_kc, d_desc)
        yield "orb_keypoints", io, lambda: plan.orb_keypoints(ptr(d_in), ptr(d_corners), 1, ptr(d_cc), 0, 1.0, ptr(d_keys), 1, ptr(d_kc))
        yield "orb_describe", io, lambda: plan.orb_describe(ptr(d_in), ptr(d_keys), 1, ptr(d_kc), 1.0, ptr(d_desc))

    plan_calls(8, 3, 8, small)
    plan_calls(8, 7, 8, fast)
    plan_calls(40, 37, 40, orb)
    # the handles that refuse at creation
    ar = Arena()
    refused(hip_ctx, ar, (), "orbpyr_create", lambda: capi.OrbPyramid(hip_ctx, 40, 37, 40, F))
    refused(hip_ctx, ar, (), "matcher_create", lambda: capi.Matcher(hip_ctx, 32, 8, 8, pairs=F))


def test_the_limit_itself_is_accepted(hip_ctx, oracle):
    """65 535 frames: a call of the refused class runs -- the fixed-point blur, 3 taps, 8 x 3 -- and equals the oracle on every frame (the
    refusal starts at >, not at >=).  So does a matcher of 65 535 pairs."""
    from compv_amd import capi
    W, H, S, F = 8, 3, 8, LIMIT
    frames = noise_frames(W, H, 1000)
    gauss = capi.gauss_kernel_fixedpoint(3, 1.0)
    exp = []
    for f in frames:
        rc_, out = oracle.convlt_fxp(f, gauss, gauss)
        assert rc_ == 0
        exp.append(out.reshape(-1))
    idx = np.arange(F) % CONTENT
    ar = Arena()
    d_in = upload(ar, frames[idx])
    d_out = ar.new(F * H * S)
    plan = capi.Plan(hip_ctx, W, H, S, F)
    try:
        import torch
        plan.convlt_fixedpoint(ptr(d_in), gauss, gauss, ptr(d_out))
        ar.check("convlt at the limit")
        want = torch.from_numpy(np.stack(exp)).to(d_out.device)[torch.from_numpy(idx).to(d_out.device)]
        assert torch.equal(d_out.view(F, -1), want)
    finally:
        plan.close()
    capi.Matcher(hip_ctx, 4, 1, 1, pairs=LIMIT, knn=1).close()
