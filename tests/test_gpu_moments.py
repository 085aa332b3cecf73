"""GPU tests of the image moments (include/compv_hip.h, "image moments"; docs/kernels/moments.md): compvhip_moments_frames, _components, _shapes and
_host against tests/moments_model.py and the fixture of the compiled reference, BIT FOR BIT -- raw and shape records alike, with the sentinel in every
record behind the bound a call serves.

Shapes: the smallest at which the kernels can go wrong.  Frames: widths around the 16-byte chunk (1, 3, 15, 16, 17), around four and 64 chunks (63 .. 65,
1023 .. 1025) and 1041; heights of 1, 2 and the rows of a workgroup - 1, + 0, + 1; strides above the width with non-zero padding; the base pointer off by
0, 1 and 3 bytes, so that a row starts at every kind of address; 1, 3 and 33 frames; both weights; 8192 x 256 of 255 (m20 above 2^53); 65 537 frames
(the sliced launch).  Components: label maps of the real compvhip_plan_components and hand-made ones: one component over many waves, a 4-connected
checkerboard (every lane its own id), counts above the capacity and below zero, padding columns full of ids, gray planes with zeros inside blobs,
both origins."""
import os
import re

import numpy as np
import pytest

import moments_cases as mc
import moments_model as mm
from components_model import COMP_DTYPE, components
from fixtures import load_golden
from gpu_support import COMP_BYTES, SENTINEL, Arena, alloc_fill, ptr, u8

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAW, SHAPE = 48, 72
WIDTHS = (1, 3, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025, 1041)


def rows_per_workgroup():
    txt = open(os.path.join(ROOT, "compv_amd", "csrc", "kernels.hpp")).read()
    return int(re.search(r"constexpr int kMomentsRows = (\d+);", txt).group(1))


def capi_():
    from compv_amd import capi
    return capi


def records(buf, n, dtype):
    return np.frombuffer(buf.cpu().numpy()[:n * dtype.itemsize].tobytes(), dtype)


def expect_raw(records_):
    return mm.raw_array(records_).view(capi_().MOMENTS_DTYPE).reshape(-1)


def assert_records(d_raw, d_shape, sums, what, served=None):
    """d_raw / d_shape hold len(sums) records; served[k] False: record k still holds the sentinel; the others equal the model on every byte"""
    capi = capi_()
    n = len(sums)
    served = [True] * n if served is None else served
    exp_raw = expect_raw([s if ok else (0,) * 6 for s, ok in zip(sums, served)])
    exp_shape = mm.shape_array([s if ok else (0,) * 6 for s, ok in zip(sums, served)], capi.MOMENTS_SHAPE_DTYPE)
    for buf, exp, size, name in ((d_raw, exp_raw, RAW, "raw"), (d_shape, exp_shape, SHAPE, "shape")):
        if buf is None:
            continue
        got = buf.cpu().numpy()[:n * size].reshape(n, size)
        want = u8(exp).reshape(n, size)
        for k in range(n):
            if served[k]:
                assert got[k].tobytes() == want[k].tobytes(), "%s: %s record %d: got %s, expected %s" % (what, name, k, np.frombuffer(got[k].tobytes(), exp.dtype)[0], exp[k])
            else:
                assert (got[k] == SENTINEL).all(), "%s: %s record %d behind the bound was written" % (what, name, k)
        assert (buf.cpu().numpy()[n * size:] == SENTINEL).all(), "%s: %s records behind the call's were written" % (what, name)


class Frames:
    """frames [F][H][S] at `off` bytes into their buffer, raw and shape records with two records of room behind them"""

    def __init__(self, ctx, planes, W, off=0, arena=None):
        self.ctx, self.W, self.off = ctx, W, off
        self.F, self.H, self.S = planes.shape
        self.ar = arena or Arena()
        body = np.full(planes.size + off, 0x5B, np.uint8)
        body[off:] = planes.reshape(-1)
        self.d_in = self.ar.new(body.size, body)
        self.ar.keep(self.d_in, body)
        self.d_raw, self.d_shape = self.ar.new((self.F + 2) * RAW), self.ar.new((self.F + 2) * SHAPE)
        self.planes = planes

    def run(self, weights, shape=True, stream=0):
        self.ctx.moments_frames(ptr(self.d_in) + self.off, self.W, self.H, self.S, self.F, ptr(self.d_raw), ptr(self.d_shape) if shape else 0, weights, stream)

    def check(self, weights, what, shape=True):
        self.ar.check(what)
        sums = [mm.raw_sums(p[:, :self.W], weights) for p in self.planes]
        assert_records(self.d_raw, self.d_shape if shape else None, sums, what)
        if not shape:
            assert (self.d_shape.cpu().numpy() == SENTINEL).all(), what
        return sums


def padded(valid, S, seed):
    """(F, H, W) -> (F, H, S) with non-zero bytes in the padding"""
    F, H, W = valid.shape
    out = np.random.default_rng(seed).integers(1, 256, (F, H, S), dtype=np.uint8)
    out[:, :, :W] = valid
    return out


# ---- frames -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", WIDTHS)
def test_frame_widths_heights_strides_and_bases(hip_ctx, W):
    R = rows_per_workgroup()
    ar = Arena()
    for n, H in enumerate((1, 2, R - 1, R, R + 1)):
        rng = np.random.default_rng(1000 * W + H)
        valid = rng.integers(0, 256, (3, H, W), dtype=np.uint8)
        valid[1][rng.integers(0, 3, (H, W)) > 0] = 0          # a sparse frame between two dense ones
        S = W + (5, 16, 1, 0, 7)[n]          # a stride that moves the rows' addresses, a multiple of 16, the width itself
        rig = Frames(hip_ctx, padded(valid, S, W + H), W, off=(0, 1, 3)[(n + W) % 3], arena=ar)
        for weights in (mm.VALUE, mm.UNIT):
            ar.refill(rig.d_raw); ar.refill(rig.d_shape)
            rig.run(weights)
            rig.check(weights, "W %d H %d S %d off %d weights %d" % (W, H, S, rig.off, weights))


@pytest.mark.parametrize("F", (1, 33))
def test_frame_counts(hip_ctx, F):
    valid = np.stack([mc.blobs(65, 17, 500 + f) for f in range(F)])
    rig = Frames(hip_ctx, padded(valid, 70, F), 65, off=1)
    rig.run(mm.VALUE, shape=False)
    sums = rig.check(mm.VALUE, "%d frames, raw only" % F, shape=False)
    assert len({s for s in sums}) == F          # the frames differ in what they give
    rig.run(mm.UNIT)
    rig.check(mm.UNIT, "%d frames" % F)


def test_frames_of_the_fixture(hip_ctx):
    """every frame case, the 2048 x 2048 one and the 8192 x 256 one (m20 above 2^53: exact here) included: the fixture's sums, the model's shape"""
    meta, arrays = load_golden("golden_moments")
    seen_big = False
    for c in mc.frame_cases():
        img = mc.frame(c)
        rig = Frames(hip_ctx, img[None], c["size"][0])
        for weights in c["weights"]:
            rig.ar.refill(rig.d_raw); rig.ar.refill(rig.d_shape)
            rig.run(weights)
            name = "%s_%s" % (c["id"], ("value", "unit")[weights])
            rig.ar.check(name)
            got = records(rig.d_raw, 1, capi_().MOMENTS_DTYPE)
            assert [int(got[0][k]) for k in mm.NAMES] == arrays["raw_" + name].tolist(), name
            assert_records(rig.d_raw, rig.d_shape, [tuple(int(v) for v in arrays["raw_" + name])], name)
            seen_big = seen_big or int(got[0]["m20"]) > 2 ** 53
    assert seen_big


def test_65537_frames(hip_ctx):
    """two slices of the frame index: 65 535 frames and 2"""
    F, W, H, S = 65537, 5, 3, 6
    valid = np.random.default_rng(77).integers(0, 256, (F, H, W), dtype=np.uint8)
    rig = Frames(hip_ctx, padded(valid, S, 78), W, off=3)
    rig.run(mm.VALUE)
    rig.ar.check("65537 frames")
    # the model, vectorised over the frames (int64 is ample at 5 x 3)
    w = valid.astype(np.int64)
    i, j = np.arange(W)[None, None, :], np.arange(H)[None, :, None]
    exp = np.stack([(w * k).sum(axis=(1, 2)) for k in (1, j, i, i * j, j * j, i * i)], axis=1).astype(np.uint64)
    got = np.frombuffer(rig.d_raw.cpu().numpy()[:F * RAW].tobytes(), np.uint64).reshape(F, 6)
    assert np.array_equal(got, exp), "first frame that differs: %d" % int(np.flatnonzero((got != exp).any(axis=1))[0])
    assert (rig.d_raw.cpu().numpy()[F * RAW:] == SENTINEL).all()
    for f in (0, 65534, 65535, 65536):          # shape records on either side of the slice border
        one = np.frombuffer(rig.d_shape.cpu().numpy()[f * SHAPE:(f + 1) * SHAPE].tobytes(), capi_().MOMENTS_SHAPE_DTYPE)
        assert one.tobytes() == mm.shape_array([tuple(int(v) for v in exp[f])], capi_().MOMENTS_SHAPE_DTYPE).tobytes(), f
    assert (rig.d_shape.cpu().numpy()[F * SHAPE:] == SENTINEL).all()


def test_the_same_call_twice_on_changed_content(hip_ctx):
    """nothing is carried from call to call and the records are cleared by the call itself: the second call's records are the second content's"""
    a = np.stack([mc.blobs(203, 33, 900 + f) for f in range(3)])
    rig = Frames(hip_ctx, padded(a, 208, 1), 203)
    rig.run(mm.VALUE)
    first = rig.check(mm.VALUE, "first content")
    b = padded(np.stack([mc.blobs(203, 33, 950 + f) for f in range(3)]), 208, 2)
    rig.planes = b
    rig.ar.reload(rig.d_in, b)
    rig.run(mm.VALUE)          # into the records of the first call, not refilled
    assert rig.check(mm.VALUE, "second content") != first


def test_shapes_alone(hip_ctx):
    """compvhip_moments_shapes on every record of the fixture and on sums at and beyond 2^53 and 2^64 - 1"""
    capi = capi_()
    _, arrays = load_golden("golden_moments")
    raw = [tuple(int(v) for v in r) for k in arrays.files if k.startswith("raw_") for r in arrays[k].reshape(-1, 6)]
    raw += [(0,) * 6, (0, 9, 9, 9, 9, 9), (2 ** 53 + 1, 2 ** 53 + 3, 2 ** 54 + 2, 2 ** 64 - 1, 2 ** 63 + 1025, 2 ** 64 - 1025), (3, 2 ** 40, 2 ** 41 + 1, 2 ** 62, 2 ** 63, 2 ** 64 - 1)]
    ar = Arena()
    host = u8(expect_raw(raw))
    d_raw = ar.new(host.size, host)
    ar.keep(d_raw, host)
    d_shape = ar.new((len(raw) + 1) * SHAPE)
    hip_ctx.moments_shapes(ptr(d_raw), len(raw), ptr(d_shape))
    ar.check("shapes")
    got = d_shape.cpu().numpy()
    assert got[:len(raw) * SHAPE].tobytes() == mm.shape_array(raw, capi.MOMENTS_SHAPE_DTYPE).tobytes() and (got[len(raw) * SHAPE:] == SENTINEL).all()
    assert got[:len(raw) * SHAPE].tobytes() == capi.moments_shape_host(raw).tobytes()          # the host form runs the same header
    hip_ctx.moments_shapes(ptr(d_raw), 0, 0)          # nothing to do


# ---- components -------------------------------------------------------------------------------------------------------------------------------
class Comps:
    """label maps [F][H][ls], component records [F][cap], counts [F] and optional gray planes [F][H][S] on the device, raw and shape records [F][cap]"""

    def __init__(self, ctx, labels, W, comps, counts, cap, gray=None, arena=None):
        self.ctx, self.W, self.cap = ctx, W, cap
        self.F, self.H, self.ls = labels.shape
        self.ar = arena or Arena()
        self.labels, self.counts, self.gray = labels, counts, gray
        self.comps = np.zeros((self.F, cap), COMP_DTYPE)
        self.comps.view(np.uint8)[...] = 0x3C          # records behind a frame's count hold no box
        for f, c in enumerate(comps):
            self.comps[f, :min(len(c), cap)] = c[:cap]
        self.d_labels = self.host(labels.astype(np.int32))
        self.d_comps = self.host(self.comps)
        self.d_counts = self.host(np.asarray(counts, np.int32))
        self.d_gray = self.host(gray) if gray is not None else None
        self.d_raw, self.d_shape = self.ar.new(self.F * cap * RAW), self.ar.new(self.F * cap * SHAPE)

    def host(self, a):
        d = self.ar.new(a.nbytes, u8(a))
        self.ar.keep(d, u8(a))
        return d

    def run(self, weights, origin, shape=True, stream=0):
        self.ctx.moments_components(ptr(self.d_labels), self.W, self.H, self.ls, ptr(self.d_comps), self.cap, ptr(self.d_counts), self.F, ptr(self.d_raw),
                                    ptr(self.d_shape) if shape else 0, ptr(self.d_gray) if self.d_gray is not None else 0, 0 if self.gray is None else self.gray.shape[2],
                                    weights, origin, stream)

    def check(self, weights, origin, what, shape=True):
        self.ar.check(what)
        sums, served = [], []
        for f in range(self.F):
            g = None if self.gray is None else self.gray[f][:, :self.W]
            got = mm.component_sums(self.labels[f][:, :self.W], self.comps[f], self.counts[f], self.cap, g, weights, origin)
            sums += got + [(0,) * 6] * (self.cap - len(got))
            served += [True] * len(got) + [False] * (self.cap - len(got))
        assert_records(self.d_raw, self.d_shape if shape else None, sums, what, served)
        return sums


def test_components_of_the_real_labeller(hip_ctx):
    """gray -> binary map -> compvhip_plan_components -> compvhip_moments_components without a host trip, for every component case of the fixture: the
    labeller's own label map (stride above W), records and counts feed the moments call"""
    capi = capi_()
    _, arrays = load_golden("golden_moments")
    for base in ("blobs97", "blobs203"):
        cases = [c for c in mc.component_cases() if c["id"].startswith(base)]
        c0 = cases[0]
        W, H = c0["size"]
        S, ls, cap = (W + 7) // 8 * 8, W + 3, 64
        fg, gray = mc.component_frame(c0)
        other = (mc.blobs(W, H, c0["seed"] + 50) != 0).astype(np.uint8) * 255          # a second frame, so that the frame offsets of every array count
        ar = Arena()
        edges = padded(np.stack([fg, other]), S, 5)
        grays = padded(np.stack([gray, gray[::-1].copy()]), S, 6)
        d_edges, d_gray = ar.new(edges.size, u8(edges)), ar.new(grays.size, u8(grays))
        ar.keep(d_edges, u8(edges)); ar.keep(d_gray, u8(grays))
        d_labels, d_comps, d_counts = ar.new(2 * H * ls * 4), ar.new(2 * cap * COMP_BYTES), ar.new(8)
        d_raw, d_shape = ar.new(2 * cap * RAW), ar.new(2 * cap * SHAPE)
        plan = capi.Plan(hip_ctx, W, H, S, 2)
        try:
            plan.components(ptr(d_edges), c0["connectivity"], c0["min_pixels"], ptr(d_labels), ls, ptr(d_comps), cap, ptr(d_counts))
            for c in cases:
                ar.refill(d_raw); ar.refill(d_shape)
                hip_ctx.moments_components(ptr(d_labels), W, H, ls, ptr(d_comps), cap, ptr(d_counts), 2, ptr(d_raw), ptr(d_shape), ptr(d_gray) if c["gray"] else 0, S,
                                           c["weights"], c["origin"])
                ar.check(c["id"])
                exp = [components(e[:, :W], c0["connectivity"], c0["min_pixels"]) for e in edges]
                assert d_counts.cpu().numpy().view(np.int32).tolist() == [len(r) for _, r in exp] and all(3 <= len(r) <= cap for _, r in exp)
                sums, served = [], []
                for f, (lab, rec) in enumerate(exp):
                    got = mm.component_sums(lab, rec, len(rec), cap, grays[f][:, :W] if c["gray"] else None, c["weights"], c["origin"])
                    sums += got + [(0,) * 6] * (cap - len(got))
                    served += [True] * len(got) + [False] * (cap - len(got))
                assert_records(d_raw, d_shape, sums, c["id"], served)
                assert mm.raw_array(sums[:len(exp[0][1])]).tolist() == arrays["raw_" + c["id"]].tolist(), c["id"]          # frame 0 is the fixture's case
        finally:
            plan.close()


def checkerboard(W, H):
    """every pixel with (x + y) even is a component of its own under 4-connectivity: ids in raster order, a lane's elements all differ"""
    return components(((np.arange(W)[None, :] + np.arange(H)[:, None]) % 2 == 0).astype(np.uint8), 4, 1)


def test_hand_made_label_maps(hip_ctx):
    """frame 0: one component spanning many waves (with a hole of background and of another id); frame 1: a checkerboard whose count lies above the
    capacity, so its label map holds ids beyond the bound; frame 2: the checkerboard again with a negative count -- nothing is served.  The padding
    columns hold served ids, negative and huge ones."""
    W, H, ls, cap = 1031, 9, 1040, 300
    big = np.ones((H, W), np.int32)
    big[3:5, 500:530] = 0
    big[6, 100:900:7] = 2
    big_rec = np.zeros(2, COMP_DTYPE)
    big_rec[0] = (0, 0, 0, 0, W - 1, H - 1, 0)
    big_rec[1] = (100, 6, 100, 6, 898, 6, 0)
    chk, chk_rec = checkerboard(W, H)
    assert len(chk_rec) > 4000
    labels = np.zeros((3, H, ls), np.int32)
    labels[:, :, W:] = np.array([1, 2, -7, 2 ** 30, 3, -2 ** 31, 299, 300, 301][:ls - W], np.int32)
    labels[0, :, :W], labels[1, :, :W], labels[2, :, :W] = big, chk, chk
    rng = np.random.default_rng(31)
    gray = rng.integers(0, 256, (3, H, W + 5), dtype=np.uint8)
    gray[:, :, ::3] = 0          # zero-valued pixels inside every blob
    gray[:, :, W:] = 255
    for g in (None, gray):
        rig = Comps(hip_ctx, labels, W, [big_rec, chk_rec, chk_rec], [2, len(chk_rec), -4], cap, g)
        for weights, origin in ((mm.VALUE, mm.ORIGIN_FRAME), (mm.VALUE, mm.ORIGIN_BOX), (mm.UNIT, mm.ORIGIN_BOX)):
            rig.ar.refill(rig.d_raw); rig.ar.refill(rig.d_shape)
            rig.run(weights, origin)
            what = "gray %s weights %d origin %d" % (g is not None, weights, origin)
            sums = rig.check(weights, origin, what)
            assert sums[0][0] == (int((big == 1).sum()) if g is None else int(mm.pixel_weights(gray[0][:, :W], weights)[big == 1].sum())), what
    # raw records alone, and a second call on changed labels into the same records
    rig.run(mm.VALUE, mm.ORIGIN_FRAME, shape=False)
    labels2 = labels.copy()
    labels2[0, :, :W] = np.where(big == 1, 2, 1)
    rig.labels = labels2
    rig.ar.reload(rig.d_labels, labels2.astype(np.int32))
    rig.ar.refill(rig.d_shape)
    rig.run(mm.VALUE, mm.ORIGIN_FRAME, shape=False)
    rig.check(mm.VALUE, mm.ORIGIN_FRAME, "changed labels, raw only", shape=False)
    assert (rig.d_shape.cpu().numpy() == SENTINEL).all()


def test_narrow_label_maps(hip_ctx):
    """widths below and around a lane's 8 elements and a wave's 512 columns; one row, several, and the rows of a wave's band - 1, + 0, + 1 and two
    bands and a bit, where a wave carries the sums of an id from row to row"""
    ar = Arena()
    R = int(re.search(r"constexpr int kMomentsCompRows = (\d+);", open(os.path.join(ROOT, "compv_amd", "csrc", "kernels.hpp")).read()).group(1))
    for W, H in ((1, 1), (7, 3), (8, 2), (9, 5), (511, 2), (512, 1), (513, 3), (37, R - 1), (37, R), (37, R + 1), (600, 2 * R + 1)):
        rng = np.random.default_rng(W * 10 + H)
        lab, rec = components(rng.integers(0, 3, (H, W)) > 0, 8, 1)
        cap = max(len(rec), 1) + 1
        gray = rng.integers(0, 256, (1, H, W), dtype=np.uint8)
        rig = Comps(hip_ctx, lab[None], W, [rec], [len(rec)], cap, gray, arena=ar)
        for origin in (mm.ORIGIN_FRAME, mm.ORIGIN_BOX):
            ar.refill(rig.d_raw); ar.refill(rig.d_shape)
            rig.run(mm.VALUE, origin)
            rig.check(mm.VALUE, origin, "%d x %d origin %d" % (W, H, origin))


# ---- calls --------------------------------------------------------------------------------------------------------------------------------------
def test_every_refusal_leaves_the_sentinels(hip_ctx):
    capi = capi_()
    lib, E = capi.load(), capi.E_INVALID_PARAMETER
    import ctypes as C
    ar = Arena()
    W, H, S, ls, cap = 20, 6, 24, 22, 4
    d_gray, d_labels = ar.new(2 * H * S, u8(np.ones(2 * H * S, np.uint8))), ar.new(2 * H * ls * 4, u8(np.ones(2 * H * ls, np.int32)))
    d_comps, d_counts = ar.new(2 * cap * COMP_BYTES, u8(np.zeros(2 * cap * 7, np.int32))), ar.new(8, u8(np.array([2, 2], np.int32)))
    d_raw, d_shape = ar.new(2 * cap * RAW + 8), ar.new(2 * cap * SHAPE + 8)
    g, l, c, n, r, s = (ptr(t) for t in (d_gray, d_labels, d_comps, d_counts, d_raw, d_shape))
    ok = capi.MomentsDesc()
    small = capi.MomentsDesc(); small.size = 16
    weights = capi.MomentsDesc(weights=2)
    origin = capi.MomentsDesc(origin=2)
    box = capi.MomentsDesc(origin=capi.MOMENTS_ORIGIN_BOX)
    d = C.byref
    h = hip_ctx.h
    frames = [(None, g, W, H, S, 2, r, s), (d(small), g, W, H, S, 2, r, s), (d(weights), g, W, H, S, 2, r, s), (d(origin), g, W, H, S, 2, r, s), (d(box), g, W, H, S, 2, r, s),
              (d(ok), None, W, H, S, 2, r, s), (d(ok), g, W, H, S, 2, None, s), (d(ok), g, 0, H, S, 2, r, s), (d(ok), g, W, 0, S, 2, r, s), (d(ok), g, 32768, 1, 32768, 1, r, s),
              (d(ok), g, 1, 32768, 1, 1, r, s), (d(ok), g, 32767, 32767, 32767, 1, r, s), (d(ok), g, 16407, 16384, 16407, 1, r, s), (d(ok), g, W, H, W - 1, 2, r, s),
              (d(ok), g, W, H, S, 0, r, s), (d(ok), g, W, H, S, 2 ** 31, r, s), (d(ok), g, W, H, S, 2, r + 4, s), (d(ok), g, W, H, S, 2, r, s + 4), (d(ok), g, W, H, S, 2, r + 1, None)]
    for args in frames:
        assert lib.compvhip_moments_frames(h, *args) == E, args[2:6]
    comps = [(None, l, W, H, ls, g, S, c, cap, n, 2, r, s), (d(small), l, W, H, ls, g, S, c, cap, n, 2, r, s), (d(weights), l, W, H, ls, g, S, c, cap, n, 2, r, s),
             (d(origin), l, W, H, ls, g, S, c, cap, n, 2, r, s), (d(ok), None, W, H, ls, g, S, c, cap, n, 2, r, s), (d(ok), l, W, H, ls, g, S, None, cap, n, 2, r, s),
             (d(ok), l, W, H, ls, g, S, c, cap, None, 2, r, s), (d(ok), l, W, H, ls, g, S, c, cap, n, 2, None, s), (d(ok), l, W, H, W - 1, g, S, c, cap, n, 2, r, s),
             (d(ok), l, W, H, ls, g, W - 1, c, cap, n, 2, r, s), (d(ok), l, 0, H, ls, g, S, c, cap, n, 2, r, s), (d(ok), l, W, 32768, ls, g, S, c, cap, n, 2, r, s),
             (d(ok), l, 32767, 32767, 32767, g, 32767, c, cap, n, 1, r, s), (d(ok), l, W, H, ls, g, S, c, 0, n, 2, r, s), (d(ok), l, W, H, ls, g, S, c, 2 ** 31, n, 2, r, s),
             (d(ok), l, W, H, ls, g, S, c, cap, n, 0, r, s), (d(ok), l + 2, W, H, ls, g, S, c, cap, n, 2, r, s), (d(ok), l, W, H, ls, g, S, c + 1, cap, n, 2, r, s),
             (d(ok), l, W, H, ls, g, S, c, cap, n + 2, 2, r, s), (d(ok), l, W, H, ls, g, S, c, cap, n, 2, r + 4, s), (d(ok), l, W, H, ls, g, S, c, cap, n, 2, r, s + 4)]
    for args in comps:
        assert lib.compvhip_moments_components(h, *args) == E, args[2:11]
    for args in ((None, r, 2, s), (d(small), r, 2, s), (d(ok), None, 2, s), (d(ok), r, 2, None), (d(ok), r + 4, 2, s), (d(ok), r, 2, s + 4), (d(ok), r, 2 ** 31, s)):
        assert lib.compvhip_moments_shapes(h, *args) == E, args[2]
    img = np.ones((H, S), np.uint8)
    raw, shape = np.full(RAW, 7, np.uint8), np.full(SHAPE, 7, np.uint8)
    p = capi._ptr
    for args in ((None, p(img), W, H, S, p(raw), p(shape)), (d(small), p(img), W, H, S, p(raw), p(shape)), (d(weights), p(img), W, H, S, p(raw), p(shape)),
                 (d(box), p(img), W, H, S, p(raw), p(shape)), (d(ok), None, W, H, S, p(raw), p(shape)), (d(ok), p(img), W, H, S, None, p(shape)),
                 (d(ok), p(img), 0, H, S, p(raw), p(shape)), (d(ok), p(img), W, H, W - 1, p(raw), p(shape)), (d(ok), p(img), 32767, 32767, 32767, p(raw), p(shape))):
        assert lib.compvhip_moments_host(h, *args) == E, args[2:5]
    assert (raw == 7).all() and (shape == 7).all()
    ar.check("refused calls")
    assert (d_raw.cpu().numpy() == SENTINEL).all() and (d_shape.cpu().numpy() == SENTINEL).all()
    assert "moments" in hip_ctx.last_error()
    # the same arguments, served: 32767 x 32767 passes the range rule with UNIT (refused above with VALUE) and fails only on the pointer
    unit = capi.MomentsDesc(weights=capi.MOMENTS_UNIT)
    assert lib.compvhip_moments_frames(h, d(unit), None, 32767, 32767, 32767, 1, r, s) == E and "null" in hip_ctx.last_error()
    assert lib.compvhip_moments_frames(h, d(ok), g, W, H, S, 2, r, s) == capi.OK
    assert lib.compvhip_moments_components(h, d(box), l, W, H, ls, None, 0, c, cap, n, 2, r, s) == capi.OK
    ar.check("served calls")
    assert not (d_raw.cpu().numpy()[:RAW] == SENTINEL).all()


def test_behind_pending_work_on_the_descriptors_stream(hip_ctx):
    """the frames reach the device on a side stream behind a delay; the calls follow on it (the descriptor's stream) and return at once"""
    import torch
    side = torch.cuda.Stream()
    valid = np.stack([mc.blobs(203, 33, 300 + f) for f in range(3)])
    rig = Frames(hip_ctx, padded(valid, 208, 3), 203)
    lab, rec = components(valid[0], 8, 1)
    crig = Comps(hip_ctx, lab[None], 203, [rec], [len(rec)], len(rec) + 1, valid[:1].copy(), arena=rig.ar)
    host = torch.from_numpy(u8(rig.planes).copy()).pin_memory()
    lab_host = torch.from_numpy(u8(lab.astype(np.int32)).copy()).pin_memory()
    rig.d_in.fill_(SENTINEL)
    crig.d_labels.fill_(0)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        torch.cuda._sleep(20_000_000)          # a few milliseconds of pending work in front of the copies
        rig.d_in.copy_(host, non_blocking=True)
        crig.d_labels.copy_(lab_host, non_blocking=True)
    rig.run(mm.VALUE, stream=side.cuda_stream)
    crig.run(mm.VALUE, mm.ORIGIN_BOX, stream=side.cuda_stream)
    side.synchronize()
    rig.check(mm.VALUE, "frames behind pending work")
    crig.check(mm.VALUE, mm.ORIGIN_BOX, "components behind pending work")


@pytest.mark.parametrize("fill", (0xFF, 0x01))
def test_host_form_cold_on_poisoned_allocations(fill):
    """the first call of a fresh context, whose staging is allocated inside the fill: from 1 x 1 on, both weights, then a larger plane (the staging
    grows) and the first one again"""
    capi = capi_()
    with alloc_fill(fill):
        ctx = capi.Context(0)
        try:
            for W, H, seed in ((1, 1, 1), (61, 37, 2), (300, 70, 3), (1, 1, 1)):
                img = np.random.default_rng(seed).integers(1 if W == 1 else 0, 256, (H, W + 3), dtype=np.uint8)[:, :W]          # a strided host plane
                for weights in (mm.VALUE, mm.UNIT):
                    raw, shape = ctx.moments(img, weights)
                    sums = mm.raw_sums(img, weights)
                    assert tuple(int(raw[k]) for k in mm.NAMES) == sums, (W, H, weights)
                    assert shape.tobytes() == mm.shape_array([sums], capi.MOMENTS_SHAPE_DTYPE)[0].tobytes(), (W, H, weights)
            # raw alone
            raw, img = np.zeros(1, capi.MOMENTS_DTYPE), np.full((2, 2), 9, np.uint8)
            desc = capi.MomentsDesc()
            import ctypes as C
            assert ctx.lib.compvhip_moments_host(ctx.h, C.byref(desc), capi._ptr(img), 2, 2, 2, capi._ptr(raw), None) == capi.OK
            assert tuple(int(raw[0][k]) for k in mm.NAMES) == (36, 18, 18, 9, 18, 18)
        finally:
            ctx.close()
