"""GPU colour conversion (compvhip_convert_frames, compvhip_convert_u8) against tests/convert_model.py on every frame and against the fixtures of
tests/golden/golden_convert.* where a frame is a golden case, byte for byte: nothing here is compared with a tolerance.

Harness of tests/gpu_support.py: every device buffer sits between two guards and starts filled with a sentinel.  An image's planes lie in one
buffer each, `frames` of them, rows rowBytes apart and frames frameBytes apart; after a call every byte of an output buffer that is no pixel -- between
a row's end and rowBytes, between frames, in front of the first plane and behind the last frame -- must still hold the sentinel, and every input must be
unchanged.  The calls allocate nothing: compvhip_live_allocations is the same before and after every device call.

The kernel's arms (compv_amd/csrc/convert_kernels.hip; one thread = 8 adjacent pixels of a row):
  word arm, whole groups      every pointer, rowBytes and frameBytes a multiple of 16: layouts "aligned" below, and the 4K rows of 3840 x 4
  byte loop, last group       the same layouts at W % 8 != 0 (7, 33, 250, 641)
  byte loop, every group      layouts "padded" (odd rowBytes, different per plane, odd frameBytes) and "shifted" (aligned strides, every plane pointer + 1)"""
import contextlib
import ctypes as C
import functools

import numpy as np
import pytest

import convert_cases as cc
import convert_model as cm
from fixtures import load_golden, md5
from gpu_support import Arena, SENTINEL, ptr

pytestmark = pytest.mark.gpu

SIZES = ((7, 5), (33, 17), (250, 3), (641, 480))
PAIR_IDS = [cm.pair_name(s, d) for s, d in cm.SERVED]
FRAMES = 3


@pytest.fixture(scope="module")
def golden():
    return {c["id"]: c for c in load_golden("golden_convert")[0]["cases"]}


@functools.lru_cache(maxsize=None)
def source_frames(src, W, H):
    """FRAMES frames of the source: the golden noise case of the size, then frames of other seeds.  Computed once, never written."""
    c = cc.BY_ID["%s_noise%dx%d" % (cm.NAMES[src], W, H)]
    frames = [cc.case_planes(c)]
    for seed in range(1, FRAMES):
        r = np.random.RandomState(7000 + 131 * seed + 97 * src + W + 7 * H)
        frames.append([r.randint(0, 256, s).astype(np.uint8) for s in cm.plane_shapes(src, W, H)])
    for f in frames:
        for p in f:
            p.setflags(write=False)
    return frames


@functools.lru_cache(maxsize=None)
def model_frames(src, dst, W, H):
    out = [cm.convert(src, dst, f, W, H) for f in source_frames(src, W, H)]
    for f in out:
        for p in f:
            p.setflags(write=False)
    return out


@contextlib.contextmanager
def no_allocation(ctx):
    before = ctx.live_allocations()
    yield
    assert ctx.live_allocations() == before


class DevImage:
    """`frames` images of one format in guarded device buffers, one per plane.  layout: "padded" (rowBytes = minimum + an odd pad that differs per plane,
    frameBytes + 7), "aligned" (everything a multiple of 16), "shifted" (aligned strides, the planes start 1 byte into their buffers), "dense"."""
    PADS = (5, 3, 9)

    def __init__(self, ar, fmt, W, H, frames, layout, content=None):
        from compv_amd import capi
        self.fmt, self.W, self.H, self.F = fmt, W, H, frames
        self.n, self.minRow, self.rows = cm.layout(fmt, W, H)
        up16 = lambda v: (v + 15) // 16 * 16          # noqa: E731
        self.rowBytes, self.frameBytes, self.off, self.bufs, self.host = [], [], [], [], []
        for p in range(self.n):
            rb = {"padded": self.minRow[p] + self.PADS[p], "dense": self.minRow[p]}.get(layout, up16(self.minRow[p]) + 16)
            fb = {"padded": rb * self.rows[p] + 7, "dense": rb * self.rows[p]}.get(layout, rb * self.rows[p] + 32)
            off = {"shifted": 1, "padded": 3}.get(layout, 0)
            h = np.full(off + frames * fb + 16, SENTINEL, np.uint8)
            if content is not None:
                for f in range(frames):
                    for j in range(self.rows[p]):
                        at = off + f * fb + j * rb
                        h[at:at + self.minRow[p]] = content[f][p][j]
            self.rowBytes.append(rb); self.frameBytes.append(fb); self.off.append(off); self.host.append(h)
            d = ar.new(h.size, h)
            if content is not None:
                ar.keep(d, h)
            self.bufs.append(d)
        self.desc = capi.Image(fmt, [ptr(b) + o for b, o in zip(self.bufs, self.off)], self.rowBytes, self.frameBytes)

    def read(self, what):
        """-> [frame][plane] dense planes; asserts that every byte that is no pixel still holds the sentinel"""
        out = [[None] * self.n for _ in range(self.F)]
        for p in range(self.n):
            h = self.bufs[p].cpu().numpy().copy()
            for f in range(self.F):
                rows = []
                for j in range(self.rows[p]):
                    at = self.off[p] + f * self.frameBytes[p] + j * self.rowBytes[p]
                    rows.append(h[at:at + self.minRow[p]].copy())
                    h[at:at + self.minRow[p]] = SENTINEL
                out[f][p] = np.stack(rows)
            assert (h == SENTINEL).all(), "%s: plane %d: %d bytes outside the pixels were written" % (what, p, int((h != SENTINEL).sum()))
        return out

    def untouched(self):
        return all((b.cpu().numpy() == SENTINEL).all() for b in self.bufs)


def run_pair(hip_ctx, src, dst, W, H, layout, frames=None, check=True):
    """src frames -> dst on the device in the given layout; returns [frame][plane]"""
    content = frames if frames is not None else source_frames(src, W, H)
    ar = Arena()
    a = DevImage(ar, src, W, H, len(content), layout, content)
    b = DevImage(ar, dst, W, H, len(content), layout)
    what = "%s %dx%d %s" % (cm.pair_name(src, dst), W, H, layout)
    with no_allocation(hip_ctx):
        hip_ctx.convert_frames(W, H, len(content), a.desc, b.desc)
        got = b.read(what)
    if check:
        ar.check(what)
    return got


def same(got, exp, what):
    assert len(got) == len(exp)
    for f, (gf, ef) in enumerate(zip(got, exp)):
        for p, (g, e) in enumerate(zip(gf, ef)):
            assert g.shape == e.shape and g.tobytes() == e.tobytes(), "%s: frame %d plane %d: %d bytes differ" % (what, f, p, int((g != e).sum()))


@pytest.mark.parametrize("pair", cm.SERVED, ids=PAIR_IDS)
def test_every_pair_in_every_layout(hip_ctx, golden, pair):
    """bit for bit against the model on 7 x 5, 33 x 17, 250 x 3 and 641 x 480, three frames: padded rowBytes (different per plane) and frameBytes, the
    sentinels in all padding and behind the last frame, every plane pointer moved by 1 byte, and the word arm"""
    src, dst = pair
    for W, H in SIZES:
        exp = model_frames(src, dst, W, H)
        g = golden["%s_noise%dx%d" % (cm.NAMES[src], W, H)]
        assert [md5(p) for p in exp[0]] == g["md5"][cm.NAMES[dst]]          # frame 0 is the golden case
        for layout in ("padded", "aligned", "shifted"):
            same(run_pair(hip_ctx, src, dst, W, H, layout), exp, "%s %dx%d %s" % (cm.pair_name(src, dst), W, H, layout))


@pytest.mark.parametrize("pair", cm.SERVED, ids=PAIR_IDS)
def test_4k_rows_take_the_word_arm(hip_ctx, pair):
    """3840 x 4: two workgroups per row, whole groups only, everything 16-byte aligned"""
    src, dst = pair
    r = np.random.RandomState(9000 + 31 * src + dst)
    frames = [[r.randint(0, 256, s).astype(np.uint8) for s in cm.plane_shapes(src, 3840, 4)]]
    same(run_pair(hip_ctx, src, dst, 3840, 4, "aligned", frames), [cm.convert(src, dst, frames[0], 3840, 4)], cm.pair_name(src, dst))
    same(run_pair(hip_ctx, src, dst, 3840, 4, "dense", frames), [cm.convert(src, dst, frames[0], 3840, 4)], cm.pair_name(src, dst))


@pytest.mark.parametrize("src,dst", [(cm.YUV444P, cm.RGBA32), (cm.YUV444P, cm.RGB24), (cm.RGB24, cm.HSV), (cm.RGB24, cm.YUV444P)], ids=lambda v: cm.NAMES[v])
def test_exhaustive_frames_equal_the_fixture(hip_ctx, golden, src, dst):
    """every (Y, U, V) / every (R, G, B) once -- every clamp, every entry of both HSV tables -- by MD5 against what the compiled reference gave"""
    c = cc.BY_ID["%s_exhaustive4096x4096" % cm.NAMES[src]]
    g = golden[c["id"]]
    assert g["checked"][cm.NAMES[dst]] == "reference"
    got = run_pair(hip_ctx, src, dst, 4096, 4096, "dense", [cc.case_planes(c)], check=False)
    assert [md5(p) for p in got[0]] == g["md5"][cm.NAMES[dst]]


def test_nv12_to_hsv_is_nv12_to_rgb24_to_hsv(hip_ctx):
    W, H = 641, 480
    frames = source_frames(cm.NV12, W, H)
    rgb = run_pair(hip_ctx, cm.NV12, cm.RGB24, W, H, "aligned", frames)
    two = run_pair(hip_ctx, cm.RGB24, cm.HSV, W, H, "padded", rgb)
    same(run_pair(hip_ctx, cm.NV12, cm.HSV, W, H, "aligned", frames), two, "NV12 -> HSV in one kernel and in two")


@pytest.mark.parametrize("pair", cm.IN_PLACE, ids=[cm.pair_name(s, d) for s, d in cm.IN_PLACE])
@pytest.mark.parametrize("layout", ["padded", "aligned"])
def test_in_place(hip_ctx, pair, layout):
    """the 3-byte-to-3-byte pairs on their own memory: same pointer, rowBytes and frameBytes"""
    from compv_amd import capi
    src, dst = pair
    for W, H in ((33, 17), (641, 480)):
        frames = source_frames(src, W, H)
        ar = Arena()
        a = DevImage(ar, src, W, H, FRAMES, layout, frames)
        ar.kept = []          # the input is rewritten
        out = capi.Image(dst, [a.desc.plane[0]], a.rowBytes, a.frameBytes)
        with no_allocation(hip_ctx):
            hip_ctx.convert_frames(W, H, FRAMES, a.desc, out)
        same(a.read("in place"), model_frames(src, dst, W, H), "%s in place, %s" % (cm.pair_name(src, dst), layout))
        ar.check("in place")


def test_refusals_write_nothing_and_name_their_reason(hip_ctx):
    from compv_amd import capi
    W, H = 16, 4
    ar = Arena()
    nv12 = DevImage(ar, cm.NV12, W, H, 2, "aligned", [[np.zeros(s, np.uint8) for s in cm.plane_shapes(cm.NV12, W, H)]] * 2)
    rgb = DevImage(ar, cm.RGB24, W, H, 2, "aligned", [[np.zeros(s, np.uint8) for s in cm.plane_shapes(cm.RGB24, W, H)]] * 2)
    rgba = DevImage(ar, cm.RGBA32, W, H, 2, "aligned")
    hsv = DevImage(ar, cm.HSV, W, H, 2, "aligned")
    yuv = DevImage(ar, cm.YUV444P, W, H, 2, "aligned")
    outs = (rgba, hsv, yuv)

    def image(d, **kw):
        """d's description with some fields replaced: fmt, plane / rowBytes / frameBytes as {index: value}"""
        im = capi.Image(kw.get("fmt", d.fmt), [d.desc.plane[p] for p in range(d.n)], d.rowBytes, d.frameBytes)
        for field in ("plane", "rowBytes", "frameBytes"):
            for i, v in kw.get(field, {}).items():
                getattr(im, field)[i] = v
        return im

    def refused(reason, src, dst, w=W, h=H, frames=2, code=capi.E_INVALID_PARAMETER):
        with no_allocation(hip_ctx):
            rc = hip_ctx.lib.compvhip_convert_frames(hip_ctx.h, w, h, frames, C.byref(src) if src is not None else None, C.byref(dst) if dst is not None else None, None)
        assert rc == code, (reason, rc)
        assert reason in hip_ctx.last_error(), (reason, hip_ctx.last_error())
        assert all(o.untouched() for o in outs), reason
        ar.check(reason)

    refused("not served", nv12.desc, image(rgb, fmt=capi.FMT_BGR24))          # YUV sources are not served to BGR outputs
    refused("not served", rgb.desc, image(hsv, fmt=capi.FMT_RGB24))
    refused("not served", image(hsv), rgba.desc)
    refused("not served", nv12.desc, image(rgba, fmt=capi.FMT_BGRA32))
    refused("unknown pixel format", nv12.desc, image(rgba, fmt=18))
    refused("unknown pixel format", image(nv12, fmt=-1), rgba.desc)
    refused("is 0", nv12.desc, rgba.desc, w=0)
    refused("is 0", nv12.desc, rgba.desc, h=0)
    refused("is 0", nv12.desc, rgba.desc, frames=0)
    refused("beyond 32767", nv12.desc, rgba.desc, w=32768)
    refused("beyond 32767", nv12.desc, rgba.desc, h=32768)
    refused("null image", None, rgba.desc)
    refused("null image", nv12.desc, None)
    refused("plane of the format is NULL", image(nv12, plane={1: None}), rgba.desc)
    refused("plane of the format is NULL", rgb.desc, image(yuv, plane={2: None}))
    refused("rowBytes below", image(nv12, rowBytes={1: W - 1}), rgba.desc)
    refused("rowBytes below", nv12.desc, image(rgba, rowBytes={0: 4 * W - 1}))
    refused("frames overlap", image(nv12, frameBytes={0: nv12.rowBytes[0] * (H - 1) + W - 1}), rgba.desc)
    refused("frames overlap", nv12.desc, image(rgba, frameBytes={0: 0}))
    # overlaps: an output plane inside an input plane, two output planes in each other, in place outside the 3-byte pairs or with other strides
    refused("overlaps an input plane", nv12.desc, image(rgba, plane={0: nv12.desc.plane[0] + 8}))
    refused("overlaps an input plane", image(rgb, fmt=capi.FMT_RGBA32, plane={0: rgba.desc.plane[0]}, rowBytes={0: rgba.rowBytes[0]}, frameBytes={0: rgba.frameBytes[0]}),
            image(hsv, plane={0: rgba.desc.plane[0]}, rowBytes={0: rgba.rowBytes[0]}, frameBytes={0: rgba.frameBytes[0]}))
    refused("two output planes overlap", rgb.desc, image(yuv, plane={1: yuv.desc.plane[0] + 1}))
    refused("in place needs", rgb.desc, image(hsv, plane={0: rgb.desc.plane[0] + 3}, rowBytes={0: rgb.rowBytes[0]}, frameBytes={0: rgb.frameBytes[0]}))
    refused("in place needs", rgb.desc, image(hsv, plane={0: rgb.desc.plane[0]}, rowBytes={0: rgb.rowBytes[0] - 16}, frameBytes={0: rgb.frameBytes[0]}))
    refused("in place needs", rgb.desc, image(hsv, plane={0: rgb.desc.plane[0]}, rowBytes={0: rgb.rowBytes[0]}, frameBytes={0: rgb.frameBytes[0] + 16}))
    # ... and the same descriptions are served once they are right
    hip_ctx.convert_frames(W, H, 2, nv12.desc, rgba.desc)
    same(rgba.read("served"), [cm.convert(cm.NV12, cm.RGBA32, [np.zeros(s, np.uint8) for s in cm.plane_shapes(cm.NV12, W, H)], W, H)] * 2, "served")


def test_old_calls_refuse_the_new_formats(hip_ctx):
    """every call that took a pixfmt before: the grayscale host and plan calls and the pipeline step"""
    import torch
    from compv_amd import capi
    W, H, S = 16, 8, 16
    packed = np.zeros((H, 4 * S), np.uint8)
    out = np.full((H, W), SENTINEL, np.uint8)
    plan = capi.Plan(hip_ctx, W, H, S, 1)
    try:
        d_in = torch.zeros(H * S * 4, dtype=torch.uint8, device="cuda:0")
        d_gray = torch.full((H * S,), SENTINEL, dtype=torch.uint8, device="cuda:0")
        d_lines = torch.zeros(64 * 20, dtype=torch.uint8, device="cuda:0")
        d_counts = torch.zeros(1, dtype=torch.int32, device="cuda:0")
        for fmt in (capi.FMT_NV12, capi.FMT_NV21, capi.FMT_YUV420P, capi.FMT_YUV422P, capi.FMT_YUV444P, capi.FMT_HSV):
            assert hip_ctx.lib.compvhip_grayscale_u8(hip_ctx.h, packed.ctypes.data, fmt, W, H, S, out.ctypes.data, W) == capi.E_INVALID_PARAMETER
            assert "colour conversion" in hip_ctx.last_error()
            with pytest.raises(capi.CompvHipError) as err:
                plan.grayscale(d_in.data_ptr(), fmt, d_gray.data_ptr())
            assert err.value.code == capi.E_INVALID_PARAMETER
            with pytest.raises(capi.CompvHipError) as err:
                plan.pipeline_ex(d_in.data_ptr(), 10.0, 20.0, 40, 0, d_gray.data_ptr(), d_lines.data_ptr(), 64, d_counts.data_ptr(), pixfmt=fmt)
            assert err.value.code == capi.E_INVALID_PARAMETER
        torch.cuda.synchronize()
        assert (out == SENTINEL).all() and bool((d_gray == SENTINEL).all()) and int(d_counts[0]) == 0
    finally:
        plan.close()


@pytest.mark.parametrize("pair", cm.SERVED, ids=PAIR_IDS)
def test_host_entry_equals_device_entry(hip_ctx, pair):
    """compvhip_convert_u8 on host planes with padded strides: the model's bytes (which the device entry gives), the host padding untouched"""
    from compv_amd import capi
    src, dst = pair
    for W, H in ((1, 1), (2, 2), (33, 17), (641, 480)):
        if (W, H) in SIZES:
            planes, exp = source_frames(src, W, H)[0], model_frames(src, dst, W, H)[0]
        else:
            planes = cc.case_planes(cc.BY_ID["%s_noise%dx%d" % (cm.NAMES[src], W, H)])
            exp = cm.convert(src, dst, planes, W, H)
        padded = []
        for i, p in enumerate(planes):
            h = np.full((p.shape[0], p.shape[1] + 3 + i), SENTINEL, np.uint8)
            h[:, :p.shape[1]] = p
            padded.append(h)
        views = [h[:, :p.shape[1]] for h, p in zip(padded, planes)]
        same([hip_ctx.convert(views, src, dst, W, H)], [exp], "host entry, dense output")
        # padded output rows, through the C call
        outs = [np.full((e.shape[0], e.shape[1] + 5 + i), SENTINEL, np.uint8) for i, e in enumerate(exp)]
        a = capi.Image(src, [h.ctypes.data for h in padded], [h.strides[0] for h in padded])
        b = capi.Image(dst, [o.ctypes.data for o in outs], [o.strides[0] for o in outs])
        with no_allocation(hip_ctx):          # the context's staging buffers hold this size since the call above
            hip_ctx._chk(hip_ctx.lib.compvhip_convert_u8(hip_ctx.h, W, H, C.byref(a), C.byref(b)))
        for o, e, h, p in zip(outs, exp, padded, planes):
            assert o[:, :e.shape[1]].tobytes() == e.tobytes() and (o[:, e.shape[1]:] == SENTINEL).all()
        for h, p in zip(padded, planes):
            assert h[:, :p.shape[1]].tobytes() == p.tobytes() and (h[:, p.shape[1]:] == SENTINEL).all()
    if (src, dst) in cm.IN_PLACE:          # host memory in place
        planes = source_frames(src, 33, 17)[0]
        buf = planes[0].copy()
        a = capi.Image(src, [buf.ctypes.data], [buf.strides[0]])
        b = capi.Image(dst, [buf.ctypes.data], [buf.strides[0]])
        hip_ctx._chk(hip_ctx.lib.compvhip_convert_u8(hip_ctx.h, 33, 17, C.byref(a), C.byref(b)))
        assert buf.tobytes() == model_frames(src, dst, 33, 17)[0][0].tobytes()


def test_65537_frames_are_sliced(hip_ctx):
    """65 537 frames of 2 x 2 NV12 -> RGBA32: two launches (65 535 + 2); every frame against its own model frame"""
    F, W, H = 65537, 2, 2
    r = np.random.RandomState(4242)
    y, uv = r.randint(0, 256, (F, 2, 2)).astype(np.uint8), r.randint(0, 256, (F, 1, 2)).astype(np.uint8)
    for layout in ("dense", "padded"):
        ar = Arena()
        a = DevImage(ar, cm.NV12, W, H, F, layout)
        b = DevImage(ar, cm.RGBA32, W, H, F, layout)
        for p, v in ((0, y), (1, uv)):          # the frames into the source's layout, vectorised (DevImage's loop is per row)
            h = a.host[p]
            rows = v.shape[1]
            idx = a.off[p] + np.arange(F)[:, None, None] * a.frameBytes[p] + np.arange(rows)[None, :, None] * a.rowBytes[p] + np.arange(2)[None, None, :]
            h[idx] = v
            a.bufs[p].copy_(ar.torch.from_numpy(h))
            ar.keep(a.bufs[p], h)
        with no_allocation(hip_ctx):
            hip_ctx.convert_frames(W, H, F, a.desc, b.desc)
        h = b.bufs[0].cpu().numpy()
        idx = b.off[0] + np.arange(F)[:, None, None] * b.frameBytes[0] + np.arange(2)[None, :, None] * b.rowBytes[0] + np.arange(8)[None, None, :]
        got = h[idx]
        # the model, frame by frame: the one chroma sample of a frame serves its four pixels
        u, v = uv[:, :, 0:1].astype(np.int32), uv[:, :, 1:2].astype(np.int32)
        rr, gg, bb = cm.yuv_to_rgb(y.astype(np.int32), u, v)
        exp = np.stack([rr, gg, bb, np.full_like(rr, 255)], axis=3).astype(np.uint8).reshape(F, 2, 8)
        assert got.tobytes() == exp.tobytes(), "%d frames differ, the first at %d" % (int((got != exp).any(axis=(1, 2)).sum()), int(np.argmax((got != exp).any(axis=(1, 2)))))
        h[idx] = SENTINEL
        assert (h == SENTINEL).all()
        ar.check("65 537 frames, " + layout)
        # a spot check of the vectorised expectation against the model's own convert()
        for f in (0, 65534, 65535, 65536):
            assert cm.convert(cm.NV12, cm.RGBA32, [y[f], uv[f]], W, H)[0].tobytes() == exp[f].tobytes()
