"""CPU tests of tests/convert_model.py, the numpy statement of the colour conversions: against plain Python loops written from the header's definition on the
tiny sizes, against every fixture of tests/golden/golden_convert.* (what tests/golden/make_golden_convert.py held against the compiled reference), and
against hand-worked literals."""
import struct

import numpy as np
import pytest

import convert_cases as cc
import convert_model as cm
from fixtures import load_golden, md5


@pytest.fixture(scope="module")
def golden():
    return load_golden("golden_convert")


# ---- plain loops: one pixel at a time, Python ints, float32 through struct -----------------------------------------------------------------------------
def f32(v):
    return struct.unpack("<f", struct.pack("<f", v))[0]          # one rounding to binary32 (the operands here are exact in float64)


def clamp8(v):
    return 0 if v < 0 else (255 if v > 255 else v)


def loop_yuv_to_rgb(y, u, v):
    yp, up, vp = y - 16, u - 127, v - 127
    return clamp8((37 * yp + 51 * vp) >> 5), clamp8((37 * yp - 13 * up - 26 * vp) >> 5), clamp8((37 * yp + 65 * up) >> 5)


def loop_round(f):
    return int(f + 0.5) if f >= 0 else int(f - 0.5)          # int() truncates


def loop_rgb_to_hsv(r, g, b):
    mx, mn = max(r, g, b), min(r, g, b)
    diff, add = (g - b, 0) if mx == r else ((b - r, 85) if mx == g else (r - g, 171))
    minus = mx - mn
    t43 = f32(43.0 * f32(1.0 / minus)) if minus else 0.0          # a product of two binary32 values is exact in float64: f32() rounds it once
    t255 = f32(255.0 * f32(1.0 / mx)) if mx else 0.0
    h = ((loop_round(f32(diff * t43)) & 255) + add) & 255
    return h, loop_round(f32(minus * t255)) & 255, mx


def loop_rgb_to_yuv(r, g, b):
    return ((33 * r + 65 * g + 13 * b) >> 7) + 16, clamp8(((-38 * r - 74 * g + 112 * b) >> 8) + 128), clamp8(((112 * r - 94 * g - 18 * b) >> 8) + 128)


def loop_source_pixel(src, planes, x, y):
    """-> ('yuv' | 'rgb' | 'y', channels) of pixel (x, y), read from the dense planes byte by byte"""
    p = [[int(v) for v in q.reshape(-1)] for q in planes]
    rb = [q.shape[1] for q in planes]
    at = lambda pl, row, byte: p[pl][row * rb[pl] + byte]          # noqa: E731
    if src in (cm.RGBA32, cm.ARGB32, cm.BGRA32):
        o = {cm.RGBA32: (0, 1, 2), cm.ARGB32: (1, 2, 3), cm.BGRA32: (2, 1, 0)}[src]
        return "rgb", tuple(at(0, y, 4 * x + k) for k in o)
    if src in (cm.RGB24, cm.BGR24):
        o = (0, 1, 2) if src == cm.RGB24 else (2, 1, 0)
        return "rgb", tuple(at(0, y, 3 * x + k) for k in o)
    if src in (cm.RGB565LE, cm.RGB565BE, cm.BGR565LE, cm.BGR565BE):
        b0, b1 = at(0, y, 2 * x), at(0, y, 2 * x + 1)
        k = (b0 << 8 | b1) if src in (cm.RGB565BE, cm.BGR565BE) else (b1 << 8 | b0)
        hi, mid, lo = (k >> 11) & 31, (k >> 5) & 63, k & 31
        hi, mid, lo = hi << 3 | hi >> 2, mid << 2 | mid >> 4, lo << 3 | lo >> 2          # bit replication
        return "rgb", ((hi, mid, lo) if src in (cm.RGB565LE, cm.RGB565BE) else (lo, mid, hi))
    if src == cm.YUYV422:
        return "yuv", (at(0, y, 2 * x), at(0, y, 4 * (x >> 1) + 1), at(0, y, 4 * (x >> 1) + 3))
    if src == cm.UYVY422:
        return "yuv", (at(0, y, 2 * x + 1), at(0, y, 4 * (x >> 1)), at(0, y, 4 * (x >> 1) + 2))
    if src == cm.Y:
        return "y", (at(0, y, x),)
    if src == cm.NV12:
        return "yuv", (at(0, y, x), at(1, y >> 1, 2 * (x >> 1)), at(1, y >> 1, 2 * (x >> 1) + 1))
    if src == cm.NV21:
        return "yuv", (at(0, y, x), at(1, y >> 1, 2 * (x >> 1) + 1), at(1, y >> 1, 2 * (x >> 1)))
    if src == cm.YUV420P:
        return "yuv", (at(0, y, x), at(1, y >> 1, x >> 1), at(2, y >> 1, x >> 1))
    if src == cm.YUV422P:
        return "yuv", (at(0, y, x), at(1, y, x >> 1), at(2, y, x >> 1))
    return "yuv", (at(0, y, x), at(1, y, x), at(2, y, x))


def loop_convert(src, dst, planes, W, H):
    out = [np.zeros(s, np.uint8) for s in cm.plane_shapes(dst, W, H)]
    for y in range(H):
        for x in range(W):
            kind, c = loop_source_pixel(src, planes, x, y)
            r, g, b = loop_yuv_to_rgb(*c) if kind == "yuv" else ((c[0],) * 3 if kind == "y" else c)
            if dst == cm.RGBA32:
                out[0][y, 4 * x:4 * x + 4] = (r, g, b, 255)
            elif dst == cm.RGB24:
                out[0][y, 3 * x:3 * x + 3] = (r, g, b)
            elif dst == cm.BGR24:
                out[0][y, 3 * x:3 * x + 3] = (b, g, r)
            elif dst == cm.HSV:
                out[0][y, 3 * x:3 * x + 3] = loop_rgb_to_hsv(r, g, b)
            else:
                for k, v in enumerate(loop_rgb_to_yuv(r, g, b)):
                    out[k][y, x] = v
    return out


TINY = [c for c in cc.CASES if c["W"] * c["H"] <= 35]          # 1 x 1, 2 x 2, 7 x 5, 16 x 2


@pytest.mark.parametrize("src", cc.SOURCES, ids=[cm.NAMES[s] for s in cc.SOURCES])
def test_model_equals_plain_loops(src):
    n = 0
    for c in TINY:
        if c["src"] != src:
            continue
        planes = cc.case_planes(c)
        for dst in cc.destinations(src):
            got, exp = cm.convert(src, dst, planes, c["W"], c["H"]), loop_convert(src, dst, planes, c["W"], c["H"])
            assert len(got) == len(exp) and all(g.dtype == np.uint8 and g.tobytes() == e.tobytes() for g, e in zip(got, exp)), (c["id"], cm.NAMES[dst])
            n += 1
    assert n >= 6


def test_hsv_loops_on_every_table_entry():
    """the loops and the model on triples that reach every max and every minus, both signs of the hue"""
    rgb = np.array([(mx, mn, (mx + mn) // 2) for mx in range(256) for mn in range(0, mx + 1, 7)] + [(0, d, 255 - d) for d in range(256)] + [(d, 255, 0) for d in range(256)], np.int32)
    h, s, v = cm.rgb_to_hsv(rgb[:, 0], rgb[:, 1], rgb[:, 2])
    for i, (r, g, b) in enumerate(rgb.tolist()):
        assert (int(h[i]), int(s[i]), int(v[i])) == loop_rgb_to_hsv(r, g, b), (r, g, b)


def test_model_equals_every_fixture(golden):
    meta, arrays = golden
    by_id = {c["id"]: c for c in meta["cases"]}
    assert sorted(by_id) == sorted(cc.BY_ID)
    seen = set()
    for c in cc.CASES:
        g = by_id[c["id"]]
        planes = cc.case_planes(c)
        assert [md5(p) for p in planes] == g["frame_md5"], c["id"]
        assert sorted(g["md5"]) == sorted(cm.NAMES[d] for d in cc.destinations(c["src"]))
        for dst in cc.destinations(c["src"]):
            out = cm.convert(c["src"], dst, planes, c["W"], c["H"])
            assert [md5(p) for p in out] == g["md5"][cm.NAMES[dst]], (c["id"], cm.NAMES[dst])
            if g["stored"]:
                for i, p in enumerate(out):
                    a = arrays[cc.key(c, dst, i)]
                    assert a.dtype == np.uint8 and a.shape == p.shape and a.tobytes() == p.tobytes()
                    seen.add(cc.key(c, dst, i))
    assert seen == set(arrays.files)


def test_fixture_is_reference_checked(golden):
    """only odd-sized cases may be model only; every even-sized case and both exhaustive frames carry the compiled reference's verdict"""
    meta, _ = golden
    for c in meta["cases"]:
        for dst, how in c["checked"].items():
            assert how == "reference" or (how.startswith("model only: ") and ((c["W"] | c["H"]) & 1)), (c["id"], dst, how)
    assert sum(1 for c in meta["cases"] if c["kind"] == "exhaustive") == 2
    assert set(meta["simd_agrees"]) == {cm.pair_name(s, d) for s, d in cm.SERVED if d != cm.HSV}
    assert meta["hsv_simd"]["triples"] == 1 << 24


def test_served_pairs():
    assert len(cm.SERVED) == len(set(cm.SERVED)) == 39
    assert not any(cm.served(s, d) for s in cm.YUV_SOURCES for d in (cm.BGR24, cm.BGRA32))          # the reference mislabels those
    assert not cm.served(cm.Y, cm.HSV) and not cm.served(cm.HSV, cm.RGB24) and not cm.served(cm.RGB24, cm.RGB24)
    assert all(cm.served(s, d) for s, d in cm.IN_PLACE)


def one(src, dst, px):
    """one pixel through the model: px = the source's bytes"""
    return [int(v) for v in cm.convert(src, dst, [np.array([[c]], np.uint8) for c in px] if src == cm.YUV444P else [np.array([px], np.uint8)], 1, 1)[0].reshape(-1)]


def test_hand_worked_literals():
    yuv = lambda y, u, v: one(cm.YUV444P, cm.RGB24, (y, u, v))          # noqa: E731
    assert yuv(16, 127, 127) == [0, 0, 0]
    assert yuv(235, 127, 127) == [253, 253, 253]                       # 37 * 219 = 8103, >> 5 = 253
    assert yuv(235, 255, 255) == [255, 97, 255]                        # R = (8103 + 6528) >> 5 = 457 -> 255; G = (8103 - 1664 - 3328) >> 5 = 97; B = (8103 + 8320) >> 5 -> 255
    assert yuv(16, 0, 0) == [0, 154, 0]                                # R = -6477 >> 5 = -203 -> 0; G = (1651 + 3302) >> 5 = 154; B = -8255 >> 5 = -258 -> 0
    assert one(cm.YUV444P, cm.RGBA32, (16, 127, 127)) == [0, 0, 0, 255]
    assert one(cm.Y, cm.RGBA32, (77,)) == [77, 77, 77, 255]
    hsv = lambda r, g, b: one(cm.RGB24, cm.HSV, (r, g, b))             # noqa: E731
    assert hsv(255, 0, 0) == [0, 255, 255]
    assert hsv(0, 255, 0) == [85, 255, 255]
    assert hsv(0, 0, 255) == [171, 255, 255]
    assert hsv(128, 128, 128) == [0, 0, 128]
    assert hsv(0, 0, 0) == [0, 0, 0]
    assert hsv(255, 0, 255) == [213, 255, 255]                         # max == r first: diff = g - b = -255, round(-43) = -43 -> 213 as uint8, + 0
    assert hsv(90, 0, 30) == [242, 255, 90]                            # diff = -30, minus = 90: -14.33 -> -14 -> 242 as uint8
    assert one(cm.RGB24, cm.YUV444P, (255, 255, 255)) == [237]         # plane 0 of three: Y = (111 * 255 >> 7) + 16 = 221 + 16
    assert one(cm.RGB24, cm.BGR24, (1, 2, 3)) == [3, 2, 1]
