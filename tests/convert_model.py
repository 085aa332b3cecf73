"""numpy statement of the colour conversions of include/compv_hip.h ("colour conversion"): layout() and convert() for every served pair.

An image is a list of dense planes, each a 2-D uint8 array of rows[p] x minRowBytes[p] (layout()).  Nothing here looks at the library: the model is held
against the compiled reference by tests/golden/make_golden_convert.py and against plain loops by tests/test_convert_model.py."""
import numpy as np

(RGBA32, ARGB32, BGRA32, RGB24, BGR24, RGB565LE, RGB565BE, BGR565LE, BGR565BE, YUYV422, UYVY422, Y,
 NV12, NV21, YUV420P, YUV422P, YUV444P, HSV) = range(18)
NAMES = ["RGBA32", "ARGB32", "BGRA32", "RGB24", "BGR24", "RGB565LE", "RGB565BE", "BGR565LE", "BGR565BE", "YUYV422", "UYVY422", "Y",
         "NV12", "NV21", "YUV420P", "YUV422P", "YUV444P", "HSV"]
FORMATS = tuple(range(18))
YUV_SOURCES = (NV12, NV21, YUV420P, YUV422P, YUV444P, YUYV422, UYVY422)
RGB_FAMILY = (RGBA32, ARGB32, BGRA32, RGB24, BGR24, RGB565LE, RGB565BE, BGR565LE, BGR565BE)

# the served (source, destination) pairs, in the order of the header's list
SERVED = ([(s, d) for d in (RGBA32, RGB24) for s in YUV_SOURCES + (Y,)]
          + [(RGBA32, RGB24), (BGRA32, RGB24), (BGR24, RGB24), (RGBA32, BGR24), (RGB24, BGR24)]
          + [(RGB24, HSV), (RGBA32, HSV)] + [(s, HSV) for s in YUV_SOURCES]
          + [(s, YUV444P) for s in RGB_FAMILY])
IN_PLACE = ((RGB24, HSV), (RGB24, BGR24), (BGR24, RGB24))          # the 3-byte-to-3-byte pairs


def served(src, dst):
    return (src, dst) in SERVED


def pair_name(src, dst):
    return "%s_to_%s" % (NAMES[src], NAMES[dst])


def layout(fmt, W, H):
    """(planes, minRowBytes[3], rows[3]); ValueError for an unknown format or a zero size"""
    if fmt not in FORMATS or W < 1 or H < 1:
        raise ValueError("unknown format or zero size")
    cw, ch = (W + 1) // 2, (H + 1) // 2
    if fmt in (RGBA32, ARGB32, BGRA32):
        return 1, [4 * W, 0, 0], [H, 0, 0]
    if fmt in (RGB24, BGR24, HSV):
        return 1, [3 * W, 0, 0], [H, 0, 0]
    if fmt in (RGB565LE, RGB565BE, BGR565LE, BGR565BE):
        return 1, [2 * W, 0, 0], [H, 0, 0]
    if fmt in (YUYV422, UYVY422):
        return 1, [4 * cw, 0, 0], [H, 0, 0]
    if fmt == Y:
        return 1, [W, 0, 0], [H, 0, 0]
    if fmt in (NV12, NV21):
        return 2, [W, 2 * cw, 0], [H, ch, 0]
    if fmt == YUV420P:
        return 3, [W, cw, cw], [H, ch, ch]
    if fmt == YUV422P:
        return 3, [W, cw, cw], [H, H, H]
    return 3, [W, W, W], [H, H, H]


def plane_shapes(fmt, W, H):
    n, rb, rows = layout(fmt, W, H)
    return [(rows[p], rb[p]) for p in range(n)]


# ---- per-pixel arithmetic on int32 arrays -----------------------------------------------------------------------------------------------------------
def yuv_to_rgb(y, u, v):
    yp, up, vp = 37 * (y - 16), u - 127, v - 127          # 127: the reference's constant
    r = np.clip((yp + 51 * vp) >> 5, 0, 255)
    g = np.clip((yp - 13 * up - 26 * vp) >> 5, 0, 255)
    b = np.clip((yp + 65 * up) >> 5, 0, 255)
    return r, g, b


def rgb_to_yuv(r, g, b):
    y = ((33 * r + 65 * g + 13 * b) >> 7) + 16
    u = np.clip(((-38 * r - 74 * g + 112 * b) >> 8) + 128, 0, 255)
    v = np.clip(((112 * r - 94 * g - 18 * b) >> 8) + 128, 0, 255)
    return y, u, v


def hsv_tables():
    """t43[i] = 43 * (1 / i), t255[i] = 255 * (1 / i): a float32 division, then a float32 product (two roundings; 43 / i is another table), entry 0 = 0"""
    i = np.arange(256, dtype=np.float32)
    with np.errstate(divide="ignore"):
        rcp = (np.float32(1) / i).astype(np.float32)
        t43, t255 = np.float32(43) * rcp, np.float32(255) * rcp
    t43[0] = t255[0] = 0
    return t43.astype(np.float32), t255.astype(np.float32)


def _round(f32):
    d = f32.astype(np.float64)
    return np.where(d >= 0, d + 0.5, d - 0.5).astype(np.int64)          # astype truncates


def rgb_to_hsv(r, g, b):
    t43, t255 = hsv_tables()
    mn, mx = np.minimum(r, np.minimum(g, b)), np.maximum(r, np.maximum(g, b))
    is_r, is_g = mx == r, mx == g
    diff = np.where(is_r, g - b, np.where(is_g, b - r, r - g))
    minus = mx - mn
    s43 = diff.astype(np.float32) * t43[minus]
    s255 = minus.astype(np.float32) * t255[mx]
    h = ((_round(s43) & 255) + np.where(is_r, 0, np.where(is_g, 85, 171))) & 255
    s = _round(s255) & 255
    return h.astype(np.int32), s.astype(np.int32), mx


def _expand565(k):
    r = (k & 0xF800) >> 8
    r = r | (r >> 5)
    g = (k & 0x07E0) >> 3
    g = g | (g >> 6)
    b = (k & 0x001F) << 3
    b = b | (b >> 5)
    return r, g, b


def _up(c, W, H, sx, sy):
    """chroma plane -> one sample per pixel: pixel (x, y) reads (x >> sx, y >> sy)"""
    c = np.repeat(c, 1 << sx, axis=1) if sx else c
    c = np.repeat(c, 1 << sy, axis=0) if sy else c
    return c[:H, :W]


def unpack(fmt, planes, W, H):
    """-> ('yuv' | 'rgb' | 'y', c0, c1, c2) as int32 arrays of H x W"""
    shapes = plane_shapes(fmt, W, H)
    assert len(planes) == len(shapes) and all(p.dtype == np.uint8 and p.shape == s for p, s in zip(planes, shapes)), (fmt, [p.shape for p in planes], shapes)
    p = [q.astype(np.int32) for q in planes]
    cw = (W + 1) // 2
    if fmt in (RGBA32, ARGB32, BGRA32):
        q = p[0].reshape(H, W, 4)
        i = {RGBA32: (0, 1, 2), ARGB32: (1, 2, 3), BGRA32: (2, 1, 0)}[fmt]
        return "rgb", q[:, :, i[0]], q[:, :, i[1]], q[:, :, i[2]]
    if fmt in (RGB24, BGR24):
        q = p[0].reshape(H, W, 3)
        return ("rgb", q[:, :, 0], q[:, :, 1], q[:, :, 2]) if fmt == RGB24 else ("rgb", q[:, :, 2], q[:, :, 1], q[:, :, 0])
    if fmt in (RGB565LE, RGB565BE, BGR565LE, BGR565BE):
        q = p[0].reshape(H, W, 2)
        k = (q[:, :, 0] << 8 | q[:, :, 1]) if fmt in (RGB565BE, BGR565BE) else (q[:, :, 1] << 8 | q[:, :, 0])
        hi, mid, lo = _expand565(k)
        return ("rgb", hi, mid, lo) if fmt in (RGB565LE, RGB565BE) else ("rgb", lo, mid, hi)
    if fmt in (YUYV422, UYVY422):
        q = p[0].reshape(H, cw, 4)
        iy, iu, iv = ((0, 2), 1, 3) if fmt == YUYV422 else ((1, 3), 0, 2)
        y = q[:, :, iy].reshape(H, 2 * cw)[:, :W]
        return "yuv", y, _up(q[:, :, iu], W, H, 1, 0), _up(q[:, :, iv], W, H, 1, 0)
    if fmt == Y:
        return "y", p[0], None, None
    if fmt in (NV12, NV21):
        q = p[1].reshape(p[1].shape[0], cw, 2)
        u, v = (q[:, :, 0], q[:, :, 1]) if fmt == NV12 else (q[:, :, 1], q[:, :, 0])
        return "yuv", p[0], _up(u, W, H, 1, 1), _up(v, W, H, 1, 1)
    if fmt == YUV420P:
        return "yuv", p[0], _up(p[1], W, H, 1, 1), _up(p[2], W, H, 1, 1)
    if fmt == YUV422P:
        return "yuv", p[0], _up(p[1], W, H, 1, 0), _up(p[2], W, H, 1, 0)
    if fmt == YUV444P:
        return "yuv", p[0], p[1], p[2]
    raise ValueError("no source format %r" % (fmt,))


def convert(src, dst, planes, W, H):
    """the destination's dense planes for the source's dense planes"""
    if not served(src, dst):
        raise ValueError("pair not served")
    kind, c0, c1, c2 = unpack(src, planes, W, H)
    if kind == "yuv":
        r, g, b = yuv_to_rgb(c0, c1, c2)
    elif kind == "y":
        r = g = b = c0
    else:
        r, g, b = c0, c1, c2
    u8 = lambda *c: np.ascontiguousarray(np.stack(c, axis=2).astype(np.uint8).reshape(H, -1))          # noqa: E731
    if dst == RGBA32:
        return [u8(r, g, b, np.full_like(r, 255))]
    if dst == RGB24:
        return [u8(r, g, b)]
    if dst == BGR24:
        return [u8(b, g, r)]
    if dst == HSV:
        return [u8(*rgb_to_hsv(r, g, b))]
    return [np.ascontiguousarray(c.astype(np.uint8)) for c in rgb_to_yuv(r, g, b)]          # YUV444P
