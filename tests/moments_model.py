"""The definition of the image moments (include/compv_hip.h, "image moments") restated: the six raw sums in Python integers -- exact whatever their size --
and the shape record (item D) in numpy float64, one rounding per operation.  tests/golden/make_golden_moments.py pins this model against the compiled
reference (CompVMathMoments); the CPU and GPU tests hold the library against the model and the fixture.

A raw record is a tuple of six Python integers in the reference's order: m00, m01, m10, m11, m02, m20."""
import numpy as np

from curvefit_model import half_angle

VALUE, UNIT = 0, 1
ORIGIN_FRAME, ORIGIN_BOX = 0, 1
NAMES = ("m00", "m01", "m10", "m11", "m02", "m20")
SHAPE_NAMES = ("xbar", "ybar", "u20", "u02", "u11", "skew", "cs", "sn")
EPS = np.finfo(np.float64).eps          # DBL_EPSILON
MAX_SIDE = 32767


def fits(w, h, weights):
    """item B and the other refusals of a size"""
    if weights not in (VALUE, UNIT) or not (1 <= w <= MAX_SIDE and 1 <= h <= MAX_SIDE) or w * h >= 2 ** 31:
        return False
    return (255 if weights == VALUE else 1) * w * h * max(w - 1, h - 1) ** 2 < 2 ** 64


def pixel_weights(plane, weights):
    """(H, W) uint8 -> int64 weights"""
    plane = np.asarray(plane)
    return (plane != 0).astype(np.int64) if weights == UNIT else plane.astype(np.int64)


def raw_sums_slow(plane, weights=VALUE):
    """item A pixel by pixel in Python integers: the definition itself (small planes only)"""
    m = [0] * 6
    for j, row in enumerate(np.asarray(plane).tolist()):
        for i, p in enumerate(row):
            w = (1 if p else 0) if weights == UNIT else p
            m[0] += w; m[1] += j * w; m[2] += i * w; m[3] += i * j * w; m[4] += j * j * w; m[5] += i * i * w
    return tuple(m)


def weighted_sums(w, x_origin=0, y_origin=0):
    """item A of an int64 weight plane whose element (j, i) sits at column x_origin + i, row y_origin + j.  A row's three sums stay below 2^63 for every
    size the calls accept (32767 columns: 255 * 32767^3 / 3 < 2^53); the rows are added up in Python integers."""
    w = np.asarray(w, np.int64)
    i = np.arange(w.shape[1], dtype=np.int64) + x_origin
    s0, s1, s2 = w.sum(axis=1).tolist(), (w * i).sum(axis=1).tolist(), (w * (i * i)).sum(axis=1).tolist()
    m = [0] * 6
    for r, (a, b, c) in enumerate(zip(s0, s1, s2)):
        j = y_origin + r
        m[0] += a; m[1] += j * a; m[2] += b; m[3] += j * b; m[4] += j * j * a; m[5] += c
    return tuple(m)


def raw_sums(plane, weights=VALUE):
    """item A of an (H, W) uint8 plane"""
    return weighted_sums(pixel_weights(plane, weights))


def component_sums(labels, comps, count, cap, gray=None, weights=VALUE, origin=ORIGIN_FRAME):
    """item E for one frame: labels (H, W) int32 (the columns below W only), comps: the records (x0 and y0 are read with ORIGIN_BOX), count: the frame's
    count -> the raw records of the ids 1 .. min(max(count, 0), cap), a list of tuples"""
    labels = np.asarray(labels)
    bound = min(max(int(count), 0), cap)
    out = []
    for cid in range(1, bound + 1):
        mask = labels == cid
        w = mask.astype(np.int64) if gray is None else pixel_weights(gray, weights) * mask
        ox, oy = (int(comps[cid - 1]["x0"]), int(comps[cid - 1]["y0"])) if origin == ORIGIN_BOX else (0, 0)
        out.append(weighted_sums(w, -ox, -oy))
    return out


def crop_of(labels, comp, cid, gray=None, weights=VALUE):
    """the blob's crop with every foreign pixel zeroed, as uint8: what the reference is run on for ORIGIN_BOX"""
    x0, y0, x1, y1 = (int(comp[k]) for k in ("x0", "y0", "x1", "y1"))
    mask = np.asarray(labels)[y0:y1 + 1, x0:x1 + 1] == cid
    if gray is None:
        return mask.astype(np.uint8)
    return (pixel_weights(np.asarray(gray)[y0:y1 + 1, x0:x1 + 1], weights) * mask).astype(np.uint8)


def shape(m):
    """item D of one raw record -> dict of SHAPE_NAMES (numpy float64) and status"""
    f = np.float64
    zero = {k: f(0.0) for k in SHAPE_NAMES}
    if m[0] == 0:
        return dict(zero, cs=f(1.0), status=1)
    M00, M01, M10, M11, M02, M20 = (f(int(v)) for v in m)          # Python rounds an integer to the nearest double, ties to even
    scale = f(1.0) / M00
    ybar, xbar = M01 * scale, M10 * scale
    u20 = (M20 * scale) - (xbar * xbar)
    u02 = (M02 * scale) - (ybar * ybar)
    u11 = (M11 * scale) - (xbar * ybar)
    den = u20 - u02
    cs, sn = half_angle(f(2.0) * u11, den) if abs(den) > EPS else (f(1.0), f(0.0))
    a = M02 - (ybar * M01)
    b = M11 - (xbar * M01)
    skew = b / a if abs(a) > EPS else f(0.0)
    return {"xbar": xbar, "ybar": ybar, "u20": u20, "u02": u02, "u11": u11, "skew": f(skew), "cs": f(cs), "sn": f(sn), "status": 0}


def theta(s):
    """the reference's theta: the angle of (cs, sn)"""
    return float(np.arctan2(s["sn"], s["cs"]))


def angle_case(s):
    """the -0 branch of atan2 plays no part: 2 * u11 != 0 or den > 0 (and the record has an orientation at all)"""
    den = s["u20"] - s["u02"]
    return s["status"] == 0 and abs(den) > EPS and (s["u11"] != 0.0 or den > 0.0)


def raw_array(records):
    """tuples -> (n, 6) uint64"""
    return np.array([[int(v) for v in r] for r in records], dtype=np.uint64).reshape(-1, 6)


def shape_array(records, dtype):
    """the shape records of raw tuples as a structured array of `dtype` (capi.MOMENTS_SHAPE_DTYPE)"""
    out = np.zeros(len(records), dtype)
    for k, r in enumerate(records):
        s = shape(r)
        for name in SHAPE_NAMES:
            out[k][name] = s[name]
        out[k]["status"] = s["status"]
    return out
