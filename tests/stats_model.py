"""The image statistics of include/compv_hip.h (section "image statistics") in numpy: integral images, histogram, equalisation, projections.

Everything is integer arithmetic but the equalisation table, which is two float32 operations on integers.  tests/golden/make_golden_stats.py holds these
functions against the compiled reference byte for byte; the device is held against them by bit pattern."""
import numpy as np

MAX_SIDE = 32767


def integral_dims(W, H):
    """(rows, cols) of the integral images of a W x H frame; ValueError where the library refuses"""
    if W < 1 or H < 1 or W > MAX_SIDE or H > MAX_SIDE or W * H >= 2 ** 31:
        raise ValueError("integral: %d x %d is refused" % (W, H))
    return H + 1, W + 1


def integral(img):
    """-> (sum, sumsq) float64 (H + 1, W + 1): sum[y][x] = the sum of p over y' < y, x' < x, sumsq the same of p * p.  int64 cumsum: exact."""
    p = np.asarray(img, np.uint8).astype(np.int64)
    rows, cols = integral_dims(p.shape[1], p.shape[0])
    s, q = np.zeros((rows, cols), np.int64), np.zeros((rows, cols), np.int64)
    s[1:, 1:] = np.cumsum(np.cumsum(p, 0), 1)
    q[1:, 1:] = np.cumsum(np.cumsum(p * p, 0), 1)
    assert q.max() < 2 ** 53
    return s.astype(np.float64), q.astype(np.float64)


def histogram(img):
    """-> uint32[256]"""
    return np.bincount(np.asarray(img, np.uint8).reshape(-1), minlength=256).astype(np.uint32)


def scale_f(scale, W, H):
    return np.float32(scale if scale > 0 else 255.0 / float(W * H))


def lut(hist, scale, W, H):
    """the equalisation table of a count vector: run = running sum modulo 2^32; v = float32(run) * scaleF, one rounding each; min(trunc(v), 255)"""
    run = (np.cumsum(np.asarray(hist).astype(np.uint64)) & np.uint64(0xffffffff)).astype(np.uint32)
    v = run.astype(np.float32) * scale_f(scale, W, H)          # uint32 -> float32 rounds to nearest even; float32 * float32 rounds once
    assert v.dtype == np.float32
    return np.minimum(np.trunc(v), np.float32(255)).astype(np.uint8)


def lut_unclamped_max(hist, scale, W, H):
    """the largest v of the table: parity with the reference holds only below 256"""
    run = (np.cumsum(np.asarray(hist).astype(np.uint64)) & np.uint64(0xffffffff)).astype(np.uint32)
    return float((run.astype(np.float32) * scale_f(scale, W, H)).max())


def equalize(img, hist=None, scale=0.0):
    """-> (out, lut); hist None: the frame's own"""
    img = np.asarray(img, np.uint8)
    t = lut(histogram(img) if hist is None else hist, scale, img.shape[1], img.shape[0])
    return t[img], t


def projections(img):
    """-> (projX int32[W] = column sums, projY int32[H] = row sums)"""
    p = np.asarray(img, np.uint8).astype(np.int64)
    return p.sum(0).astype(np.int32), p.sum(1).astype(np.int32)
