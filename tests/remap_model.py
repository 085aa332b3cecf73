"""The definition of the remap and of the inverse warp (include/compv_hip.h, section "remap and inverse warp") in numpy: what
CompVImageRemap::process and CompVImage::warpInverse of the reference compute for float32 maps and matrices, bit for bit
(tests/golden/make_golden_remap.py asserts that against the compiled reference on every byte).

All arithmetic is float32 with one rounding per operation -- numpy's float32 operators do that -- except the three fused multiply-adds of the
bilinear value, which round once over product and sum.  fma32 computes them exactly: the product of two float32 is exact in float64, the
sum is then rounded to float64 and to float32, and that double rounding differs from the single one only where the float64 sum was inexact
and sits on a float32 rounding midpoint (or below the float32 normal range); exactly those elements are recomputed with fractions.Fraction."""
from fractions import Fraction

import numpy as np

NEAREST, BILINEAR, BILINEAR_FLOAT32 = 0, 1, 2
F32 = np.float32


def _round_fraction_to_f32(q):
    """the float32 nearest to the Fraction q, ties to even"""
    lo = F32(float(q))          # float(q) is correctly rounded to float64; its float32 is one of the two neighbours of q, or q itself
    cands = sorted({float(np.nextafter(lo, F32(-np.inf))), float(lo), float(np.nextafter(lo, F32(np.inf)))})
    best = min(cands, key=lambda c: (abs(Fraction(c) - q), int(np.array(c, F32).view(np.uint32)) & 1))
    return F32(best)


def fma32(a, b, c):
    """fma(a, b, c) in float32, one rounding, element-wise on float32 arrays of finite values"""
    a, b, c = (np.asarray(v, F32) for v in np.broadcast_arrays(a, b, c))
    prod = a.astype(np.float64) * b.astype(np.float64)          # exact: 24 + 24 bits
    c64 = c.astype(np.float64)
    s = prod + c64
    out = s.astype(F32)
    # was the float64 sum inexact?  (two-sum residual)
    bb = s - prod
    err = (prod - (s - bb)) + (c64 - bb)
    midpoint = (s.view(np.uint64) & np.uint64((1 << 29) - 1)) == np.uint64(1 << 28)
    tiny = np.abs(s) < 2.0 ** -120
    redo = np.flatnonzero(((err != 0) & midpoint) | (tiny & (s != 0)))
    if redo.size:
        out = out.copy()
        fa, fb, fc, fo = a.ravel(), b.ravel(), c.ravel(), out.reshape(-1)
        for k in redo:
            fo[k] = _round_fraction_to_f32(Fraction(float(fa[k])) * Fraction(float(fb[k])) + Fraction(float(fc[k])))
    fma32.redone += int(redo.size)
    return out


fma32.redone = 0          # elements that went through the exact path so far (the golden generator reports it)


def running_sum(first, step, n):
    """t[0] = first, t[k] = t[k - 1] + step: sequential float32 additions"""
    t = np.empty(n, F32)
    t[0] = F32(first)
    step = F32(step)
    for k in range(1, n):
        t[k] = t[k - 1] + step
    return t


def warp_tables(M, w_out, h_out):
    """-> (ac, df, gi, by, ey, hy) of a (2, 3) or (3, 3) float32 matrix; gi, hy are None for two rows (compv_image.cxx:1031-1048,1114-1137)"""
    M = np.asarray(M, F32)
    assert M.shape in ((2, 3), (3, 3))
    ac, df = running_sum(M[0, 2], M[0, 0], w_out), running_sum(M[1, 2], M[1, 0], w_out)
    by, ey = running_sum(0, M[0, 1], h_out), running_sum(0, M[1, 1], h_out)
    if M.shape[0] == 2:
        return ac, df, None, by, ey, None
    return ac, df, running_sum(M[2, 2], M[2, 0], w_out), by, ey, running_sum(0, M[2, 1], h_out)


def warp_coords(M, w_out, h_out):
    """the (h_out, w_out) float32 planes x, y of an inverse warp"""
    ac, df, gi, by, ey, hy = warp_tables(M, w_out, h_out)
    X, Y = ac[None, :] + by[:, None], df[None, :] + ey[:, None]
    if gi is None:
        return X, Y
    Z = gi[None, :] + hy[:, None]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        s = F32(1.0) / Z          # correctly rounded
        return X * s, Y * s


def clip_roi(roi, w_in, h_in):
    """compv_image_remap.cxx:346-360; roi = (left, right, top, bottom) or None -> the four float32"""
    w1, h1 = F32(w_in - 1), F32(h_in - 1)
    if roi is None:
        return F32(0), w1, F32(0), h1

    def clip3(lo, hi, v):          # COMPV_MATH_CLIP3
        return lo if v < lo else (hi if v > hi else v)
    left, right, top, bottom = (F32(v) for v in roi)
    left = clip3(F32(0), w1, left)
    right = clip3(left, w1, right)
    top = clip3(F32(0), h1, top)
    bottom = clip3(top, h1, bottom)
    return left, right, top, bottom


def remap(img, x, y, interp=BILINEAR, roi=None, default=0):
    """img (Hin, Win) uint8, x, y (Hout, Wout) float32 -> (Hout, Wout) uint8, or float32 for BILINEAR_FLOAT32"""
    assert img.dtype == np.uint8 and img.ndim == 2
    x, y = np.asarray(x, F32), np.asarray(y, F32)
    h_in, w_in = img.shape
    left, right, top, bottom = clip_roi(roi, w_in, h_in)
    with np.errstate(invalid="ignore"):
        inside = (x >= left) & (x <= right) & (y >= top) & (y <= bottom)
    f32_out = interp == BILINEAR_FLOAT32
    out = np.full(x.shape, default, F32 if f32_out else np.uint8)
    xs, ys = x[inside], y[inside]
    if interp == NEAREST:
        xi = (xs.astype(np.float64) + 0.5).astype(np.int64)
        yi = (ys.astype(np.float64) + 0.5).astype(np.int64)
        out[inside] = img[yi, xi]
        return out
    assert interp in (BILINEAR, BILINEAR_FLOAT32)
    one = F32(1.0)
    x1, y1 = xs.astype(np.int32), ys.astype(np.int32)          # truncation
    x2 = np.minimum((xs + one).astype(np.int32), w_in - 1)
    y2 = np.minimum((ys + one).astype(np.int32), h_in - 1)
    xf, yf = xs - x1.astype(F32), ys - y1.astype(F32)
    xy = xf * yf
    A, B, C = ((one - xf) - yf) + xy, xf - xy, yf - xy
    i11, i12, i21, i22 = (img[r, c].astype(F32) for r, c in ((y1, x1), (y1, x2), (y2, x1), (y2, x2)))
    p = fma32(i22, xy, fma32(i21, C, fma32(i12, B, i11 * A)))
    if f32_out:
        out[inside] = p
    else:
        assert ((p >= 0) & (p < 256)).all()
        out[inside] = p.astype(np.int32).astype(np.uint8)          # truncation
    return out


def warp_inverse(img, M, w_out, h_out, interp=BILINEAR, default=0):
    """CompVImage::warpInverse: the remap at the coordinates of the matrix, ROI = the whole frame"""
    x, y = warp_coords(M, w_out, h_out)
    return remap(img, x, y, interp, None, default)
