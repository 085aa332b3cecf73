"""Paragraph F of the remap definition (include/compv_hip.h, section "remap and inverse warp") in numpy: the bicubic interpolation of
CompVImageRemap::process and CompVImage::warpInverse as the reference's plain leaves compute it (compv_image_remap.cxx:293-310,
compv_image_scale_bicubic.cxx:34-101), bit for bit -- tests/golden/make_golden_bicubic.py asserts that against the compiled reference with its SIMD
flags off, on every element.

Every array below is float32 and every operator is numpy's float32 operator: one rounding per operation, nothing fused, no float64 anywhere.
Coordinates, the ROI and the inside test are those of tests/remap_model.py (a NaN is outside)."""
import numpy as np

import remap_model as rm

BICUBIC, BICUBIC_FLOAT32 = 4, 5
F32 = np.float32
_H, _1H, _2, _2H = F32(0.5), F32(1.5), F32(2.0), F32(2.5)


def hermite_row(A, B, C, D, t, t2, t3):
    """HERMITE4_32F_C: the four taps of a source row"""
    a = ((D - A) * _H) + ((B - C) * _1H)
    b = ((A + (B * -_2H)) + (C * _2)) + (D * -_H)
    c = (C - A) * _H
    return ((a * t3) + (c * t)) + ((b * t2) + B)


def hermite_col(A, B, C, D, t, t2, t3):
    """HERMITE1_32F_C: the four row values; another association of the same polynomial"""
    a = ((A * -_H) + (B * _1H)) + ((C * -_1H) + (D * _H))
    b = (A + (B * -_2H)) + ((C * _2) + (D * -_H))
    c = (A * -_H) + (C * _H)
    return ((a * t3) + (c * t)) + ((b * t2) + B)


def split(v):
    """-> (int part by truncation, t, t2, t3) of float32 coordinates v >= 0"""
    v = np.asarray(v, F32)
    t = v - np.floor(v)
    t2 = t * t
    return v.astype(np.int32), t, t2, t2 * t


def clip255(v):
    """COMPV_MATH_CLIP3(0, 255, v) by compares: a negative zero stays"""
    return np.where(v < F32(0), F32(0), np.where(v > F32(255), F32(255), v)).astype(F32)


def unclipped(img, xs, ys, row=hermite_row, col=hermite_col):
    """the value v of F for float32 coordinates inside the frame (1-D arrays)"""
    h_in, w_in = img.shape
    xi, xf, xf2, xf3 = split(xs)
    yi, yf, yf2, yf3 = split(ys)
    assert all(a.dtype == F32 for a in (xf, xf2, xf3, yf, yf2, yf3))
    xk = [np.clip(xi - 1 + k, 0, w_in - 1) for k in range(4)]
    yk = [np.clip(yi - 1 + k, 0, h_in - 1) for k in range(4)]
    c = [row(*(img[yk[r], xk[k]].astype(F32) for k in range(4)), xf, xf2, xf3) for r in range(4)]
    v = col(c[0], c[1], c[2], c[3], yf, yf2, yf3)
    assert v.dtype == F32
    return v


def inside_of(img, x, y, roi):
    h_in, w_in = img.shape
    left, right, top, bottom = rm.clip_roi(roi, w_in, h_in)
    with np.errstate(invalid="ignore"):
        return (x >= left) & (x <= right) & (y >= top) & (y <= bottom)


def remap(img, x, y, interp=BICUBIC, roi=None, default=0, row=hermite_row, col=hermite_col):
    """img (Hin, Win) uint8, x, y (Hout, Wout) float32 -> (Hout, Wout) uint8, or float32 for BICUBIC_FLOAT32"""
    assert img.dtype == np.uint8 and img.ndim == 2 and interp in (BICUBIC, BICUBIC_FLOAT32)
    x, y = np.asarray(x, F32), np.asarray(y, F32)
    inside = inside_of(img, x, y, roi)
    w = clip255(unclipped(img, x[inside], y[inside], row, col))
    if interp == BICUBIC_FLOAT32:
        out = np.full(x.shape, default, F32)
        out[inside] = w
    else:
        out = np.full(x.shape, default, np.uint8)
        out[inside] = w.astype(np.int32).astype(np.uint8)          # truncation
    return out


def warp_inverse(img, M, w_out, h_out, interp=BICUBIC, default=0):
    """CompVImage::warpInverse: the remap at the coordinates of the matrix, ROI = the whole frame"""
    x, y = rm.warp_coords(M, w_out, h_out)
    return remap(img, x, y, interp, None, default)
