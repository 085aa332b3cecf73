"""The lens distortion model of include/compv_hip.h ("lens undistortion", items A - F) in numpy: what CompVCalibUtils::initUndistMap, dist2DPoints, proj2D
and undist2DImage of the reference compute, bit for bit (tests/golden/make_golden_undistort.py asserts that against the compiled reference on every
element).

Every array and scalar below has the case's own dtype (float32 or float64) and every operator is numpy's operator of that dtype: one rounding per
operation, nothing fused, nothing widened.  The image form is tests/remap_model.py / tests/bicubic_model.py on the float32 map."""
import numpy as np

import bicubic_model as bm
import remap_model as rm

F32, F64 = np.float32, np.float64
NAMES = ("fx", "fy", "cx", "cy", "skew", "k1", "k2", "p1", "p2", "kinv11", "kinv21", "kinv31", "kinv22", "kinv32")          # the record's order


def coeffs(K, d, dtype=F32):
    """item A -> the record of 14 values of dtype, or None where fx * fy == 0"""
    T = np.dtype(dtype).type
    K, d = np.asarray(K, T), np.asarray(d, T).ravel()
    assert K.shape == (3, 3) and 2 <= d.size <= 4
    fx, skew, cx, fy, cy = K[0, 0], K[0, 1], K[0, 2], K[1, 1], K[1, 2]
    prod = fx * fy
    if prod == 0:
        return None
    det = T(1) / prod
    k1, k2 = d[0], d[1]
    p1 = d[2] if d.size > 2 else T(0)
    p2 = d[3] if d.size > 3 else T(0)
    kinv11 = fy * det
    kinv21 = -(skew * det)
    kinv31 = ((skew * cy) - (fy * cx)) * det
    kinv22 = fx * det
    kinv32 = -((cy * fx) * det)
    c = np.array([fx, fy, cx, cy, skew, k1, k2, p1, p2, kinv11, kinv21, kinv31, kinv22, kinv32], T)
    assert c.dtype == T
    return c


def distort(c, x, y):
    """item B on arrays x, y of c's dtype -> (u, v)"""
    T = c.dtype.type
    fx, fy, cx, cy, skew, k1, k2, p1, p2 = c[:9]
    one, two = T(1), T(2)
    x, y = np.asarray(x, T), np.asarray(y, T)
    with np.errstate(over="ignore", invalid="ignore"):
        x2, y2 = x * x, y * y
        r2 = x2 + y2
        r4 = r2 * r2
        rdist = (one + k1 * r2) + k2 * r4
        x, y = x * rdist, y * rdist
        a1 = two * (x * y)
        a2, a3 = r2 + two * x2, r2 + two * y2
        x = x + ((p1 * a1) + (p2 * a2))
        y = y + ((p1 * a3) + (p2 * a1))
        u = ((x * fx) + (skew * y)) + cx
        v = (y * fy) + cy
    assert u.dtype == T and v.dtype == T
    return u, v


def entry(c, X, Y):
    """items C and D: Kinv, then B; X, Y arrays (broadcast against each other) of c's dtype"""
    T = c.dtype.type
    kinv11, kinv21, kinv31, kinv22, kinv32 = c[9:]
    X, Y = np.asarray(X, T), np.asarray(Y, T)
    x = ((kinv11 * X) + (kinv21 * Y)) + kinv31
    y = (kinv22 * Y) + kinv32
    x, y = np.broadcast_arrays(x, y)
    return distort(c, x, y)


def map_planes(K, d, w_out, h_out, x0=0, y0=0, dtype=F32):
    """initUndistMap: the (h_out, w_out) planes mapX, mapY of dtype for the window at origin (x0, y0)"""
    T = np.dtype(dtype).type
    c = coeffs(K, d, T)
    X = (x0 + np.arange(w_out)).astype(T)[None, :]
    Y = (y0 + np.arange(h_out)).astype(T)[:, None]
    u, v = entry(c, X, Y)
    return np.ascontiguousarray(u), np.ascontiguousarray(v)


def dist_points(K, d, pts, dtype=None):
    """dist2DPoints: pts (n, 2) -> (n, 2) of the points' dtype"""
    pts = np.asarray(pts)
    T = np.dtype(dtype or pts.dtype).type
    u, v = entry(coeffs(K, d, T), pts[:, 0].astype(T), pts[:, 1].astype(T))
    return np.stack([u, v], axis=1)


def proj2d(K, d, R, t, pts):
    """proj2D: pts (n, 3) float64 under the pose R (3, 3), t (3,) -> (n, 2) float64; z == 0 keeps x and y"""
    c = coeffs(K, d, F64)
    R, t, pts = np.asarray(R, F64).reshape(3, 3), np.asarray(t, F64).ravel(), np.asarray(pts, F64)
    xp, yp, zp = pts[:, 0], pts[:, 1], pts[:, 2]
    x = ((R[0, 0] * xp + R[0, 1] * yp) + R[0, 2] * zp) + t[0]
    y = ((R[1, 0] * xp + R[1, 1] * yp) + R[1, 2] * zp) + t[1]
    z = ((R[2, 0] * xp + R[2, 1] * yp) + R[2, 2] * zp) + t[2]
    with np.errstate(divide="ignore"):
        s = np.where(z != 0, F64(1.0) / np.where(z != 0, z, F64(1.0)), F64(1.0))
    u, v = distort(c, x * s, y * s)
    return np.stack([u, v], axis=1)


INTERPS = (rm.NEAREST, rm.BILINEAR, rm.BILINEAR_FLOAT32, bm.BICUBIC, bm.BICUBIC_FLOAT32)
INTERP_NAMES = {rm.NEAREST: "nearest", rm.BILINEAR: "bilinear", rm.BILINEAR_FLOAT32: "bilinear_f32", bm.BICUBIC: "bicubic", bm.BICUBIC_FLOAT32: "bicubic_f32"}


def remap_on(img, mx, my, interp, roi=None, default=0):
    """item F on given float32 planes"""
    if interp in (bm.BICUBIC, bm.BICUBIC_FLOAT32):
        return bm.remap(img, mx, my, interp, roi, default)
    return rm.remap(img, mx, my, interp, roi, default)


def undistort(img, K, d, w_out=None, h_out=None, x0=0, y0=0, interp=rm.BILINEAR, roi=None, default=0):
    """undist2DImage: img (Hin, Win) uint8 -> the (h_out, w_out) window, uint8 or float32"""
    h, w = img.shape
    mx, my = map_planes(K, d, w if w_out is None else w_out, h if h_out is None else h_out, x0, y0, F32)
    return remap_on(img, mx, my, interp, roi, default)


def outside_share(img_w, img_h, mx, my, roi=None):
    left, right, top, bottom = rm.clip_roi(roi, img_w, img_h)
    with np.errstate(invalid="ignore"):
        return 1.0 - float(((mx >= left) & (mx <= right) & (my >= top) & (my <= bottom)).mean())
