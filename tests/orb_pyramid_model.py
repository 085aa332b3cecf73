"""The definition of the bilinear scale and the ORB scale pyramid (include/compv_hip.h, sections A - D; docs/kernels/scale.md, docs/kernels/orb.md) in
numpy: the fixed-point scaler of CompVImageScaleBilinear, the level geometry and quotas of CompVImageScalePyramid / CompVCornerDeteORB::processLevelAt,
detection per level (fast_model, orb_model) with the lists concatenated in level order, and description of every keypoint on the plane of its own level."""
import numpy as np

import fast_model as fm
import orb_model as om

F32 = np.float32
MIN_SIDE = 2 * om.BORDER + 1          # 37: a smaller level is empty
MAX_LEVELS = 16


# ---- A. bilinear scale ---------------------------------------------------------------------------------------------------------------------
def scale_steps(w_in, h_in, w_out, h_out):
    """(sx, sy), or None when a ratio lies outside (0, 256) or a size is 0"""
    if min(w_in, h_in, w_out, h_out) < 1:
        return None
    fx, fy = F32(w_in) / F32(w_out), F32(h_in) / F32(h_out)
    if not (0 < fx < 256 and 0 < fy < 256):
        return None
    return int(fx * F32(256.0)), int(fy * F32(256.0))


def reads_inside(w_in, h_in, w_out, h_out):
    """does rule 3 stay inside the plane without the clamp (every strict downscale does)"""
    sx, sy = scale_steps(w_in, h_in, w_out, h_out)
    return (((w_out - 1) * sx) >> 8) + 1 <= w_in - 1 and (((h_out - 1) * sy) >> 8) + 1 <= h_in - 1


def scale(img, w_out, h_out):
    """-> the (h_out, w_out) plane; the source's own size is a copy"""
    h_in, w_in = img.shape
    if (w_out, h_out) == (w_in, h_in):
        return img.copy()
    st = scale_steps(w_in, h_in, w_out, h_out)
    assert st is not None, "ratio outside (0, 256)"
    sx, sy = st
    x = np.arange(w_out, dtype=np.uint32) * np.uint32(sx)
    y = np.arange(h_out, dtype=np.uint32) * np.uint32(sy)
    nx, ny = (x >> 8).astype(np.int64), (y >> 8).astype(np.int64)
    x0, y0 = (x & 255)[None, :], (y & 255)[:, None]
    x1, y1 = 255 - x0, 255 - y0
    c0, c1 = np.minimum(nx, w_in - 1), np.minimum(nx + 1, w_in - 1)
    r0, r1 = np.minimum(ny, h_in - 1), np.minimum(ny + 1, h_in - 1)
    src = img.astype(np.uint32)
    A = src[r0][:, c0] * x1 + src[r0][:, c1] * x0
    B = src[r1][:, c0] * x1 + src[r1][:, c1] * x0
    return ((((y1 * A) >> 16) + ((y0 * B) >> 16)) & 255).astype(np.uint8)


# ---- B. geometry, C.2 quotas ---------------------------------------------------------------------------------------------------------------
def scale_factors(levels, scale_factor):
    """(sf[0 .. levels - 1] float32, sfs float32), accumulated as the reference's constructor does"""
    f = F32(scale_factor)
    sf, sfs, run = [F32(1.0)], F32(1.0), f
    for _ in range(1, levels):
        sf.append(run)
        sfs = F32(sfs + run)
        run = F32(run * f)
    return np.array(sf, F32), sfs


def geometry(W, H, levels=8, scale_factor=0.83, max_features=2000):
    """-> list of dicts {W, H, S, scale, quota, empty}; S = W rounded up to 8 (level 0: the caller's), 0 for an empty level; quota 0 = no cut"""
    assert 1 <= levels <= MAX_LEVELS and 0 < scale_factor < 1 and W >= MIN_SIDE and H >= MIN_SIDE
    sf, sfs = scale_factors(levels, scale_factor)
    out = []
    for l in range(levels):
        w, h = (W, H) if l == 0 else (int(F32(W) * sf[l]), int(F32(H) * sf[l]))
        quota = 0
        if max_features > 0:
            nf = F32(F32(max_features) / sfs) * sf[l]
            quota = max(10, int(np.float64(nf) + 0.5))
        empty = w < MIN_SIDE or h < MIN_SIDE
        out.append({"W": w, "H": h, "S": 0 if empty else (w + 7) // 8 * 8, "scale": sf[l], "quota": quota, "empty": empty})
    return out


def planes(img, geo):
    """the level planes (None for an empty level); level 0 is the frame itself"""
    return [None if g["empty"] else (img if l == 0 else scale(img, g["W"], g["H"])) for l, g in enumerate(geo)]


# ---- C. detection, D. description ----------------------------------------------------------------------------------------------------------
def detect(img, levels=8, scale_factor=0.83, threshold=20, fast_type=9, nonmax=True, max_features=2000, corner_cap=None):
    """-> (keypoints KEYPOINT_DTYPE in level order, survivors per level, FAST count per level after the cut, the level planes).  corner_cap: a level's
    corner list is truncated to its raster prefix of that length."""
    H, W = img.shape
    geo = geometry(W, H, levels, scale_factor, max_features)
    pl = planes(img, geo)
    keys, level_counts, level_corners = [], [], []
    for l, (g, p) in enumerate(zip(geo, pl)):
        if p is None:
            level_counts.append(0); level_corners.append(0)
            continue
        corners, _ = fm.fast(p, threshold, fast_type, nonmax, g["quota"] if max_features > 0 else -1)
        level_corners.append(len(corners))
        if corner_cap is not None:
            corners = corners[:corner_cap]
        k, _ = om.keypoints(p, corners, l, g["scale"])
        level_counts.append(len(k))
        keys.append(k)
    allk = np.concatenate(keys) if keys else np.zeros(0, om.KEYPOINT_DTYPE)
    return allk, np.array(level_counts, np.int32), np.array(level_corners, np.int32), pl


def describe(pl, geo, keys):
    """-> (n, 32) uint8: every keypoint on the blurred plane of its own level; a level outside the table or an empty one gives a zero row.  pl: the level
    planes (unblurred) as planes() returns them."""
    out = np.zeros((len(keys), 32), np.uint8)
    for l, (g, p) in enumerate(zip(geo, pl)):
        sel = np.nonzero(keys["level"] == l)[0]
        if p is None or len(sel) == 0:
            continue
        out[sel] = om.describe(om.blur(p), keys[sel], g["scale"])
    return out
