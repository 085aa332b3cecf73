"""The RANSAC line and parabola fits of include/compv_hip.h ("RANSAC curve fitting", items A - G) in numpy: the definition the device and
compv_amd/csrc/curvefit_math.hpp equal bit for bit.

Elementwise float64 operations only -- every +, -, *, /, sqrt below is ONE IEEE binary64 operation on arrays, in the order the definition gives; no
np.sum over floats, no np.dot, no fused multiply-add, no transcendental function.  Everything is vectorised over the tries of a set.  The hash, sum64
and the half-angle formulas are the homography's (tests/homography_model.py)."""
import numpy as np

import homography_model as hm

LINE, PARABOLA, PARABOLA_SIDEWAYS = 0, 1, 2
MODELS = (LINE, PARABOLA, PARABOLA_SIDEWAYS)
DRAWS = 64
RESULT_DTYPE = np.dtype([("A", "<f8"), ("B", "<f8"), ("C", "<f8"), ("inliers", "<i4"), ("bestTry", "<i4"), ("status", "<i4"), ("k", "<i4")])   # compvhip_curvefit_result
COMP_DTYPE = np.dtype([("x", "<i4"), ("y", "<i4"), ("x0", "<i4"), ("y0", "<i4"), ("x1", "<i4"), ("y1", "<i4"), ("pixels", "<i4")])          # compvhip_component

_QUIET = dict(divide="ignore", invalid="ignore", over="ignore", under="ignore")


def model_points(model):
    return 2 if model == LINE else 3


# ---- A. samples ----------------------------------------------------------------------------------------------------------------------------
def samples(model, seed, set_index, k, tries):
    """int32 [tries][m]: the m distinct indices of every try of set `set_index` among k > m points (homography item A with m slots)"""
    m = model_points(model)
    assert k > m
    t = np.arange(tries, dtype=np.uint32)
    with np.errstate(over="ignore"):
        base = hm.lowbias32(hm.lowbias32(np.uint32(seed) ^ np.uint32(set_index)) + t)
    out = np.full((tries, m), -1, np.int64)
    filled = np.zeros(tries, np.int64)
    rows = np.arange(tries)
    for c in range(DRAWS):
        if (filled == m).all():
            break
        with np.errstate(over="ignore"):
            u = hm.lowbias32(base + np.uint32(c))
        idx = ((u.astype(np.uint64) * np.uint64(k)) >> np.uint64(32)).astype(np.int64)
        take = (filled < m) & ~(out == idx[:, None]).any(axis=1)
        out[rows[take], filled[take]] = idx[take]
        filled[take] += 1
    for r in np.nonzero(filled < m)[0]:          # 64 draws did not fill the slots: the smallest unused indices
        idx = 0
        while filled[r] < m:
            if idx not in out[r, :filled[r]]:
                out[r, filled[r]] = idx
                filled[r] += 1
            idx += 1
    return out.astype(np.int32)


# ---- B. model of a sample ------------------------------------------------------------------------------------------------------------------
def xy_of(model, px, py):
    """the coordinates a model takes for its x and its y"""
    return (py, px) if model == PARABOLA_SIDEWAYS else (px, py)


def curve_of(model, px, py):
    """px, py: [n][m] -> A, B, C [n], ok [n] (False: rejected)"""
    px, py = np.asarray(px, np.float64), np.asarray(py, np.float64)
    with np.errstate(**_QUIET):
        if model == LINE:
            x0, y0, x1, y1 = px[:, 0], py[:, 0], px[:, 1], py[:, 1]
            ok = ~((x0 == x1) & (y0 == y1))
            return y1 - y0, x0 - x1, (x1 * y0) - (x0 * y1), ok
        x, y = xy_of(model, px, py)
        x1, y1, x2, y2, x3, y3 = x[:, 0], y[:, 0], x[:, 1], y[:, 1], x[:, 2], y[:, 2]
        ok = ~((x1 == x2) | (x1 == x3) | (x2 == x3))
        scale = 1.0 / (((x1 - x2) * (x1 - x3)) * (x2 - x3))
        A = (((x3 * (y2 - y1)) + (x2 * (y1 - y3))) + (x1 * (y3 - y2))) * scale
        B = ((((x3 * x3) * (y1 - y2)) + ((x2 * x2) * (y3 - y1))) + ((x1 * x1) * (y2 - y3))) * scale
        C = (((((x2 * x3) * (x2 - x3)) * y1) + (((x3 * x1) * (x3 - x1)) * y2)) + (((x1 * x2) * (x1 - x2)) * y3)) * scale
        return A, B, C, ok


# ---- C. residual ---------------------------------------------------------------------------------------------------------------------------
def prepared(model, A, B, C):
    if model != LINE:
        return A, B, C
    with np.errstate(**_QUIET):
        s = 1.0 / np.sqrt((A * A) + (B * B))
        return A * s, B * s, C * s


def residuals(model, A, B, C, pts):
    """A, B, C: [n] (as given, not yet scaled); pts: [k][2] -> [n][k]"""
    A, B, C = (np.atleast_1d(np.asarray(v, np.float64)) for v in (A, B, C))
    a, b, c = (v[:, None] for v in prepared(model, A, B, C))
    px, py = pts[:, 0][None, :], pts[:, 1][None, :]
    with np.errstate(**_QUIET):
        if model == LINE:
            return np.abs(((a * px) + c) + (b * py))
        x, y = xy_of(model, px, py)
        return np.abs((((a * (x * x)) + c) + (b * x)) - y)


# ---- E. refit ------------------------------------------------------------------------------------------------------------------------------
def half_angle(y, x):
    """(cos, sin) of atan2(y, x) / 2, homography item D"""
    with np.errstate(**_QUIET):
        rho = np.sqrt(x * x + y * y)
        c2, s2 = x / rho, y / rho
        if c2 >= 0.0:
            cs = np.sqrt((1.0 + c2) * 0.5)
            return cs, s2 / (2.0 * cs)
        mag = np.sqrt((1.0 - c2) * 0.5)
        sn = mag if (s2 == 0.0 or s2 > 0.0) else -mag
        return s2 / (2.0 * sn), sn


def refit(model, sel):
    """sel: [n][2], n > m inliers in index order -> (ok, A, B, C)"""
    n = len(sel)
    with np.errstate(**_QUIET):
        inv = np.float64(1.0) / np.float64(n)
        if model == LINE:
            mx, my = hm.sum64(sel[:, 0]) * inv, hm.sum64(sel[:, 1]) * inv
            a, b = sel[:, 0] - mx, sel[:, 1] - my
            num = hm.sum64(a * b) * np.float64(-2.0)
            den = hm.sum64((b * b) - (a * a))
            cs, sn = (np.float64(1.0), np.float64(0.0)) if (num == 0.0 and den == 0.0) else half_angle(num, den)
            return True, cs, sn, -((mx * cs) + (my * sn))
        x, y = xy_of(model, sel[:, 0], sel[:, 1])
        mean = hm.sum64(x) * inv
        u = x - mean
        uu = u * u
        s = [hm.sum64(v) for v in (u, uu, uu * u, uu * uu, y, u * y, uu * y)]
        m00, m01, m02, m11, m12, m22 = s[3], s[2], s[1], s[1], s[0], np.float64(n)
        r0, r1, r2 = s[6], s[5], s[4]
        c00, c01, c02 = (m11 * m22) - (m12 * m12), (m02 * m12) - (m01 * m22), (m01 * m12) - (m02 * m11)
        c11, c12, c22 = (m00 * m22) - (m02 * m02), (m01 * m02) - (m00 * m12), (m00 * m11) - (m01 * m01)
        det = ((m00 * c00) + (m01 * c01)) + (m02 * c02)
        if det == 0.0 or not np.isfinite(det):
            return False, 0.0, 0.0, 0.0
        a = (((c00 * r0) + (c01 * r1)) + (c02 * r2)) / det
        b = (((c01 * r0) + (c11 * r1)) + (c12 * r2)) / det
        c = (((c02 * r0) + (c12 * r1)) + (c22 * r2)) / det
        return True, a, b - ((2.0 * a) * mean), (c - (b * mean)) + (a * (mean * mean))


# ---- the whole call for one set ------------------------------------------------------------------------------------------------------------
def find(points, count, model, tries, threshold=1.0, seed=0, set_index=0, sample_list=None):
    """points: [pointCap][2]; count: the set's (clamped here; None: pointCap) -> dict(result (RESULT_DTYPE scalar), mask uint8 [k], counts per try or
    None when no try runs (k <= m), samples, k)"""
    points = np.asarray(points, np.float64).reshape(-1, 2)
    k = len(points) if count is None else max(0, min(int(count), len(points)))
    m = model_points(model)
    res = np.zeros((), RESULT_DTYPE)
    res["bestTry"], res["k"] = -1, k
    pts = points[:k]
    if k < m:
        res["status"] = 2
        return dict(result=res, mask=np.zeros(k, np.uint8), counts=None, samples=None, k=k)
    if k == m:
        A, B, C, ok = curve_of(model, pts[None, :, 0], pts[None, :, 1])
        if ok[0]:
            res["A"], res["B"], res["C"], res["inliers"], res["bestTry"] = A[0], B[0], C[0], m, 0
        else:
            res["status"] = 1
        return dict(result=res, mask=np.full(k, 1 if ok[0] else 0, np.uint8), counts=None, samples=None, k=k)
    q = samples(model, seed, set_index, k, tries) if sample_list is None else np.asarray(sample_list, np.int32).reshape(tries, m)
    in_range = ((q >= 0) & (q < k)).all(axis=1)
    qs = np.where(in_range[:, None], q, 0)
    A, B, C, ok = curve_of(model, pts[qs, 0], pts[qs, 1])
    live = in_range & ok
    d = residuals(model, A, B, C, pts)
    inl = (d < threshold) & live[:, None]
    counts = inl.sum(axis=1).astype(np.int32)
    bt = int(np.argmax(counts))          # the largest count, then the smallest t
    mask = np.zeros(k, np.uint8)
    if counts[bt] < m:
        res["status"] = 1
        return dict(result=res, mask=mask, counts=counts, samples=q, k=k, distances=d)
    mask = inl[bt].astype(np.uint8)
    sel = pts[inl[bt]]
    if len(sel) == m:
        fa, fb, fc, fok = curve_of(model, sel[None, :, 0], sel[None, :, 1])
        fok, fa, fb, fc = bool(fok[0]), fa[0], fb[0], fc[0]
    else:
        fok, fa, fb, fc = refit(model, sel)
    if fok:
        res["A"], res["B"], res["C"] = fa, fb, fc
    else:
        res["A"], res["B"], res["C"], res["status"] = A[bt], B[bt], C[bt], 3
    res["inliers"], res["bestTry"] = counts[bt], bt
    return dict(result=res, mask=mask, counts=counts, samples=q, k=k, distances=d)


def curve_y(model, A, B, C, x):
    """the fitted curve as a function of its abscissa: a parabola's y(x) (a sideways one's x(y)); a line's y(x), or x(y) when |A| > |B|"""
    x = np.asarray(x, np.float64)
    if model == LINE:
        return -(A * x + C) / B if abs(B) >= abs(A) else -(B * x + C) / A
    return (A * x) * x + B * x + C


# ---- G. gather from a label map ------------------------------------------------------------------------------------------------------------
def gather(labels, W, comps, comp_count, comp_cap, point_cap):
    """labels: int32 [H][labelStride] of ONE frame; comps: COMP_DTYPE [compCap] -> points float64 [compCap][pointCap][2] (NaN where not written),
    counts int32 [compCap]"""
    H = labels.shape[0]
    pts = np.full((comp_cap, point_cap, 2), np.nan)
    counts = np.zeros(comp_cap, np.int32)
    for c in range(min(max(int(comp_count), 0), comp_cap)):
        r = comps[c]
        x0, y0, x1, y1 = max(int(r["x0"]), 0), max(int(r["y0"]), 0), min(int(r["x1"]), W - 1), min(int(r["y1"]), H - 1)
        if r["pixels"] <= 0 or x0 > x1 or y0 > y1:
            continue
        step = (int(r["pixels"]) + point_cap - 1) // point_cap
        ys, xs = np.nonzero(labels[y0:y1 + 1, x0:x1 + 1] == c + 1)          # raster order
        taken = np.arange(0, len(ys), step)[:point_cap]
        pts[c, :len(taken), 0] = (xs[taken] + x0).astype(np.float64)
        pts[c, :len(taken), 1] = (ys[taken] + y0).astype(np.float64)
        counts[c] = len(taken)
    return pts, counts
