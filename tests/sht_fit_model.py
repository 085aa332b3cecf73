"""Hough line refinement in plain numpy and Python integers: the definition of include/compv_hip.h (compvhip_line_fit) restated, the
yardstick of tests/test_gpu_sht_fit.py.  It shares no code with the kernel; tests/test_sht_fit_model.py pins it against the oracle's
accumulator, a brute-force scan of the whole image and drawn lines.

Rule 1 (the band) is int64 numpy on the vote's Q16 tables (oracle_bindings.Oracle.sht_tables), rule 2 (the moments) exact int64 sums, rule 3
(the central moments) Python integers, rule 4 (the fit) is np.float64 scalars, one rounding per operation, in the order of the definition.
"""
import math

import numpy as np

FIT_DTYPE = np.dtype([("line", "<i4"), ("pixels", "<i4"), ("sx", "<i8"), ("sy", "<i8"), ("sxx", "<i8"), ("sxy", "<i8"), ("syy", "<i8"),
                      ("nx", "<f8"), ("ny", "<f8"), ("rho", "<f8"), ("rms2", "<f8")])
MAX_HALF_WIDTH = 8
MAX_SIDE = 8192


def is_x_major(sinQ, cosQ, col):
    return int(sinQ[col]) >= abs(int(cosQ[col]))


def band_pixels(edges, sinQ, cosQ, row, col, b, rng=None):
    """Rule 1: (xs, ys), int64 arrays of the edge pixels in the band of half width b around cell (row, col); rng = (p0, p1) keeps the pixels
    whose major coordinate lies in [p0, p1].  The candidates of a position come from a float estimate widened far beyond its error (the
    band is at most 25 pixels wide at a position); the vote's expression decides."""
    H, W = edges.shape
    rho, s, c = (W + H) - int(row), int(sinQ[col]), int(cosQ[col])
    xm = s >= abs(c)
    N, Nm = (W, H) if xm else (H, W)
    cp, cm = (c, s) if xm else (s, c)
    p0, p1 = (0, N - 1) if rng is None else (max(int(rng[0]), 0), min(int(rng[1]), N - 1))
    if p1 < p0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    p = np.arange(p0, p1 + 1, dtype=np.int64)
    centre = np.floor_divide((rho << 16) + 32768 - p * cp, cm)
    k = np.arange(-16, 17, dtype=np.int64)
    m = centre[:, None] + k[None, :]
    pp = np.broadcast_to(p[:, None], m.shape)
    ok = (np.abs(((pp * cp + m * cm) >> 16) - rho) <= b) & (m >= 0) & (m < Nm)
    mi = np.clip(m, 0, Nm - 1)
    ok &= (edges[mi, pp] if xm else edges[pp, mi]) != 0
    return (pp[ok], m[ok]) if xm else (m[ok], pp[ok])


def moments(xs, ys):
    """Rule 2: (n, sx, sy, sxx, sxy, syy) as Python integers.  The sums are taken in int64, which holds them exactly (coordinates below
    8192 and at most 204 800 pixels: every sum is below 2^44)."""
    x = np.asarray(xs, np.int64)
    y = np.asarray(ys, np.int64)
    assert len(x) <= 25 * MAX_SIDE and (len(x) == 0 or max(int(x.max()), int(y.max())) < MAX_SIDE)
    return (len(x), int(x.sum()), int(y.sum()), int((x * x).sum()), int((x * y).sum()), int((y * y).sum()))


def central(mom):
    """Rule 3 in Python integers: (A, B, C)."""
    n, sx, sy, sxx, sxy, syy = mom
    return n * sxx - sx * sx, n * sxy - sx * sy, n * syy - sy * sy


def fit(mom):
    """Rule 4: (valid, nx, ny, rho, rms2) as np.float64; every line below is one rounded operation per operator, in the stated order."""
    f = np.float64
    n, sx, sy = mom[0], mom[1], mom[2]
    A, B, C = central(mom)
    assert max(abs(A), abs(B), abs(C)) < 2 ** 63
    a, bb, c = f(A), f(B), f(C)             # int -> binary64, round to nearest even
    d = a - c
    bb2 = bb * bb
    s = np.sqrt(d * d + f(4.0) * bb2)
    zero = f(0.0)
    if n < 2 or s == 0:
        return False, zero, zero, zero, zero
    if d >= 0:
        u = -(f(2.0) * bb)
        v = d + s
    else:
        u = s - d
        v = -(f(2.0) * bb)
    h = np.sqrt(u * u + v * v)
    nx = u / h
    ny = v / h
    if ny < 0 or (ny == 0 and nx < 0):
        nx, ny = -nx, -ny
    nd = f(n)
    rho = (nx * f(sx) + ny * f(sy)) / nd
    t = (a + c) - s
    rms2 = (t if t > 0 else zero) / (f(2.0) * nd * nd)
    return True, nx, ny, rho, rms2


def record(line, mom):
    """Rule 5: one FIT_DTYPE record (a numpy void)."""
    valid, nx, ny, rho, rms2 = fit(mom)
    out = np.zeros(1, FIT_DTYPE)
    out[0] = (line, mom[0], mom[1], mom[2], mom[3], mom[4], mom[5], nx, ny, rho, rms2)
    return out[0], valid


def line_fit(edges, sinQ, cosQ, row, col, b, line=0, rng=None):
    xs, ys = band_pixels(edges, sinQ, cosQ, row, col, b, rng)
    return record(line, moments(xs, ys))


def frame_fits(edges, sinQ, cosQ, cells, b, R, max_lines=0, segs=None):
    """Rule 6 for one frame: cells = [(row, col)] in the order of the frame's line array, R = accumulator rows.  Per line (segs is None):
    record i for line i of the lines considered.  Per segment: record j for segs[j] (records with line, x0, y0, x1, y1 fields); a segment
    whose line is not one of the lines considered, or a cell outside the R x T accumulator, has an empty band.  Returns (FIT_DTYPE array,
    [valid])."""
    T = len(sinQ)
    n = len(cells) if max_lines <= 0 else min(len(cells), max_lines)
    recs, valid = [], []

    def one(idx, line, rng):
        if 0 <= line < n and 0 <= cells[line][0] < R and 0 <= cells[line][1] < T:
            r, v = line_fit(edges, sinQ, cosQ, cells[line][0], cells[line][1], b, line, rng)
        else:
            r, v = record(line, (0, 0, 0, 0, 0, 0))
        recs.append(r)
        valid.append(v)

    if segs is None:
        for i in range(n):
            one(i, i, None)
    else:
        for j, sg in enumerate(segs):
            line = int(sg["line"])
            xm = is_x_major(sinQ, cosQ, cells[line][1]) if 0 <= line < n and 0 <= cells[line][1] < T else True
            one(j, line, (int(sg["x0"]), int(sg["x1"])) if xm else (int(sg["y0"]), int(sg["y1"])))
    out = np.zeros(len(recs), FIT_DTYPE)
    for i, r in enumerate(recs):
        out[i] = r
    return out, valid


def refine_lines(lines, fits, valid):
    """Rule 7: a copy of `lines` (records with rho, theta, strength, row, col) with the valid fits written in.  theta goes through atan2:
    the one value of the feature with a tolerance (1 float32 ulp)."""
    out = lines.copy()
    for i, (r, v) in enumerate(zip(fits, valid)):
        if v:
            out["rho"][i] = np.float32(r["rho"])
            out["theta"][i] = np.float32(np.arctan2(r["ny"], r["nx"]))
            out["strength"][i] = r["pixels"]
    return out


def fitted_theta_rho(r):
    """(theta in degrees, rho) of a valid record."""
    return math.degrees(math.atan2(float(r["ny"]), float(r["nx"]))), float(r["rho"])
