"""Pins tests/sht_fit_model.py (the numpy / Python-integer restatement of the line-fit definition in include/compv_hip.h), so that the GPU
test is not the model checking its own twin:

* rule 1 against a brute-force scan of the whole image with the vote's expression, on the sizes of tests/plan_geometries.py and on
  hand-drawn maps whose moments and fits are known by construction;
* rule 1 against the ORACLE's accumulator: with b = 0 the band of an oracle line holds `strength` pixels, with b > 0 the sum of the
  accumulator cells (row - b .. row + b, col), rows clipped to the accumulator;
* rule 4 on ten drawn lines whose true parameters are known: the fit lands within 0.02 degrees and 0.15 pixels of them, and closer in
  angle than the accumulator cell it started from;
* the invalid fits (no pixel, one pixel, an isotropic blob), the int64 bound of rule 3 at its worst case, and the per-segment ranges.
"""
import math

import numpy as np
import pytest

from oracle_bindings import synth_frame
from plan_geometries import GEOMETRIES
from sht_fit_model import (FIT_DTYPE, MAX_HALF_WIDTH, MAX_SIDE, band_pixels, central, fit, fitted_theta_rho, frame_fits, is_x_major, line_fit,
                           moments, refine_lines)
from sht_segments_model import frame_segments


def brute_band(edges, sinQ, cosQ, row, col, b, rng=None):
    """Rule 1 on every pixel of the image: the set of (x, y) of the band."""
    H, W = edges.shape
    x = np.broadcast_to(np.arange(W, dtype=np.int64)[None, :], (H, W))
    y = np.broadcast_to(np.arange(H, dtype=np.int64)[:, None], (H, W))
    v = (x * int(cosQ[col]) + y * int(sinQ[col])) >> 16
    hit = (np.abs(v - ((W + H) - row)) <= b) & (edges != 0)
    if rng is not None:
        major = x if is_x_major(sinQ, cosQ, col) else y
        hit &= (major >= rng[0]) & (major <= rng[1])
    ys, xs = np.nonzero(hit)
    return set(zip(xs.tolist(), ys.tolist()))


def model_band(edges, sinQ, cosQ, row, col, b, rng=None):
    xs, ys = band_pixels(edges, sinQ, cosQ, row, col, b, rng)
    out = set(zip(xs.tolist(), ys.tolist()))
    assert len(out) == len(xs)          # no pixel twice
    return out


def cell_of(W, H, sinQ, cosQ, x, y, col):
    return (W + H) - ((x * int(cosQ[col]) + y * int(sinQ[col])) >> 16)


@pytest.mark.parametrize("W,H,S,F,theta", GEOMETRIES, ids=lambda v: str(v))
def test_band_is_the_brute_force_scan(oracle, W, H, S, F, theta):
    R, T, _ = oracle.sht_dims(W, H, theta)
    sinQ, cosQ = oracle.sht_tables(theta, T)
    rng = np.random.default_rng(W * 31 + H)
    edges = (rng.random((H, W)) < 0.2).astype(np.uint8) * 255
    edges[H // 2, :] = 255
    edges[:, W // 2] = 255
    ys, xs = np.nonzero(edges)
    cols = sorted({0, T - 1, T // 2, T // 4, 3 * T // 4} | set(rng.integers(0, T, 5).tolist()))
    for col in cols:
        k = int(rng.integers(0, len(xs)))
        row = cell_of(W, H, sinQ, cosQ, int(xs[k]), int(ys[k]), col)
        N = W if is_x_major(sinQ, cosQ, col) else H
        for b in (0, 1, 3, 8):
            want = brute_band(edges, sinQ, cosQ, row, col, b)
            assert (int(xs[k]), int(ys[k])) in want
            assert model_band(edges, sinQ, cosQ, row, col, b) == want, (row, col, b)
        r = (N // 3, N // 3 + max(1, N // 4))
        assert model_band(edges, sinQ, cosQ, row, col, 3, r) == brute_band(edges, sinQ, cosQ, row, col, 3, r), (row, col, r)
        assert model_band(edges, sinQ, cosQ, row, col, 3, (-5, N + 9)) == brute_band(edges, sinQ, cosQ, row, col, 3), (row, col)
        assert model_band(edges, sinQ, cosQ, row, col, 3, (N, N + 9)) == set()
    # the rows at the ends of the accumulator: bands that hang over its edge
    for row, col in ((0, T // 2), (R - 1, T // 2), (W + H, 0), (W + H + 3, T - 1)):
        assert model_band(edges, sinQ, cosQ, row, col, 8) == brute_band(edges, sinQ, cosQ, row, col, 8), (row, col)


@pytest.mark.parametrize("name,col,pixel_of_q,normal,rho", [
    ("horizontal", 90, lambda q: (q, 20), (0.0, 1.0), 20.0),
    ("vertical_theta0", 0, lambda q: (30, q), (1.0, 0.0), 30.0),
    ("deg45", 45, lambda q: (q, 60 - q), (math.sqrt(0.5), math.sqrt(0.5)), 60 * math.sqrt(0.5)),
    ("deg135_negative_cos", 135, lambda q: (q, q + 11), (-math.sqrt(0.5), math.sqrt(0.5)), 11 * math.sqrt(0.5)),
])
def test_hand_drawn_lines(oracle, name, col, pixel_of_q, normal, rho):
    """A one-pixel line of 48 pixels and a second, parallel one four cells away: b = 0 and b = 2 see the first alone (exact moments, zero
    residual), b = 8 sees both."""
    W, H, theta = 80, 70, 1.0
    R, T, _ = oracle.sht_dims(W, H, theta)
    sinQ, cosQ = oracle.sht_tables(theta, T)
    pts = [pixel_of_q(q) for q in range(3, 51)]
    off = (0, 5) if name != "vertical_theta0" else (5, 0)       # five pixels along y (x for the vertical line): 3.5 to 5 rho cells away
    far = [(x + off[0], y + off[1]) for x, y in pts]
    edges = np.zeros((H, W), np.uint8)
    for x, y in pts + far:
        edges[y, x] = 255
    rows = {cell_of(W, H, sinQ, cosQ, x, y, col) for x, y in pts}
    assert len(rows) == 1
    row = rows.pop()
    for b in (0, 2):
        assert model_band(edges, sinQ, cosQ, row, col, b) == brute_band(edges, sinQ, cosQ, row, col, b) == set(pts), b
        rec, valid = line_fit(edges, sinQ, cosQ, row, col, b, line=7)
        xs, ys = [p[0] for p in pts], [p[1] for p in pts]
        assert valid and rec["line"] == 7 and rec["pixels"] == 48
        assert (rec["sx"], rec["sy"]) == (sum(xs), sum(ys))
        assert (rec["sxx"], rec["sxy"], rec["syy"]) == (sum(x * x for x in xs), sum(x * y for x, y in zip(xs, ys)), sum(y * y for y in ys))
        assert abs(rec["nx"] - normal[0]) < 1e-15 and abs(rec["ny"] - normal[1]) < 1e-15
        assert abs(rec["rho"] - rho) < 1e-12 and rec["rms2"] == 0.0
    assert model_band(edges, sinQ, cosQ, row, col, 8) == brute_band(edges, sinQ, cosQ, row, col, 8) == set(pts + far)
    rec, valid = line_fit(edges, sinQ, cosQ, row, col, 8)
    assert valid and rec["pixels"] == 96 and rec["rms2"] > 1.0
    # two parallel pieces, the second shifted along an axis and not along the normal: the normal turns a little on the diagonals
    assert abs(rec["nx"] - normal[0]) < 0.02 and abs(rec["ny"] - normal[1]) < 0.02


@pytest.mark.parametrize("W,H,tl,th,theta,thr", [(640, 480, 59., 119., 1.0, 100), (641, 480, 59., 119., 1.0, 100), (1282, 720, 0.8, 1.6, 1.0, 100),
                                                 (640, 480, 59., 119., 0.5, 100)], ids=lambda v: str(v))
def test_band_count_is_the_oracle_accumulator_column_sum(oracle, W, H, tl, th, theta, thr):
    rc, edges = oracle.canny(synth_frame(W, H), tl, th)
    assert rc == 0
    acc = oracle.sht_acc(edges, theta)
    R, T, _ = oracle.sht_dims(W, H, theta)
    sinQ, cosQ = oracle.sht_tables(theta, T)
    lines = oracle.sht_lines_from_acc(acc, W, H, theta, thr)
    assert len(lines) > 20
    for l in lines:
        row, col, strength = l[3], l[4], l[2]
        xs, ys = band_pixels(edges, sinQ, cosQ, row, col, 0)
        assert len(xs) == strength == int(acc[row, col]), (row, col)
    cells = [(l[3], l[4]) for l in lines[::max(1, len(lines) // 40)]]
    cells += [(0, T // 2), (3, T // 3), (R - 1, 1), (R - 4, T - 1)]           # bands clipped by the accumulator's first and last rows
    for row, col in cells:
        for b in (1, 3, 8):
            xs, ys = band_pixels(edges, sinQ, cosQ, row, col, b)
            assert len(xs) == int(acc[max(row - b, 0):min(row + b, R - 1) + 1, col].sum()), (row, col, b)


# (theta in degrees, rho) of the drawn lines; only (45, 350) sits on a 1-degree bin
DRAWN = [(30.4, 300.3), (90.45, 200.7), (0.3, 320.2), (135.5, -50.4), (60.37, 410.1), (179.6, -300.5), (45, 350), (100.25, 150.6), (12.6, 500.2),
         (89.5, 100)]


def rasterise(W, H, theta_deg, rho):
    """x cos(theta) + y sin(theta) = rho, one pixel per position of its major axis (the nearest one)."""
    c, s = math.cos(math.radians(theta_deg)), math.sin(math.radians(theta_deg))
    e = np.zeros((H, W), np.uint8)
    if abs(s) >= abs(c):
        x = np.arange(W)
        y = np.rint((rho - x * c) / s).astype(np.int64)
        ok = (y >= 0) & (y < H)
        e[y[ok], x[ok]] = 255
    else:
        y = np.arange(H)
        x = np.rint((rho - y * s) / c).astype(np.int64)
        ok = (x >= 0) & (x < W)
        e[y[ok], x[ok]] = 255
    return e


def line_error(theta_deg, rho, theta0, rho0):
    """(angle error in degrees, rho error) between two (theta, rho) lines; (theta, rho) and (theta +- 180, -rho) are one line."""
    dt = theta_deg - theta0
    if dt > 90:
        dt, rho = dt - 180, -rho
    elif dt < -90:
        dt, rho = dt + 180, -rho
    return abs(dt), abs(rho - rho0)


@pytest.mark.parametrize("theta0,rho0", DRAWN, ids=lambda v: str(v))
def test_drawn_lines_are_recovered(oracle, theta0, rho0):
    W, H, theta = 640, 480, 1.0
    edges = rasterise(W, H, theta0, rho0)
    assert int((edges != 0).sum()) > 200
    acc = oracle.sht_acc(edges, theta)
    R, T, step = oracle.sht_dims(W, H, theta)
    sinQ, cosQ = oracle.sht_tables(theta, T)
    row, col = np.unravel_index(int(np.argmax(acc)), acc.shape)
    rec, valid = line_fit(edges, sinQ, cosQ, int(row), int(col), 3)
    assert valid
    t, r = fitted_theta_rho(rec)
    dt, dr = line_error(t, r, theta0, rho0)
    cell_dt, _ = line_error(math.degrees(col * step), float((W + H) - row), theta0, rho0)
    print("drawn (%g, %g): cell (%d, %d) off by %.3f deg; fit off by %.4f deg, %.4f px, %d pixels" % (theta0, rho0, row, col, cell_dt, dt, dr, rec["pixels"]))
    assert dt <= 0.02 and dr <= 0.15, (dt, dr)
    if theta0 != round(theta0):
        assert dt < cell_dt, (dt, cell_dt)
    assert abs(math.hypot(rec["nx"], rec["ny"]) - 1.0) < 1e-15 and rec["ny"] >= 0


def test_invalid_fits(oracle):
    W, H, theta = 40, 30, 1.0
    R, T, _ = oracle.sht_dims(W, H, theta)
    sinQ, cosQ = oracle.sht_tables(theta, T)
    col = 90
    edges = np.zeros((H, W), np.uint8)
    row = cell_of(W, H, sinQ, cosQ, 10, 10, col)
    for n_pix in (0, 1):
        if n_pix:
            edges[10, 10] = 255
        rec, valid = line_fit(edges, sinQ, cosQ, row, col, 3, line=2)
        assert not valid and rec["pixels"] == n_pix and rec["line"] == 2
        assert rec["nx"] == rec["ny"] == rec["rho"] == rec["rms2"] == 0.0
        assert (rec["sx"], rec["sy"], rec["sxx"], rec["sxy"], rec["syy"]) == ((10, 10, 100, 100, 100) if n_pix else (0, 0, 0, 0, 0))
    # an isotropic 2 x 2 blob: A == C, B == 0, no direction
    edges[10:12, 10:12] = 255
    rec, valid = line_fit(edges, sinQ, cosQ, row, col, 3)
    assert rec["pixels"] == 4 and central(moments(*band_pixels(edges, sinQ, cosQ, row, col, 3))) == (4, 0, 4)
    assert not valid and rec["nx"] == rec["ny"] == rec["rho"] == rec["rms2"] == 0.0
    # frame_fits: a cell outside the accumulator and a segment of a line that is not there have empty bands
    fits, valid = frame_fits(edges, sinQ, cosQ, [(row, col), (R, col), (row, T)], 3, R)
    assert fits["pixels"].tolist() == [4, 0, 0] and fits["line"].tolist() == [0, 1, 2] and valid == [False] * 3
    segs = np.zeros(2, [("line", "<i4"), ("x0", "<i4"), ("y0", "<i4"), ("x1", "<i4"), ("y1", "<i4"), ("support", "<i4")])
    segs[0] = (0, 10, 10, 10, 10, 1)
    segs[1] = (5, 0, 0, 39, 29, 1)
    fits, valid = frame_fits(edges, sinQ, cosQ, [(row, col)], 3, R, segs=segs)
    assert fits["pixels"].tolist() == [2, 0] and fits["line"].tolist() == [0, 5]


def test_central_moments_stay_below_2_63_at_the_worst_case(oracle):
    """Every pixel an edge, the longest line the call accepts, the widest band: the count per position is at most 25 and A, B, C fit int64."""
    W, H, theta = MAX_SIDE, 40, 1.0
    R, T, _ = oracle.sht_dims(W, H, theta)
    sinQ, cosQ = oracle.sht_tables(theta, T)
    edges = np.full((H, W), 255, np.uint8)
    worst = 0
    for col in (90, 45, 135, 60, 120):
        assert is_x_major(sinQ, cosQ, col)
        row = cell_of(W, H, sinQ, cosQ, W // 2, H // 2, col)
        xs, ys = band_pixels(edges, sinQ, cosQ, row, col, MAX_HALF_WIDTH)
        per_position = np.bincount(xs)
        assert per_position.max() <= (2 * MAX_HALF_WIDTH + 1) * 65536 // 46340 + 1 == 25
        mom = moments(xs, ys)
        assert mom[0] <= 25 * MAX_SIDE == 204800
        A, B, C = central(mom)
        worst = max(worst, abs(A), abs(B), abs(C))
        assert fit(mom)[0]
    assert worst < 2 ** 63
    # the bound of the definition: n^2 * 8191^2 with n = 204 800
    assert 204800 ** 2 * 8191 ** 2 < 2 ** 63
    # the tall twin: an all-foreground strip 8192 rows high, y-major
    edges = np.full((MAX_SIDE, 40), 255, np.uint8)
    R, T, _ = oracle.sht_dims(40, MAX_SIDE, theta)
    sinQ, cosQ = oracle.sht_tables(theta, T)
    row = cell_of(40, MAX_SIDE, sinQ, cosQ, 20, MAX_SIDE // 2, 0)
    mom = moments(*band_pixels(edges, sinQ, cosQ, row, 0, MAX_HALF_WIDTH))
    assert mom[0] == 17 * MAX_SIDE and max(abs(v) for v in central(mom)) < 2 ** 63


def test_segment_ranges_partition_the_line(oracle):
    """The fits over a line's segments (minLength = 1) add up to the line's own moments: with maxGap = N there is one segment from the first
    to the last support pixel, with smaller gaps several that partition the support.  With b > 0 a range can only drop pixels."""
    W, H, theta = 640, 480, 1.0
    rc, edges = oracle.canny(synth_frame(W, H), 59., 119.)
    assert rc == 0
    acc = oracle.sht_acc(edges, theta)
    R, T, _ = oracle.sht_dims(W, H, theta)
    sinQ, cosQ = oracle.sht_tables(theta, T)
    lines = oracle.sht_lines_from_acc(acc, W, H, theta, 100)
    cells = [(l[3], l[4]) for l in lines[:24]]
    whole, _ = frame_fits(edges, sinQ, cosQ, cells, 0, R)
    names = ["pixels", "sx", "sy", "sxx", "sxy", "syy"]
    several = 0
    for max_gap in (max(W, H), 2, 0):
        segs = frame_segments(edges, sinQ, cosQ, cells, 1, max_gap)
        if max_gap == max(W, H):
            assert segs["line"].tolist() == list(range(len(cells)))
        several += len(segs) > len(cells)
        parts, _ = frame_fits(edges, sinQ, cosQ, cells, 0, R, segs=segs)
        assert parts["line"].tolist() == segs["line"].tolist() and parts["pixels"].tolist() == segs["support"].tolist()
        for i in range(len(cells)):
            sel = parts[parts["line"] == i]
            for k in names:
                assert int(sel[k].astype(object).sum()) == int(whole[k][i]), (max_gap, i, k)
        wide, _ = frame_fits(edges, sinQ, cosQ, cells, 3, R)
        cut, _ = frame_fits(edges, sinQ, cosQ, cells, 3, R, segs=segs)
        for i in range(len(cells)):
            assert int(cut["pixels"][cut["line"] == i].sum()) <= int(wide["pixels"][i])
    assert several == 2


def test_refined_lines_keep_the_cell_and_take_the_fit(oracle):
    W, H, theta = 640, 480, 1.0
    edges = rasterise(W, H, 30.4, 300.3)
    edges[5, 5] = 255
    R, T, step = oracle.sht_dims(W, H, theta)
    sinQ, cosQ = oracle.sht_tables(theta, T)
    acc = oracle.sht_acc(edges, theta)
    row, col = (int(v) for v in np.unravel_index(int(np.argmax(acc)), acc.shape))
    lone = cell_of(W, H, sinQ, cosQ, 5, 5, col)                          # a parallel cell far from the drawn line: one pixel
    lines = np.zeros(2, [("rho", "<f4"), ("theta", "<f4"), ("strength", "<i4"), ("row", "<i4"), ("col", "<i4")])
    lines[0] = ((W + H) - row, col * step, acc[row, col], row, col)
    lines[1] = ((W + H) - lone, col * step, 1, lone, col)
    fits, valid = frame_fits(edges, sinQ, cosQ, [(row, col), (lone, col)], 3, R)
    assert valid == [True, False] and fits.dtype == FIT_DTYPE
    out = refine_lines(lines, fits, valid)
    assert out[1] == lines[1]                                            # an invalid fit copies the line
    assert (out["row"][0], out["col"][0]) == (row, col) and out["strength"][0] == fits["pixels"][0]
    assert out["rho"][0] == np.float32(fits["rho"][0]) and abs(math.degrees(out["theta"][0]) - 30.4) < 0.02
