"""The inputs of the remap / inverse-warp fixtures, regenerated from seeds: tests/golden/make_golden_remap.py runs the compiled reference on them, the
tests run the model and the GPU on them.  tests/golden/golden_remap.json / .npz hold the reference's OUTPUTS only."""
import numpy as np

import fast_model as fm
import remap_model as rm

F32 = np.float32
# Win, Hin, Wout, Hout.  Wout % 4 covers 0 .. 3; 261 is wider than one 256-pixel tile; 40 is the one width with Wout % 8 == 0, where the reference's float32
# output is sound and is recorded.
SIZES = ((64, 48, 61, 37), (200, 150, 203, 97), (33, 9, 40, 40), (129, 65, 7, 5), (200, 150, 261, 9), (64, 48, 30, 11))
INTERP_NAMES = {rm.NEAREST: "nearest", rm.BILINEAR: "bilinear", rm.BILINEAR_FLOAT32: "bilinear_f32"}


def frame(w, h, seed, kind="noise"):
    return fm.noise(w, h, seed) if kind == "noise" else fm.blocks(w, h, seed)


def random_map(w, h, w_out, h_out, seed):
    """float32 maps reaching 3 pixels outside the frame; the exact edge values 0, W - 1, W - 1.5, 0.5 (and the same for y, in every pairing that fits)
    sit at the start of the first row.  The second row starts with the float32 just below a power of two, in x, in y and in both: there x + 1.f lands in
    the next binade and rounds UP to an integer, so the bilinear neighbour is x1 + 2, not x1 + 1 -- the reference's arithmetic, which the definition keeps."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-3.0, w + 2.0, (h_out, w_out)).astype(F32)
    y = rng.uniform(-3.0, h + 2.0, (h_out, w_out)).astype(F32)
    ex, ey = (0.0, w - 1.0, w - 1.5, 0.5), (0.0, h - 1.0, h - 1.5, 0.5)
    for k in range(min(w_out, 16)):
        x[0, k], y[0, k] = ex[k % 4], ey[k // 4]
    below = lambda v: np.nextafter(F32(v), F32(0))          # noqa: E731
    px, py = [1 << e for e in range(12) if (1 << e) <= w - 2], [1 << e for e in range(12) if (1 << e) <= h - 2]
    for k in range(min(w_out, 12)):
        vx, vy = px[k % len(px)], py[(k // 2) % len(py)]
        x[1, k], y[1, k] = (below(vx), vy + 0.25) if k % 3 == 0 else (vx + 0.75, below(vy)) if k % 3 == 1 else (below(vx), below(vy))
    return x, y


def skips_a_neighbour(v, n):
    """the coordinates of v (inside 0 .. n - 1) whose second bilinear neighbour lies 2 beyond the first"""
    v = np.asarray(v, F32)
    with np.errstate(invalid="ignore"):
        ok = (v >= 0) & (v <= n - 1)
    t = np.where(ok, v, 0)
    return ok & (np.minimum((t + F32(1)).astype(np.int32), n - 1) - t.astype(np.int32) == 2)


def interps_of(w_out, reference=True):
    """the interpolations a case runs: float32 output only where the reference's is sound (Wout % 8 == 0)"""
    return (rm.NEAREST, rm.BILINEAR) + ((rm.BILINEAR_FLOAT32,) if w_out % 8 == 0 or not reference else ())


def remap_cases():
    """dicts: id, size (Win, Hin, Wout, Hout), frame seed, map seed, roi (left, right, top, bottom) or None, default value"""
    out = [{"id": "map%d" % k, "size": s, "seed": 61000 + k, "map_seed": 62000 + k, "roi": None, "default": (0, 77, 255, 9, 0, 200)[k]} for k, s in enumerate(SIZES)]
    # a caller's ROI that the clip changes on three sides: left below 0, bottom beyond the frame, right and top inside it
    out.append({"id": "map_roi", "size": SIZES[1], "seed": 61100, "map_seed": 62100, "roi": (-5.0, 120.25, 3.5, 400.0), "default": 31})
    return out


def matrices(w, h, w_out, h_out):
    """name -> (rows, 3) float32: a rotated and scaled 2 x 3, a shift that leaves most of the output outside, a mild homography"""
    sx, sy, c, s = w / w_out, h / h_out, np.cos(0.2), np.sin(0.2)
    return {
        "affine": np.array([[sx * c, -sx * s, 1.5], [sy * s, sy * c, -2.25]], F32),
        "mostly_outside": np.array([[1.0, 0.0, w - 3.5], [0.0, 1.0, h - 2.5]], F32),
        "homography": np.array([[sx, 0.05, -1.0], [0.02, sy, 0.5], [1e-3, 5e-4, 1.0]], F32),
    }


# Z = 2 - 0.25 i changes sign at column 8, where it is exactly 0: X * (1 / 0) is an infinity there, Y * (1 / 0) an infinity too except in row 0, where
# Y == 0 makes it a NaN.  Columns 9 .. 13 have X < 0, Z < 0 and Y <= 0: coordinates inside the frame.
Z_SIGN = np.array([[3.0, 0.0, -40.0], [0.0, -1.0, 0.0], [-0.25, 0.0, 2.0]], F32)


def warp_cases():
    """dicts: id, size, frame seed, M, default value, nearest_by_reference"""
    out = []
    for k, s in enumerate(SIZES):
        for name, M in matrices(*s).items():
            out.append({"id": "warp%d_%s" % (k, name), "size": s, "seed": 63000 + k, "M": M, "default": (0, 128, 5, 250, 17, 0)[k], "nan": False})
    # The reference's NEAREST leaf tests `x < left || x > right || ...` and so takes a NaN for inside and reads wherever the cast lands: the case is run
    # through the reference for the bilinear forms only (whose leaf uses ordered compares, the rule of the definition); nearest rests on the model.
    out.append({"id": "warp_z_sign", "size": SIZES[0], "seed": 63100, "M": Z_SIGN, "default": 99, "nan": True})
    return out
