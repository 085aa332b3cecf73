"""The inputs of the lens-undistortion fixtures, written out or regenerated from seeds: tests/golden/make_golden_undistort.py runs the compiled reference
on them, the tests run the model, the host code and the GPU on them.  tests/golden/golden_undistort.json / .npz hold the OUTPUTS only.

Shapes: the smallest at which the kernels can go wrong.  61 and 203 are no multiple of 4 (the partial lane group); 40 x 40 takes the vector stores and
the float32 output; 257 x 3 crosses the 256-wide tile; 1 x 1; a 30 x 11 window at origin (17, 9) of a 64 x 48 frame.  nd of 2, 3 and 4, skew zero and
non-zero, a barrel set (nothing outside at 61 x 37) and three pincushion sets (about a third outside, so no test passes on default bytes alone)."""
import numpy as np

import remap_cases as rc

F32, F64 = np.float32, np.float64
BARREL = (-0.31, 0.12, 0.0011, -0.0007)


def camera(w, h, skew=0.0):
    """a plausible camera of a w x h frame: focal lengths near the width, the principal point off the centre by a fraction of a pixel"""
    return [[0.9 * w + 0.37, skew, 0.5 * w - 0.3], [0.0, 0.88 * w + 0.11, 0.5 * h + 0.45], [0.0, 0.0, 1.0]]


def image_cases():
    """dicts: id, size (Win, Hin, Wout, Hout), origin (x0, y0), K (3 x 3), d (2 .. 4), frame seed, roi (left, right, top, bottom) or None, default value.
    whole: the window is the whole frame, so CompVCalibUtils::undist2DImage can produce it."""
    out = [
        {"id": "pin61", "size": (61, 37, 61, 37), "origin": (0, 0), "K": camera(61, 37), "d": (0.9, 0.4, 0.002, -0.001), "seed": 71000, "roi": None, "default": 0},
        {"id": "barrel61", "size": (61, 37, 61, 37), "origin": (0, 0), "K": camera(61, 37, 0.25), "d": BARREL, "seed": 71001, "roi": None, "default": 77},
        {"id": "pin203", "size": (203, 97, 203, 97), "origin": (0, 0), "K": camera(203, 97, 0.7), "d": (1.5, 0.0), "seed": 71002, "roi": None, "default": 255},
        {"id": "pin40", "size": (40, 40, 40, 40), "origin": (0, 0), "K": camera(40, 40), "d": (0.6, -0.2, 0.01), "seed": 71003, "roi": None, "default": 9},
        {"id": "barrel257", "size": (257, 3, 257, 3), "origin": (0, 0), "K": camera(257, 3, -0.4), "d": BARREL, "seed": 71004, "roi": None, "default": 200},
        {"id": "one", "size": (1, 1, 1, 1), "origin": (0, 0), "K": [[1.5, 0.0, 0.0], [0.0, 1.25, 0.0], [0.0, 0.0, 1.0]], "d": BARREL[:2], "seed": 71005, "roi": None, "default": 31},
        {"id": "window", "size": (64, 48, 30, 11), "origin": (17, 9), "K": camera(64, 48, 0.1), "d": BARREL, "seed": 71006, "roi": None, "default": 5},
        # a caller's ROI that the clip changes on three sides: left below 0, bottom beyond the frame, right and top inside it
        {"id": "roi203", "size": (203, 97, 203, 97), "origin": (0, 0), "K": camera(203, 97, 0.7), "d": BARREL[:3], "seed": 71007, "roi": (-5.0, 120.25, 3.5, 400.0),
         "default": 31},
    ]
    for c in out:
        w, h, wo, ho = c["size"]
        c["whole"] = (wo, ho) == (w, h) and c["origin"] == (0, 0)
    return out


def case(cid):
    return next(c for c in image_cases() if c["id"] == cid)


def frame(c, k=0):
    """frame k of a case: (Hin, Win) uint8"""
    w, h = c["size"][:2]
    return np.ascontiguousarray(rc.frame(w, h, c["seed"] + 1000 * k))


def cameras_for_frames(c, count):
    """`count` cameras around the case's: K (count, 3, 3), d (count, nd) float64 -- every frame of a rig has its own"""
    K = np.repeat(np.asarray(c["K"], F64)[None], count, axis=0)
    d = np.repeat(np.asarray(c["d"], F64)[None], count, axis=0)
    for k in range(count):
        K[k, 0, 0] *= 1.0 + 0.013 * k
        K[k, 0, 2] += 0.8 * k
        K[k, 1, 2] -= 0.6 * k
        d[k, 0] *= 1.0 - 0.2 * k
    return K, d


POINT_NS = (1, 63, 64, 65, 200)


def point_cases():
    """dicts: id, n, dtype, the image case whose camera serves, seed.  n around the 64 lanes of a wave and beyond one; both types"""
    cams = ("pin61", "pin203", "pin40", "window", "barrel61")
    return [{"id": "pts%d_%s" % (n, "f32" if t is F32 else "f64"), "n": n, "dtype": t, "camera": cams[k], "seed": 72000 + 10 * k + (t is F64)}
            for k, n in enumerate(POINT_NS) for t in (F32, F64)]


def points(c):
    """(n, 2) of the case's dtype: pixels in and a little around the camera's frame"""
    w, h = case(c["camera"])["size"][:2]
    rng = np.random.default_rng(c["seed"])
    return np.stack([rng.uniform(-4.0, w + 4.0, c["n"]), rng.uniform(-4.0, h + 4.0, c["n"])], axis=1).astype(c["dtype"])


def _rot(ax, ay, az):
    cx, sx, cy, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
    return (np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1.0]]) @ np.array([[cy, 0, sy], [0, 1.0, 0], [-sy, 0, cy]]) @ np.array([[1.0, 0, 0], [0, cx, -sx], [0, sx, cx]]))


def proj_cases():
    """dicts: id, n, camera, R (3, 3), t (3,), seed, zp.  z0: the third row of R is (0, 0, 1) and tz = -1, so every point with zp == 1 has z == 0 EXACTLY
    (the branch s = 1); its other points have zp in {2, 0.5}.  zp1: a general pose, zp = 1 throughout (a planar pattern)."""
    return [
        {"id": "proj_z0", "n": 77, "camera": "pin203", "R": [[0.98, -0.17, 0.05], [0.17, 0.98, 0.02], [0.0, 0.0, 1.0]], "t": [0.1, -0.2, -1.0], "seed": 73000, "zp": (1.0, 2.0, 0.5)},
        {"id": "proj_zp1", "n": 65, "camera": "barrel61", "R": _rot(0.11, -0.07, 0.3).tolist(), "t": [-0.4, 0.25, 3.0], "seed": 73001, "zp": (1.0,)},
    ]


def proj_points(c):
    """(n, 3) float64: pattern coordinates of a few units, zp cycling through the case's values"""
    rng = np.random.default_rng(c["seed"])
    zp = np.array([c["zp"][k % len(c["zp"])] for k in range(c["n"])])
    return np.stack([rng.uniform(-2.0, 2.0, c["n"]), rng.uniform(-1.5, 1.5, c["n"]), zp], axis=1).astype(F64)
