"""The inputs of the bicubic fixtures (tests/golden/golden_bicubic.json / .npz, written by tests/golden/make_golden_bicubic.py) and of the tests that
use them: the remap and warp cases of tests/remap_cases.py as they stand -- frame 0 is rc.frame(w, h, seed), a noise frame -- plus narrow sources,
where the four taps clamp on both sides at once, and a map with NaN and infinite entries.

S of a narrow source is the source stride the host checker (tests/host/bicubic_math_check.cpp) runs it at: below 4 it gathers single bytes, from 4 on
it reads a tap row as one 4-byte word the way the kernel does.  The library's own calls never see a stride below 8 (a plan's stride is a multiple of
8, the host calls stage a plane at a multiple of 64), so the GPU tests run these sources through the host calls and, where a plan takes the size, at S = 8."""
import numpy as np

import bicubic_model as bm
import remap_cases as rc

F32 = np.float32
INTERPS = (bm.BICUBIC, bm.BICUBIC_FLOAT32)
INTERP_NAMES = {bm.BICUBIC: "bicubic", bm.BICUBIC_FLOAT32: "bicubic_f32"}

# Win, Hin, S, Wout, Hout
NARROW = ((1, 1, 1, 5, 3),          # one pixel: all 16 taps are it
          (3, 2, 3, 6, 4),          # narrower than the 4 taps, stride below a 4-byte word
          (3, 2, 8, 6, 4),          # the same frame where a word fits: base 0, selectors 0 .. 2
          (4, 4, 4, 7, 5),          # the base clamp max(Win - 4, 0) = 0: one word is the whole row
          (5, 4, 5, 9, 3))          # both clamps one column apart: base 0 or 1


def remap_cases():
    return rc.remap_cases()


def warp_cases():
    return rc.warp_cases()


def narrow_map(w, h, w_out, h_out, seed):
    """float32 maps reaching one pixel outside the frame; the first row starts with the corners, the integers and the values half a pixel inside the last one"""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1.0, w, (h_out, w_out)).astype(F32)
    y = rng.uniform(-1.0, h, (h_out, w_out)).astype(F32)
    ex = (0.0, w - 1.0, max(w - 1.5, 0.0), min(0.5, w - 1.0), float(np.nextafter(F32(w - 1), F32(0))) if w > 1 else 0.0)
    ey = (0.0, h - 1.0, max(h - 1.5, 0.0), min(0.5, h - 1.0), float(np.nextafter(F32(h - 1), F32(0))) if h > 1 else 0.0)
    for k in range(w_out):
        x[0, k], y[0, k] = ex[k % 5], ey[(k // 2) % 5]
        x[h_out - 1, k], y[h_out - 1, k] = ex[(k + 1) % 5], ey[k % 5]
    return x, y


def narrow_cases():
    """dicts: id, size (Win, Hin, Wout, Hout), S, frame seed, map seed, default value"""
    return [{"id": "narrow%dx%d_s%d" % (w, h, s), "size": (w, h, wo, ho), "S": s, "seed": 67000 + k, "map_seed": 68000 + k, "roi": None, "default": (7, 250, 250, 0, 131)[k]}
            for k, (w, h, s, wo, ho) in enumerate(NARROW)]


NAN_ENTRIES = ((0, 0, np.nan, 1.0), (1, 5, 1.0, np.nan), (2, 9, np.inf, 1.0), (3, 60, 1.0, -np.inf), (36, 60, -np.inf, np.nan), (7, 13, np.nan, np.nan))


def nan_case():
    """every coordinate inside the frame except NAN_ENTRIES (row, column, x, y).  Model only: the reference's bicubic leaf tests `x < left || ...`, takes
    a NaN for inside and reads wherever the cast lands."""
    return {"id": "map_nan", "size": rc.SIZES[0], "seed": 64001, "map_seed": 64002, "roi": None, "default": 201, "nan": True}


def nan_map():
    w, h, wo, ho = rc.SIZES[0]
    x, y = rc.random_map(w, h, wo, ho, 64002)
    x, y = np.clip(x, 0, w - 1).astype(F32), np.clip(y, 0, h - 1).astype(F32)
    for (j, i, vx, vy) in NAN_ENTRIES:
        x[j, i], y[j, i] = vx, vy
    return x, y


def map_of(c):
    """the maps of a remap, narrow or NaN case"""
    w, h, wo, ho = c["size"]
    if c["id"] == "map_nan":
        return nan_map()
    if c["id"].startswith("narrow"):
        return narrow_map(w, h, wo, ho, c["map_seed"])
    return rc.random_map(w, h, wo, ho, c["map_seed"])


def all_map_cases():
    return remap_cases() + narrow_cases() + [nan_case()]


def key(cid, interp):
    return "%s_%s" % (cid, INTERP_NAMES[interp])
