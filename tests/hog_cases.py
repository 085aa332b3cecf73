"""The HOG test cases and their frames, shared by tests/golden/make_golden_hog.py, the CPU tests and tests/test_gpu_hog.py.

A case is (id, W, H, frame kind, opts): the frame is generated, never stored (numpy's legacy RandomState is stable across versions).  Layouts are written
(block, stride, cell, nbins) like the reference's unit test; the sizes are the smallest at which each rule of the definition is exercised:
 16 x 16 defaults   one block, every pixel next to a border rule
 37 x 29            ragged in both axes
 64 x 48 (8,4,8)    stride = cell / 2: the last cell column AND row are left out (at 37 x 29 none is: 28 + 8 <= 37 and 20 + 8 <= 29)
 (12,6,6)           a cell width that is no multiple of 4;  (8x16, 4x8, 4x8, 6 unsigned): rectangular, block count 6
 block == cell, 15 bins: block count 15 = 8 + 4 + 3, every part of the norm's summation order;  360 bins: the largest histogram"""
import numpy as np

import hog_model as hm


def noise(W, H, seed=1):
    return np.random.RandomState(1000 + seed).randint(0, 256, (H, W)).astype(np.uint8)


def blocks(W, H, seed=1):
    """5 wide, 7 high rectangles of one random value each: flat interiors (zero gradients) and axis-aligned edges (gy = 0 with gx < 0: the dropped vote)"""
    r = np.random.RandomState(2000 + seed).randint(0, 256, ((H + 6) // 7, (W + 4) // 5)).astype(np.uint8)
    return np.ascontiguousarray(np.repeat(np.repeat(r, 7, 0), 5, 1)[:H, :W])


def checkerboard(W, H, seed=0):
    """0 / 255 in 2 x 2 squares (in 1 x 1 squares the central differences would all be 0): |gx| = |gy| = 255 away from the border, the largest
    magnitude a frame can hold, sqrt(2) * 255; shifted by one pixel per seed"""
    y, x = np.mgrid[0:H, 0:W]
    return (((((x + seed) >> 1) + (y >> 1)) & 1) * 255).astype(np.uint8)


def constant(W, H, seed=0):
    return np.full((H, W), (77 + 50 * seed) & 255, np.uint8)


FRAMES = {"noise": noise, "blocks": blocks, "checkerboard": checkerboard, "constant": constant}


def frame(kind, W, H, seed=1):
    return FRAMES[kind](W, H, seed)


def layout(block, stride, cell, nbins=9, norm=hm.NORM_L2HYS, signed=True, interp=hm.INTERP_BILINEAR):
    """block / stride / cell: a number (square) or (w, h)"""
    bw, bh = (block, block) if np.isscalar(block) else block
    sw, sh = (stride, stride) if np.isscalar(stride) else stride
    cw, ch = (cell, cell) if np.isscalar(cell) else cell
    return dict(blockW=bw, blockH=bh, strideW=sw, strideH=sh, cellW=cw, cellH=ch, nbins=nbins, blockNorm=norm,
                gradientSigned=hm.GRADIENT_SIGNED if signed else hm.GRADIENT_UNSIGNED, interp=interp)


ALL_NORMS = [hm.NORM_NONE, hm.NORM_L1, hm.NORM_L1SQRT, hm.NORM_L2, hm.NORM_L2HYS]
NORM_NAMES = {v: k for k, v in hm.NORMS.items()}

# the seven layouts of the definition's check against the reference
LAYOUTS = {
    "b16s8c8": layout(16, 8, 8),
    "b8s4c8": layout(8, 4, 8),
    "b8s4c4": layout(8, 4, 4),
    "b12s6c6": layout(12, 6, 6),
    "b16s8c8n18": layout(16, 8, 8, 18),
    "b16s8c8u": layout(16, 8, 8, 9, signed=False),
    "rect6u": layout((8, 16), (4, 8), (4, 8), 6, signed=False),
}


def _cases():
    out = []

    def add(cid, W, H, kind, o):
        assert hm.geometry(W, H, o) is not None, cid
        out.append(dict(id=cid, W=W, H=H, kind=kind, opts=o))
    for name, o in LAYOUTS.items():                                   # bilinear on every layout, 37 x 29 noise
        add("%s_noise37x29" % name, 37, 29, "noise", o)
    for signed in (True, False):                                      # nearest, signed and unsigned: the dropped vote (blocks: gy = 0 with gx < 0)
        o = layout(16, 8, 8, signed=signed, interp=hm.INTERP_NEAREST)
        for kind in ("noise", "blocks"):
            add("nearest_%s_%s37x29" % ("s" if signed else "u", kind), 37, 29, kind, o)
    for norm in ALL_NORMS:                                            # all five norms at counts 36, 9 and 15
        add("norm_%s_c36_noise37x29" % NORM_NAMES[norm], 37, 29, "noise", layout(16, 8, 8, norm=norm))
        add("norm_%s_c9_noise37x29" % NORM_NAMES[norm], 37, 29, "noise", layout(8, 4, 8, norm=norm))
        add("norm_%s_c15_noise37x29" % NORM_NAMES[norm], 37, 29, "noise", layout(8, 8, 8, 15, norm=norm, signed=False))
    for norm in (hm.NORM_NONE, hm.NORM_L2HYS):
        for kind, W, H in (("blocks", 37, 29), ("noise", 64, 48), ("blocks", 64, 48)):
            add("norm_%s_c36_%s%dx%d" % (NORM_NAMES[norm], kind, W, H), W, H, kind, layout(16, 8, 8, norm=norm))
    add("b8s4c8_noise64x48", 64, 48, "noise", layout(8, 4, 8))        # cells left out in both axes
    add("b16s8c8_noise16x16", 16, 16, "noise", layout(16, 8, 8))      # one block
    add("n360_noise16x16", 16, 16, "noise", layout(16, 8, 8, 360))    # the largest histogram
    add("n2u_noise16x16", 16, 16, "noise", layout(16, 8, 8, 2, signed=False))   # the smallest: both neighbours of a bin are the other bin
    for norm in ALL_NORMS:                                            # the constant frame: zeros under every norm
        add("norm_%s_constant37x29" % NORM_NAMES[norm], 37, 29, "constant", layout(16, 8, 8, norm=norm))
    add("b16s8c8_checkerboard37x29", 37, 29, "checkerboard", layout(16, 8, 8))          # the largest magnitudes
    add("nearest_u_checkerboard37x29", 37, 29, "checkerboard", layout(16, 8, 8, signed=False, interp=hm.INTERP_NEAREST))
    add("b8c8_noise8x8", 8, 8, "noise", layout(8, 8, 8))              # the frame of the large-batch test: one cell, one block
    add("b16s8c8_noise521x19", 521, 19, "noise", layout(16, 8, 8))    # 65 cells across: one past a wave's 64
    add("b16s8c8_noise19x521", 19, 521, "noise", layout(16, 8, 8))    # 65 cell rows
    add("b64c64_noise130x70", 130, 70, "noise", layout(64, 64, 64))   # a large cell
    return out


CASES = _cases()
BY_ID = {c["id"]: c for c in CASES}
assert len(BY_ID) == len(CASES)
# the one case run with the reference's AVX2 + FMA3 leaf switched on (cell width 8): recorded for docs/kernels/hog.md, compared with nothing
AVX2_CASE = "b16s8c8_noise37x29"
# descriptors up to this many floats are stored in the npz; larger ones as an MD5 of their bytes
STORE_LIMIT = 4096


def case_frame(c, seed=1):
    return frame(c["kind"], c["W"], c["H"], seed)
