"""The HOG definition of include/compv_hip.h ("HOG descriptors", items 1 - 8) in numpy float32: one IEEE binary32 rounding per operation, the divide and
the square root correctly rounded, nothing flushed to zero.  tests/golden/make_golden_hog.py holds it against the compiled reference (CompVHOG's
COMPV_HOGS_ID with AVX2 and FMA3 switched off) byte for byte; the host checker (tests/host/hog_math_check.cpp) and the kernels are held against it.

The pixels of all cells are processed side by side (one numpy operation per pixel POSITION of a cell), which keeps the per-histogram order of the
definition: row-major inside a cell, in BILINEAR first the neighbour bin, then the pixel's own."""
import numpy as np

NORM_NONE, NORM_L1, NORM_L1SQRT, NORM_L2, NORM_L2HYS = 1, 2, 3, 4, 5          # COMPVHIP_HOG_NORM_* (0: the default, L2HYS)
GRADIENT_SIGNED, GRADIENT_UNSIGNED = 1, 2                                      # COMPVHIP_HOG_GRADIENT_* (0: the default, signed)
INTERP_NEAREST, INTERP_BILINEAR, INTERP_BILINEAR_LUT = 1, 2, 3                 # COMPVHIP_HOG_INTERP_* (0: the default, BILINEAR); _LUT is refused
NORMS = {"none": NORM_NONE, "l1": NORM_L1, "l1sqrt": NORM_L1SQRT, "l2": NORM_L2, "l2hys": NORM_L2HYS}

f32 = np.float32
EPS_ATAN = f32(2.2204460492503131e-16)                                         # compv_math.cxx:39
P1, P3, P5, P7 = f32(57.2836266), f32(-18.6674461), f32(8.91400051), f32(-2.53972459)          # compv_math.cxx:40-43
EPS_NORM = f32(1e-6)                                                           # hog_std.cxx:96-97
EPS_NORM2 = EPS_NORM * EPS_NORM
HYS_MAX = f32(0.2)

DEFAULTS = dict(blockW=16, blockH=16, strideW=8, strideH=8, cellW=8, cellH=8, nbins=9, blockNorm=NORM_L2HYS, gradientSigned=GRADIENT_SIGNED, interp=INTERP_BILINEAR)
FIELDS = ["blockW", "blockH", "strideW", "strideH", "cellW", "cellH", "nbins", "blockNorm", "gradientSigned", "interp"]


def resolve(opts=None):
    """a dict of some of FIELDS (a missing or zero field takes the default) -> all ten"""
    o = dict(DEFAULTS)
    for k, v in (opts or {}).items():
        assert k in DEFAULTS, k
        if v:
            o[k] = int(v)
    return o


def geometry(W, H, opts=None):
    """-> dict(cellsX, cellsY, validX, validY, blocksX, blocksY, cpbX, cpbY, stepX, stepY, count, descLen), or None where item 8 refuses"""
    o = resolve(opts)
    if min(o[k] for k in FIELDS) < 1:
        return None
    if o["blockNorm"] > NORM_L2HYS or o["gradientSigned"] > GRADIENT_UNSIGNED or o["interp"] not in (INTERP_NEAREST, INTERP_BILINEAR):
        return None
    theta_max = 360 if o["gradientSigned"] == GRADIENT_SIGNED else 180
    if o["nbins"] < 2 or o["nbins"] > 360 or theta_max % o["nbins"]:
        return None
    g = {}
    for ax, size in (("W", W), ("H", H)):
        block, stride, cell = o["block" + ax], o["stride" + ax], o["cell" + ax]
        if block % cell or not (stride == cell or (2 * stride == cell and block == cell)) or size < block:
            return None
        ratio = f32(stride) / f32(cell)                                        # szStrideInCellsCount, hog_std.cxx:219
        cells = int(f32(size // cell) / ratio)                                 # :238-239
        valid = cells - (1 if (cells - 1) * stride + cell > size else 0)       # xGuard / yGuard, :249,255
        x = "X" if ax == "W" else "Y"
        g["cells" + x], g["valid" + x] = cells, valid
        g["blocks" + x] = (size - block) // stride + 1                         # :320-321
        g["cpb" + x] = block // cell
        g["step" + x] = int(float(ratio) + 0.5)                                # COMPV_MATH_ROUNDFU_2_NEAREST_INT, :355,357
    g["count"] = g["cpbX"] * g["cpbY"] * o["nbins"]
    g["descLen"] = g["blocksX"] * g["blocksY"] * g["count"]
    return g


def gradients(img):
    """item 1: central differences, 0 on the frame's border columns (gx) / rows (gy)"""
    I = np.asarray(img, np.uint8).astype(f32)
    gx, gy = np.zeros_like(I), np.zeros_like(I)
    gx[:, 1:-1] = I[:, 2:] - I[:, :-2]
    gy[1:-1, :] = I[2:, :] - I[:-2, :]
    return gx, gy


def magnitude(gx, gy):
    return np.sqrt(gx * gx + gy * gy)                                          # item 2


def direction(gx, gy):
    """item 3: degrees in [0, 360]"""
    ax, ay = np.abs(gx), np.abs(gy)
    flat = ax >= ay
    c = np.where(flat, ay, ax) / (np.where(flat, ax, ay) + EPS_ATAN)
    c2 = c * c
    p = (((P7 * c2 + P5) * c2 + P3) * c2 + P1) * c
    a = np.where(flat, p, f32(90) - p)
    a = np.where(gx < 0, f32(180) - a, a)
    return np.where(gy < 0, f32(360) - a, a).astype(f32)


def cell_histograms(img, opts=None):
    """items 1 - 5: -> float32 [cellsY][cellsX][nbins]; the left-out cells hold 0"""
    o = resolve(opts)
    H, W = img.shape
    g = geometry(W, H, o)
    assert g is not None
    nb = o["nbins"]
    gx, gy = gradients(img)
    mag, ang = magnitude(gx, gy), direction(gx, gy)
    theta_max = f32(360 if o["gradientSigned"] == GRADIENT_SIGNED else 180)
    w = f32(int(theta_max) // nb)
    s = f32(1) / w
    theta = np.where(ang > theta_max, ang - theta_max, ang).astype(f32)
    vy, vx = g["validY"], g["validX"]
    hist = np.zeros((g["cellsY"], g["cellsX"], nb), f32)
    if vy < 1 or vx < 1:
        return hist
    h = np.zeros((vy * vx, nb), f32)
    rows = np.arange(vy * vx)
    oy = (np.arange(vy) * o["strideH"])[:, None]
    ox = (np.arange(vx) * o["strideW"])[None, :]
    for j in range(o["cellH"]):
        for i in range(o["cellW"]):
            m = mag[oy + j, ox + i].reshape(-1)
            t = theta[oy + j, ox + i].reshape(-1)
            if o["interp"] == INTERP_NEAREST:
                b = (t * s).astype(np.int32)
                keep = b < nb                                                  # b == nbins (theta == thetaMax): the vote is dropped
                h[rows[keep], b[keep]] += m[keep]
            else:
                b = (t * s - f32(0.5)).astype(np.int32)                        # truncation
                d = (t - b.astype(f32) * w) * s - f32(0.5)
                v = np.abs(m * d)
                other = np.where(d >= 0, b + 1, b - 1)
                other = np.where(other < 0, nb - 1, np.where(other > nb - 1, 0, other))
                h[rows, other] += v                                            # first the neighbour ...
                h[rows, b] += m - v                                            # ... then the pixel's own bin
    hist[:vy, :vx] = h.reshape(vy, vx, nb)
    return hist


def _ordered_sum(vals):
    """item 7's summation order over the last axis of vals [blocks][count]"""
    count = vals.shape[1]
    c8, c4 = count & ~7, count & ~3
    acc0 = np.zeros((vals.shape[0], 4), f32)
    acc1 = np.zeros((vals.shape[0], 4), f32)
    for i in range(0, c8, 8):
        acc0 = acc0 + vals[:, i:i + 4]
        acc1 = acc1 + vals[:, i + 4:i + 8]
    if c4 > c8:
        acc0 = acc0 + vals[:, c8:c8 + 4]
    a = acc0 + acc1
    total = (a[:, 0] + a[:, 2]) + (a[:, 1] + a[:, 3])
    for i in range(c4, count):
        total = total + vals[:, i]
    return total


def _l1(v):
    return v * (f32(1) / (_ordered_sum(v) + EPS_NORM))[:, None]


def _l2(v):
    return v * (f32(1) / np.sqrt(_ordered_sum(v * v) + EPS_NORM2))[:, None]


def normalize(v, norm):
    """item 7 on float32 [blocks][count]"""
    if norm == NORM_NONE:
        return v
    if norm == NORM_L1:
        return _l1(v)
    if norm == NORM_L1SQRT:
        return np.sqrt(_l1(v))
    if norm == NORM_L2:
        return _l2(v)
    assert norm == NORM_L2HYS
    return _l2(np.minimum(_l2(v), HYS_MAX))


def blocks(hist, g, o):
    """item 6: the cells of every block, row-major blocks, inside a block cell row / cell / bin -> float32 [blocks][count]"""
    nb = o["nbins"]
    out = np.zeros((g["blocksY"], g["blocksX"], g["cpbY"], g["cpbX"] * nb), f32)
    for by in range(g["blocksY"]):
        for bx in range(g["blocksX"]):
            y0, x0 = by * g["stepY"], bx * g["stepX"]
            out[by, bx] = hist[y0:y0 + g["cpbY"], x0:x0 + g["cpbX"]].reshape(g["cpbY"], -1)
    return out.reshape(g["blocksY"] * g["blocksX"], g["count"])


def hog(img, opts=None):
    """-> (descriptor float32 [descLen], cell map float32 [cellsY][cellsX][nbins])"""
    o = resolve(opts)
    g = geometry(img.shape[1], img.shape[0], o)
    assert g is not None, "refused parameters"
    hist = cell_histograms(img, o)
    return np.ascontiguousarray(normalize(blocks(hist, g, o), o["blockNorm"]), f32).reshape(-1), hist
