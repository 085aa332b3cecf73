"""ORB keypoints and descriptors as include/compv_hip.h and docs/kernels/orb.md define them, in numpy: the border erase, the intensity-centroid
moments and orientation, the Q16 Gaussian blur and the rotated BRIEF-256/31.  float32 arithmetic step by step (every product and sum is one numpy
float32 operation, so nothing is fused), atan2 / cos / sin in float64 rounded once to float32, np.rint (ties to even) for the rotated coordinates.
Pinned to literals and to the compiled reference's outputs (tests/golden/golden_orb.json) by tests/test_orb_model.py; the GPU tests compare the
library with it byte for byte.

The model and a device can disagree only where a float64 atan2 / cos / sin lies within about 2^-50 relative of a float32 rounding midpoint and the
two libms round it to different sides: about 1e-8 per value."""
import numpy as np

BORDER = 18          # (31 + 5) >> 1
RADIUS = 15
KEYPOINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("strength", "<f4"), ("orient", "<f4"), ("level", "<i4"), ("size", "<f4")])
CORNER_DTYPE = np.dtype([("x", "<i4"), ("y", "<i4"), ("strength", "<i4")])
F32 = np.float32
PI_F = F32(3.1415926535897932384626433)
K180_OVER_PI = F32(180.0) / PI_F          # float32 quotients, as base/math/compv_math.cxx evaluates them
KPI_OVER_180 = PI_F / F32(180.0)
FIXED_ORIENTS = (0.0, 45.0, 60.0, 90.0, 180.0, 270.0, 359.99997)

# The rBRIEF pattern of the ORB method, one word per test: int8 AX | AY << 8 | BX << 16 | BY << 24
PATTERN = np.array([
    0x0509fd08, 0xf4070204, 0x02f809f5, 0xf30cf407, 0x0c02f302, 0x0601f901, 0xfcfef6fe, 0xf8f5f3f3,
    0xf7f4fdf3, 0x090b040a, 0xf7f8f8f3, 0x0cf707f5, 0x060c0707, 0x00fdfbfc, 0xfdf402f3, 0x05f900f7,
    0xff0cfa0c, 0x0cfe06fd, 0xf8fcf3fa, 0xf80cf30b, 0x01050704, 0xfd0afd05, 0x0c06f903, 0xfefaf9f8,
    0xf6ff0bfe, 0x0af80cf3, 0xfdfb03f9, 0x07fd02fc, 0x0bfaf4f6, 0xf906f405, 0xff07fa05, 0xfb040001,
    0xf30b0b09, 0x0c040704, 0x0404ff02, 0x07fef4fc, 0xf6f9fbf8, 0x0c090b04, 0xf301f800, 0x02f8fef3,
    0x03fefefd, 0xf7fc09fa, 0x070a0c08, 0x03010900, 0xf60bfb07, 0x00f5faf3, 0x010c070a, 0x0cfafdfa,
    0xfc0cf70a, 0xf4f808f3, 0xfcf800f3, 0x08070303, 0xf90a0705, 0xf40107ff, 0x0605f603, 0xf603fc02,
    0x05f300f3, 0x0cf4f9f3, 0x08f503f3, 0x07fc0cf9, 0x080cf606, 0xfaf9fff7, 0x0c00fbfe, 0x05f905f4,
    0xf308f603, 0x05fcf9f9, 0xf9fffefd, 0xf5050902, 0xf3fbf3f5, 0xff0006ff, 0x0205fd05, 0x0cfcf3fc,
    0x06f7faf7, 0xfcf8f6f4, 0xfd0c020a, 0x0c0c0c07, 0x05faf3f9, 0x04fd09fc, 0x020cff07, 0x01fb06f9,
    0x05f40bf3, 0xfafe07fd, 0xf90cf807, 0xf4f5f9f3, 0x0c0cfd01, 0x0003fa02, 0xf3fe03fc, 0x0901f3ff,
    0xfa080107, 0x0c03ff01, 0x060c0109, 0x03fff7ff, 0x05f6f3f3, 0x0c0a0707, 0x090cfb0c, 0x0b070306,
    0x0a06f305, 0x0302f402, 0xfa040803, 0xf30c0602, 0x030af409, 0x09f904f8, 0xfafc0cf5, 0xf8020c01,
    0xfc07f706, 0xfe030302, 0x000b0306, 0xf808fd03, 0x03090807, 0xfcfafbf5, 0x0afb0bf6, 0x0cfdf8fb,
    0x00f705f6, 0xfa0cff08, 0xf506fa04, 0x07f80cf6, 0x0706fe04, 0x0cfe00fe, 0x02fbf8fb, 0x0c0afa07,
    0xf8f8f3f7, 0xfefbf3fb, 0xf309f808, 0x00f7f5f7, 0xfe01f801, 0x0109fc07, 0xfcff01fe, 0xf50cfa0b,
    0x04faf7f4, 0x0c070703, 0x080a0505, 0x0802fc00, 0xf3fb0cf7, 0x0c020700, 0x070102ff, 0xf7070b05,
    0xf8060503, 0x09f8fcf3, 0xfdfd09fb, 0xf4fdf9fc, 0x00080506, 0x0cfa06f9, 0xfefb06f3, 0x0a03f601,
    0xfc080104, 0xf302fefe, 0x0c0cf402, 0xfa00f3fe, 0x03090104, 0xfbfdf6fa, 0x01fff3fd, 0xf50c0507,
    0xf905fe04, 0xfbf709f3, 0x06080107, 0x0607f807, 0x01f9fcf9, 0xf8f90bf8, 0xf8f406f3, 0x09030402,
    0x030cfb0a, 0x07fafbfa, 0xf809fd08, 0x0802f402, 0x03f6fef5, 0xf7f9f3f4, 0xfbf600f5, 0x080bfd05,
    0x0cfff3fe, 0x0900f8ff, 0xfbf4f5f3, 0x0bf6fef6, 0xf3fe09fd, 0x0203fd02, 0x00fcf3f7, 0xf6fd06fc,
    0xf9fe0cfc, 0x09fcf5fa, 0x0b06fd06, 0x05fb0bf3, 0x060c0b0b, 0xfe0cfb07, 0x07000cff, 0xfefdf8fc,
    0x07fa01f9, 0xf3f8f4f3, 0xf8fafef9, 0xf7fa05f8, 0x05fcfffb, 0x0af807f3, 0xf3050501, 0xf30a0001,
    0xff0a0c09, 0xf70af805, 0xf3010bff, 0x02fafdf7, 0x0c01f6ff, 0xf6f801f3, 0xfa0af508, 0xfa03f302,
    0xf70cf307, 0xf9fbf6f6, 0xf3f8f8f6, 0x0508fa04, 0xf3080c03, 0xfdfd02fc, 0xf40af305, 0xff05f304,
    0x03fc09f7, 0xf7030300, 0x01fa01f4, 0xf8040203, 0x09f6f6f6, 0x0c0cf308, 0xfbfaf4f8, 0x07030202,
    0xf80b060a, 0xf4080806, 0x05fa0af9, 0x09fdf7fd, 0x05fff3ff, 0x04fdf9fd, 0x03f8fef8, 0x0c0c0204,
    0x0b03fb02, 0xf30bf706, 0x0c07ff03, 0x040cff0b, 0x06fd00fd, 0x0c04f504, 0x0102fc02, 0x01f8faf6,
    0x01f507f3, 0xf3f50cf3, 0xf30b0006, 0x0401ff00, 0xfef703f3, 0xfdfa08f7, 0xfef8faf3, 0x0a08f705,
    0xf7030702, 0xfffffaff, 0xfe0b0509, 0xf80cfd0b, 0x05030003, 0x0a0004ff, 0x0504fa03, 0x05f600f3,
    0x0b0c0805, 0xfa090908, 0xf408fc07, 0x09f604f6, 0x040c0307, 0xfe0af909, 0xfe0c0007, 0xf500faff,
], dtype=np.uint32)


def pattern():
    """-> AX, AY, BX, BY as float32 arrays of 256"""
    b = PATTERN.view(np.int8).reshape(256, 4)
    return tuple(b[:, k].astype(F32) for k in range(4))


DX = [int(np.sqrt(RADIUS * RADIUS - k * k)) for k in range(RADIUS + 1)]
_DISC = np.array([(i, j) for j in range(-RADIUS, RADIUS + 1) for i in range(-DX[abs(j)], DX[abs(j)] + 1)], np.int64)          # (i, j)


def admissible(x, y, W, H):
    """not erased by eraseTooCloseToBorder with b = 18"""
    x, y = np.asarray(x), np.asarray(y)
    return ~((x < BORDER) | (x + BORDER >= W) | (y < BORDER) | (y + BORDER >= H))


def moments(img, xs, ys):
    """-> (m01, m10) int32 arrays: sums of j * I and i * I over the disc of radius 15 around every (x, y)"""
    xs, ys = np.asarray(xs, np.int64), np.asarray(ys, np.int64)
    if len(xs) == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.int32)
    v = img[ys[:, None] + _DISC[None, :, 1], xs[:, None] + _DISC[None, :, 0]].astype(np.int64)
    return (v * _DISC[None, :, 1]).sum(axis=1).astype(np.int32), (v * _DISC[None, :, 0]).sum(axis=1).astype(np.int32)


def orient_of(m01, m10):
    """the canonical orientation in degrees, float32, in [0, 360]"""
    rad = np.arctan2(np.asarray(m01, np.float64), np.asarray(m10, np.float64)).astype(F32)
    o = rad * K180_OVER_PI
    return np.where(o < 0, o + F32(360.0), o).astype(F32)


def keypoints(img, corners, level=0, scale=1.0):
    """corners (CORNER_DTYPE) of one level -> (KEYPOINT_DTYPE records of the survivors in their order, (n, 2) int32 {m01, m10})"""
    H, W = img.shape
    scale = F32(scale)
    c = corners[admissible(corners["x"], corners["y"], W, H)]
    m01, m10 = moments(img, c["x"], c["y"])
    k = np.zeros(len(c), KEYPOINT_DTYPE)
    x, y = c["x"].astype(F32), c["y"].astype(F32)
    if level != 0:
        sfi = F32(1.0) / scale
        x, y = x * sfi, y * sfi
    k["x"], k["y"], k["strength"], k["orient"], k["level"], k["size"] = x, y, c["strength"].astype(F32), orient_of(m01, m10), level, F32(31.0) / scale
    return k, np.stack([m01, m10], axis=1).astype(np.int32).reshape(len(c), 2)


def gauss_kernel_q16(size=5, sigma=2.0):
    """CompVMathGauss::kernelDim1FixedPoint (compv_math_gauss.h:24-55 with T = float, then compv_math_convlt.h:88), operation by operation"""
    sigma = F32(sigma)
    half = size >> 1
    s2x2 = F32(2.0) * (sigma * sigma)
    a = F32(1.0 / np.sqrt(np.pi * np.float64(s2x2)))
    f = np.zeros(size, F32)
    f[half] = a
    total = a
    for x in range(1, half + 1):
        k = F32(np.float64(a) * np.exp(-np.float64(F32(x * x) / s2x2)))
        f[half + x] = f[half - x] = k
        total = total + (k + k)
    total = F32(1.0) / total
    return np.array([int(v * total * F32(65535.0)) for v in f], np.uint16)


def blur(img):
    """CompVMathConvlt::convlt1FixedPoint with the Q16 Gaussian (5, 2.0) on both axes: horizontal pass, u8, vertical pass; zero output border of 2"""
    H, W = img.shape
    k = gauss_kernel_q16().astype(np.uint32)
    src = img.astype(np.uint32)
    hz = np.zeros((H, W), np.uint32)
    hz[:, 2:W - 2] = np.minimum(sum((src[:, t:W - 4 + t] * k[t]) >> 16 for t in range(5)), 255)
    out = np.zeros((H, W), np.uint32)
    out[2:H - 2, :] = np.minimum(sum((hz[t:H - 4 + t, :] * k[t]) >> 16 for t in range(5)), 255)
    return out.astype(np.uint8)


def centre(v, scale):
    """(int)((double)(v * scale) + 0.5), and whether that is a finite value an int32 holds"""
    with np.errstate(all="ignore"):
        d = (np.asarray(v, F32) * F32(scale)).astype(np.float64) + 0.5
        ok = np.isfinite(d) & (np.abs(d) < 2.0 ** 31)
        return np.where(ok, np.trunc(np.where(ok, d, 0.0)), -1).astype(np.int64), ok


def canonical_cos_sin(orient):
    a = np.asarray(orient, F32) * KPI_OVER_180
    return np.cos(a.astype(np.float64)).astype(F32), np.sin(a.astype(np.float64)).astype(F32), a


def describe(blurred, keys, scale=1.0):
    """-> (n, 32) uint8: row q is the descriptor of keys[q] on the BLURRED plane; a key too close to a border gets a zero row"""
    H, W = blurred.shape
    n = len(keys)
    out = np.zeros((n, 32), np.uint8)
    if n == 0:
        return out
    xi, okx = centre(keys["x"], scale)
    yi, oky = centre(keys["y"], scale)
    inside = okx & oky & (xi >= BORDER) & (xi < W - BORDER) & (yi >= BORDER) & (yi < H - BORDER)
    fcos, fsin, _ = canonical_cos_sin(keys["orient"][inside])
    fcos, fsin = fcos[:, None], fsin[:, None]
    AX, AY, BX, BY = (p[None, :] for p in pattern())
    cx, cy = xi[inside][:, None], yi[inside][:, None]

    def sample(PX, PY):
        x = np.rint(PX * fcos - PY * fsin).astype(np.int64)          # two float32 products, one float32 difference; ties to even
        y = np.rint(PX * fsin + PY * fcos).astype(np.int64)
        return blurred[cy + y, cx + x]

    bits = sample(AX, AY) < sample(BX, BY)
    out[inside] = np.packbits(bits, axis=1, bitorder="little")
    return out


# ---- frame content (with fast_model's noise and blocks) -----------------------------------------------------------------------------------
def constant(W, H, level=97):
    return np.full((H, W), level, np.uint8)


def ramp(W, H):
    """horizontal ramp: every column constant, so m01 == 0"""
    return np.tile((np.arange(W) * 3 % 256).astype(np.uint8), (H, 1))


def mirrored(img):
    """left half mirrored onto the right about the central column (W odd) or the central gap (W even): m10 == 0 at the centre of an odd width"""
    out = img.copy()
    W = img.shape[1]
    out[:, W - (W // 2):] = img[:, :W // 2][:, ::-1]
    return out
