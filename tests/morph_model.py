"""The definitions of the thresholding and morphology calls (include/compv_hip.h, docs/kernels/morph.md) in plain numpy; what the GPU is
compared with byte for byte (tests/test_gpu_morph.py), pinned on the CPU by tests/test_morph_model.py: hand-computed literals and
MD5s recorded from the compiled reference (tests/golden/golden_morph.json).

  threshold:  out = in > t8 ? 0xff : 0, t8 = (uint8)(clip(threshold, 0, 255) + 0.5)             compv_image_threshold.cxx:118-180,320-347
  adaptive:   mean = Q16 box filter (hz pass, u8, vt pass, zero border of blockSize/2), then
              out = ((in - mean + 255 >= 256 - d) != invert) ? m : 0                             compv_image_threshold.cxx:183-317
  morph:      interior = min / max over the strel's members, then the border rows and columns   compv_math_morph.cxx:125-247,542-692
  strel:      RECT / CROSS / DIAMOND masks                                                       compv_math_morph.cxx:476-540

All arithmetic is integer; nothing here has a tolerance.
"""
import numpy as np

# COMPV_MATH_MORPH_OP_TYPE_*, COMPV_MATH_MORPH_STREL_TYPE_*, COMPV_BORDER_TYPE_* (compv_common.h:306-310,402-419)
ERODE, DILATE, OPEN, CLOSE = 0, 1, 2, 3
RECT, DIAMOND, CROSS = 0, 1, 2
BORDER_ZERO, BORDER_REPLICATE = 0, 2


def round_u8(v):
    """COMPV_MATH_ROUNDFU_2_NEAREST_INT(COMPV_MATH_CLIP3(0, 255, v)): clip, add a half, truncate."""
    return int(min(max(float(v), 0.0), 255.0) + 0.5)


def threshold(img, thr):
    if thr < 0:
        raise ValueError("threshold < 0")
    return np.where(np.asarray(img, np.uint8) > round_u8(thr), 255, 0).astype(np.uint8)


def mean_weight(block_size):
    """The one Q16 tap of CompVKernel::mean: (uint16)((1.f / blockSize) * 0xffff), in float32."""
    return int(np.uint16(np.float32(np.float32(1.0) / np.float32(block_size)) * np.float32(0xffff)))


def box_mean(img, block_size):
    """convlt1FixedPoint with block_size equal taps: every tap contributes (p * k) >> 16, a pass saturates its sum once."""
    img = np.asarray(img, np.uint8)
    H, W = img.shape
    r = block_size >> 1
    k = mean_weight(block_size)

    def one_pass(src, axis):
        q = (src.astype(np.int64) * k) >> 16
        c = np.cumsum(q, axis=axis)
        c = np.concatenate([np.zeros_like(np.take(c, [0], axis=axis)), c], axis=axis)
        n = src.shape[axis]
        s = np.take(c, np.arange(block_size, n + 1), axis=axis) - np.take(c, np.arange(0, n + 1 - block_size), axis=axis)
        out = np.zeros(src.shape, np.uint8)
        sl = [slice(None), slice(None)]
        sl[axis] = slice(r, n - r)
        out[tuple(sl)] = np.minimum(s, 255).astype(np.uint8)
        return out

    return one_pass(one_pass(img, 1), 0)


def adaptive(img, block_size, delta, max_val=255.0, invert=False):
    img = np.asarray(img, np.uint8)
    H, W = img.shape
    if not (block_size & 1) or block_size < 3 or W < block_size or H < block_size or max_val < 0:
        raise ValueError("adaptive threshold parameters")
    d = round_u8(delta)
    m = round_u8(max_val)
    mean = box_mean(img, block_size)
    hit = (img.astype(np.int32) - mean.astype(np.int32) + 255) >= (256 - d)
    return np.where(hit != bool(invert), m, 0).astype(np.uint8)


def strel(kind, w, h):
    """buildStructuringElementGeneric: [h][w] uint8, 0xff marks a member."""
    if w < 1 or h < 1:
        raise ValueError("empty structuring element")
    s = np.zeros((h, w), np.uint8)
    if kind == RECT:
        s[:] = 255
    elif kind == CROSS:
        s[h >> 1, :] = 255
        s[:, w >> 1] = 255
    elif kind == DIAMOND:
        if w != h:
            raise ValueError("a diamond is square")
        c = w >> 1
        for j in range(h):
            half = j if j <= (h >> 1) else h - 1 - j
            s[j, c - half:c + half + 1] = 255
    else:
        raise ValueError("structuring element type")
    return s


def basic(img, se, dilate, border):
    """One basicOper: interior from the members (same offsets for erode and dilate: no reflection), then the vertical border
    ((sh + 1) >> 1 rows top and bottom), then the horizontal one (sw >> 1 columns left and right)."""
    img = np.asarray(img, np.uint8)
    se = np.asarray(se)
    H, W = img.shape
    sh, sw = se.shape
    if not se.any() or W < sw or H < sh:
        raise ValueError("structuring element empty or larger than the image")
    wd, hd, hb = sw >> 1, sh >> 1, (sh + 1) >> 1
    oh, ow = H - 2 * hd, W - 2 * wd
    out = np.zeros((H, W), np.uint8)
    acc = None
    for j, i in zip(*np.nonzero(se)):
        v = img[j:j + oh, i:i + ow]
        acc = v.copy() if acc is None else (np.maximum(acc, v) if dilate else np.minimum(acc, v))
    out[hd:hd + oh, wd:wd + ow] = acc
    edge = img if border == BORDER_REPLICATE else np.zeros_like(img)
    out[:hb] = edge[:hb]
    out[H - hb:] = edge[H - hb:]
    if wd:
        out[:, :wd] = edge[:, :wd]
        out[:, W - wd:] = edge[:, W - wd:]
    return out


def morph(img, se, op, border=BORDER_REPLICATE):
    if border not in (BORDER_ZERO, BORDER_REPLICATE):
        raise ValueError("border type")
    if op == ERODE:
        return basic(img, se, False, border)
    if op == DILATE:
        return basic(img, se, True, border)
    if op == OPEN:
        return basic(basic(img, se, False, border), se, True, border)
    if op == CLOSE:
        return basic(basic(img, se, True, border), se, False, border)
    raise ValueError("morph op")
