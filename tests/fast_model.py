"""FAST corner detection as include/compv_hip.h and docs/kernels/fast.md define it, in numpy: score map, non-maximum suppression, the
raster-ordered corner list and the canonical maxFeatures cut.  Pinned to hand-computed literals and to the compiled reference's outputs
(tests/golden/golden_fast.json) by tests/test_fast_model.py; the GPU tests compare the library with it byte for byte.

Also the seeded frame content the fixture generator and the tests share (integer arithmetic only: any machine regenerates the same bytes)."""
import numpy as np

# clockwise from the top: (dx, dy)
RING = ((0, -3), (1, -3), (2, -2), (3, -1), (3, 0), (3, 1), (2, 2), (1, 3), (0, 3), (-1, 3), (-2, 2), (-3, 1), (-3, 0), (-3, -1), (-2, -2), (-1, -3))
CORNER_DTYPE = np.dtype([("x", "<i4"), ("y", "<i4"), ("strength", "<i4")])


def _ring_differences(img, t):
    H, W = img.shape
    assert W >= 7 and H >= 7
    t = min(max(int(t), 0), 255)
    I = img.astype(np.int16)
    c = I[3:H - 3, 3:W - 3]
    b, d = np.minimum(255, c + t), np.maximum(0, c - t)
    ring = [I[3 + dy:H - 3 + dy, 3 + dx:W - 3 + dx] for (dx, dy) in RING]
    return np.stack([np.maximum(0, d - p) for p in ring]), np.stack([np.maximum(0, p - b) for p in ring])


def score_map_direct(img, t, N):
    """The definition, arc by arc.  (H, W) uint8: max over the 16 arcs of N consecutive ring positions of the arc's smallest darker / brighter
    difference; 0 outside 3 <= x < W - 3, 3 <= y < H - 3."""
    assert N in (9, 12)
    H, W = img.shape
    D, B = _ring_differences(img, t)
    best = np.zeros(D.shape[1:], np.int16)
    for k in range(16):
        arc = [(k + j) & 15 for j in range(N)]
        best = np.maximum(best, np.maximum(D[arc].min(axis=0), B[arc].min(axis=0)))
    out = np.zeros((H, W), np.uint8)
    out[3:H - 3, 3:W - 3] = best
    return out


def score_map(img, t, N):
    """score_map_direct with the arc minima built by doubling (runs of 2, 4, 8, then 8 + 1 or 8 + 4 positions): the same values, several times
    faster on the frames of the GPU tests.  tests/test_fast_model.py holds the two against each other."""
    assert N in (9, 12)
    H, W = img.shape
    out = np.zeros((H, W), np.uint8)
    best = None
    for V in _ring_differences(img, t):
        m2 = np.minimum(V, np.roll(V, -1, axis=0))
        m4 = np.minimum(m2, np.roll(m2, -2, axis=0))
        m8 = np.minimum(m4, np.roll(m4, -4, axis=0))
        arcs = np.minimum(m8, np.roll(V if N == 9 else m4, -8, axis=0)).max(axis=0)
        best = arcs if best is None else np.maximum(best, arcs)
    out[3:H - 3, 3:W - 3] = best
    return out


def nms(scores):
    """a pixel with score s > 0 is dropped when any of its 8 neighbours scores >= s (all comparisons on the scores before suppression)"""
    H, W = scores.shape
    p = np.zeros((H + 2, W + 2), np.int32)
    p[1:-1, 1:-1] = scores
    m = np.zeros((H, W), np.int32)
    for dy in (0, 1, 2):
        for dx in (0, 1, 2):
            if (dy, dx) != (1, 1):
                m = np.maximum(m, p[dy:dy + H, dx:dx + W])
    return np.where(scores.astype(np.int32) > m, scores, 0).astype(np.uint8)


def records(scores, t):
    """raster-ordered {x, y, strength = score + t - 1} of every non-zero score"""
    t = min(max(int(t), 0), 255)
    ys, xs = np.nonzero(scores)          # row-major: y, then x
    rec = np.zeros(len(xs), CORNER_DTYPE)
    rec["x"], rec["y"], rec["strength"] = xs, ys, scores[ys, xs].astype(np.int32) + t - 1
    return rec


def cut(rec, max_features):
    """the canonical cut: with s* the max_features-th largest strength, every corner with strength >= s*, in raster order"""
    if max_features <= 1 or len(rec) <= max_features:
        return rec
    s_star = np.sort(rec["strength"])[::-1][max_features - 1]
    return rec[rec["strength"] >= s_star]


def fast(img, t, N=9, nonmax=True, max_features=-1):
    """-> (records, score map as compvhip_plan_fast writes it: after NMS when NMS is on, untouched by the cut)"""
    s = score_map(img, t, N)
    if nonmax:
        s = nms(s)
    return cut(records(s, t), max_features), s


# ---- frame content ---------------------------------------------------------------------------------------------------------------------
def noise(W, H, seed):
    return np.random.default_rng(seed).integers(0, 256, (H, W), dtype=np.uint8)


def blocks(W, H, seed):
    """rectangles of random gray levels on a random flat ground, then a 3 x 3 box blur (edge replicated, integer division): real corners, soft
    edges and flat plateaus"""
    rng = np.random.default_rng(seed)
    img = np.full((H, W), int(rng.integers(0, 256)), np.int32)
    for _ in range(max(4, W * H // 300)):
        x, y = int(rng.integers(0, W)), int(rng.integers(0, H))
        w, h = int(rng.integers(2, 24)), int(rng.integers(2, 24))
        img[y:y + h, x:x + w] = int(rng.integers(0, 256))
    p = np.pad(img, 1, mode="edge")
    acc = sum(p[dy:dy + H, dx:dx + W] for dy in range(3) for dx in range(3))
    return (acc // 9).astype(np.uint8)


def seam_noise(W, H, seed, tw=128, th=32):
    """flat gray except for noise in the 4 columns either side of every multiple of tw and the 4 rows either side of every multiple of th: all
    corners sit on the tile seams of the score kernel (an arc of 9 cannot lie inside a band seen from outside it)"""
    rng = np.random.default_rng(seed)
    img = np.full((H, W), 128, np.uint8)
    rnd = rng.integers(0, 256, (H, W), dtype=np.uint8)
    band = np.zeros((H, W), bool)
    for x0 in range(tw, W + 4, tw):
        band[:, max(0, x0 - 4):x0 + 4] = True
    for y0 in range(th, H + 4, th):
        band[max(0, y0 - 4):y0 + 4, :] = True
    img[band] = rnd[band]
    return img


def tied_arcs(W, H, seed, t=20):
    """isolated arcs of 9 brighter ring pixels around centres 10 apart on a flat ground of 100, each exceeding b = 100 + t by 1, 2 or 3: many
    corners, three strengths"""
    rng = np.random.default_rng(seed)
    img = np.full((H, W), 100, np.uint8)
    for cy in range(4, H - 4, 10):
        for cx in range(4, W - 4, 10):
            k0, delta = int(rng.integers(0, 16)), int(rng.integers(1, 4))
            for j in range(9):
                dx, dy = RING[(k0 + j) & 15]
                img[cy + dy, cx + dx] = 100 + t + delta
    return img
