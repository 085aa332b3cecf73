"""What the morphology GPU test shares with the large-batch test: the structuring elements and the text-like stroke frames."""
import numpy as np

import morph_model as mm


def off_centre(sw, sh, j, i):
    s = np.zeros((sh, sw), np.uint8)
    s[j, i] = 7
    return s


STRELS = {
    "rect3x3": mm.strel(mm.RECT, 3, 3), "rect1x5": mm.strel(mm.RECT, 1, 5), "rect5x1": mm.strel(mm.RECT, 5, 1), "rect15x3": mm.strel(mm.RECT, 15, 3),
    "rect3x15": mm.strel(mm.RECT, 3, 15), "cross5x5": mm.strel(mm.CROSS, 5, 5), "cross31x3": mm.strel(mm.CROSS, 31, 3), "diamond7x7": mm.strel(mm.DIAMOND, 7, 7),
    "random5x7": (np.random.default_rng(57).random((7, 5)) < 0.4).astype(np.uint8) * 255, "single": off_centre(5, 3, 0, 4),
}
assert STRELS["random5x7"].any()


def strokes(W, H, seed):
    """binary {0, 255} text-like strokes"""
    rng = np.random.default_rng(seed)
    img = np.zeros((H, W), np.uint8)
    for _ in range(max(3, W * H // 60)):
        x, y, ln = int(rng.integers(0, W)), int(rng.integers(0, H)), int(rng.integers(2, 9))
        if rng.integers(0, 2):
            img[y, x:x + ln] = 255
        else:
            img[y:y + ln, x] = 255
    return img
