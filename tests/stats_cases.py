"""The image statistics test cases and their frames, shared by tests/golden/make_golden_stats.py, the CPU tests and tests/test_gpu_stats.py.

A case is (id, W, H, frame kind): the frame is generated, never stored (numpy's legacy RandomState is stable across versions).  The sizes are the smallest at
which each path of the kernels is taken (compv_amd/csrc/kernels.hpp: kStatsTile 64 columns, kStatsBandRows 16 rows; the band-sums kernel takes four columns per
thread, one wave up to 256 columns, 256 threads = 1024 columns at a time beyond; the histogram and equalisation kernels cut a frame into chunks of at least
16 rows that four waves walk row by row, four pixels per lane = 256 columns at a time):
 1 x 1, 1 x 300, 300 x 1, 7 x 5    single pixels, rows and columns; 5 rows: one past the four waves of a chunk
 65 x 3, 64 x 33                   one past / exactly a tile of the integral kernel; one row past two bands
 33 x 17                           one past a band, and one past a 16-row chunk
 257 x 66                          one past 256 columns: the 256-thread form of the band-sums kernel, a second step of a histogram row
 521 x 19, 19 x 521, 1030 x 70     several tiles, 33 bands and chunks, six columns past the 1024 of a band-sums step
 widths with W % 4 = 1, 2, 3 (37, 1030, 19): every length of a last, partial group of four pixels"""
import numpy as np


def const0(W, H, seed=0):
    return np.zeros((H, W), np.uint8)


def const255(W, H, seed=0):
    return np.full((H, W), 255, np.uint8)


def ramp(W, H, seed=0):
    y, x = np.mgrid[0:H, 0:W]
    return ((x * 3 + y * 7 + seed) & 255).astype(np.uint8)


def noise(W, H, seed=1):
    return np.random.RandomState(3000 + seed).randint(0, 256, (H, W)).astype(np.uint8)


def text(W, H, seed=1):
    """sparse, text-like: a bright page with dark strokes of 1 x 3 to 2 x 7 pixels in lines nine rows apart"""
    r = np.random.RandomState(4000 + seed)
    img = np.full((H, W), 230, np.uint8)
    for y0 in range(1, H, 9):
        x = int(r.randint(0, 4))
        while x < W:
            w, h = int(r.randint(1, 3)), int(r.randint(3, 8))
            img[y0:y0 + h, x:x + w] = r.randint(0, 60)
            x += w + int(r.randint(1, 6))
    return img


FRAMES = {"const0": const0, "const255": const255, "ramp": ramp, "noise": noise, "text": text}
KINDS = tuple(FRAMES)
SHAPES = ((1, 1), (1, 300), (300, 1), (7, 5), (65, 3), (64, 33), (33, 17), (257, 66), (521, 19), (19, 521), (1030, 70))          # (W, H)
STORE_LIMIT = 600          # pixels: the fixture keeps the arrays of cases up to this size, an MD5 of every array of every case


def frame(kind, W, H, seed=1):
    return FRAMES[kind](W, H, seed)


def _case(W, H, kind):
    return dict(id="%s%dx%d" % (kind, W, H), W=W, H=H, kind=kind)


# every shape on noise; every kind at 37 x 29 (ragged in both axes) and at 1 x 1; text and ramp on the widest shapes
CASES = [_case(W, H, "noise") for W, H in SHAPES]
CASES += [_case(37, 29, k) for k in KINDS] + [_case(1, 1, k) for k in KINDS if k != "noise"]
CASES += [_case(257, 66, "text"), _case(257, 66, "ramp"), _case(1030, 70, "text"), _case(1030, 70, "const255")]
BY_ID = {c["id"]: c for c in CASES}
assert len(BY_ID) == len(CASES)

# the scale of the clamped arm: with 1.0 the table is min(running sum, 255)
CLAMP_SCALE = 1.0


def case_frame(c):
    return frame(c["kind"], c["W"], c["H"], 1)


def other_hist(c):
    """a caller's histogram for the case: the counts of another frame of the same size, so every v stays below 256 with the default scale"""
    return np.bincount(noise(c["W"], c["H"], 11).reshape(-1), minlength=256).astype(np.uint32)
