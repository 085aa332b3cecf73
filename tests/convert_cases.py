"""The colour conversion test cases and their frames, shared by tests/golden/make_golden_convert.py, the CPU tests, tests/host/convert_math_check.cpp's
driver and tests/test_gpu_convert.py.

A case is (id, source format, W, H, frame kind): the source planes are generated, never stored (numpy's legacy RandomState is stable across versions), and
every destination the source is served to belongs to the case.  The kernel gives a thread 8 adjacent pixels of a row, 256 threads a workgroup:
 1 x 1, 2 x 2        one pixel; one chroma sample for four pixels
 7 x 5               odd in both axes: a partial group only, a last chroma column and row that serve one pixel column / row
 16 x 2              two whole groups, nothing else
 33 x 17             four whole groups and a partial one of one pixel, odd height
 250 x 3             31 whole groups and a partial one of two pixels
 641 x 480           one per source format: a camera frame one column too wide -- 81 groups, the last of one pixel
 4096 x 4096         exhaustive: YUV444P with every (Y, U, V) once and RGB24 with every (R, G, B) once (two workgroups per row); together they reach every
                     entry of both HSV tables and every clamp"""
import numpy as np

import convert_model as cm

SIZES = ((1, 1), (2, 2), (7, 5), (16, 2), (33, 17), (250, 3))          # (W, H)
BIG = (641, 480)
EXHAUSTIVE = (4096, 4096)
STORE_LIMIT = 600          # pixels: the fixture keeps the planes of cases up to this size, an MD5 of every plane of every case
SOURCES = tuple(f for f in cm.FORMATS if f != cm.HSV)


def destinations(src):
    return [d for s, d in cm.SERVED if s == src]


def _case(src, W, H, kind):
    return dict(id="%s_%s%dx%d" % (cm.NAMES[src], kind, W, H), src=src, W=W, H=H, kind=kind)


CASES = []
for _src in SOURCES:
    CASES += [_case(_src, W, H, "noise") for W, H in SIZES]
    CASES += [_case(_src, 33, 17, "gradient"), _case(_src, 16, 2, "gradient"), _case(_src, 7, 5, "const0"), _case(_src, 7, 5, "const255")]
    CASES.append(_case(_src, BIG[0], BIG[1], "noise"))
CASES += [_case(cm.YUV444P, EXHAUSTIVE[0], EXHAUSTIVE[1], "exhaustive"), _case(cm.RGB24, EXHAUSTIVE[0], EXHAUSTIVE[1], "exhaustive")]
BY_ID = {c["id"]: c for c in CASES}
assert len(BY_ID) == len(CASES)
SMALL = [c for c in CASES if c["W"] * c["H"] <= STORE_LIMIT]


def case_planes(c):
    """the source's dense planes (convert_model.plane_shapes)"""
    shapes = cm.plane_shapes(c["src"], c["W"], c["H"])
    kind = c["kind"]
    if kind == "exhaustive":
        i = np.arange(4096 * 4096, dtype=np.uint32).reshape(4096, 4096)
        ch = [(i & 255).astype(np.uint8), ((i >> 8) & 255).astype(np.uint8), (i >> 16).astype(np.uint8)]
        return ch if c["src"] == cm.YUV444P else [np.ascontiguousarray(np.stack(ch, axis=2).reshape(4096, 3 * 4096))]
    if kind == "const0":
        return [np.zeros(s, np.uint8) for s in shapes]
    if kind == "const255":
        return [np.full(s, 255, np.uint8) for s in shapes]
    if kind == "gradient":
        out = []
        for p, (rows, cols) in enumerate(shapes):
            y, x = np.mgrid[0:rows, 0:cols]
            out.append(((x * 5 + y * 11 + 40 * p) & 255).astype(np.uint8))
        return out
    r = np.random.RandomState(5000 + 97 * c["src"] + c["W"] + 7 * c["H"])
    return [r.randint(0, 256, s).astype(np.uint8) for s in shapes]


def key(c, dst, plane):
    return "%s_%s_%d" % (c["id"], cm.NAMES[dst], plane)
