"""The content sequences of tests/test_gpu_content_sequences.py: what one live handle is fed call after call.

Built with numpy alone from fixed seeds, so that tests/test_content_sequences.py can check on the CPU -- with the oracle and the stage models -- that every
sequence really has the properties its GPU test relies on (a tile column of 256 and more, line counts either side of a sort chunk, slice counts, a cut at a
tie, ...).  Nothing here reads a file outside tests/.

A sequence is a list of steps, a step is (frames, parameters).  A batch has F = 3 frames and frame f of step k takes content class (k + f) % classes: in every
step one frame shrinks while another grows, so that a mistake made per batch cannot cancel out.  run_order() is the order the GPU driver makes the calls in:
every step, then the first one again.
"""
import numpy as np

F = 3
SEED = 20261019

# compvhip_canny thresholdType / what capi.THRESHOLD_* say (no import of the binding: this module is numpy only)
GRADIENT, PERCENT_OF_MEAN, OTSU = 0, 1, 2


def class_of(step, frame, classes):
    return (step + frame) % classes


def run_order(steps):
    """indices of the calls on one handle: every step in turn, then the first again"""
    return list(range(len(steps))) + [0]


def rng_of(*key):
    return np.random.default_rng([SEED] + [int(k) for k in key])


# ---------------------------------------------------------------------------------------------------------------------------------------------
# (a) Canny, SHT and the pipeline on one plan
# ---------------------------------------------------------------------------------------------------------------------------------------------
# (W, H, S).  No row of tests/plan_geometries.py fits: a (tile, theta) column of the vote reaches 256 only when a vote tile is at least 256 pixels long, and a
# plan of three small frames is "starved" (planVoteTiles, api.cpp) and gets a finer grid -- 1545 x 33 is about the smallest three-frame plan whose tiles are 288
# columns wide.  Ragged widths (W % 8 == 1), S > W (S - W = 7), at least four 496-column Canny tiles per row, at least two SWAR row tiles.  2113 = 1 (mod 16)
# is a GAP width (plan_geometries.has_coverage_gap), 1545 is not; 2113 x 70 also has two resolve bands of 64 rows and two resolve chunks of 2048 columns per
# frame, so that the hysteresis hands its change flags (`dirty`) between neighbouring workgroups.
PLAN_GEOMETRIES = [(1545, 33, 1552), (2113, 70, 2120)]
PLAN_CLASSES = ("noise", "bars", "constant", "shifted")
BAR_ROWS = (6, 20)          # first rows of the two horizontal bars, three rows tall
BAR_SHIFT = 5               # "shifted": the same bars five rows lower, clear of the rows their edges held
BAR_MARGIN = 8              # columns left free at either end of a bar

# between steps everything changes: ksize 3 <-> 5, the threshold mode (PERCENT_OF_MEAN and OTSU derive per-frame thresholds on the device), the SHT threshold
# and maxLines
PLAN_PARAMS = [
    dict(ksize=3, mode=GRADIENT, tl=59.0, th=119.0, thr=40, max_lines=0),
    dict(ksize=5, mode=GRADIENT, tl=400.0, th=900.0, thr=12, max_lines=5),
    dict(ksize=3, mode=PERCENT_OF_MEAN, tl=0.68, th=1.36, thr=25, max_lines=0),
    dict(ksize=5, mode=OTSU, tl=0.5, th=1.0, thr=9, max_lines=3),
    dict(ksize=3, mode=GRADIENT, tl=20.0, th=200.0, thr=60, max_lines=0),
]


def plan_frame(kind, W, H, key):
    if kind == "noise":
        return rng_of(1, *key).integers(0, 256, (H, W), dtype=np.uint8)
    if kind == "constant":
        return np.full((H, W), 90, np.uint8)
    img = np.full((H, W), 40, np.uint8)
    dy = BAR_SHIFT if kind == "shifted" else 0
    for y in BAR_ROWS:
        img[y + dy:y + dy + 3, BAR_MARGIN:W - BAR_MARGIN] = 220
    return img


def plan_sequence(W, H):
    """[(frames (F, H, W) uint8, params)] of PLAN_PARAMS' steps"""
    steps = []
    for k, prm in enumerate(PLAN_PARAMS):
        kinds = [PLAN_CLASSES[class_of(k, f, len(PLAN_CLASSES))] for f in range(F)]
        frames = np.stack([plan_frame(kind, W, H, (k, f)) for f, kind in enumerate(kinds)])
        steps.append((frames, dict(prm, kinds=kinds)))
    return steps


def vote_tile_size(W, H, nx, ny):
    """(TW, TH) of the vote's nx x ny tile grid (voteGridTables, api.cpp): the grids are tried in order of tile count, splitting the dimension with the longer
    tile side; TW is rounded up to 32 columns, which may save a column of tiles"""
    def ceil_div(a, b):
        return -(-a // b)

    gx = gy = 1
    for _ in range(512):
        TW = ceil_div(ceil_div(W, gx), 32) * 32
        if (ceil_div(W, TW), gy) == (nx, ny):
            return TW, ceil_div(H, gy)
        if W / gx >= H / gy:
            gx += 1
        else:
            gy += 1
    raise AssertionError("no split gives a %d x %d grid on %d x %d" % (nx, ny, W, H))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# (b) the line sort on a live plan: foreign edge maps at threshold 1
# ---------------------------------------------------------------------------------------------------------------------------------------------
SORT_CHUNK = 4096           # kShtSortChunk: lines per chunk of the device sort
SORT_MAX_CHUNKS = 32        # kShtSortMaxChunks: beyond 32 chunks of line capacity a plan sorts with the library
SORT_GEOMETRY = (321, 241, 328)                          # ragged, S > W; R * T > 32 * 4096, so that a line capacity can pass 131 072
SORT_CLASSES = ("three_chunks", "part_chunk", "none", "two_chunks")
SORT_DENSITY = {"three_chunks": 0.01, "part_chunk": 0.0012, "none": 0.0, "two_chunks": 0.0035}
SORT_LINE_CAPS = [16, 10000, 16, 10000]                  # the caller's capacity per step; the plan keeps the larger key buffers
SORT_BIG_CAP = SORT_CHUNK * SORT_MAX_CHUNKS + 1          # the step that takes the plan off the device sort for good


def sort_edge_map(kind, W, H, key):
    """a random edge map of a few per cent: at threshold 1 nearly every local maximum of the accumulator is a line"""
    return (rng_of(2, *key).random((H, W)) < SORT_DENSITY[kind]).astype(np.uint8) * 255


def sort_sequence():
    """[(edge maps (F, H, W) uint8, dict(line_cap, kinds))]: SHT threshold 1, every line kept"""
    W, H, _ = SORT_GEOMETRY
    steps = []
    for k, cap in enumerate(SORT_LINE_CAPS):
        kinds = [SORT_CLASSES[class_of(k, f, len(SORT_CLASSES))] for f in range(F)]
        maps = np.stack([sort_edge_map(kind, W, H, (k, f)) for f, kind in enumerate(kinds)])
        steps.append((maps, dict(line_cap=cap, kinds=kinds)))
    return steps


# ---------------------------------------------------------------------------------------------------------------------------------------------
# (e) the matcher: device counts that change between calls on one handle
# ---------------------------------------------------------------------------------------------------------------------------------------------
MATCH_SLICE = 128           # train rows per slice workgroup (match_kernels.hip)
MATCH = dict(desc_bytes=32, q_stride=48, t_stride=36, qcap=2 * MATCH_SLICE + 3, tcap=2 * MATCH_SLICE + 3, pairs=F, knn=2)
# Query and train counts per pair (rotated by the step, so that every pair takes every count) and what the good list filters by; a shared train set takes t[0].
# The forward pass runs ceil(T / 128) train slices; the cross check runs the same kernels with the roles swapped, so ceil(Q / 128) reverse slices.  Forward:
# 3 -> 1 -> 0 -> 3 -> 3 -> 1 slices.  Under crossCheck (steps 0, 1, 3, 5; off in between, which leaves the reverse lists as they were): 3 reverse slices over a
# full train side, 1 over a smaller non-zero one, none, then 2 / 3 / 1.
MATCH_STEPS = [
    dict(kind="all_slices", q=[259, 258, 257], t=[259, 258, 257], cross_check=True, ratio=0.8, max_distance=-1),
    dict(kind="one_slice", q=[128, 77, 1], t=[128, 77, 5], cross_check=True, ratio=0.8, max_distance=60),
    dict(kind="no_train", q=[259, 2, 130], t=[0, 0, 0], cross_check=False, ratio=0.0, max_distance=-1),
    dict(kind="no_query", q=[0, 0, 0], t=[259, 130, 5], cross_check=True, ratio=0.8, max_distance=-1),
    dict(kind="all_slices", q=[130, 257, 64], t=[258, 257, 259], cross_check=False, ratio=0.8, max_distance=-1),
    dict(kind="one_slice", q=[129, 259, 100], t=[100, 128, 60], cross_check=True, ratio=0.0, max_distance=-1),
]


def match_slices(t):
    return -(-t // MATCH_SLICE)


def match_steps(shared):
    """MATCH_STEPS with the counts of step k rotated by k (a shared train set has one count: the first)"""
    out = []
    for k, s in enumerate(MATCH_STEPS):
        r = k % F
        t = s["t"][r:] + s["t"][:r]
        out.append(dict(s, q=s["q"][r:] + s["q"][:r], t=t[:1] if shared else t))
    return out


def match_descriptors(shared):
    """(query [pairs][qcap][q_stride], train [sets][tcap][t_stride]) uint8: random train rows; query i of pair p is train row (7 i + 3 p) % tcap of its set with up
    to 40 bits flipped, so that most queries have a clear best neighbour whatever prefix of the train rows a step leaves valid; the stride padding holds random
    bytes and a 255"""
    m = MATCH
    sets = 1 if shared else m["pairs"]
    rng = rng_of(5, int(shared))
    train = rng.integers(0, 256, (sets, m["tcap"], m["t_stride"]), dtype=np.uint8)
    query = rng.integers(0, 256, (m["pairs"], m["qcap"], m["q_stride"]), dtype=np.uint8)
    train[:, :, m["desc_bytes"]] = 255
    query[:, :, m["desc_bytes"]] = 255
    for p in range(m["pairs"]):
        for i in range(m["qcap"]):
            row = train[0 if shared else p, (7 * i + 3 * p) % m["tcap"], :m["desc_bytes"]].copy()
            for b in rng.integers(0, m["desc_bytes"] * 8, rng.integers(0, 41)):
                row[b >> 3] ^= np.uint8(1 << (b & 7))
            query[p, i, :m["desc_bytes"]] = row
    return query, train


# ---------------------------------------------------------------------------------------------------------------------------------------------
# (f) the homography handle
# ---------------------------------------------------------------------------------------------------------------------------------------------
HOMOGRAPHY = dict(pairs=F, point_cap=129, max_tries=257)
HOMOGRAPHY_CLASSES = ("planted_large", "three_points", "collinear", "four_points", "planted_other")
# tries 257 <-> 63; the device generator, then given quads, then the generator again; a mask given and not
HOMOGRAPHY_STEPS = [
    dict(tries=257, given_quads=False, mask=True, seed=11),
    dict(tries=63, given_quads=True, mask=False, seed=12),
    dict(tries=257, given_quads=False, mask=True, seed=13),
    dict(tries=63, given_quads=True, mask=True, seed=14),
    dict(tries=257, given_quads=False, mask=False, seed=15),
]


def homography_points(kind, key):
    """(src [k][2], dst [k][2]) float64 of one pair"""
    import homography_cases as hc
    if kind == "planted_large":
        return hc.planted(129, 0.3, 300 + key)[:2]
    if kind == "planted_other":
        return hc.planted(65, 0.6, 400 + key)[:2]
    if kind == "three_points":
        return hc.planted(3, 0.0, 500 + key)[:2]
    if kind == "four_points":
        return hc.planted(4, 0.0, 600 + key)[:2]
    return hc.line_case(20)          # every source on one line: every quad is collinear, no try stores a hypothesis


def homography_sequence():
    """[(per pair (src, dst), dict(tries, given_quads, mask, seed, kinds))]"""
    steps = []
    for k, prm in enumerate(HOMOGRAPHY_STEPS):
        kinds = [HOMOGRAPHY_CLASSES[class_of(k, p, len(HOMOGRAPHY_CLASSES))] for p in range(HOMOGRAPHY["pairs"])]
        steps.append(([homography_points(kind, 10 * k + p) for p, kind in enumerate(kinds)], dict(prm, kinds=kinds)))
    return steps


# ---------------------------------------------------------------------------------------------------------------------------------------------
# (d) FAST on one plan
# ---------------------------------------------------------------------------------------------------------------------------------------------
FAST_GEOMETRIES = [(40, 37, 40, F), (131, 45, 136, F)]          # the smallest admissible ORB frame, and a ragged one with S > W, past a 128-column tile
FAST_CLASSES = ("many", "none", "handful", "ties")
# the threshold, N 9 <-> 12, nonmax and maxFeatures change; the score map is the caller's or the plan's; records or counts only
FAST_STEPS = [
    dict(t=20, N=9, nonmax=True, max_features=-1, scores=True, records=True),
    dict(t=5, N=12, nonmax=False, max_features=-1, scores=False, records=False),
    dict(t=20, N=9, nonmax=True, max_features=10, scores=True, records=True),
    dict(t=40, N=12, nonmax=True, max_features=3, scores=False, records=True),
    dict(t=10, N=9, nonmax=False, max_features=-1, scores=True, records=False),
    dict(t=20, N=9, nonmax=True, max_features=10, scores=False, records=True),
]


def fast_frame(kind, W, H, key):
    import fast_model as fm
    seed = 1000 + 17 * key[0] + key[1]
    if kind == "many":
        return fm.noise(W, H, seed)
    if kind == "none":
        return np.full((H, W), 77, np.uint8)
    if kind == "ties":
        return fm.tied_arcs(W, H, seed)
    img = np.full((H, W), 60, np.uint8)          # a handful: isolated bright pixels of different strengths, at other positions in every step
    rng = rng_of(6, *key)
    for i in range(4):
        x, y = int(rng.integers(4, W - 4)), int(rng.integers(4, H - 4))
        img[y, x] = 150 + 25 * i
    return img


def fast_sequence(W, H):
    steps = []
    for k, prm in enumerate(FAST_STEPS):
        kinds = [FAST_CLASSES[class_of(k, f, len(FAST_CLASSES))] for f in range(F)]
        steps.append((np.stack([fast_frame(kind, W, H, (k, f)) for f, kind in enumerate(kinds)]), dict(prm, kinds=kinds)))
    return steps


# ---------------------------------------------------------------------------------------------------------------------------------------------
# (g) calls that look stateless and own scratch: Otsu's histograms, morphTmp, HOG's cell map
# ---------------------------------------------------------------------------------------------------------------------------------------------
SCRATCH_GEOMETRY = (257, 70, 264)          # ragged, S > W, one column past a 256-column morph tile, three 32-row tiles
OTSU_CLASSES = ("noise", "constant", "dark_bimodal", "bright_bimodal")


def otsu_frame(kind, W, H, key):
    rng = rng_of(7, *key)
    if kind == "noise":
        return rng.integers(0, 256, (H, W), dtype=np.uint8)
    if kind == "constant":
        return np.full((H, W), 255, np.uint8)          # the whole histogram in the last bin
    lo, hi = (10, 60) if kind == "dark_bimodal" else (180, 250)
    img = np.where(rng.random((H, W)) < 0.3, hi, lo).astype(np.int32) + rng.integers(-5, 6, (H, W))
    return np.clip(img, 0, 255).astype(np.uint8)


def otsu_sequence():
    W, H, _ = SCRATCH_GEOMETRY
    steps = []
    for k in range(5):
        kinds = [OTSU_CLASSES[class_of(k, f, len(OTSU_CLASSES))] for f in range(F)]
        steps.append((np.stack([otsu_frame(kind, W, H, (k, f)) for f, kind in enumerate(kinds)]), dict(kinds=kinds)))
    return steps


# morphology and the in-place adaptive threshold share morphTmp: structuring element (kind, w, h), op, border / block size, delta
ERODE, DILATE, OPEN, CLOSE = 0, 1, 2, 3
RECT, DIAMOND, CROSS = 0, 1, 2
BORDER_ZERO, BORDER_REPLICATE = 0, 2
MORPH_STEPS = [
    dict(call="morph", strel=(RECT, 15, 3), op=OPEN, border=BORDER_REPLICATE),
    dict(call="adaptive", block=5, delta=3.0, invert=False),
    dict(call="morph", strel=(CROSS, 5, 5), op=CLOSE, border=BORDER_ZERO),
    dict(call="adaptive", block=15, delta=-2.0, invert=True),
    dict(call="morph", strel=(DIAMOND, 7, 7), op=OPEN, border=BORDER_ZERO),
    dict(call="morph", strel=(RECT, 3, 15), op=CLOSE, border=BORDER_REPLICATE),
]
MORPH_CLASSES = ("noise", "strokes", "constant", "blobs")


def morph_frame(kind, W, H, key):
    rng = rng_of(8, *key)
    if kind == "noise":
        return rng.integers(0, 256, (H, W), dtype=np.uint8)
    if kind == "constant":
        return np.full((H, W), 200, np.uint8)
    img = np.zeros((H, W), np.uint8)
    for _ in range(W * H // (60 if kind == "strokes" else 400)):
        x, y = int(rng.integers(0, W)), int(rng.integers(0, H))
        if kind == "strokes":
            ln = int(rng.integers(2, 9))
            if rng.integers(0, 2):
                img[y, x:x + ln] = 255
            else:
                img[y:y + ln, x] = 255
        else:
            img[y:y + int(rng.integers(3, 12)), x:x + int(rng.integers(3, 12))] = int(rng.integers(100, 256))
    return img


def morph_sequence():
    W, H, _ = SCRATCH_GEOMETRY
    steps = []
    for k, prm in enumerate(MORPH_STEPS):
        kinds = [MORPH_CLASSES[class_of(k, f, len(MORPH_CLASSES))] for f in range(F)]
        steps.append((np.stack([morph_frame(kind, W, H, (k, f)) for f, kind in enumerate(kinds)]), dict(prm, kinds=kinds)))
    return steps


# HOG with the plan's own cell map (d_cells NULL): bin count, cell size and norm change between calls (tests/hog_model.py's option names and values)
HOG_SIZE = (77, 45)
HOG_STEPS = [
    dict(blockW=16, blockH=16, strideW=8, strideH=8, cellW=8, cellH=8, nbins=9, blockNorm=5),
    dict(blockW=8, blockH=8, strideW=4, strideH=4, cellW=4, cellH=4, nbins=18, blockNorm=2),
    dict(blockW=16, blockH=16, strideW=16, strideH=16, cellW=16, cellH=16, nbins=4, blockNorm=4),
    dict(blockW=12, blockH=12, strideW=6, strideH=6, cellW=6, cellH=6, nbins=9, blockNorm=3),
    dict(blockW=8, blockH=8, strideW=8, strideH=8, cellW=8, cellH=8, nbins=2, blockNorm=1),
]
HOG_CLASSES = ("noise", "constant", "blocks", "checkerboard")


def hog_sequence():
    import hog_cases as hc
    W, H = HOG_SIZE
    steps = []
    for k, prm in enumerate(HOG_STEPS):
        kinds = [HOG_CLASSES[class_of(k, f, len(HOG_CLASSES))] for f in range(F)]
        steps.append(([hc.frame(kind, W, H, 1 + 10 * k + f) for f, kind in enumerate(kinds)], dict(opts=prm, kinds=kinds)))
    return steps


# ---------------------------------------------------------------------------------------------------------------------------------------------
# (c) segments, fits and components behind every step of (a): (minLength, maxGap, halfWidth, connectivity, minPixels) of step k
# ---------------------------------------------------------------------------------------------------------------------------------------------
FEATURE_PARAMS = [
    dict(min_length=1, max_gap=0, half_width=0, conn=8, min_pixels=1),
    dict(min_length=5, max_gap=2, half_width=3, conn=4, min_pixels=3),
    dict(min_length=1, max_gap=2000, half_width=8, conn=8, min_pixels=1),
    dict(min_length=20, max_gap=1, half_width=1, conn=4, min_pixels=10),
    dict(min_length=3, max_gap=0, half_width=2, conn=8, min_pixels=2),
]
FEATURE_LINES = 24          # lines per frame the walks take (maxLines)
# what the caller passes for (d_labels, compCap) at step k: counts only, then everything, then records without a label map
FEATURE_OUTPUTS = [(False, 0), (True, 64), (False, 64)]


# ---------------------------------------------------------------------------------------------------------------------------------------------
# (h) KHT on a plan: edge maps drawn directly (one-pixel strokes are what the linking stage walks)
# ---------------------------------------------------------------------------------------------------------------------------------------------
KHT_GEOMETRY = (321, 243, 336)
KHT_CLASSES = ("busy", "empty", "other")
# the order alternates; COMPVHIP_KHT_GROUP (frames per stage group; None: the default of 8, one group) splits the batch of three into three and two groups
KHT_STEPS = [
    dict(order="reference", group=None, threshold=12),
    dict(order="canonical", group=1, threshold=12),
    dict(order="reference", group=2, threshold=20),
    dict(order="canonical", group=None, threshold=12),
]


def kht_edge_map(kind, W, H, key):
    e = np.zeros((H, W), np.uint8)
    if kind == "empty":
        return e
    rng = rng_of(9, KHT_CLASSES.index(kind), *key)
    for _ in range(14 if kind == "busy" else 9):
        x0, y0, x1, y1 = (int(rng.integers(2, W - 2)), int(rng.integers(2, H - 2)), int(rng.integers(2, W - 2)), int(rng.integers(2, H - 2)))
        n = max(abs(x1 - x0), abs(y1 - y0)) + 1
        xs = np.rint(np.linspace(x0, x1, n)).astype(np.int64)
        ys = np.rint(np.linspace(y0, y1, n)).astype(np.int64)
        e[ys, xs] = 255
    return e


def kht_sequence():
    W, H, _ = KHT_GEOMETRY
    steps = []
    for k, prm in enumerate(KHT_STEPS):
        kinds = [KHT_CLASSES[class_of(k, f, len(KHT_CLASSES))] for f in range(F)]
        steps.append((np.stack([kht_edge_map(kind, W, H, (k, f)) for f, kind in enumerate(kinds)]), dict(prm, kinds=kinds)))
    return steps


# ---------------------------------------------------------------------------------------------------------------------------------------------
# (d) ORB on one plan (the corner lists are the GPU rig's own; their device counts change) and the ORB pyramid
# ---------------------------------------------------------------------------------------------------------------------------------------------
ORB_GEOMETRIES = FAST_GEOMETRIES
ORB_CLASSES = ("many", "none", "handful")
# corners: how much of a frame's list its device count admits ("all", "none", 3), rotated over the frames like the content; keyCap 0 <-> > 0; blur 1 <-> 0
ORB_COUNTS = ("all", "none", 3)
ORB_STEPS = [
    dict(level=0, scale=1.0, records=True, blur=True, moments=True),
    dict(level=1, scale=0.83, records=False, blur=True, moments=False),
    dict(level=0, scale=1.0, records=True, blur=False, moments=False),
    dict(level=1, scale=0.83, records=True, blur=True, moments=True),
    dict(level=0, scale=1.0, records=True, blur=False, moments=True),
]


def orb_sequence(W, H):
    steps = []
    for k, prm in enumerate(ORB_STEPS):
        kinds = [ORB_CLASSES[class_of(k, f, len(ORB_CLASSES))] for f in range(F)]
        counts = [ORB_COUNTS[class_of(k + 1, f, len(ORB_COUNTS))] for f in range(F)]
        steps.append((np.stack([fast_frame(kind, W, H, (50 + k, f)) for f, kind in enumerate(kinds)]), dict(prm, kinds=kinds, counts=counts)))
    return steps


ORBPYR_GEOMETRY = (100, 90, 112, 5, 0.83, 400)         # W, H, S, levels, scale factor, maxFeatures: five levels; the quotas still cut the busy frames
ORBPYR_STEPS = 4


def orbpyr_frame(kind, W, H, key):
    if kind != "handful":
        return fast_frame(kind, W, H, key)
    img = np.full((H, W), 60, np.uint8)                 # isolated bright pixels at least 30 from every border: corners that survive on the first levels
    rng = rng_of(10, *key)
    for i in range(5):
        img[int(rng.integers(30, H - 30)), int(rng.integers(30, W - 30))] = 150 + 20 * i
    return img


def orbpyr_sequence():
    W, H = ORBPYR_GEOMETRY[:2]
    steps = []
    for k in range(ORBPYR_STEPS):
        kinds = [ORB_CLASSES[class_of(k, f, len(ORB_CLASSES))] for f in range(F)]
        steps.append((np.stack([orbpyr_frame(kind, W, H, (70 + k, f)) for f, kind in enumerate(kinds)]), dict(kinds=kinds)))
    return steps
