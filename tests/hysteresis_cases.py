"""Adversarial inputs for the Canny hysteresis (canny_resolve_kernel and the round / replay logic of api.cpp), two plain models of it
and the predicates that say what a case reaches.  Importable without a GPU: tests/test_hysteresis_cases.py checks every row of CASES
on the CPU against the oracle, tests/test_gpu_hysteresis.py runs the same rows on the GPU.

The kernel works on cells of BAND rows x CHUNK columns, one workgroup each; inside a cell a thread owns rpg consecutive rows of one
32-pixel word.  A launch ("round") floods every cell once from the halo it loaded at entry; launches repeat until nothing changes.
What a case claims is always measured on the masks the oracle's NMS produces (weak = g_nms > tLow, strong = g_nms > tHigh), never
assumed from the drawing.

Models
  expected_edges   the fixed point by definition: 8-connected components of the weak mask that hold a strong pixel.
  cell_rounds      cell-synchronous flood: every cell floods to its own fixed point from the edge snapshot taken at the start of the
                   round.  The kernel never sees less than that snapshot (it may see pixels neighbours wrote earlier in the same
                   launch), so the model's count of productive rounds is an UPPER bound for the GPU.
  crossing_depth   k = the largest number of cell-border crossings any kept pixel needs on its best path from a strong pixel (breadth
                   first over the per-cell components).  A cell floods once per launch from the halo it loaded at entry, so within one
                   launch a path cannot come back into a cell it has left: k crossings are k + 1 path pieces in alternating cells, a
                   launch completes at most one piece per cell the component touches, and the GPU needs at least
                   ceil((k + 1) / cells) productive launches -- ceil((k + 1) / 2) >= ceil(k / 2) for a zigzag over one border.
"""
import numpy as np
from scipy import ndimage, sparse
from scipy.sparse import csgraph

BAND = 64                  # kBandH: rows per cell
CHUNK = 2048               # kBandWords * 32: columns per cell
WORD = 32
RESOLVE_THREADS = 512      # kResolveThreads
SPEC_ROUNDS = 3            # kSpecRounds: rounds enqueued blind
TICKET_FLAGS = 4           # round flags an asynchronous ticket reports
WRAP_SLOTS = 8             # COMPVHIP_RESOLVE_WRAP=8 in the wrap tests
DEPTH_THRESHOLDS = (SPEC_ROUNDS, TICKET_FLAGS, WRAP_SLOTS)
T_LOW, T_HIGH = 10.0, 200.0
BASE, WEAK = 100, 112      # a 12-level step is weak for (10, 200) under the 3x3 Sobel
EIGHT = np.ones((3, 3), bool)
FOUR = ndimage.generate_binary_structure(2, 1)


# ---------------------------------------------------------------------------------------------------------------
# geometry of the kernel's work split
# ---------------------------------------------------------------------------------------------------------------
def chunk_words(W, chunk):
    wb = (W + WORD - 1) // WORD
    return min(CHUNK // WORD, wb - chunk * (CHUNK // WORD))


def rows_per_group(W, H, band=0, chunk=0):
    """rpg of canny_resolve_kernel for one cell: ceil(rows / (512 / cw))."""
    cw = chunk_words(W, chunk)
    rows = min(BAND, H - band * BAND)
    return -(-rows // (RESOLVE_THREADS // cw))


def row_group_borders(W, H, chunk=0):
    """Rows y such that y - 1 and y belong to different row groups of the same band (chunk's column of cells)."""
    out = []
    for b in range(-(-H // BAND)):
        rpg = rows_per_group(W, H, b, chunk)
        rows = min(BAND, H - b * BAND)
        out += [b * BAND + r for r in range(rpg, rows, rpg)]
    return out


# ---------------------------------------------------------------------------------------------------------------
# models
# ---------------------------------------------------------------------------------------------------------------
def masks(gnms, lo, hi):
    return gnms > lo, gnms > hi


def expected_edges(gnms, lo, hi, structure=EIGHT):
    weak, strong = masks(gnms, lo, hi)
    lab, n = ndimage.label(weak, structure=structure)
    keep = np.zeros(n + 1, bool)
    keep[np.unique(lab[strong])] = True
    keep[0] = False
    return keep[lab]


def cell_rounds(weak, strong, band=BAND, chunk=CHUNK):
    """Productive rounds of the cell-synchronous model and its result."""
    H, W = weak.shape
    E = strong.copy()
    rounds = 0
    while True:
        front = ndimage.binary_dilation(E, EIGHT) & weak & ~E
        if not front.any():
            return rounds, E
        new = E.copy()
        ys, xs = np.nonzero(front)
        for b, c in sorted(set(zip((ys // band).tolist(), (xs // chunk).tolist()))):
            sl = (slice(b * band, min(H, (b + 1) * band)), slice(c * chunk, min(W, (c + 1) * chunk)))
            new[sl] |= ndimage.binary_propagation(front[sl], structure=EIGHT, mask=weak[sl])
        E = new
        rounds += 1


def cell_components(weak, band=BAND, chunk=CHUNK):
    """Labels of the weak mask's 8-connected components taken cell by cell (no component spans a cell border)."""
    H, W = weak.shape
    lab = np.zeros((H, W), np.int32)
    n = 0
    for y0 in range(0, H, band):
        for x0 in range(0, W, chunk):
            sl = (slice(y0, min(H, y0 + band)), slice(x0, min(W, x0 + chunk)))
            l, k = ndimage.label(weak[sl], structure=EIGHT)
            lab[sl] = np.where(l > 0, l + n, 0)
            n += k
    return lab, n


def _neighbour_pairs(lab):
    """Label pairs (a, b), a != b, of 8-adjacent pixels."""
    H, W = lab.shape
    out = []
    for dy, dx in ((0, 1), (1, 0), (1, 1), (1, -1)):
        a = lab[0:H - dy, max(0, -dx):W - max(0, dx)]
        b = lab[dy:H, max(0, dx):W - max(0, -dx)]
        m = (a > 0) & (b > 0) & (a != b)
        if m.any():
            out.append(np.stack([a[m], b[m]], 1))
    if not out:
        return np.zeros((0, 2), np.int64)
    p = np.unique(np.concatenate(out), axis=0)
    return np.concatenate([p, p[:, ::-1]])


def crossing_levels(weak, strong, band=BAND, chunk=CHUNK):
    """Per pixel: the least number of cell-border crossings from a strong pixel or a neighbour of one (-1: not kept)."""
    lab, n = cell_components(weak, band, chunk)
    level = np.full(n + 1, -1, np.int64)
    pairs = _neighbour_pairs(lab)
    adj = {}
    for a, b in pairs.tolist():
        adj.setdefault(a, []).append(b)
    # a cell's first flood starts from every strong pixel it sees, those in its halo included
    cur = [int(v) for v in np.unique(lab[ndimage.binary_dilation(strong, EIGHT) & weak]) if v > 0]
    for v in cur:
        level[v] = 0
    d = 0
    while cur:
        d += 1
        nxt = []
        for a in cur:
            for b in adj.get(a, ()):
                if level[b] < 0:
                    level[b] = d
                    nxt.append(b)
        cur = nxt
    level[0] = -1
    return level[lab]


def crossing_depth(weak, strong, band=BAND, chunk=CHUNK):
    """(k, cells): the deepest kept pixel's crossing count and the number of cells the kept pixels touch."""
    lv = crossing_levels(weak, strong, band, chunk)
    ys, xs = np.nonzero(lv >= 0)
    cells = len(set(zip((ys // band).tolist(), (xs // chunk).tolist())))
    return int(lv.max()), cells


def launches_lower_bound(k, cells=2):
    return -(-(k + 1) // max(cells, 1))


# ---------------------------------------------------------------------------------------------------------------
# predicates: which borders the kept pixels cross, in which directions, and whether only diagonally
# ---------------------------------------------------------------------------------------------------------------
def _links(mask):
    """All 8-neighbour links (y0, x0, y1, x1) between pixels of mask, each once."""
    H, W = mask.shape
    out = []
    for dy, dx in ((0, 1), (1, 0), (1, 1), (1, -1)):
        a = mask[0:H - dy, max(0, -dx):W - max(0, dx)]
        b = mask[dy:H, max(0, dx):W - max(0, -dx)]
        y0, x0 = np.nonzero(a & b)
        x0 = x0 + max(0, -dx)
        out.append((y0, x0, y0 + dy, x0 + dx))
    return [np.concatenate(v) for v in zip(*out)]


def _graph(mask, cut=None):
    idx = np.full(mask.shape, -1, np.int64)
    n = int(mask.sum())
    idx[mask] = np.arange(n)
    y0, x0, y1, x1 = _links(mask)
    if cut is not None:
        ok = ~cut(y0, x0, y1, x1)
        y0, x0, y1, x1 = y0[ok], x0[ok], y1[ok], x1[ok]
    g = sparse.coo_matrix((np.ones(len(y0), np.int8), (idx[y0, x0], idx[y1, x1])), shape=(n, n)).tocsr()
    return idx, g


def geodesic(keep, strong):
    """8-connected step distance of every kept pixel from the strong pixels (-1 elsewhere)."""
    idx, g = _graph(keep)
    d = csgraph.dijkstra(g, directed=False, indices=idx[strong & keep], unweighted=True, min_only=True)
    dist = np.full(keep.shape, -1, np.int32)
    dist[keep] = np.where(np.isfinite(d), d, -1).astype(np.int32)
    return dist


def crosses(v0, v1, borders):
    """Per link: do the coordinates v0 -> v1 step over one of the borders (a border b lies between b - 1 and b)?"""
    lo, hi = np.minimum(v0, v1), np.maximum(v0, v1)
    return (hi > lo) & np.isin(hi, np.asarray(list(borders), np.int64))


def cut_flood(weak, strong, cut):
    """The 8-connected fixed point with the links removed for which cut(y0, x0, y1, x1) is true."""
    idx, g = _graph(weak, cut)
    _, lab = csgraph.connected_components(g, directed=False)
    good = np.zeros(lab.max() + 1 if lab.size else 1, bool)
    good[lab[idx[strong & weak]]] = True
    out = np.zeros(weak.shape, bool)
    out[weak] = good[lab]
    return out


def border_cut(cls, W, H):
    """The links whose removal a "diag" claim of class cls is about: diagonal links over a band border ("band"), over the chunk border
    ("chunk"), over a band border where two words of one chunk meet ("bandword"), and the links that step over a band border and the
    chunk border at once ("corner")."""
    bands, chunks = list(range(BAND, H, BAND)), list(range(CHUNK, W, CHUNK))
    words = [x for x in range(WORD, W, WORD) if x % CHUNK]
    if cls == "band":
        return lambda y0, x0, y1, x1: crosses(y0, y1, bands) & (x0 != x1)
    if cls == "chunk":
        return lambda y0, x0, y1, x1: crosses(x0, x1, chunks) & (y0 != y1)
    if cls == "bandword":
        return lambda y0, x0, y1, x1: crosses(y0, y1, bands) & crosses(x0, x1, words)
    assert cls == "corner", cls
    return lambda y0, x0, y1, x1: crosses(y0, y1, bands) & crosses(x0, x1, chunks)


def lost_without(weak, strong, cls):
    """Kept pixels that are lost when the links of border_cut(cls) are removed: the far side turns on only through them."""
    H, W = weak.shape
    return int((cut_flood(weak, strong, None) & ~cut_flood(weak, strong, border_cut(cls, W, H))).sum())


def forward_links(dist, ys=None, xs=None):
    """Links (y, x, dy, dx) of the breadth-first order -- q = p + (dy, dx) with dist[q] == dist[p] + 1 -- that cross a border: between
    rows y - 1 | y for y in ys, between columns x - 1 | x for x in xs.  With both given: links that cross a row border AND a column
    border at once (the corner)."""
    H, W = dist.shape
    out = []
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if not (dy or dx):
                continue
            p = dist[max(0, -dy):H - max(0, dy), max(0, -dx):W - max(0, dx)]
            q = dist[max(0, dy):H - max(0, -dy), max(0, dx):W - max(0, -dx)]
            py, px = np.nonzero((p >= 0) & (q == p + 1))
            py += max(0, -dy); px += max(0, -dx)
            m = np.ones(len(py), bool)
            if ys is not None:
                m &= np.isin(np.maximum(py, py + dy), ys) & (dy != 0)
            if xs is not None:
                m &= np.isin(np.maximum(px, px + dx), xs) & (dx != 0)
            out += [(int(a), int(b), dy, dx) for a, b in zip(py[m], px[m])]
    return out


def directions(links):
    return {(dy, dx) for _, _, dy, dx in links}


# ---------------------------------------------------------------------------------------------------------------
# drawing: low-contrast lines along a path; the contrast ramps up to a strong seed at the path's start
# ---------------------------------------------------------------------------------------------------------------
def rasterize(pts):
    """(y, x) pixels of a polyline whose segments are horizontal, vertical or at 45 degrees."""
    path = [tuple(pts[0])]
    for (y1, x1) in pts[1:]:
        y0, x0 = path[-1]
        sy, sx = np.sign(y1 - y0), np.sign(x1 - x0)
        n = max(abs(y1 - y0), abs(x1 - x0))
        assert (y1 - y0 == 0 or abs(y1 - y0) == n) and (x1 - x0 == 0 or abs(x1 - x0) == n), "segments are straight or at 45 degrees"
        path += [(y0 + int(sy) * t, x0 + int(sx) * t) for t in range(1, n + 1)]
    return path


def draw(W, H, pts, thick=3, seed=True, ramp=25, img=None):
    img = np.full((H, W), BASE, np.uint8) if img is None else img
    path = rasterize(pts)
    for y, x in path:
        assert 2 <= y and y + thick + 2 <= H and 2 <= x and x + thick + 2 <= W, ("path leaves the frame", y, x, W, H)
        img[y:y + thick, x:x + thick] = WEAK
    if seed:
        for t, (y, x) in enumerate(path[:ramp]):
            img[y:y + thick, x:x + thick] = max(WEAK, 255 - 6 * t)
    return img


def zigzag_rows_frame(W, H, k, y_border=BAND, x0=20, pitch=12, reach=24, seed=True):
    """k vertical runs that each cross the row border once, joined alternately below and above it."""
    top, bot = y_border - reach, y_border + reach
    pts = [(top, x0)]
    for i in range(k):
        x = x0 + i * pitch
        pts += [(bot, x), (bot, x + pitch)] if i % 2 == 0 else [(top, x), (top, x + pitch)]
    return draw(W, H, pts[:-1], seed=seed)


def zigzag_cols_frame(W, H, k, x_border=CHUNK, y0=6, pitch=12, reach=40, seed=True):
    """k horizontal runs that each cross the column border once, joined alternately right and left of it."""
    left, right = x_border - reach, x_border + reach
    pts = [(y0, left)]
    for i in range(k):
        y = y0 + i * pitch
        pts += [(y, right), (y + pitch, right)] if i % 2 == 0 else [(y, left), (y + pitch, left)]
    return draw(W, H, pts[:-1], seed=seed)


def spiral_frame(W, H, pitch=24, margin=8, seed=True):
    """An inward rectangular spiral from the top left corner: over several cells in both axes it runs right, down, left and up,
    against the dispatch order in every direction."""
    l, t, r, b = margin, margin, W - margin - 6, H - margin - 6
    pts = [(t, l)]
    while r - l > 2 * pitch and b - t > 2 * pitch:
        pts += [(t, r), (b, r), (b, l + pitch), (t + pitch, l + pitch)]
        l, t, r, b = l + pitch, t + pitch, r - pitch, b - pitch
    return draw(W, H, pts, seed=seed)


def maze_frame(W, H, pitch=12, seed=True):
    """A frame-filling serpentine of weak lines with one seed at its start (the existing tests' frame, any size); without the seed
    nothing in it is strong."""
    pts = [(6, 8)]
    right = True
    for y in range(6, H - 12 - pitch, pitch):
        x = W - 14 if right else 8
        pts += [(y, x), (y + pitch, x)]
        right = not right
    return draw(W, H, pts, seed=seed)


def natural_frame(W, H, seed=7):
    """Smooth low-frequency content: a sum of a few long sinusoids, quantised to 8 bits; at low thresholds its level lines give long
    closed contours."""
    rng = np.random.default_rng(seed)
    y = np.arange(H)[:, None] / float(max(H, W))
    x = np.arange(W)[None, :] / float(max(H, W))
    v = np.zeros((H, W))
    for _ in range(6):
        fy, fx = rng.uniform(1, 9, 2)
        v += rng.uniform(0.3, 1.0) * np.sin(2 * np.pi * (fy * y + fx * x) + rng.uniform(0, 6.28))
    v = (v - v.min()) / (v.max() - v.min())
    return np.round(v * 255).astype(np.uint8)


def text_frame(W, H, seed):
    """Text-like page: short strokes, diagonals and small glyph boxes in dark ink on a light background, at two or three scales
    (many small components, many short lines)."""
    rng = np.random.default_rng(seed)
    img = np.full((H, W), int(rng.integers(170, 240)), np.uint8)
    img += rng.integers(0, 6, (H, W), dtype=np.uint8)
    for scale in (1, 2, 4)[:2 + seed % 2]:
        n = max(2, W * H // (120 * scale * scale))
        xs = rng.integers(0, W, n); ys = rng.integers(0, H, n)
        kinds = rng.integers(0, 4, n); lens = rng.integers(2, 9, n) * scale; inks = rng.integers(0, 100, n)
        for x, y, k, ln, ink in zip(xs, ys, kinds, lens, inks):
            t = scale
            if k == 0:
                img[y:y + t, x:x + ln] = ink
            elif k == 1:
                img[y:y + ln, x:x + t] = ink
            elif k == 2:
                img[y:y + ln, x:x + t] = ink; img[y:y + ln, x + ln - t:x + ln] = ink
                img[y:y + t, x:x + ln] = ink; img[y + ln - t:y + ln, x:x + ln] = ink
            else:
                d = np.arange(ln)
                for o in range(t):
                    yy, xx = y + d, x + d + o
                    m = (yy < H) & (xx < W)
                    img[yy[m], xx[m]] = ink
    return img


def variants(img):
    """The frame and its seven flips / transposes: (same-shape four, transposed four)."""
    same = [img, img[::-1], img[:, ::-1], img[::-1, ::-1]]
    same = [np.ascontiguousarray(v) for v in same]
    return same, [np.ascontiguousarray(v.T) for v in same]


def step_frame(W, H, pts, seed=True, step=12, transpose=False):
    """A one-sided step: everything below the polyline pts -- (y, x) vertices, x from 0 to W - 1 -- is 12 levels brighter.  Its NMS
    chain is a single OPEN chain from the left frame edge to the right one (a drawn line gives two chains joined at both ends, so no
    single link of it matters); where the polyline has slope 1 / 2 every link of the chain is diagonal.  The contrast ramps down from a
    strong start at the left end.  transpose: the frame is built H x W and transposed, so the chain runs from top to bottom."""
    f = np.floor(np.interp(np.arange(W), [p[1] for p in pts], [p[0] for p in pts]) + 1e-9).astype(int)
    img = np.where(np.arange(H)[:, None] >= f[None, :], WEAK, BASE).astype(np.uint8)
    if seed:
        for t in range(-(-(255 - WEAK) // step)):
            img[f[t + 2]:f[t + 2] + 3, t + 2] = max(WEAK, 255 - step * t)
    return np.ascontiguousarray(img.T) if transpose else img


# Open chains whose far side hangs on ONE diagonal link, each after three crossings of the same border (pieces A, B, A, B: the fourth
# piece cannot be flooded in launch 0, so the link is seen by the border test of a later launch, not by the full flood of launch 0).
# The anchor offsets (-1) were found by search on the oracle's masks; lost_without() proves them.
def open_band_word(W=512, H=128, xw=256):
    """... over the band border y = 63 | 64 exactly where two words meet (x = xw - 1 | xw): only hrow[-1] >> 31 of the row pass sees it."""
    xa = xw - 1
    return step_frame(W, H, [(30, 0), (30, 40), (90, 100), (40, 150), (40, xa - 48), (88, xa + 48), (88, W - 1)])


def open_chunk_midband(W=2176, H=100):
    """... over the chunk border x = 2047 | 2048 in the middle of a band: only the r +- 1 halo rows of the column pass see it."""
    return step_frame(H, W, [(2040, 0), (2040, 4), (2054, 18), (2042, 30), (2042, 32), (2056, 60), (2056, H - 1)], transpose=True)


def open_corner(s=0, W=2176, H=192):
    """... from cell (1, 0) into cell (2, 1) over the corner (127, 2047 + s) -> (128, 2048 + s); cells (1, 1) and (2, 0) hold no weak
    pixel, so with s = 0 the diagonal cell is the only neighbour that ever changes."""
    xa = CHUNK - 1 + s
    return step_frame(W, H, [(30, 0), (30, 40), (90, 100), (40, 150), (100, 210), (100, xa - 56), (156, xa + 56), (156, W - 1)])


# ---------------------------------------------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------------------------------------------
K5 = (70.0, 1400.0)        # thresholds that make the same 12-level step weak and the ramp's start strong under the 5x5 kernel


def _case(name, gen, W, H, ksizes=(3,), thr=(T_LOW, T_HIGH), **claims):
    return {"name": name, "gen": gen, "W": W, "H": H, "ksizes": ksizes, "thr": thr, "claims": claims}


# Claims (all measured on the oracle's masks by tests/test_hysteresis_cases.py):
#   borders   classes the kept pixels cross by a breadth-first link: "rowgroup" (for the row's rpg), "word", "band", "chunk", "corner"
#   rpg       rows per thread in the cell (band 0, chunk 0) of this width
#   diag      classes of border links (border_cut) without which kept pixels are lost: the far side hangs on such a link
#   k, cells  at least k cell-border crossings on the best path, kept pixels in exactly `cells` cells (None: not claimed)
#   kept      "all" (every weak pixel is kept), "none", or "some"
#   widths    width classes: "nc2" (W > 2048), "cw56" (W = 3840), "cw1" (last chunk one word), "lastband" (last band under 8 rows)
CASES = [
    _case("cross-rpg1", lambda: draw(256, 160, [(8, 8), (120, 8), (120, 60), (20, 160), (20, 225), (140, 225)]), 256, 160,
          borders=("rowgroup", "word", "band"), rpg=1, kept="all"),
    _case("cross-rpg5", lambda: draw(1100, 134, [(8, 8), (124, 8), (124, 400), (24, 500), (24, 900), (124, 1000)]), 1100, 134,
          ksizes=(3, 5), borders=("rowgroup", "word", "band"), rpg=5, kept="all", widths=("lastband",)),
    _case("cross-chunk-3840", lambda: draw(3840, 134, [(8, 1900), (8, 2200), (108, 2100), (108, 2000), (124, 2000), (124, 2400), (24, 2500)]),
          3840, 134, borders=("rowgroup", "word", "band", "chunk"), rpg=8, kept="all", widths=("nc2", "cw56", "lastband")),
    _case("cross-lastword", lambda: draw(2080, 70, [(10, 1990), (10, 2070), (40, 2040), (60, 2040)]), 2080, 70,
          borders=("word", "chunk"), rpg=8, kept="all", widths=("nc2", "cw1", "lastband")),
] + [
    _case("open-band-word", open_band_word, 512, 128, borders=("band", "word"), rpg=2, k=3, cells=2, kept="all", diag=("band", "bandword")),
    _case("open-chunk-midband", open_chunk_midband, 2176, 100, borders=("chunk",), rpg=8, k=3, cells=None, kept="all", diag=("chunk",),
          widths=("nc2",)),
    _case("open-corner-4096", lambda: open_corner(0, 4096, 192), 4096, 192, borders=("band", "chunk", "corner"), rpg=8, k=4, cells=3, kept="all",
          diag=("band", "chunk", "corner"), widths=("nc2",), symmetric=True),
] + [
    _case("corner%+d" % s, (lambda s=s: open_corner(s)), 2176, 192, borders=("band", "chunk") + (("corner",) if s == 0 else ()), rpg=8,
          k=4, cells=3 if s == 0 else 4, kept="all", diag=("band",) + (("chunk", "corner") if s == 0 else ()), widths=("nc2",))
    for s in (-2, -1, 0, 1)
] + [
    _case("zigzag-band-k8", lambda: zigzag_rows_frame(256, 128, 8), 256, 128, borders=("band",), rpg=1, k=8, cells=2, kept="all"),
    _case("zigzag-band-k10", lambda: zigzag_rows_frame(1100, 128, 10, x0=500), 1100, 128, borders=("band",), rpg=5, k=10, cells=2, kept="all"),
    _case("zigzag-band-k18", lambda: zigzag_rows_frame(1100, 128, 18, x0=500), 1100, 128, ksizes=(3, 5), borders=("band",), rpg=5, k=18, cells=2,
          kept="all"),
    _case("zigzag-chunk-k10", lambda: zigzag_cols_frame(2300, 70, 10, y0=2, pitch=6), 2300, 70, borders=("chunk",), rpg=8, k=10, cells=2, kept="all",
          widths=("nc2", "lastband")),
    _case("zigzag-chunk-k26", lambda: zigzag_cols_frame(2300, 330, 26), 2300, 330, borders=("chunk", "band"), rpg=8, k=26, cells=None, kept="all",
          widths=("nc2",)),
    _case("spiral", lambda: spiral_frame(4200, 200), 4200, 200, borders=("chunk", "band"), rpg=8, k=20, cells=None, kept="all", widths=("nc2",)),
    _case("maze-seeded", lambda: maze_frame(2300, 200), 2300, 200, borders=("chunk", "band"), rpg=8, k=8, cells=None, kept="all", widths=("nc2",)),
    _case("maze-unseeded", lambda: maze_frame(2300, 200, seed=False), 2300, 200, kept="none", widths=("nc2",)),
    _case("text", lambda: text_frame(2300, 200, 3), 2300, 200, thr=(20.0, 60.0), kept="some", widths=("nc2",)),
    _case("natural", lambda: natural_frame(2300, 200), 2300, 200, thr=(2.0, 30.0), borders=("chunk", "band"), k=3, cells=None, kept="some",
          widths=("nc2",)),
]
BY_NAME = {c["name"]: c for c in CASES}


def thresholds_for(case, ksize):
    return case["thr"] if ksize == 3 else K5


def border_sets(W, H):
    """Border positions per class: rows for "rowgroup" / "band", columns for "word" / "chunk"."""
    bands = list(range(BAND, H, BAND))
    chunks = list(range(CHUNK, W, CHUNK))
    return {"rowgroup": {"ys": row_group_borders(W, H)}, "band": {"ys": bands},
            "word": {"xs": [x for x in range(WORD, W, WORD) if x % CHUNK]}, "chunk": {"xs": chunks},
            "corner": {"ys": bands, "xs": chunks}}


def measure(case_img, gnms, lo, hi):
    """Everything the table claims, measured on the masks: {"links": {class: links}, "diag": {class: bool}, "k", "cells", "kept"}."""
    H, W = case_img.shape
    weak, strong = masks(gnms, lo, hi)
    keep = expected_edges(gnms, lo, hi)
    out = {"kept": "none" if not keep.any() else ("all" if (keep == weak).all() else "some"), "links": {}, "diag": {}, "k": -1, "cells": 0}
    if keep.any():
        dist = geodesic(keep, strong)
        for cls, sel in border_sets(W, H).items():
            out["links"][cls] = forward_links(dist, sel.get("ys"), sel.get("xs")) if all(len(v) for v in sel.values()) else []
        out["k"], out["cells"] = crossing_depth(weak, strong)
        out["weak"], out["strong"] = weak, strong
    return out
