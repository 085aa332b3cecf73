"""Pins tests/sht_segments_model.py (the numpy restatement of the line-segment definition in include/compv_hip.h), so that the GPU test is
not the model checking its own twin:

* rule 3 against the ORACLE's accumulator: the support pixels of a line's cell, counted by the model, are the cell's votes;
* the model's candidate window (est - 1 .. est + 2) against a brute-force scan of the whole image with the vote's expression;
* hand-drawn maps whose segments are known by construction: pieces cut with gaps of maxGap and maxGap + 1 and one piece of
  length minLength - 1, on a horizontal, a vertical (theta = 0: sinQ = 0), a 45-degree and a 135-degree (cosQ < 0) line;
* lines that touch the image corners or leave it through the top / bottom (positions without a support pixel inside the image).
"""
import numpy as np
import pytest

from oracle_bindings import synth_frame
from sht_segments_model import SEG_DTYPE, frame_segments, line_occupancy, line_segments


def brute_support(edges, sinQ, cosQ, row, col):
    """Rule 1 on every pixel of the image: the (x, y) of the edge pixels that vote for cell (row, col)."""
    H, W = edges.shape
    x = np.arange(W, dtype=np.int64)[None, :]
    y = np.arange(H, dtype=np.int64)[:, None]
    hit = (((x * int(cosQ[col]) + y * int(sinQ[col])) >> 16) == (W + H) - row) & (edges != 0)
    ys, xs = np.nonzero(hit)
    return set(zip(xs.tolist(), ys.tolist()))


def model_support(edges, sinQ, cosQ, row, col):
    """The same set through the model's occupancy: first[p], and first[p] + 1 where cnt[p] == 2 (rule 2: the support pixels of a position
    are a contiguous run of at most 2 minor coordinates)."""
    cnt, first, xm = line_occupancy(edges, sinQ, cosQ, row, col)
    assert cnt.max(initial=0) <= 2
    out = set()
    for p in np.flatnonzero(cnt).tolist():
        for m in range(int(first[p]), int(first[p]) + int(cnt[p])):
            out.add((p, m) if xm else (m, p))
    return out


@pytest.mark.parametrize("W,H,tl,th,theta,thr", [(640, 480, 59., 119., 1.0, 100), (641, 480, 59., 119., 1.0, 100), (1282, 720, 0.8, 1.6, 1.0, 100),
                                                 (640, 480, 59., 119., 0.5, 100)], ids=lambda v: str(v))
def test_support_count_is_the_oracle_accumulator_cell(oracle, W, H, tl, th, theta, thr):
    rc, edges = oracle.canny(synth_frame(W, H), tl, th)
    assert rc == 0
    acc = oracle.sht_acc(edges, theta)
    R, T, _ = oracle.sht_dims(W, H, theta)
    sinQ, cosQ = oracle.sht_tables(theta, T)
    lines = oracle.sht_lines_from_acc(acc, W, H, theta, thr)
    assert len(lines) > 20
    for i, l in enumerate(lines):
        row, col, strength = l[3], l[4], l[2]
        cnt, first, xm = line_occupancy(edges, sinQ, cosQ, row, col)
        assert int(cnt.sum()) == int(acc[row, col]) == strength, (row, col)
        assert cnt.max() <= 2
        # Sigma support over the (1, N) segments of a line (everything bridged) is its strength
        segs = line_segments(cnt, first, xm, i, 1, max(W, H))
        assert len(segs) == 1 and segs[0][5] == strength
    # the support SET against the brute-force predicate, for a sample of lines and of arbitrary non-empty cells
    rng = np.random.default_rng(W + H)
    cells = [(l[3], l[4]) for l in lines[::max(1, len(lines) // 12)]]
    rows, cols = np.nonzero(acc)
    pick = rng.choice(len(rows), 12, replace=False)
    cells += list(zip(rows[pick].tolist(), cols[pick].tolist()))
    for row, col in cells:
        want = brute_support(edges, sinQ, cosQ, row, col)
        assert len(want) == acc[row, col]
        assert model_support(edges, sinQ, cosQ, row, col) == want, (row, col)


def test_every_cell_of_a_full_map_including_corners_and_exits(oracle):
    """Every pixel an edge, 23 x 17, every theta of a 1-degree table, every cell: lines through the corner pixels, lines that enter and
    leave through the top or the bottom (positions without a support pixel inside the image), empty cells."""
    W, H, theta = 23, 17, 1.0
    edges = np.full((H, W), 255, np.uint8)
    acc = oracle.sht_acc(edges, theta)
    R, T, _ = oracle.sht_dims(W, H, theta)
    sinQ, cosQ = oracle.sht_tables(theta, T)
    corners = {(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1)}
    seen_corners, partial = set(), 0
    for col in range(T):
        for row in range(R):
            cnt, first, xm = line_occupancy(edges, sinQ, cosQ, row, col)
            assert int(cnt.sum()) == int(acc[row, col]), (row, col)
            if not acc[row, col]:
                assert line_segments(cnt, first, xm, 0, 1, 0) == []
                continue
            want = brute_support(edges, sinQ, cosQ, row, col)
            assert model_support(edges, sinQ, cosQ, row, col) == want, (row, col)
            seen_corners |= want & corners
            partial += int((cnt == 0).any())
            segs = line_segments(cnt, first, xm, 0, 1, 0)
            assert sum(s[5] for s in segs) == acc[row, col]
            for _, x0, y0, x1, y1, _ in segs:
                assert (x0, y0) in want and (x1, y1) in want
    assert seen_corners == corners and partial > 100


# ---- hand-drawn maps ---------------------------------------------------------------------------------------------
MIN_LENGTH, MAX_GAP = 5, 2
# parameter values q that are drawn, piece by piece: [3, 10] -- gap of MAX_GAP (bridged) -- [13, 20] -- gap of MAX_GAP + 1 (split) --
# [24, 27] (length MIN_LENGTH - 1: dropped) -- gap of MAX_GAP + 1 -- [31, 50]
PIECES = [(3, 10), (13, 20), (24, 27), (31, 50)]
GROUPS = [(3, 20, 16), (31, 50, 20)]          # (first q, last q, pixels) of the segments that remain


def drawn(pixel_of_q, W, H):
    e = np.zeros((H, W), np.uint8)
    for a, b in PIECES:
        for q in range(a, b + 1):
            x, y = pixel_of_q(q)
            e[y, x] = 255
    return e


@pytest.mark.parametrize("name,col,pixel_of_q", [
    ("horizontal", 90, lambda q: (q, 20)),
    ("vertical_theta0", 0, lambda q: (30, q)),
    ("deg45", 45, lambda q: (q, 60 - q)),
    ("deg135_negative_cos", 135, lambda q: (q, q + 11)),
])
def test_hand_drawn_pieces(oracle, name, col, pixel_of_q):
    W, H, theta = 80, 70, 1.0
    R, T, _ = oracle.sht_dims(W, H, theta)
    sinQ, cosQ = oracle.sht_tables(theta, T)
    s, c = int(sinQ[col]), int(cosQ[col])
    if name == "vertical_theta0":
        assert s == 0
    if name == "deg135_negative_cos":
        assert c < 0
    edges = drawn(pixel_of_q, W, H)
    # the drawing sits on ONE accumulator cell (the vote's expression on the drawn pixels, nothing of the model)
    ys, xs = np.nonzero(edges)
    rhos = set(((xs.astype(np.int64) * c + ys.astype(np.int64) * s) >> 16).tolist())
    assert len(rhos) == 1, rhos
    row = (W + H) - rhos.pop()
    assert oracle.sht_acc(edges, theta)[row, col] == len(xs)
    # expected records from the construction: the position is x when sinQ >= |cosQ|, else y; segments ascend in the position
    x_major = s >= abs(c)
    exp = []
    for qa, qb, n in GROUPS:
        a, b = pixel_of_q(qa), pixel_of_q(qb)
        if (a[0] if x_major else a[1]) > (b[0] if x_major else b[1]):
            a, b = b, a
        exp.append((0, a[0], a[1], b[0], b[1], n))
    exp.sort(key=lambda r: r[1] if x_major else r[2])
    got = frame_segments(edges, sinQ, cosQ, [(row, col)], MIN_LENGTH, MAX_GAP)
    assert got.dtype == SEG_DTYPE and got.tolist() == exp
    # one pixel less of gap tolerance splits the bridged pair; minLength - 1 lets the short piece in
    assert len(frame_segments(edges, sinQ, cosQ, [(row, col)], MIN_LENGTH, MAX_GAP - 1)) == 3
    assert len(frame_segments(edges, sinQ, cosQ, [(row, col)], MIN_LENGTH - 1, MAX_GAP)) == 3
    assert len(frame_segments(edges, sinQ, cosQ, [(row, col)], 1, MAX_GAP + 1)) == 1
    one = frame_segments(edges, sinQ, cosQ, [(row, col)], 1, 0)
    assert len(one) == len(PIECES) and int(one["support"].sum()) == len(xs)


def test_order_line_index_then_position_and_max_lines(oracle):
    """Two drawn lines given in both orders: records follow the line ARRAY (index ascending), then the position; max_lines cuts the array."""
    W, H, theta = 80, 70, 1.0
    R, T, _ = oracle.sht_dims(W, H, theta)
    sinQ, cosQ = oracle.sht_tables(theta, T)
    edges = drawn(lambda q: (q, 60), W, H) | drawn(lambda q: (60, q), W, H)      # row 60 and column 60 are not drawn on by the other line
    cells = []
    for col, (x, y) in ((90, (3, 60)), (0, (60, 3))):
        cells.append(((W + H) - ((x * int(cosQ[col]) + y * int(sinQ[col])) >> 16), col))
    a = frame_segments(edges, sinQ, cosQ, cells, MIN_LENGTH, MAX_GAP)
    b = frame_segments(edges, sinQ, cosQ, cells[::-1], MIN_LENGTH, MAX_GAP)
    assert a["line"].tolist() == [0, 0, 1, 1] and b["line"].tolist() == [0, 0, 1, 1]
    assert a[["x0", "y0", "x1", "y1"]].tolist() == b[["x0", "y0", "x1", "y1"]][[2, 3, 0, 1]].tolist()
    assert a["x0"].tolist()[:2] == [3, 31] and a["y0"].tolist()[2:] == [3, 31]
    assert a["support"].tolist() == [16, 20, 16, 20]
    assert frame_segments(edges, sinQ, cosQ, cells, MIN_LENGTH, MAX_GAP, max_lines=1).tolist() == a[:2].tolist()


def test_line_leaving_through_the_bottom(oracle):
    """The 135-degree cell of the diagonals y = x + 10 and y = x + 11 (46340 * 10 and 46340 * 11 share the quotient 7) in a 40 x 30 map
    of edges everywhere: two support pixels per position until the diagonals leave through the bottom row, none inside the image after."""
    W, H, theta, col = 40, 30, 1.0, 135
    R, T, _ = oracle.sht_dims(W, H, theta)
    sinQ, cosQ = oracle.sht_tables(theta, T)
    s, c = int(sinQ[col]), int(cosQ[col])
    edges = np.full((H, W), 255, np.uint8)
    row = (W + H) - ((0 * c + 11 * s) >> 16)
    assert brute_support(edges, sinQ, cosQ, row, col) == {(x, x + 10) for x in range(20)} | {(x, x + 11) for x in range(19)}
    # x-major: positions x = 0 .. 19, the smaller y of a position is x + 10; y-major: positions y = 10 .. 29, the smaller x is y - 11 (0 at y = 10)
    exp = (0, 0, 10, 19, 29, 39) if s >= abs(c) else (0, 0, 10, 18, 29, 39)
    assert frame_segments(edges, sinQ, cosQ, [(row, col)], 1, 0).tolist() == [exp]
