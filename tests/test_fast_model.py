"""tests/fast_model.py against the compiled reference's recorded outputs (tests/golden/golden_fast.json, written by
tests/golden/make_golden_fast.py) and against hand-computed literals.  CPU only.

The fixture MD5s cover the (x, y, strength) triples of CompVCornerDeteFAST::process on one thread: N 9 and 12, NMS on and off, t in {1, 20, 100},
noise and blurred blocks, five sizes down to 7 x 7 (one interior pixel).  That the model -- which evaluates every arc of every interior pixel and
has none of the early exits of CompVFastDataRow_C -- reproduces all of them confirms that those exits are necessary conditions only."""
import hashlib

import numpy as np
import pytest

import fast_model as fm
from fixtures import load_golden

GOLDEN = load_golden("golden_fast")[0]
CASES = GOLDEN["cases"]


def case_frame(c):
    return (fm.noise if c["content"] == "noise" else fm.blocks)(c["W"], c["H"], c["seed"])


def test_fixture_covers_the_grid():
    assert len(CASES) == 5 * 2 * 2 * 2 * 3
    assert {(c["W"], c["H"], c["S"]) for c in CASES} == {(7, 7, 7), (20, 20, 20), (130, 17, 160), (642, 31, 704), (200, 258, 200)}
    assert {c["N"] for c in CASES} == {9, 12} and {c["nonmax"] for c in CASES} == {0, 1} and {c["threshold"] for c in CASES} == {1, 20, 100}
    assert sum(c["count"] for c in CASES) > 100000 and any(c["count"] > GOLDEN["cut"] and c["content"] == "blocks" for c in CASES)


@pytest.mark.parametrize("size", sorted({(c["W"], c["H"]) for c in CASES}), ids=lambda s: "%dx%d" % s)
def test_model_equals_every_fixture(size):
    for c in (c for c in CASES if (c["W"], c["H"]) == size):
        rec, _ = fm.fast(case_frame(c), c["threshold"], c["N"], bool(c["nonmax"]), -1)
        triples = np.stack([rec["x"], rec["y"], rec["strength"]], axis=1).astype("<i4")
        assert len(rec) == c["count"], c
        assert hashlib.md5(np.ascontiguousarray(triples).tobytes()).hexdigest() == c["md5"], c


@pytest.mark.parametrize("size", sorted({(c["W"], c["H"]) for c in CASES}), ids=lambda s: "%dx%d" % s)
def test_canonical_cut_brackets_the_reference_cut(size):
    """the canonical set contains the reference's maxFeatures = 50 set (as strength multisets: which corners of a tie the reference keeps is
    unspecified), and that set contains every corner with strength > s*"""
    from collections import Counter
    K = GOLDEN["cut"]
    for c in (c for c in CASES if (c["W"], c["H"]) == size):
        full, _ = fm.fast(case_frame(c), c["threshold"], c["N"], bool(c["nonmax"]), -1)
        canon = fm.cut(full, K)
        ref = Counter(c["cut_strengths"])
        if len(full) <= K:
            assert len(canon) == len(full) and sorted(full["strength"].tolist()) == c["cut_strengths"], c
            continue
        s_star = np.sort(full["strength"])[::-1][K - 1]
        assert canon.tobytes() == full[full["strength"] >= s_star].tobytes()
        assert len(canon) >= K and sum(ref.values()) >= K, c
        have = Counter(canon["strength"].tolist())
        assert all(have[s] >= n for s, n in ref.items()), c                                   # canonical contains the reference's
        above = Counter(full["strength"][full["strength"] > s_star].tolist())
        assert all(ref[s] == n for s, n in above.items()), c                                   # ... which holds everything above the cut
        assert min(ref) >= s_star, c


# ---- literals ----------------------------------------------------------------------------------------------------------------------------
def ring_frame(ground, centre, values, W=11, H=9, cx=5, cy=4):
    img = np.full((H, W), ground, np.uint8)
    img[cy, cx] = centre
    for (dx, dy), v in zip(fm.RING, values):
        if v is not None:
            img[cy + dy, cx + dx] = v
    return img


def test_single_bright_pixel_on_black():
    """Every pixel AROUND a lone bright pixel scores 0 (each sees one brighter ring pixel: no arc).  The pixel itself does score: its ring is a
    full darker circle, so its score is d - 0 = 200 - t (the compiled reference agrees: the `lone` entry of the fixture file)."""
    img = np.zeros((9, 11), np.uint8)
    img[4, 5] = 200
    for N in (9, 12):
        s = fm.score_map(img, 20, N)
        assert s[4, 5] == 180 and np.count_nonzero(s) == 1
    lone = GOLDEN["lone"]
    rec, _ = fm.fast(img, 20, 9, True)
    assert [[int(r["x"]), int(r["y"]), int(r["strength"])] for r in rec] == lone == [[5, 4, 199]]


def test_arc_of_9_exactly_one_past_the_threshold_scores_1():
    t = 20
    arc = [100 + t + 1] * 9 + [100] * 7                     # nine ring pixels brighter than b = 120 by 1
    img = ring_frame(100, 100, arc)
    assert fm.score_map(img, t, 9)[4, 5] == 1
    assert fm.score_map(img, t, 12)[4, 5] == 0
    assert fm.score_map(ring_frame(100, 100, [100 + t] * 9 + [100] * 7), t, 9)[4, 5] == 0          # exactly at the threshold: not brighter
    rec, _ = fm.fast(img, t, 9, False)
    assert [(int(r["x"]), int(r["y"]), int(r["strength"])) for r in rec if (r["x"], r["y"]) == (5, 4)] == [(5, 4, 1 + t - 1)]
    # the arc may wrap around position 15 -> 0, and the score is the arc's SMALLEST difference
    wrap = [None] * 16
    for k in range(12, 21):
        wrap[k & 15] = 10 + (k - 12)                         # darker than d = 80 by 70 .. 62
    assert fm.score_map(ring_frame(100, 100, [100 if v is None else v for v in wrap]), t, 9)[4, 5] == 62


def test_arcs_one_short_score_zero():
    assert fm.score_map(ring_frame(100, 100, [200] * 8 + [100] * 8), 20, 9)[4, 5] == 0
    assert fm.score_map(ring_frame(100, 100, [0] * 11 + [100] * 5), 20, 12)[4, 5] == 0
    assert fm.score_map(ring_frame(100, 100, [0] * 11 + [100] * 5), 20, 9)[4, 5] == 80
    assert fm.score_map(ring_frame(100, 100, [0] * 12 + [100] * 4), 20, 12)[4, 5] == 80
    # eight darker and eight brighter: neither kind has nine in a row
    assert fm.score_map(ring_frame(100, 100, [0] * 8 + [255] * 8), 20, 9)[4, 5] == 0


def test_equal_adjacent_scores_are_both_suppressed():
    s = np.zeros((9, 11), np.uint8)
    s[4, 4] = s[4, 5] = 7          # a tie: both go
    s[2, 8] = 9
    s[3, 9] = 8                    # the diagonal neighbour of a larger score goes, the larger one stays
    s[7, 2] = 1                    # alone: stays
    out = fm.nms(s)
    assert out[4, 4] == 0 and out[4, 5] == 0 and out[2, 8] == 9 and out[3, 9] == 0 and out[7, 2] == 1
    assert np.count_nonzero(out) == 2


def test_border_pixels_never_score():
    rng = np.random.default_rng(3)
    for (W, H) in ((7, 7), (8, 13), (40, 9)):
        img = rng.integers(0, 2, (H, W), dtype=np.uint8) * 255
        for N in (9, 12):
            s = fm.score_map(img, 1, N)
            inner = np.zeros_like(s, bool)
            inner[3:H - 3, 3:W - 3] = True
            assert not s[~inner].any()
    img = np.zeros((7, 7), np.uint8)
    img[3, 3] = 255
    rec, s = fm.fast(img, 1, 12, True)
    assert s[3, 3] == 254 and [(int(r["x"]), int(r["y"]), int(r["strength"])) for r in rec] == [(3, 3, 254)]


def test_cut_keeps_ties_in_raster_order():
    rec = np.zeros(7, fm.CORNER_DTYPE)
    rec["x"] = np.arange(7)
    rec["strength"] = [5, 9, 5, 7, 5, 9, 1]
    assert fm.cut(rec, 3)["x"].tolist() == [1, 3, 5]                 # s* = 7
    assert fm.cut(rec, 4)["x"].tolist() == [0, 1, 2, 3, 4, 5]        # s* = 5: all three 5s stay
    assert fm.cut(rec, 2)["x"].tolist() == [1, 5]
    assert fm.cut(rec, 1)["x"].tolist() == list(range(7)) and fm.cut(rec, -1)["x"].tolist() == list(range(7)) and fm.cut(rec, 7)["x"].tolist() == list(range(7))


def test_doubling_equals_the_arc_by_arc_definition():
    for (W, H, seed) in ((7, 7, 1), (23, 11, 2), (64, 40, 3)):
        for img in (fm.noise(W, H, seed), fm.blocks(W, H, seed), fm.seam_noise(W, H, seed, 16, 8), fm.tied_arcs(W, H, seed)):
            for t in (0, 1, 20, 100, 255):
                for N in (9, 12):
                    assert fm.score_map(img, t, N).tobytes() == fm.score_map_direct(img, t, N).tobytes(), (W, H, t, N)


def test_test_content_has_what_it_promises():
    s = fm.score_map(fm.seam_noise(300, 70, 5), 20, 9)
    ys, xs = np.nonzero(s)
    assert len(xs) > 50 and all(min(x % 128, 128 - x % 128) <= 4 or min(y % 32, 32 - y % 32) <= 4 for x, y in zip(xs, ys))
    rec, _ = fm.fast(fm.tied_arcs(100, 60, 6), 20, 9, True)
    assert len(rec) >= 40 and set(rec["strength"].tolist()) <= {20, 21, 22} and len(set(rec["strength"].tolist())) == 3
