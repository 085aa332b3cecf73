"""tests/morph_model.py pinned on the CPU: literals worked out by hand from the definitions of include/compv_hip.h, and every MD5 that
tests/golden/make_golden_morph.py recorded from the compiled reference (tests/golden/golden_morph.json)."""
import numpy as np
import pytest

import morph_model as mm
from fixtures import load_golden, md5

GOLD = load_golden("golden_morph")[0]


def frame(c):
    return np.random.default_rng(c["seed"]).integers(0, 256, size=(c["H"], c["S"]), dtype=np.uint8)[:, :c["W"]]


# ---- hand-computed literals ------------------------------------------------------------------------------------------------------------
def test_enums_are_the_reference_values():
    assert GOLD["enums"] == {"ERODE": mm.ERODE, "DILATE": mm.DILATE, "OPEN": mm.OPEN, "CLOSE": mm.CLOSE, "RECT": mm.RECT, "DIAMOND": mm.DIAMOND,
                             "CROSS": mm.CROSS, "BORDER_ZERO": mm.BORDER_ZERO, "BORDER_REPLICATE": mm.BORDER_REPLICATE}


def test_off_centre_member_is_the_anchor_for_erode_and_dilate():
    """7x7 image img[y][x] = 10 y + x, 3x3 strel whose one member is (j, i) = (0, 2): the interior cell (y, x) takes in(y - 1 + 0, x - 1 + 2) =
    in(y - 1, x + 1) for erode AND for dilate (no reflection).  sh = 3: hb = 2 border rows top and bottom, so only rows 2..4 keep it."""
    img = (10 * np.arange(7)[:, None] + np.arange(7)[None, :]).astype(np.uint8)
    se = np.zeros((3, 3), np.uint8)
    se[0, 2] = 1
    exp = np.array([[0, 0, 0, 0, 0, 0, 0],
                    [0, 0, 0, 0, 0, 0, 0],
                    [0, 12, 13, 14, 15, 16, 0],
                    [0, 22, 23, 24, 25, 26, 0],
                    [0, 32, 33, 34, 35, 36, 0],
                    [0, 0, 0, 0, 0, 0, 0],
                    [0, 0, 0, 0, 0, 0, 0]], np.uint8)
    assert mm.morph(img, se, mm.ERODE, mm.BORDER_ZERO).tolist() == exp.tolist()
    assert mm.morph(img, se, mm.DILATE, mm.BORDER_ZERO).tolist() == exp.tolist()
    rep = exp.copy()
    rep[:2] = img[:2]; rep[5:] = img[5:]; rep[:, 0] = img[:, 0]; rep[:, 6] = img[:, 6]
    assert mm.morph(img, se, mm.ERODE, mm.BORDER_REPLICATE).tolist() == rep.tolist()


def test_vertical_border_is_hb_rows():
    """sh = 1: hb = 1, the first and last rows are copied (REPLICATE) or cleared (ZERO) although a 1-row strel reaches no other row;
    sh = 3: hb = 2, rows 1 and H - 2 are overwritten although they were computed."""
    img = np.array([[9, 1, 9, 9, 9],
                    [9, 1, 9, 9, 9],
                    [9, 9, 9, 1, 9],
                    [9, 9, 9, 1, 9],
                    [9, 9, 9, 1, 9]], np.uint8)
    row3 = np.ones((1, 3), np.uint8)
    # erode with a 3x1 row: interior columns 1..3 take the min of three neighbours; rows 0 and 4 are border
    assert mm.morph(img, row3, mm.ERODE, mm.BORDER_ZERO).tolist() == [[0, 0, 0, 0, 0],
                                                                     [0, 1, 1, 9, 0],
                                                                     [0, 9, 1, 1, 0],
                                                                     [0, 9, 1, 1, 0],
                                                                     [0, 0, 0, 0, 0]]
    assert mm.morph(img, row3, mm.ERODE, mm.BORDER_REPLICATE).tolist() == [[9, 1, 9, 9, 9],
                                                                          [9, 1, 1, 9, 9],
                                                                          [9, 9, 1, 1, 9],
                                                                          [9, 9, 1, 1, 9],
                                                                          [9, 9, 9, 1, 9]]
    col3 = np.ones((3, 1), np.uint8)
    # erode with a 1x3 column: wd = 0 (no column border), hb = 2: only row 2 keeps min(in[1], in[2], in[3])
    assert mm.morph(img, col3, mm.ERODE, mm.BORDER_ZERO).tolist() == [[0, 0, 0, 0, 0],
                                                                     [0, 0, 0, 0, 0],
                                                                     [9, 1, 9, 1, 9],
                                                                     [0, 0, 0, 0, 0],
                                                                     [0, 0, 0, 0, 0]]
    assert mm.morph(img, col3, mm.ERODE, mm.BORDER_REPLICATE).tolist() == [[9, 1, 9, 9, 9],
                                                                          [9, 1, 9, 9, 9],
                                                                          [9, 1, 9, 1, 9],
                                                                          [9, 9, 9, 1, 9],
                                                                          [9, 9, 9, 1, 9]]


def test_adaptive_boundary_in_equals_mean_minus_delta():
    """blockSize 3: k = (uint16)((1.f / 3) * 65535) = 21845.  A constant 90 plane: (90 * 21845) >> 16 = 29 per tap, 87 per horizontal sum;
    (87 * 21845) >> 16 = 28 per tap, so mean = 84 at the one interior cell of a 3x3 image.  With the centre at 79 its tap is 26: the middle row
    sums 84, the column (87, 84, 87) gives 28 + 27 + 28 = 83.  in = 79, mean = 83: with delta = 4, in == mean - delta exactly and the LUT index
    79 - 83 + 255 = 251 lies below its first maxVal slot 256 - 4 = 252: a miss.  With delta = 5 the slot is 251: a hit."""
    assert mm.mean_weight(3) == 21845
    img = np.full((3, 3), 90, np.uint8)
    assert mm.box_mean(img, 3).tolist() == [[0, 0, 0], [0, 84, 0], [0, 0, 0]]
    img[1, 1] = 79
    assert mm.box_mean(img, 3)[1, 1] == 83
    # in == mean - delta exactly: a miss
    assert mm.adaptive(img, 3, 4.0)[1, 1] == 0
    # delta = 5: 251 >= 251 holds -> hit
    assert mm.adaptive(img, 3, 5.0)[1, 1] == 255
    # on the border mean = 0: 90 + 255 >= 256 - d always holds
    assert mm.adaptive(img, 3, 0.0)[0].tolist() == [255, 255, 255]
    assert mm.adaptive(img, 3, 5.0, 100.0, True).tolist() == [[0, 0, 0], [0, 0, 0], [0, 0, 0]]
    assert mm.adaptive(img, 3, 4.0, 100.4, True)[1, 1] == 100


def test_threshold_rounding():
    img = np.arange(256, dtype=np.uint8).reshape(16, 16)
    assert (mm.threshold(img, 0.4) == np.where(img > 0, 255, 0)).all()       # t8 = 0
    assert (mm.threshold(img, 127.5) == np.where(img > 128, 255, 0)).all()   # t8 = 128
    assert (mm.threshold(img, 300.0) == 0).all()                             # clipped to 255: nothing is greater
    with pytest.raises(ValueError):
        mm.threshold(img, -0.1)


def test_diamond_and_cross_literals():
    assert (mm.strel(mm.DIAMOND, 5, 5) != 0).astype(int).tolist() == [[0, 0, 1, 0, 0], [0, 1, 1, 1, 0], [1, 1, 1, 1, 1], [0, 1, 1, 1, 0], [0, 0, 1, 0, 0]]
    assert (mm.strel(mm.CROSS, 5, 3) != 0).astype(int).tolist() == [[0, 0, 1, 0, 0], [1, 1, 1, 1, 1], [0, 0, 1, 0, 0]]
    assert mm.strel(mm.RECT, 2, 1).tolist() == [[255, 255]]


# ---- the compiled reference ----------------------------------------------------------------------------------------------------------------
def test_fixture_is_complete():
    assert len(GOLD["morph"]) == 3 * 6 * 4 * 2 and len(GOLD["strel"]) == 11 and len(GOLD["threshold"]) == 3 * 4
    assert len(GOLD["adaptive"]) == 3 * 3 * 3 * 2 * 2
    assert all(c["md5"] for c in GOLD["morph"]) and all(c["md5"] for c in GOLD["threshold"])
    # the reference is given no image smaller than the block (outside the convolution's domain): exactly those have no MD5
    assert all((c["md5"] is None) == (min(c["W"], c["H"]) < c["blockSize"]) for c in GOLD["adaptive"])


@pytest.mark.parametrize("c", GOLD["strel"], ids=lambda c: "t%d_%dx%d" % (c["type"], c["w"], c["h"]))
def test_strel_matches_reference(c):
    assert md5(mm.strel(c["type"], c["w"], c["h"])) == c["md5"]


def test_mean_tap_matches_reference():
    assert {str(b): mm.mean_weight(b) for b in range(3, 33, 2)} == GOLD["mean_tap"]


def test_morph_matches_reference():
    for c in GOLD["morph"]:
        se = mm.strel(c["type"], c["sw"], c["sh"])
        assert md5(mm.morph(frame(c), se, c["op"], c["border"])) == c["md5"], c


def test_threshold_matches_reference():
    for c in GOLD["threshold"]:
        assert md5(mm.threshold(frame(c), c["threshold"])) == c["md5"], c


def test_adaptive_matches_reference():
    for c in GOLD["adaptive"]:
        if c["md5"] is None:
            with pytest.raises(ValueError):
                mm.adaptive(frame(c), c["blockSize"], c["delta"], c["maxVal"], c["invert"])
        else:
            assert md5(mm.adaptive(frame(c), c["blockSize"], c["delta"], c["maxVal"], c["invert"])) == c["md5"], c
