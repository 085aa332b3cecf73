"""tests/moments_model.py -- the definition of the image moments in Python integers and numpy float64 -- against the fixture the compiled reference
made (tests/golden/make_golden_moments.py: every bit of the six sums and of skew, the angle within the bound) and against literals worked out by hand."""
import numpy as np
import pytest

import moments_cases as mc
import moments_model as mm
from fixtures import load_golden


@pytest.fixture(scope="module")
def golden():
    return load_golden("golden_moments")


def test_sums_by_hand():
    """a 3 x 2 plane: p = [[1, 0, 2], [0, 3, 4]]"""
    p = np.array([[1, 0, 2], [0, 3, 4]], np.uint8)
    #          m00 = 1 + 2 + 3 + 4;  m01 = 1 * (3 + 4);  m10 = 2 * 2 + 1 * 3 + 2 * 4;  m11 = 1 * 3 + 2 * 4;  m02 = 3 + 4;  m20 = 4 * 2 + 1 * 3 + 4 * 4
    assert mm.raw_sums(p) == mm.raw_sums_slow(p) == (10, 7, 15, 11, 7, 27)
    assert mm.raw_sums(p, mm.UNIT) == mm.raw_sums_slow(p, mm.UNIT) == (4, 2, 5, 3, 2, 9)


def test_shape_by_hand():
    """m00 10, m01 20, m10 30, m11 70, m02 50, m20 100: ybar 2, xbar 3, u20 = u02 = u11 = 1, den 0 -> (1, 0); a = 50 - 40, b = 70 - 60 -> skew 1;
    with m20 140: u20 5, den 4, atan2(2, 4) / 2"""
    s = mm.shape((10, 20, 30, 70, 50, 100))
    assert [float(s[k]) for k in mm.SHAPE_NAMES] == [3.0, 2.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.0] and s["status"] == 0
    s = mm.shape((10, 20, 30, 70, 50, 140))
    assert float(s["u20"]) == 5.0 and mm.angle_case(s)
    assert abs(mm.theta(s) - 0.5 * np.arctan2(2.0, 4.0)) < 1e-15
    assert abs(float(s["cs"]) ** 2 + float(s["sn"]) ** 2 - 1.0) < 1e-15
    empty = mm.shape((0, 0, 0, 0, 0, 0))
    assert empty["status"] == 1 and float(empty["cs"]) == 1.0 and all(float(empty[k]) == 0.0 for k in mm.SHAPE_NAMES if k != "cs")


def test_a_single_pixel_has_no_orientation_and_no_skew():
    c = mc.frame_case("corner_br")
    s = mm.shape(mm.raw_sums(mc.frame(c)))
    assert (float(s["xbar"]), float(s["ybar"])) == (32.0, 20.0) and (float(s["cs"]), float(s["sn"]), float(s["skew"])) == (1.0, 0.0, 0.0)


def test_the_range_rule():
    assert mm.fits(3840, 2160, mm.VALUE) and mm.fits(16384, 16384, mm.VALUE) and mm.fits(32767, 32767, mm.UNIT) and not mm.fits(32767, 32767, mm.VALUE)
    assert not mm.fits(0, 5, mm.UNIT) and not mm.fits(5, 32768, mm.UNIT) and not mm.fits(5, 5, 2)
    # both sides of 2^64: 255 * 16406 * 16384 * 16405^2 = 0.99999 * 2^64, with 16407 columns 1.00017 * 2^64; the same at 2056 / 2057 x 32767
    assert mm.fits(16406, 16384, mm.VALUE) and not mm.fits(16407, 16384, mm.VALUE) and mm.fits(16407, 16384, mm.UNIT)
    assert mm.fits(2056, 32767, mm.VALUE) and not mm.fits(2057, 32767, mm.VALUE) and mm.fits(32767, 2056, mm.VALUE) and not mm.fits(32767, 2057, mm.VALUE)
    # the rule is sufficient: the all-255 frame of the largest VALUE size stays below 2^64 in its largest sum
    w, h = 16406, 16384
    assert 255 * h * sum(i * i for i in range(w)) < 2 ** 64 and 255 * sum(range(w)) * sum(range(h)) < 2 ** 64


@pytest.mark.parametrize("small", [c for c in mc.frame_cases() if c["size"][0] * c["size"][1] <= 4000], ids=lambda c: c["id"])
def test_row_sums_equal_the_definition(small):
    img = mc.frame(small)
    for weights in small["weights"]:
        assert mm.raw_sums(img, weights) == mm.raw_sums_slow(img, weights)


def test_frames_against_the_fixture(golden):
    meta, arrays = golden
    seen = 0
    for rec in meta["frames"]:
        c = mc.frame_case(rec["case"])
        sums = mm.raw_sums(mc.frame(c), rec["weights"])
        assert list(sums) == rec["sums"] and arrays["raw_" + rec["id"]].tolist() == rec["sums"], rec["id"]
        if rec.get("model_only"):
            assert max(sums) >= 2 ** 53
            continue
        s = mm.shape(sums)
        assert float(s["skew"]).hex() == rec["skew"], rec["id"]
        if mm.angle_case(s):
            assert abs(mm.theta(s) - float.fromhex(rec["theta"])) <= 4 * meta["max_angle_distance"], rec["id"]
            seen += 1
    assert seen >= 15 and 0 < meta["max_angle_distance"] < 1e-15
    assert [m["id"] for m in meta["model_only"]] == [mc.BIG + "_value"]


@pytest.mark.parametrize("c", mc.component_cases(), ids=lambda c: c["id"])
def test_components_against_the_fixture(golden, c):
    meta, arrays = golden
    labels, comps = mc.labelled(c)
    gray = mc.component_frame(c)[1] if c["gray"] else None
    sums = mm.component_sums(labels, comps, len(comps), len(comps), gray, c["weights"], c["origin"])
    assert mm.raw_array(sums).tolist() == arrays["raw_" + c["id"]].tolist()
    for k, m in enumerate(sums):
        s = mm.shape(m)
        assert np.float64(s["skew"]).tobytes() == arrays["skew_" + c["id"]][k].tobytes()
        if mm.angle_case(s):
            assert abs(mm.theta(s) - arrays["theta_" + c["id"]][k]) <= 4 * meta["max_angle_distance"]
    # a clipped call serves a prefix; a negative count serves nothing
    assert mm.component_sums(labels, comps, len(comps), 2, gray, c["weights"], c["origin"]) == sums[:2]
    assert mm.component_sums(labels, comps, -3, 5, gray, c["weights"], c["origin"]) == []
    if c["origin"] == mm.ORIGIN_BOX:          # the crop's own sums are the BOX sums
        k = len(comps) - 1
        assert mm.raw_sums(mm.crop_of(labels, comps[k], k + 1, gray, c["weights"])) == sums[k]
