"""tests/orb_model.py (the ORB definition in numpy) against the compiled reference's recorded outputs (tests/golden/golden_orb.json, written by
tests/golden/make_golden_orb.py) and against hand-made literals.  No GPU, no reference library needed.

What is held bit for bit: the patch moments on every point; the blurred plane (MD5) against both the record and the project's convolution oracle;
the descriptors on every point whose glibc cosf / sinf equal the canonical value (`libm_exact`; at least 95 % of the points).  The reference
detector's own orientation goes through atan2f, so it is held to 1e-4 degrees (circular): atan2f's documented <= 2 ULP at pi (4.8e-7 rad =
2.7e-5 degrees) plus the float32 roundings of `* 180 / pi` and `+ 360` on both sides, each <= half an ULP at 360 = 1.5e-5 degrees."""
import hashlib

import numpy as np
import pytest

import fast_model as fm
import orb_model as om
from fixtures import load_golden


@pytest.fixture(scope="module")
def gold():
    return load_golden("golden_orb")


def f32(bits):
    return np.array(bits, np.uint32).view(np.float32)


def plane_of(case, arrays):
    if case["content"] == "level1_plane":
        p = arrays["level1_plane"]
        assert p.shape == (case["H"], case["W"])
        return p
    return fm.noise(case["W"], case["H"], case["seed"]) if case["content"] == "noise" else fm.blocks(case["W"], case["H"], case["seed"])


def keys_of(rec, level, scale):
    k = np.zeros(len(rec["x_bits"]), om.KEYPOINT_DTYPE)
    k["x"], k["y"], k["orient"], k["level"], k["size"] = f32(rec["x_bits"]), f32(rec["y_bits"]), f32(rec["orient_bits"]), level, np.float32(31.0) / scale
    return k


def test_pattern_and_disc():
    AX, AY, BX, BY = om.pattern()
    for p in (AX, AY, BX, BY):
        assert p.dtype == np.float32 and len(p) == 256 and p.min() >= -13 and p.max() <= 12
    assert (AX[0], AY[0], BX[0], BY[0]) == (8, -3, 9, 5) and (AX[255], AY[255], BX[255], BY[255]) == (-1, -6, 0, -11)   # the first and last test of the published pattern
    assert om.DX == [15, 14, 14, 14, 14, 14, 13, 13, 12, 12, 11, 10, 9, 7, 5, 0]
    # every rotated pattern point stays within 18 of the centre: 13 * sqrt(2) = 18.38 rounds to 18
    for deg in np.arange(0.0, 360.0, 0.25, dtype=np.float32):
        c, s, _ = om.canonical_cos_sin(np.array([deg], np.float32))
        for PX, PY in ((AX, AY), (BX, BY)):
            assert np.abs(np.rint(PX * c - PY * s)).max() <= om.BORDER and np.abs(np.rint(PX * s + PY * c)).max() <= om.BORDER
    # float32 quotients: 180.f / pi_f is 0x42652ee0, one ULP below the float32 nearest to 180 / pi
    assert np.array([om.K180_OVER_PI, om.KPI_OVER_180], np.float32).view(np.uint32).tolist() == [0x42652ee0, 0x3c8efa35]


def test_moments_equal_the_reference_on_every_point(gold):
    g, _ = gold
    assert sorted({(c["W"], c["H"]) for c in g["moments"]}) == [(37, 37), (64, 41), (200, 258)]
    n = 0
    for c in g["moments"]:
        img = fm.noise(c["W"], c["H"], c["seed"]) if c["content"] == "noise" else fm.blocks(c["W"], c["H"], c["seed"])
        m01, m10 = om.moments(img, c["x"], c["y"])
        assert m01.tolist() == c["m01"] and m10.tolist() == c["m10"], (c["W"], c["H"], c["content"])
        n += len(c["x"])
    assert n >= 200


def test_blurred_plane_equals_the_reference_and_the_convolution_oracle(gold, oracle):
    g, arrays = gold
    assert (om.gauss_kernel_q16() == oracle.gauss_kernel_fxp(5, 2.0)).all()
    for c in g["descriptors"]:
        plane = plane_of(c, arrays)
        k = oracle.gauss_kernel_fxp(5, 2.0)
        rc, orc = oracle.convlt_fxp(np.ascontiguousarray(plane), k, k)
        assert rc == 0
        assert hashlib.md5(np.ascontiguousarray(orc).tobytes()).hexdigest() == c["blurred_md5"], (c["W"], c["H"], c["content"])
        assert (om.blur(plane) == orc).all()


def test_descriptors_equal_the_reference_where_its_libm_is_exact(gold):
    g, arrays = gold
    exact = total = 0
    levels = set()
    every = []
    for c in g["descriptors"]:
        scale = f32([c["scale_bits"]])[0]
        plane = plane_of(c, arrays)
        keys = keys_of(c, c["level"], scale)
        want = np.frombuffer(bytes.fromhex(c["desc"]), np.uint8).reshape(-1, 32)
        got = om.describe(om.blur(plane), keys, scale)
        assert got.shape == want.shape
        ok = np.array([ch == "1" for ch in c["libm_exact"]])
        assert (got[ok] == want[ok]).all(), (c["W"], c["H"], c["content"], np.nonzero((got != want).any(axis=1) & ok)[0][:8])
        exact += int(ok.sum()); total += len(ok)
        levels.add(c["level"])
        every.append(want)
    assert levels == {0, 1} and total >= 300 and exact >= 0.95 * total, (exact, total)
    b = np.unpackbits(np.concatenate(every), axis=1).astype(bool)
    assert b.any(axis=0).all() and (~b).any(axis=0).all()          # every one of the 256 tests takes both values


def test_fixed_orientations_are_among_the_fed_points(gold):
    g, _ = gold
    fed = np.concatenate([f32(c["orient_bits"]) for c in g["descriptors"] if c["level"] == 0])
    for o in om.FIXED_ORIENTS:
        assert (fed == np.float32(o)).any(), o


def test_reference_detector_orientation_is_within_1e_4_degrees(gold):
    g, arrays = gold
    seen = set()
    for c in g["descriptors"]:
        if "dete" not in c:
            continue
        scale = f32([c["scale_bits"]])[0]
        plane = plane_of(c, arrays)
        d = c["dete"]
        xi, okx = om.centre(f32(d["x_bits"]), scale)
        yi, oky = om.centre(f32(d["y_bits"]), scale)
        assert okx.all() and oky.all() and len(xi) > 20 and om.admissible(xi, yi, c["W"], c["H"]).all()
        m01, m10 = om.moments(plane, xi, yi)
        mine, theirs = om.orient_of(m01, m10).astype(np.float64), f32(d["orient_bits"]).astype(np.float64)
        diff = np.abs(mine - theirs)
        diff = np.minimum(diff, 360.0 - diff)
        assert diff.max() <= 1e-4, diff.max()
        assert (theirs >= 0).all() and (theirs <= 360).all()
        seen.add(c["level"])
    assert seen == {0, 1}


def test_constant_frame_literal():
    img = om.constant(64, 50, 97)
    c = np.zeros(2, om.CORNER_DTYPE)
    c["x"], c["y"], c["strength"] = [30, 17], [25, 25], [9, 9]          # the second lies 17 from the left border: erased
    k, m = om.keypoints(img, c, 0, 1.0)
    assert len(k) == 1 and m.tolist() == [[0, 0]]
    assert k[0].tolist() == (30.0, 25.0, 9.0, 0.0, 0, 31.0)
    assert not om.describe(om.blur(img), k, 1.0).any()          # a == b everywhere: no bit set


def test_mirrored_frame_literal():
    W, H = 63, 50
    img = om.mirrored(fm.noise(W, H, 77))
    assert (img == img[:, ::-1]).all()
    c = np.zeros(1, om.CORNER_DTYPE)
    c["x"], c["y"] = W // 2, 25
    k, m = om.keypoints(img, c, 0, 1.0)
    assert m[0, 1] == 0 and m[0, 0] != 0          # m10 == 0
    assert k["orient"][0] in (np.float32(90.0), np.float32(270.0))
    r = om.ramp(W, H)
    k, m = om.keypoints(r, c, 0, 1.0)
    assert m[0, 0] == 0          # a horizontal ramp has no vertical moment


def test_border_erase_and_level_scaling():
    W, H = 70, 60
    img = fm.noise(W, H, 5)
    xs = [17, 18, W - 19, W - 18, 30, 30, 30, 30]
    ys = [30, 30, 30, 30, 17, 18, H - 19, H - 18]
    c = np.zeros(len(xs), om.CORNER_DTYPE)
    c["x"], c["y"], c["strength"] = xs, ys, np.arange(len(xs))
    k, _ = om.keypoints(img, c, 0, 1.0)
    assert k["strength"].tolist() == [1, 2, 5, 6]          # 18 and W - 19 stay, 17 and W - 18 go; the order is kept
    s = np.float32(0.83)
    k1, _ = om.keypoints(img, c, 1, s)
    assert (k1["x"] == k["x"] * (np.float32(1) / s)).all() and (k1["size"] == np.float32(31) / s).all() and (k1["orient"] == k["orient"]).all()
    # a key inside the margin, or holding no number at all, gets a zero row in its own place
    bad = k.copy()
    bad["x"][1], bad["y"][2] = 17.4, np.nan
    d, good = om.describe(om.blur(img), bad, 1.0), om.describe(om.blur(img), k, 1.0)
    assert not d[1].any() and not d[2].any() and (d[[0, 3]] == good[[0, 3]]).all() and good.any(axis=1).all()
