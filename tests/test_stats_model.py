"""CPU tests of tests/stats_model.py, the numpy statement of the image statistics: against plain Python loops, against the closed forms of a constant frame,
against every fixture of tests/golden/golden_stats.* (which the generator held against the compiled reference byte for byte), and the equalisation table
where float32(running sum) first rounds and where it is clamped."""
import numpy as np
import pytest

import stats_cases as sc
import stats_model as sm
from fixtures import load_golden, md5


def model_arrays(c):
    img, hist = sc.case_frame(c), sc.other_hist(c)
    s, q = sm.integral(img)
    px, py = sm.projections(img)
    own, lut_own = sm.equalize(img)
    given, lut_given = sm.equalize(img, hist)
    clamped, lut_clamped = sm.equalize(img, None, sc.CLAMP_SCALE)
    return dict(sum=s, sumsq=q, hist=sm.histogram(img), eq_own=own, eq_given=given, projX=px, projY=py, lut_own=lut_own, lut_given=lut_given,
                eq_clamped=clamped, lut_clamped=lut_clamped)


@pytest.mark.parametrize("W,H", [(1, 1), (1, 7), (7, 1), (5, 3), (33, 17)])
def test_model_against_plain_loops(W, H):
    img = sc.noise(W, H, 5)
    p = [[int(v) for v in row] for row in img]
    s, q = sm.integral(img)
    assert s.shape == q.shape == (H + 1, W + 1) and s.dtype == q.dtype == np.float64
    for y in range(H + 1):
        for x in range(W + 1):
            assert s[y, x] == sum(p[j][i] for j in range(y) for i in range(x))
            assert q[y, x] == sum(p[j][i] ** 2 for j in range(y) for i in range(x))
    hist = [0] * 256
    for row in p:
        for v in row:
            hist[v] += 1
    assert sm.histogram(img).tolist() == hist and sm.histogram(img).dtype == np.uint32
    px, py = sm.projections(img)
    assert px.dtype == py.dtype == np.int32
    assert px.tolist() == [sum(p[j][i] for j in range(H)) for i in range(W)]
    assert py.tolist() == [sum(p[j]) for j in range(H)]
    # the table: float32 scalars, one operation at a time
    scale = np.float32(255.0 / float(W * H))
    run, lut = 0, []
    for h in hist:
        run = (run + h) & 0xffffffff
        v = np.float32(np.float32(run) * scale)
        lut.append(min(int(v), 255))
    out, t = sm.equalize(img)
    assert t.tolist() == lut and t.dtype == np.uint8
    assert out.tolist() == [[lut[v] for v in row] for row in p]


@pytest.mark.parametrize("W,H", [(1, 1), (37, 29), (300, 2)])
def test_closed_forms_of_a_constant_255_frame(W, H):
    img = sc.const255(W, H)
    s, q = sm.integral(img)
    yx = np.outer(np.arange(H + 1), np.arange(W + 1))
    assert (s == 255.0 * yx).all() and (q == 65025.0 * yx).all()
    px, py = sm.projections(img)
    assert (px == 255 * H).all() and px.size == W and (py == 255 * W).all() and py.size == H
    h = sm.histogram(img)
    assert h[255] == W * H and h.sum() == W * H


def test_model_against_every_fixture():
    meta, arrays = load_golden("golden_stats")
    meta = meta["cases"]
    assert [c["id"] for c in meta] == [c["id"] for c in sc.CASES]
    seen = 0
    for g in meta:
        c = sc.BY_ID[g["id"]]
        assert (g["W"], g["H"], g["kind"]) == (c["W"], c["H"], c["kind"]) and g["frame_md5"] == md5(sc.case_frame(c))
        m = model_arrays(c)
        assert {k: md5(v) for k, v in m.items()} == g["md5"], g["id"]
        assert g["stored"] == (c["W"] * c["H"] <= sc.STORE_LIMIT)
        for k, v in m.items():
            name = "%s_%s" % (k, g["id"])
            assert (name in arrays.files) == g["stored"]
            if g["stored"]:
                assert arrays[name].dtype == v.dtype and arrays[name].shape == v.shape and arrays[name].tobytes() == v.tobytes(), name
                seen += 1
    assert seen == len(arrays.files) and seen > 0


def test_table_where_float32_of_the_running_sum_rounds():
    """5000 x 3400 pixels: the running sum passes 2^24, the first place where float32(run) is no longer run"""
    W, H = 5000, 3400
    hist = np.zeros(256, np.uint32)
    hist[0], hist[1], hist[2], hist[200] = (1 << 24) - 1, 2, 1, W * H - (1 << 24) - 2
    assert int(hist.sum()) == W * H
    run = np.cumsum(hist.astype(np.uint64))
    assert float(np.float32(run[1])) != float(run[1]) and float(np.float32(run[0])) == float(run[0])          # 2^24 + 1 is not a float32
    scale = np.float32(255.0 / float(W * H))
    expect = [min(int(np.float32(np.float32(int(r)) * scale)), 255) for r in run]
    t = sm.lut(hist, 0.0, W, H)
    assert t.tolist() == expect and t[255] == 255 and t[0] == int(np.float32(np.float32((1 << 24) - 1) * scale))
    # the running sum is taken modulo 2^32
    wrap = np.zeros(256, np.uint32)
    wrap[0], wrap[1] = 0xffffffff, 7
    assert sm.lut(wrap, 1.0, W, H).tolist()[:3] == [255, 6, 6]


def test_a_clamped_table():
    """scale 1.0 on a 16 x 16 frame: the table is min(running sum, 255); the reference's own conversion is undefined from 256 on"""
    img = sc.noise(16, 16, 3)
    out, t = sm.equalize(img, None, sc.CLAMP_SCALE)
    run = np.cumsum(sm.histogram(img).astype(np.int64))
    assert t.tolist() == np.minimum(run, 255).tolist()
    assert run[-1] == 256 and t[-1] == 255 and sm.lut_unclamped_max(sm.histogram(img), sc.CLAMP_SCALE, 16, 16) == 256.0
    assert (out == t[img]).all()
