"""tests/match_model.py against the records of the compiled reference (tests/golden/golden_match.json, written by
tests/golden/make_golden_match.py) and against literals worked out by hand."""
import hashlib

import numpy as np
import pytest

import match_model as mm
from fixtures import load_golden

GOLDEN = load_golden("golden_match")[0]


def md5(m):
    flat = np.ascontiguousarray(m).view("<i4")
    return hashlib.md5(flat.tobytes()).hexdigest()


def test_fixture_covers_what_it_should():
    cases = GOLDEN["cases"]
    assert len(cases) == 2 * 3 * 25 * 4
    assert {c["cols"] for c in cases} == {32, 8, 5} and {c["knn"] for c in cases} == {1, 2, 3, 8}
    assert {(c["Q"], c["T"]) for c in cases} == {(q, t) for q in (1, 2, 3, 65, 300) for t in (1, 2, 3, 65, 300)}
    assert any(c["knn"] > c["T"] and c["rows"] == c["T"] for c in cases)
    assert GOLDEN["enums"]["sizeof_CompVDMatch"] == mm.MATCH_DTYPE.itemsize == 16
    assert GOLDEN["big"]["md5"] == GOLDEN["big"]["md5_threads"] and GOLDEN["big"]["threads_used"] > 1


@pytest.mark.parametrize("kind", ["uniform", "ties"])
@pytest.mark.parametrize("cols", [32, 8, 5])
def test_model_reproduces_the_reference(kind, cols):
    """knn_reference (the reference's insertion) reproduces every recorded MD5.  knn (the canonical (distance, train index) order of the device call)
    has the same distances everywhere and the same records wherever a query's first rows + 1 distances are distinct -- and does differ from the
    reference on the tie-heavy cases: the reference's order among equal distances is not the stable one."""
    n = differ = 0
    cache = {}
    for c in GOLDEN["cases"]:
        if c["content"] != kind or c["cols"] != cols:
            continue
        key = (c["Q"], c["T"], c["seed"])
        if key not in cache:
            q, t = mm.content(kind, c["Q"], cols, c["seed"]), mm.content(kind, c["T"], cols, c["seed"] + 100000)
            cache[key] = (q, t, mm.distances(q, t))
        q, t, D = cache[key]
        ref = mm.knn_reference(q, t, c["knn"], D)
        assert ref.shape == (c["rows"], c["Q"]) and md5(ref) == c["md5"], c
        m = mm.knn(q, t, c["knn"], D)
        assert m.shape == ref.shape and (m["distance"] == ref["distance"]).all() and (m["queryIdx"] == ref["queryIdx"]).all(), c
        s = np.sort(D, axis=1)[:, :c["rows"] + 1]
        distinct = (np.diff(s, axis=1) != 0).all(axis=1)
        assert (m["trainIdx"][:, distinct] == ref["trainIdx"][:, distinct]).all(), c
        differ += int((m["trainIdx"] != ref["trainIdx"]).any())
        n += 1
    assert n == 100
    if kind == "ties":
        assert differ > 0


def test_model_reproduces_the_large_case():
    b = GOLDEN["big"]
    q, t = mm.content(b["content"], b["Q"], b["cols"], b["seed"]), mm.content(b["content"], b["T"], b["cols"], b["seed"] + 100000)
    D = mm.distances(q, t)
    assert md5(mm.knn_reference(q, t, b["knn"], D)) == b["md5"]
    assert (mm.knn(q, t, b["knn"], D)["distance"] == mm.knn_reference(q, t, b["knn"], D)["distance"]).all()


def test_reference_order_on_a_literal():
    """distances of one query to train rows 0..3: 5, 5, 3, 9.  Stable order: t2 (3), t0 (5), t1 (5).  The reference: t0 and t1 fill the list as
    [t0, t1]; t2 takes the head, the displaced t0 is not smaller than t1 and walks past it: [t2, t1, t0] with three rows, [t2, t1] with two."""
    q = np.zeros((1, 4), np.uint8)
    t = np.array([[0x1f, 0, 0, 0], [0, 0x1f, 0, 0], [0x07, 0, 0, 0], [0xff, 0x01, 0, 0]], np.uint8)
    assert mm.distances(q, t).tolist() == [[5, 5, 3, 9]]
    assert mm.knn(q, t, 3)["trainIdx"][:, 0].tolist() == [2, 0, 1] and mm.knn(q, t, 2)["trainIdx"][:, 0].tolist() == [2, 0]
    assert mm.knn_reference(q, t, 3)["trainIdx"][:, 0].tolist() == [2, 1, 0] and mm.knn_reference(q, t, 2)["trainIdx"][:, 0].tolist() == [2, 1]
    assert mm.knn_reference(q, t, 3)["distance"][:, 0].tolist() == [3, 5, 5]


def test_tie_heavy_content_has_ties():
    q, t = mm.tie_heavy(65, 32, 1), mm.tie_heavy(300, 32, 2)
    D = mm.distances(q, t)
    s = np.sort(D, axis=1)
    assert (s[:, 0] == s[:, 1]).mean() > 0.9          # nearly every query has two train rows at its best distance


Q3 = np.array([[0x00, 0x00, 0x00, 0x00],
               [0xff, 0x00, 0x00, 0x00],
               [0x0f, 0x0f, 0x00, 0x00]], np.uint8)
T4 = np.array([[0x01, 0x00, 0x00, 0x00],          # d: q0 1, q1 7, q2 7
               [0x00, 0x80, 0x00, 0x00],          # d: q0 1, q1 9, q2 9      q0: an exact tie between t0 and t1
               [0xff, 0x0f, 0x00, 0x00],          # d: q0 12, q1 4, q2 4
               [0xf0, 0x00, 0x00, 0xf0]], np.uint8)          # d: q0 8, q1 8, q2 16


def test_hand_computed_literal():
    D = mm.distances(Q3, T4)
    assert D.tolist() == [[1, 1, 12, 8], [7, 9, 4, 8], [7, 9, 4, 16]]
    m = mm.knn(Q3, T4, 3)
    assert m.shape == (3, 3)
    # neighbour rows: q0 -> t0, t1 (tie at 1: the lower index first), t3; q1 -> t2, t0, t3; q2 -> t2, t0, t1
    assert m["trainIdx"].tolist() == [[0, 2, 2], [1, 0, 0], [3, 3, 1]]
    assert m["distance"].tolist() == [[1, 4, 4], [1, 7, 7], [8, 8, 9]]
    assert m["queryIdx"].tolist() == [[0, 1, 2]] * 3 and not m["imageIdx"].any()
    # a second exact tie: two equal train rows
    T = np.vstack([T4[2], T4[2], T4[0]])
    m = mm.knn(Q3, T, 8)
    assert m.shape == (3, 3) and m["trainIdx"][:, 1].tolist() == [0, 1, 2] and m["distance"][:, 1].tolist() == [4, 4, 7]
    dev = mm.knn_device(Q3, T, 4)
    assert dev.shape == (4, 3) and dev[3]["trainIdx"].tolist() == [-1] * 3 and dev[3]["distance"].tolist() == [mm.INT32_MAX] * 3
    assert dev[3]["queryIdx"].tolist() == [0, 1, 2]


def test_good_list_where_each_test_removes_a_different_query():
    # q0: d0 = 1, d1 = 1            fails the ratio test (1 < 0.8 * 1 is false)
    # q1: d0 = 4, d1 = 7            passes all three
    # q2: d0 = 4 at t2, but t2's best query is q1 (4, lower index)      fails the cross check
    # q3: d0 = 5, d1 = 7            passes ratio (5 < 5.6), fails d0 <= 4
    q = np.vstack([Q3, [[0x01, 0x00, 0xf8, 0x00]]]).astype(np.uint8)
    D = mm.distances(q, T4)
    assert D[3].tolist() == [5, 7, 16, 14]
    none = mm.good(q, T4, 2)
    assert none["queryIdx"].tolist() == [0, 1, 2, 3]
    ratio = mm.good(q, T4, 2, ratio=0.8)
    assert ratio["queryIdx"].tolist() == [1, 2, 3]          # 1 < 0.8 fails; 4 < 5.6; 4 < 5.6; 5 < 5.6
    dist = mm.good(q, T4, 2, max_distance=4)
    assert dist["queryIdx"].tolist() == [0, 1, 2]
    cross = mm.good(q, T4, 2, cross_check=True)
    assert cross["queryIdx"].tolist() == [0, 1]          # q2 loses t2 to q1; q3's best row t0 belongs to q0
    both = mm.good(q, T4, 2, ratio=0.8, max_distance=4, cross_check=True)
    assert both.tolist() == [(1, 2, 0, 4)]
    # a ratio whose product is not exactly representable: 0.7 * 7 = 4.8999999999999995 in binary64
    assert 0.7 * 7.0 != 4.9 and mm.good(q, T4, 2, ratio=0.7)["queryIdx"].tolist() == [1, 2]          # q3: 5 < 4.8999... is false
    # fewer than two train rows: the ratio test passes none; without it every query is good
    assert len(mm.good(q, T4[:1], 2, ratio=0.99)) == 0 and len(mm.good(q, T4[:1], 2)) == 4
    assert len(mm.good(q[:0], T4, 2)) == 0 and len(mm.good(q, T4[:0], 2)) == 0
