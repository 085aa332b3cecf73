"""tests/curvefit_model.py -- the numpy definition of the RANSAC line and parabola fits -- against the fixture tests/golden/golden_curvefit.* (generated
by tests/golden/make_golden_curvefit.py, which held the model against the compiled reference: items B and C bit for bit, planted sets within 1e-6 px),
and the definition's properties."""
import numpy as np
import pytest

import curvefit_cases as cc
import curvefit_model as cm
from fixtures import GOLDEN_DIR, load_golden


@pytest.fixture(scope="module")
def golden():
    return load_golden("golden_curvefit")


def check_stored(arrays, cid, out):
    assert out["result"].tobytes() == arrays["result_" + cid].tobytes(), cid
    assert out["mask"].tobytes() == arrays["mask_" + cid].tobytes(), cid
    if out["counts"] is not None:
        assert out["counts"].tolist() == arrays["counts_" + cid].tolist(), cid
        assert out["samples"].tolist() == arrays["samples_" + cid].tolist(), cid


def test_model_equals_the_fixture(golden):
    meta, arrays = golden
    assert len(meta["cases"]) == 2 * len(cm.MODELS) * len(cc.KS) * len(cc.SHARES) and len(meta["direct"]) == 15 and meta["distances"] == 10
    for d in meta["direct"]:
        pts = arrays["pts_" + d["id"]]
        out = cm.find(pts, len(pts), d["model"], 1, cc.THRESHOLD)
        check_stored(arrays, d["id"], out)
        assert out["result"]["status"] == d["status"]
    for c in meta["cases"]:
        pts = arrays["pts_" + c["id"]]
        out = cm.find(pts, c["k"], c["model"], c["tries"], c["threshold"], seed=c["seed"])
        check_stored(arrays, c["id"], out)
        assert c["px"] <= 1e-6          # what the generator asserted: against the reference (planted) or the independent solve (noisy)
        if c["kind"] == "planted":
            assert (out["mask"] != 0).tolist() == (arrays["inl_" + c["id"]] != 0).tolist() and c["inliers"] == c["planted"]


def test_fixture_sets_are_the_case_generators(golden):
    meta, arrays = golden
    for c in meta["cases"]:
        make = cc.planted if c["kind"] == "planted" else cc.noisy
        pts, inl, _ = make(c["model"], c["k"], c["share"], 1)
        assert pts.tobytes() == arrays["pts_" + c["id"]].tobytes() and inl.tolist() == (arrays["inl_" + c["id"]] != 0).tolist()


def test_residuals_equal_the_fixture(golden):
    _, arrays = golden
    import sys
    sys.path.insert(0, GOLDEN_DIR)
    from make_golden_curvefit import CURVES
    for model in cm.MODELS:
        for i, p in enumerate(CURVES[model]):
            got = cm.residuals(model, p[0], p[1], p[2], arrays["cloud"])[0]
            assert got.tobytes() == arrays["dist_m%d_%d" % (model, i)].tobytes(), (model, p)


@pytest.mark.parametrize("model", cm.MODELS)
def test_a_sample_fits_its_own_points(model):
    """no try of a set with distinct abscissas is rejected, and a model holds its own sample when the threshold is at least its rounding: the unscaled
    line A x + B y + C is exactly 0 there, the scaled one of item C within a few ulp of |C| / sqrt(A^2 + B^2); a parabola within the rounding of its
    coefficients.  So a best always exists on such a set."""
    m = cm.model_points(model)
    pts, _, _ = cc.planted(model, 40, 1.0, 3)          # all outliers: scattered integer points
    q = cm.samples(model, 5, 0, 40, 64)
    thr = 1e-9 if model == cm.LINE else 1e-6
    out = cm.find(pts, 40, model, 64, thr, sample_list=q)
    d = out["distances"]
    assert (out["counts"] >= m).all() and out["result"]["status"] == 0
    for t in range(64):
        assert (d[t, q[t]] < thr).all(), t
    if model == cm.LINE:
        A, B, C, ok = cm.curve_of(model, pts[q, 0], pts[q, 1])
        assert ok.all() and not ((A[:, None] * pts[q, 0] + B[:, None] * pts[q, 1]) + C[:, None]).any()


@pytest.mark.parametrize("model", cm.MODELS)
def test_samples_are_distinct_and_in_range(model):
    m = cm.model_points(model)
    for seed, s, k, tries in [(0, 0, m + 1, 300), (0xffffffff, 65534, 9, 200), (77, 2, 65, 65), (0x80000000, 31, 2000, 500)]:
        q = cm.samples(model, seed, s, k, tries)
        assert q.shape == (tries, m) and (q >= 0).all() and (q < k).all() and all(len(set(r)) == m for r in q.tolist())
    assert cm.samples(model, 3, 0, 50, 100).tolist() != cm.samples(model, 3, 1, 50, 100).tolist()


@pytest.mark.parametrize("model", cm.MODELS)
def test_ties_go_to_the_smaller_try(model):
    m = cm.model_points(model)
    pts, inl, _ = cc.planted(model, 30, 0.3, 4)
    good = np.nonzero(inl)[0][:m]
    bad = np.nonzero(~inl)[0][:m]
    q = np.stack([bad, good, good, good[::-1]]).astype(np.int32)
    out = cm.find(pts, 30, model, 4, sample_list=q)
    assert out["counts"][1] == out["counts"][2] == inl.sum() and out["result"]["bestTry"] == 1 and out["result"]["status"] == 0


@pytest.mark.parametrize("model", cm.MODELS)
def test_small_and_degenerate_sets(model):
    m = cm.model_points(model)
    pts, _, _ = cc.planted(model, 12, 0.0, 5)
    r = cm.find(pts, m - 1, model, 8)
    assert r["result"]["status"] == 2 and r["result"]["k"] == m - 1 and r["result"]["bestTry"] == -1 and len(r["mask"]) == m - 1 and not r["mask"].any()
    assert cm.find(pts, -4, model, 8)["result"]["k"] == 0 and cm.find(pts, 99, model, 8)["result"]["k"] == 12
    r = cm.find(pts, m, model, 8)
    assert r["result"]["status"] == 0 and r["result"]["inliers"] == m and r["result"]["bestTry"] == 0 and r["mask"].all() and r["counts"] is None
    A, B, C, ok = cm.curve_of(model, pts[None, :m, 0], pts[None, :m, 1])
    assert ok[0] and (r["result"]["A"], r["result"]["B"], r["result"]["C"]) == (A[0], B[0], C[0])
    r = cm.find(cc.all_equal(m), m, model, 8)
    assert r["result"]["status"] == 1 and not r["mask"].any() and r["result"].tobytes()[:24] == bytes(24)
    r = cm.find(cc.all_equal(20), 20, model, 50)
    assert r["result"]["status"] == 1 and not r["counts"].any() and not r["mask"].any()
    r = cm.find(cc.same_abscissa(model, 20), 20, model, 50)
    if model == cm.LINE:
        assert r["result"]["status"] == 0 and r["result"]["inliers"] == 20 and abs(r["result"]["A"]) == 1.0 and r["result"]["B"] == 0.0 and r["result"]["C"] == -3.0 * r["result"]["A"]
    else:
        assert r["result"]["status"] == 1


@pytest.mark.parametrize("model", cm.MODELS)
def test_nan_point_and_denormal_threshold(model):
    pts, inl, _ = cc.planted(model, 40, 0.3, 6)
    bad = pts.copy()
    victim = int(np.nonzero(inl)[0][3])
    bad[victim] = np.nan
    r = cm.find(bad, 40, model, 100)
    expect = inl.copy()
    expect[victim] = False
    assert r["result"]["status"] == 0 and (r["mask"] != 0).tolist() == expect.tolist() and np.isfinite([r["result"]["A"], r["result"]["B"], r["result"]["C"]]).all()
    q = cm.samples(model, 0, 0, 40, 100)
    assert not r["counts"][(q == victim).any(axis=1)].any()          # a try that draws the NaN point has a NaN model and no inlier
    r = cm.find(pts, 40, model, 100, threshold=5e-324)
    assert r["result"]["status"] in (0, 1) and (r["counts"] <= inl.sum()).all()
    if r["result"]["status"] == 0:          # only residuals of exactly 0 are below the smallest denormal
        d = r["distances"][r["result"]["bestTry"]]
        assert ((d == 0.0) == (r["mask"] != 0)).all()


def test_refit_failure_keeps_the_best_trys_own_model():
    """four points whose centred abscissas make the normal matrix singular cannot exist for distinct x; a determinant that overflows can: status 3"""
    x = np.array([-1e80, 0.0, 1e80, 2e80, 3e80])
    pts = np.stack([x, np.zeros(5)], axis=1)
    r = cm.find(pts, 5, cm.PARABOLA, 1, threshold=1.0, sample_list=np.array([[0, 1, 2]], np.int32))
    assert r["counts"][0] == 5 and r["result"]["status"] == 3 and r["result"]["inliers"] == 5
    A, B, C, ok = cm.curve_of(cm.PARABOLA, pts[None, :3, 0], pts[None, :3, 1])
    assert ok[0] and r["result"].tobytes()[:24] == np.array([A[0], B[0], C[0]]).tobytes()
