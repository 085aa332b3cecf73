"""compv_amd/csrc/curvefit_math.hpp -- the arithmetic the curve-fit kernels are made of -- run on the host by tests/host/curvefit_math_check.cpp
(standard library only, no GPU) and held against tests/curvefit_model.py bit for bit: samples, per-try inlier counts, the result record, the mask.
The GPU tests (tests/test_gpu_curvefit.py) hold the kernels against the same model."""
import struct
import subprocess

import numpy as np
import pytest

import curvefit_cases as cc
import curvefit_model as cm
from host_programs import WARN, build, host_cxx


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = build("curvefit_math_check.cpp", tmp_path_factory.mktemp("curvefit"), host_cxx(), ["-O2", "-ffp-contract=off", *WARN])

    def run(pts, model, tries, threshold=cc.THRESHOLD, seed=0, set_index=0, samples=None):
        k, m = len(pts), cm.model_points(model)
        d = exe.parent
        with open(d / "in.bin", "wb") as f:
            f.write(struct.pack("<iiiiiId", k, tries, int(samples is not None), set_index, model, seed, threshold))
            f.write(np.ascontiguousarray(pts, np.float64).tobytes())
            if samples is not None:
                f.write(np.ascontiguousarray(samples, np.int32).tobytes())
        r = subprocess.run([str(exe), str(d / "in.bin"), str(d / "out.bin")], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stdout + r.stderr
        raw = open(d / "out.bin", "rb").read()
        o = cm.RESULT_DTYPE.itemsize
        out = dict(result=np.frombuffer(raw[:o], cm.RESULT_DTYPE)[0], mask=np.frombuffer(raw[o:o + k], np.uint8))
        o += k
        out["counts"] = np.frombuffer(raw[o:o + 4 * tries], np.int32)
        out["samples"] = np.frombuffer(raw[o + 4 * tries:o + 4 * tries + 4 * m * tries], np.int32).reshape(tries, m)
        return out
    return run


def same(got, exp, what):
    assert got["result"].tobytes() == exp["result"].tobytes(), (what, got["result"], exp["result"])
    assert got["mask"].tobytes() == exp["mask"].tobytes(), what
    if exp["counts"] is not None:
        assert got["counts"].tolist() == exp["counts"].tolist(), what
        assert got["samples"].tolist() == exp["samples"].tolist(), what


@pytest.mark.parametrize("model", cm.MODELS)
@pytest.mark.parametrize("k", cc.KS)
def test_header_equals_the_model_on_planted_and_noisy_sets(checker, model, k):
    for share in cc.SHARES:
        for make in (cc.planted, cc.noisy):
            pts, inl, _ = make(model, k, share, 1)
            tries = 65 if k < 129 else 200
            exp = cm.find(pts, k, model, tries, seed=k + 11, set_index=3)
            same(checker(pts, model, tries, seed=k + 11, set_index=3), exp, (model, k, share, make.__name__))
            assert exp["result"]["status"] == 0 and exp["result"]["inliers"] >= cm.model_points(model)
            if make is cc.planted and tries == 200:
                assert (exp["mask"] != 0).tolist() == inl.tolist()


@pytest.mark.parametrize("model", cm.MODELS)
def test_header_equals_the_model_on_the_edge_cases(checker, model):
    m = cm.model_points(model)
    pts, _, _ = cc.planted(model, 12, 0.3, 2)
    for k in (0, m - 1, m, m + 1):          # status 2, the direct path, the smallest set that draws
        exp = cm.find(pts[:k], k, model, 8, seed=4)
        same(checker(pts[:k], model, 8, seed=4), exp, (model, k))
        assert exp["result"]["status"] == (2 if k < m else 0)
    # explicit samples: two equal samples at different t, an index outside [0, k), a repeated index (rejected)
    q = np.array([[0, 1, 2], [3, 4, 5], [0, 1, 2], [0, 12, 1], [-1, 2, 3], [4, 4, 4]], np.int32)[:, :m]
    exp = cm.find(pts, 12, model, len(q), sample_list=q)
    same(checker(pts, model, len(q), samples=q), exp, (model, "explicit samples"))
    assert exp["counts"][0] == exp["counts"][2] and exp["counts"][5] == 0 and (m == 2 or exp["counts"][3] == 0) and exp["counts"][4] == 0
    # every try rejected: the status 1 path
    exp = cm.find(cc.all_equal(20), 20, model, 64)
    same(checker(cc.all_equal(20), model, 64), exp, (model, "all equal"))
    assert exp["result"]["status"] == 1 and not exp["counts"].any() and exp["result"]["bestTry"] == -1
    exp = cm.find(cc.all_equal(m), m, model, 4)
    same(checker(cc.all_equal(m), model, 4), exp, (model, "k = m rejected"))
    assert exp["result"]["status"] == 1 and not exp["mask"].any()
    col = cc.same_abscissa(model, 20)
    exp = cm.find(col, 20, model, 64)
    same(checker(col, model, 64), exp, (model, "same abscissa"))
    assert exp["result"]["status"] == (0 if model == cm.LINE else 1)
    # a NaN point is never an inlier; a denormal threshold keeps the exact fits only
    bad = pts.copy()
    bad[5] = np.nan
    exp = cm.find(bad, 12, model, 64, seed=9)
    same(checker(bad, model, 64, seed=9), exp, (model, "NaN point"))
    assert exp["mask"][5] == 0 and exp["result"]["status"] == 0
    exp = cm.find(pts, 12, model, 64, threshold=5e-324, seed=9)
    same(checker(pts, model, 64, threshold=5e-324, seed=9), exp, (model, "denormal threshold"))


def test_a_failed_refit_keeps_the_best_trys_own_model(checker):
    x = np.array([-1e80, 0.0, 1e80, 2e80, 3e80])          # the refit's moments overflow: its determinant is not finite
    pts = np.stack([x, np.zeros(5)], axis=1)
    q = np.array([[0, 1, 2]], np.int32)
    exp = cm.find(pts, 5, cm.PARABOLA, 1, sample_list=q)
    same(checker(pts, cm.PARABOLA, 1, samples=q), exp, "failed refit")
    assert exp["result"]["status"] == 3 and exp["result"]["inliers"] == 5
