"""compv_amd/csrc/homography_math.hpp -- the arithmetic the homography kernels are made of -- run on the host by tests/host/homography_math_check.cpp
(standard library only, no GPU) and held against tests/homography_model.py bit for bit: quads, per-try inlier counts, variances and rotation counts,
the result record, the mask.  The GPU tests (tests/test_gpu_homography.py) hold the kernels against the same model."""
import struct
import subprocess

import numpy as np
import pytest

import homography_cases as hc
import homography_model as hm
from host_programs import WARN, build, host_cxx


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = build("homography_math_check.cpp", tmp_path_factory.mktemp("homography"), host_cxx(), ["-O2", "-ffp-contract=off", *WARN])

    def run(src, dst, tries, threshold=30.0, seed=0, pair=0, quads=None):
        k = len(src)
        d = exe.parent
        with open(d / "in.bin", "wb") as f:
            f.write(struct.pack("<iiiiIid", k, tries, int(quads is not None), pair, seed, 0, threshold))
            f.write(np.ascontiguousarray(src, np.float64).tobytes() + np.ascontiguousarray(dst, np.float64).tobytes())
            if quads is not None:
                f.write(np.ascontiguousarray(quads, np.int32).tobytes())
        r = subprocess.run([str(exe), str(d / "in.bin"), str(d / "out.bin")], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stdout + r.stderr
        raw = open(d / "out.bin", "rb").read()
        o = hm.RESULT_DTYPE.itemsize
        out = dict(result=np.frombuffer(raw[:o], hm.RESULT_DTYPE)[0], mask=np.frombuffer(raw[o:o + k], np.uint8))
        o += k
        out["counts"] = np.frombuffer(raw[o:o + 4 * tries], np.int32)
        out["variances"] = np.frombuffer(raw[o + 4 * tries:o + 12 * tries], np.float64)
        out["rotations"] = np.frombuffer(raw[o + 12 * tries:o + 16 * tries], np.int32)
        out["quads"] = np.frombuffer(raw[o + 16 * tries:o + 32 * tries], np.int32).reshape(tries, 4)
        return out
    return run


def same(got, exp, what):
    assert got["result"].tobytes() == exp["result"].tobytes(), (what, got["result"], exp["result"])
    assert got["mask"].tobytes() == exp["mask"].tobytes(), what
    if exp["counts"] is not None:
        assert got["counts"].tolist() == exp["counts"].tolist(), what
        assert got["variances"].tobytes() == np.ascontiguousarray(exp["variances"]).tobytes(), what
        assert got["rotations"].tolist() == exp["rotations"].tolist(), what


@pytest.mark.parametrize("k", hc.KS)
def test_header_equals_the_model_on_planted_cases(checker, k):
    for share in hc.SHARES:
        src, dst, inl = hc.planted(k, share, 1)
        tries = 65 if k < 129 else 200
        exp = hm.find(src, dst, k, tries, seed=k + 11, pair=3)
        got = checker(src, dst, tries, seed=k + 11, pair=3)
        assert got["quads"].tolist() == exp["quads"].tolist()
        same(got, exp, (k, share))
        assert exp["result"]["status"] == 0 and exp["result"]["rotations"] > 0


def test_header_equals_the_model_on_the_edge_cases(checker):
    src, dst, _ = hc.planted(9, 0.0, 2)
    q = hc.edge_quads(9)
    exp = hm.find(src, dst, 9, len(q), quad_list=q)
    same(checker(src, dst, len(q), quads=q), exp, "edge quads")
    assert exp["counts"][1] < 4 and exp["counts"][2] == 0 and exp["counts"][4] == 0 and exp["counts"][0] >= 4
    src, dst, _ = hc.collinear_case()
    q = np.array([[0, 1, 2, 3], [3, 2, 1, 0], [4, 5, 6, 8]], np.int32)
    exp = hm.find(src, dst, 9, 3, quad_list=q)
    same(checker(src, dst, 3, quads=q), exp, "collinear")
    assert exp["counts"].tolist()[:2] == [0, 0] and exp["rotations"].tolist()[:2] == [0, 0] and exp["counts"][2] >= 4
    src[:4, 0] = 33.0                                     # a vertical line
    exp = hm.find(src, dst, 9, 3, quad_list=q)
    same(checker(src, dst, 3, quads=q), exp, "vertical")
    assert exp["counts"].tolist()[:2] == [0, 0]
    src, dst, _ = hc.planted(20, 1.0, 3)                  # all outliers: a quad still fits its own four points, so a best exists
    exp = hm.find(src, dst, 20, 64, threshold=0.5)
    same(checker(src, dst, 64, threshold=0.5), exp, "all outliers")
    assert exp["result"]["status"] == 0 and 4 <= exp["result"]["inliers"] < 8
    src, dst = hc.line_case(20)                           # every source on one line: every try is collinear and scores 0 -- the status 1 path
    exp = hm.find(src, dst, 20, 64)
    same(checker(src, dst, 64), exp, "no best")
    assert exp["result"]["status"] == 1 and exp["result"]["inliers"] == 0 and exp["result"]["rotations"] > 0 and not exp["counts"].any()
    exp = hm.find(src[:3], dst[:3], 3, 8)
    same(checker(src[:3], dst[:3], 8), exp, "k = 3")
    assert exp["result"]["status"] == 2 and not exp["result"]["H"].any()
