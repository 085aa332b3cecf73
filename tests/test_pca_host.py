"""compv_amd/csrc/pca_math.hpp -- the dot product, the centring, the mean and the model-file parser the PCA kernels and host entry points are made of -- run
on the host by tests/host/pca_math_check.cpp (a stand-alone program with its own main, standard library only, no GPU, built with AddressSanitizer and UBSan,
nothing preloaded) and held against the fixture of the compiled reference on every bit: in one call, and fed the way the kernels feed the header (chunks of
16 * k columns, accumulators kept across chunks)."""
import re
import struct
import subprocess

import numpy as np
import pytest

import pca_cases as pc
import pca_fixture as pf
import pca_model as pm
from host_programs import ASAN_UBSAN_STATIC, WARN, build, host_cxx


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = build("pca_math_check.cpp", tmp_path_factory.mktemp("pca"), host_cxx(), ["-O2", "-g", "-ffp-contract=off", *WARN, *ASAN_UBSAN_STATIC])
    folder = exe.parent

    def run(mode, src, blob=None):
        if blob is not None:
            src = folder / "in.bin"
            src.write_bytes(blob)
        r = subprocess.run([str(exe), mode, str(src), str(folder / "out.bin")], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        return (folder / "out.bin").read_bytes()
    return run


def f32(a):
    return np.ascontiguousarray(a, np.float32).tobytes()


def same(a, b):
    return pm.bits(a).tobytes() == pm.bits(b).tobytes()


def project(checker, x, mean, vectors, chunk):
    n, D = x.shape
    M = vectors.shape[0]
    blob = struct.pack("<5i", n, D, M, int(mean is not None), chunk) + (f32(mean) if mean is not None else b"") + f32(vectors) + f32(x)
    out = np.frombuffer(checker("project", None, blob), np.float32)
    assert out.size == 2 * n * M
    return out[:n * M].reshape(n, M), out[n * M:].reshape(n, M)


@pytest.mark.parametrize("cid", [r["id"] for r in pf.project_cases()])
def test_projection_two_ways_against_the_fixture(checker, cid):
    rec = next(r for r in pf.project_cases() if r["id"] == cid)
    mean, vectors, _ = pf.model(rec["model"])
    x = pf.case_rows(cid)
    for chunk in (16, 64):
        one, fed = project(checker, x, mean, vectors, chunk)
        assert same(one, pf.expected(cid)) and same(fed, pf.expected(cid)), chunk
    one, fed = project(checker, x, None, vectors, 48)
    assert same(one, pf.expected_raw(cid)) and same(fed, pf.expected_raw(cid))


def test_mulabt_and_the_denormal_case(checker):
    _, arrays = pf.golden()
    for a_rows, b_rows, cols in pc.mulabt_cases():
        A, B = pc.mulabt_inputs(a_rows, b_rows, cols)
        one, fed = project(checker, A, None, B, 32)
        exp = arrays["mulabt_%d_%d_%d" % (a_rows, b_rows, cols)]
        assert same(one, exp) and same(fed, exp)
    x, v = pc.denormal_case()
    one, fed = project(checker, x, None, v, 16)
    assert same(one, arrays["raw_" + pc.DENORMAL]) and same(fed, arrays["raw_" + pc.DENORMAL])


@pytest.mark.parametrize("n,D", pc.COVARIANCE)
def test_mean_and_covariance_two_ways(checker, n, D):
    obs, mean, cov = pf.covariance_case(n, D)
    out = np.frombuffer(checker("covariance", None, struct.pack("<3i", n, D, 32) + f32(obs)), np.float32)
    assert out.size == D + 2 * D * D
    assert same(out[:D], mean) and same(out[D:D + D * D], cov) and same(out[D + D * D:], cov)


def test_the_parser_against_the_fixture(checker, tmp_path):
    names = pf.kept_models() + [r["id"] for r in pf.golden()[0]["composed"]]
    assert len(names) >= 21
    for name in names:
        path = tmp_path / (name + ".json")
        path.write_text(pf.model_text(name))
        out = checker("parse", path)
        ok, D, M = struct.unpack_from("<3i", out)
        mean, vectors, values = pf.model(name)
        assert ok == 1 and (D, M) == (mean.size, values.size), name
        got = np.frombuffer(out, np.float32, D + M * D + M, 12)
        assert same(got, np.concatenate([mean, vectors.ravel(), values])), name


def test_the_parser_refuses(checker, tmp_path):
    good = pf.model_text("pca_hand_d4_m3")
    bad = {"truncated": good[:len(good) // 2], "empty": "", "array": "[1,2]", "f64": good.replace('"32f"', '"64f"', 1), "count": good.replace('"size":[1,4]', '"size":[1,5]'),
           "shape": good.replace('"size":[1,4]', '"size":[2,2]'), "overflow": re.sub(r'"data":\[ [^,]+,', '"data":[ 1e39,', good, 1),
           "nan": re.sub(r'"data":\[ [^,]+,', '"data":[ NaN,', good, 1), "trailing": good + "x", "no values": good.replace('"values"', '"valuez"'), "twice": good.replace('"comment": "composed by tests/pca_cases.py"', good[good.index('"values"'):good.index('"vectors"')].rstrip().rstrip(",")),
           "no digits behind the point": good.replace('"size":[1,4]', '"size":[1,4.]')}
    for what, text in bad.items():
        assert text != good, what
        path = tmp_path / "bad.json"
        path.write_text(text)
        assert struct.unpack_from("<3i", checker("parse", path)) == (0, 0, 0), what
    assert struct.unpack_from("<3i", checker("parse", tmp_path / "missing.json")) == (0, 0, 0)
