"""CPU tests of the PCA boundary of the C ABI (include/compv_hip.h, "PCA projection"): the exports exist, are bound and keep their argument order, follow the
header's rules (no stream parameter: the stream travels in the descriptor; no handle type; no name ending in _u8 or _f64), the refusals that need no device
hold, compvhip_pca_model_parse returns the arrays of the reference's read for every kept file and refuses malformed ones writing nothing, and
compvhip_pca_dot_host equals tests/pca_model.py on every bit."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import pca_cases as pc
import pca_fixture as pf
import pca_model as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAMS = {
    "compvhip_pca_project": "ctx desc d_mean d_vectors vecStride dim components d_in n inStride d_out outStride",
    "compvhip_mulabt_f32": "ctx desc d_A aRows aStride d_B bRows bStride cols d_R rStride",
    "compvhip_pca_covariance": "ctx desc d_obs n obsStride dim d_mean d_covar covStride d_scratch",
    "compvhip_pca_covariance_scratch": "n dim bytes",
    "compvhip_pca_project_host": "ctx desc mean vectors vecStride dim components in n inStride out outStride",
    "compvhip_pca_model_parse": "path dim components mean vectors values",
    "compvhip_pca_dot_host": "a b n out",
}


def header():
    return open(os.path.join(ROOT, "include", "compv_hip.h")).read()


def test_exports_are_declared_bound_and_in_order():
    from compv_amd import capi
    lib = capi.load()
    txt = re.sub(r"/\*.*?\*/", " ", header(), flags=re.S)
    decls = dict(re.findall(r"COMPVHIP_API\s+[\w\s\*]+?\b(compvhip_(?:pca_\w+|mulabt_\w+))\s*\(([^)]*)\)\s*;", txt))
    assert sorted(decls) == sorted(PARAMS)
    for name, params in decls.items():
        assert [re.search(r"(\w+)\s*$", p).group(1) for p in params.split(",")] == PARAMS[name].split(), name
        assert name in capi.EXPORTS and hasattr(lib, name), name
        assert not re.search(r"void\s*\*\s*stream", params) and not name.endswith(("_u8", "_f64")), name
        assert len(getattr(lib, name).argtypes) == len(PARAMS[name].split()), name
    body = re.search(r"typedef struct compvhip_pca_desc \{(.*?)\} compvhip_pca_desc;", header(), re.S).group(1)
    assert re.search(r"void\*\s+hipStream;", body) and C.sizeof(capi.PcaDesc) == 16
    assert not re.search(r"typedef\s+struct\s+compvhip_pca\w*\s+compvhip_pca\w*\s*;", header())          # no opaque handle


def test_refusals_that_need_no_device():
    from compv_amd import capi
    lib = capi.load()
    d = C.byref(capi.PcaDesc())
    E = capi.E_INVALID_PARAMETER
    assert lib.compvhip_pca_project(None, d, None, None, 4, 4, 2, None, 1, 4, None, 2) == E
    assert lib.compvhip_mulabt_f32(None, d, None, 1, 4, None, 1, 4, 4, None, 1) == E
    assert lib.compvhip_pca_covariance(None, d, None, 2, 4, 4, None, None, 4, None) == E
    assert lib.compvhip_pca_project_host(None, d, None, None, 4, 4, 2, None, 1, 4, None, 2) == E
    b = C.c_size_t(77)
    for n, dim in ((0, 5), (5, 0), (2 ** 31, 5), (5, 2 ** 20 + 1), (2 ** 31 - 1, 2 ** 20)):
        assert lib.compvhip_pca_covariance_scratch(n, dim, C.byref(b)) == E and b.value == 77, (n, dim)
    assert lib.compvhip_pca_covariance_scratch(5, 5, None) == E
    assert capi.pca_covariance_scratch(1, 5) == 5 * 16 * 4 and capi.pca_covariance_scratch(33, 17) == 17 * 48 * 4 and capi.pca_covariance_scratch(64, 2 ** 20) == 2 ** 28
    out = C.c_float(5.0)
    one = np.ones(4, np.float32)
    assert lib.compvhip_pca_dot_host(None, capi._ptr(one), 4, C.byref(out)) == E and lib.compvhip_pca_dot_host(capi._ptr(one), None, 4, C.byref(out)) == E and out.value == 5.0
    assert lib.compvhip_pca_dot_host(capi._ptr(one), capi._ptr(one), 4, None) == E


@pytest.mark.parametrize("D", [0, 1, 3, 4, 5, 15, 16, 17, 19, 20, 36])
def test_dot_host(D):
    from compv_amd import capi
    a, b = pc.rows(6, max(D, 1), 40 + D)[:, :D], pc.rows(6, max(D, 1), 90 + D)[:, :D]
    exp = pm.dot16(a, b)
    for i in range(6):
        for j in range(6):
            got = capi.pca_dot(a[i], b[j])
            assert np.float32(got).tobytes() == exp[i, j].tobytes(), (D, i, j)
    if D == 0:
        assert capi.pca_dot([], []).tobytes() == np.float32(0).tobytes()          # +0
    if D >= 5:
        assert pm.bits(exp).tobytes() != pm.bits(pm.dot_left_to_right(a, b)).tobytes()


def test_model_parse_on_every_kept_file():
    from compv_amd import capi
    names = pf.kept_models()
    assert len(names) == 19
    for name in names:
        m = capi.PcaModel.from_file(pf.model_path(name))
        mean, vectors, values = pf.model(name)
        assert (m.dim, m.components) == vectors.shape[::-1], name
        assert pm.bits(m.mean).tobytes() == pm.bits(mean).tobytes() and pm.bits(m.vectors).tobytes() == pm.bits(vectors).tobytes() and pm.bits(m.values).tobytes() == pm.bits(values).tobytes(), name


def test_model_parse_on_the_composed_files(tmp_path):
    from compv_amd import capi
    for rec in pf.golden()[0]["composed"]:
        path = tmp_path / (rec["id"] + ".json")
        path.write_text(pf.model_text(rec["id"]))
        m = capi.PcaModel.from_file(str(path))
        assert pc.sha256(np.concatenate([m.mean, m.vectors.ravel(), m.values])) == rec["arrays_sha256"], rec["id"]


def test_model_parse_refuses_and_writes_nothing(tmp_path):
    from compv_amd import capi
    lib = capi.load()
    good = pf.model_text("pca_hand_d4_m3")
    vectors_at, values_at = good.index('"vectors"'), good.index('"values"')
    bad = {"truncated": good[:len(good) // 2], "cut in a number": good[:vectors_at + 30], "empty": "", "array": "[1,2]", "f64": good.replace('"32f"', '"64f"', 1),
           "count": good.replace('"size":[1,4]', '"size":[1,5]'), "shape": good.replace('"size":[1,4]', '"size":[2,2]'),
           "overflow": re.sub(r'"data":\[ [^,]+,', '"data":[ 1e39,', good, 1), "nan": re.sub(r'"data":\[ [^,]+,', '"data":[ NaN,', good, 1),
           "trailing": good + "x", "no values": good.replace('"values"', '"valuez"'), "unquoted": good.replace('"type":"32f"', '"type":32f', 1),
           "missing comma": good.replace('"size":[1,4],', '"size":[1,4]'), "mean twice": good.replace('"comment": "composed by tests/pca_cases.py"', good[values_at:vectors_at].rstrip().rstrip(","))}
    dim, comps = C.c_int32(-5), C.c_int32(-6)
    arrays = [np.full(64, 7, np.uint8) for _ in range(3)]
    for what, text in bad.items():
        assert text != good, what
        path = tmp_path / "bad.json"
        path.write_text(text)
        rc = lib.compvhip_pca_model_parse(os.fsencode(str(path)), C.byref(dim), C.byref(comps), *[capi._ptr(a) for a in arrays])
        assert rc == capi.E_INVALID_PARAMETER and (dim.value, comps.value) == (-5, -6) and all((a == 7).all() for a in arrays), what
        with pytest.raises(capi.CompvHipError):
            capi.PcaModel.from_file(str(path))
    assert lib.compvhip_pca_model_parse(os.fsencode(str(tmp_path / "missing.json")), C.byref(dim), C.byref(comps), None, None, None) == capi.E_INVALID_PARAMETER
    assert lib.compvhip_pca_model_parse(None, C.byref(dim), C.byref(comps), None, None, None) == capi.E_INVALID_PARAMETER
    assert lib.compvhip_pca_model_parse(os.fsencode(pf.model_path("pca_hand_d4_m3")), None, C.byref(comps), None, None, None) == capi.E_INVALID_PARAMETER
    # limits: D beyond 2^20 (a mean of 2^20 + 1 zeros, no vectors to match: refused before or at the limit check either way)
    big = '{"mean":{"type":"32f","size":[1,%d],"data":[%s]},"vectors":{"type":"32f","size":[1,%d],"data":[%s]},"values":{"type":"32f","size":[1,1],"data":[1]}}'
    n = 2 ** 20 + 1
    zeros = ",".join("0" * 1 for _ in range(n))
    path = tmp_path / "big.json"
    path.write_text(big % (n, zeros, n, zeros))
    assert lib.compvhip_pca_model_parse(os.fsencode(str(path)), C.byref(dim), C.byref(comps), None, None, None) == capi.E_INVALID_PARAMETER
    n = 2 ** 20
    zeros = ",".join("0" for _ in range(n))
    path.write_text(big % (n, zeros, n, zeros))
    assert lib.compvhip_pca_model_parse(os.fsencode(str(path)), C.byref(dim), C.byref(comps), None, None, None) == capi.OK and (dim.value, comps.value) == (2 ** 20, 1)
