"""tests/pca_model.py -- the numpy float32 restatement of the PCA projection -- against the fixture of the compiled reference (tests/golden/golden_pca.*,
written by tests/golden/make_golden_pca.py): every stored projection, the outputs without a mean, mulABt, the denormal case, the means and the covariances,
on every bit."""
import numpy as np
import pytest

import pca_cases as pc
import pca_fixture as pf
import pca_model as pm


def same(a, b):
    return np.shape(a) == np.shape(b) and pm.bits(a).tobytes() == pm.bits(b).tobytes()


def test_the_fixture_covers_what_it_should():
    meta, arrays = pf.golden()
    dims = {r["dim"] for r in meta["trained"] + meta["hand"] + meta["composed"]}
    comps = {r["components"] for r in meta["trained"] + meta["hand"] + meta["composed"]}
    assert {1, 3, 4, 15, 16, 19, 31, 32, 33, 5, 17, 20, 36, 67, 441, 3780} <= dims and {1, 63, 64, 65, 92} <= comps
    assert {r["n"] for r in meta["project"]} >= {1, 2, 63, 64, 65, 100}
    assert [tuple(c) for c in meta["mulabt"]] == pc.mulabt_cases()
    assert [(r["n"], r["dim"]) for r in meta["covariance"]] == pc.COVARIANCE
    assert any(r["rows"] == "reference" and (r["n"], r["dim"], r["components"]) == (100, 441, 92) for r in meta["project"])


@pytest.mark.parametrize("cid", [r["id"] for r in pf.project_cases()])
def test_projection_equals_the_reference(cid):
    rec = next(r for r in pf.project_cases() if r["id"] == cid)
    mean, vectors, _ = pf.model(rec["model"])
    x = pf.case_rows(cid)
    assert same(pm.project(x, mean, vectors), pf.expected(cid))
    pf.expected_raw(cid)          # asserts the digest of the outputs without a mean
    if rec["dim"] >= 5:
        assert not same(pm.dot_left_to_right(pm.centre(x, mean), vectors), pf.expected(cid))


def test_mulabt_and_the_denormal_case():
    _, arrays = pf.golden()
    for a_rows, b_rows, cols in pc.mulabt_cases():
        A, B = pc.mulabt_inputs(a_rows, b_rows, cols)
        assert same(pm.mulabt(A, B), arrays["mulabt_%d_%d_%d" % (a_rows, b_rows, cols)])
    x, v = pc.denormal_case()
    exp = arrays["raw_" + pc.DENORMAL]
    assert same(pm.mulabt(x, v), exp)
    assert ((exp != 0) & (np.abs(exp) < pm.TINY)).any() and not same(pm.dot16(x, v, ftz=True), exp)


@pytest.mark.parametrize("n,D", pc.COVARIANCE)
def test_mean_and_covariance(n, D):
    obs, mean, cov = pf.covariance_case(n, D)          # asserts the reference's mean and the covariance's digest
    assert same(cov, cov.T) and cov.shape == (D, D)
    if n == 1:
        assert not cov.any() and same(mean, obs[0])


def test_the_dot_is_symmetric_and_three_columns_have_one_order():
    a, b = pc.rows(9, 53, 77), pc.rows(7, 53, 78)
    assert same(pm.dot16(a, b), pm.dot16(b, a).T)
    a, b = pc.rows(9, 3, 79), pc.rows(7, 3, 80)
    assert same(pm.dot16(a, b), pm.dot_left_to_right(a, b))
